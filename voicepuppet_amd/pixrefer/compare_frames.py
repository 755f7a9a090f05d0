#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Per-frame L1, MSE, PSNR and SSIM between two runs, computed on the device (voicepuppet_amd.metrics.FrameMetrics):

    python voicepuppet_amd/pixrefer/compare_frames.py A B [--out metrics.json]

A and B are two directories of <i>.jpg with the same indices and sizes - two infer_bfmvid / infer_stream outputs (bf16 against f32, the
device JPEG encoder against PIL's) - or two `bench.py --dump-outputs` directories, whose generator output Outputs.npy (float32
[N, H, H, 3] in [0, 1]) is compared.  The .jpg files are decoded on the device (JpegDecoder; a file it refuses is decoded by PIL and
uploaded) and never come back to the host.  One line per frame, then mean, min, max and the worst frame per metric (the lowest PSNR and
SSIM, the highest L1 and MSE); --out writes the same as JSON.  The reference has no counterpart.

Either side may also be a Motion-JPEG .avi file (voicepuppet_amd.avi_read.AviReader): its frame i is compared with <i>.jpg of the other
side, or with frame i of the other file.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

sys.path.append(os.getcwd())

COLUMNS = ("L1", "MSE", "PSNR", "SSIM")
CHUNK = 64                        # frame pairs per compare call


def numbered_jpgs(d):
  """{i: path} of the <i>.jpg files of directory d"""
  out = {}
  for name in os.listdir(d):
    m = re.fullmatch(r"(\d+)\.jpg", name)
    if m:
      out[int(m.group(1))] = os.path.join(d, name)
  return out


def avi_frames(path):
  """{i: (AviReader, i)} of the frames of a Motion-JPEG AVI file"""
  from voicepuppet_amd.avi_read import AviReader
  try:
    reader = AviReader(path, batch=CHUNK)
  except ValueError as e:
    raise SystemExit("compare_frames: %s" % e)
  return {i: (reader, i) for i in range(reader.frames)}


def pair_up(a, b):
  """-> ("jpg", indices, paths of a, paths of b) or ("npy", None, array path of a, array path of b); SystemExit names what is missing.
  A frame of an .avi side stands in the path lists as (AviReader, index)."""
  from voicepuppet_amd.avi_read import is_avi
  avi = [os.path.isfile(d) and is_avi(d) for d in (a, b)]
  for d, v in zip((a, b), avi):
    if not v and not os.path.isdir(d):
      raise SystemExit("compare_frames: %s is neither a directory nor an AVI file" % d)
  na, nb = os.path.join(a, "Outputs.npy"), os.path.join(b, "Outputs.npy")
  ja, jb = (avi_frames(d) if v else numbered_jpgs(d) for d, v in zip((a, b), avi))
  if not any(avi) and not ja and not jb and os.path.exists(na) and os.path.exists(nb):
    return "npy", None, na, nb
  if not ja or not jb:
    raise SystemExit("compare_frames: no <i>.jpg files (and no Outputs.npy in both) under %s" % (a if not ja else b))
  only = sorted(set(ja) ^ set(jb))
  if only:
    raise SystemExit("compare_frames: %s is in only one of the two %s" % (", ".join("%d.jpg" % i for i in only[:8]) if not any(avi) else
                                                                         "frame " + ", ".join("%d" % i for i in only[:8]),
                                                                         "directories" if not any(avi) else "clips"))
  idx = sorted(ja)
  return "jpg", idx, [ja[i] for i in idx], [jb[i] for i in idx]


class DeviceFrames:
  """load(paths) -> list of device uint8 [H, W, 3] tensors, decoded on the device where the decoder takes the file"""

  def __init__(self):
    self.dec = None

  def load(self, paths):
    import torch
    from PIL import Image
    from voicepuppet_amd import jpeg_dec as jd
    if isinstance(paths[0], tuple):                 # frames of an .avi side: (AviReader, index), a run of consecutive indices
      reader, first = paths[0]
      return list(reader.read(first, len(paths)))
    datas = []
    for p in paths:
      with open(p, "rb") as f:
        datas.append(f.read())
    infos = [jd.parse(d) for d in datas]
    sizes = [(i.height, i.width) for i in infos if not i.refused]
    H, W = (max(s[0] for s in sizes), max(s[1] for s in sizes)) if sizes else (16, 16)
    nbytes = max(len(d) for d in datas)
    if self.dec is None or self.dec.max_height < H or self.dec.max_width < W or self.dec.max_files < len(paths) or self.max_bytes < nbytes:
      self.dec = jd.JpegDecoder(max(len(paths), CHUNK), H, W, bgr=False, max_file_bytes=max(nbytes, 1 << 22))
      self.max_bytes = max(nbytes, 1 << 22)
    dec = self.dec
    out = torch.zeros(len(paths), dec.max_height, dec.max_width, 3, dtype=torch.uint8, device="cuda")
    status = torch.zeros(len(paths), dtype=torch.int32, device="cuda")
    items = [None if i.refused else (d, i, None, None, p) for d, i, p in zip(datas, infos, paths)]
    if any(it is not None for it in items):
      dec.decode_into(items, out, out.stride(1), out.stride(0), status, raise_bad=False)
    bad = status.cpu().numpy() != 0
    frames = []
    for k, (info, p) in enumerate(zip(infos, paths)):
      if info.refused or bad[k]:                    # outside the device decoder's subset, or corrupt for it: libjpeg's decode, uploaded
        frames.append(torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy()).cuda())
      else:
        frames.append(out[k, :info.height, :info.width])
    return frames


class DeviceCompare:
  """compare(a, b, value_range=...) for stacked device tensors -> host float64 [n, 4]"""

  def __init__(self):
    self.fm = None

  def __call__(self, a, b, value_range=(0, 255)):
    import torch
    from voicepuppet_amd.metrics import FrameMetrics
    a, b = (torch.as_tensor(x).cuda() for x in (a, b))
    n, H, W = a.shape[:3]
    if self.fm is None or self.fm.max_frames < n or self.fm.max_height < H or self.fm.max_width < W:
      self.fm = FrameMetrics(max(n, CHUNK), H, W)
    return self.fm.compare(a, b, value_range=value_range).cpu().numpy()


def summarise(rows):
  rows = np.asarray(rows, np.float64)
  s = {"frames": int(len(rows))}
  for j, k in enumerate(COLUMNS):
    col = rows[:, j]
    worst = int(np.argmin(col) if k in ("PSNR", "SSIM") else np.argmax(col))
    s[k] = {"mean": float(col.mean()), "min": float(col.min()), "max": float(col.max()), "worst": worst}
  return s


def _stack(frames):
  if isinstance(frames[0], np.ndarray):
    return np.stack(frames)
  import torch
  return torch.stack(frames)


def main(argv=None, load=None, compare=None):
  """load / compare: stand-ins for the device halves (tests without a GPU); None: the device."""
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("a", metavar="A", help="a directory of <i>.jpg, a Motion-JPEG .avi file, or a bench.py --dump-outputs directory")
  ap.add_argument("b", metavar="B", help="the directory to compare it with: the same indices and sizes")
  ap.add_argument("--out", metavar="FILE", default=None, help="write the per-frame numbers and the summary as JSON")
  args = ap.parse_args(argv)
  kind, idx, pa, pb = pair_up(args.a, args.b)
  compare = compare or DeviceCompare()
  rows = []
  if kind == "npy":
    xa, xb = np.load(pa), np.load(pb)
    if xa.shape != xb.shape or xa.ndim != 4 or xa.shape[3] != 3 or xa.dtype != np.float32 or xb.dtype != np.float32:
      raise SystemExit("compare_frames: Outputs.npy must be float32 [N, H, W, 3] of one shape in both directories: %s %s against %s %s "
                       "(a dump over bench.py's size cap is a flat sample and cannot be compared as frames)"
                       % (xa.dtype, xa.shape, xb.dtype, xb.shape))
    idx = list(range(len(xa)))
    for i0 in range(0, len(xa), CHUNK):
      rows += np.asarray(compare(xa[i0:i0 + CHUNK], xb[i0:i0 + CHUNK], value_range=(0, 1))).tolist()
  else:
    load = load or DeviceFrames().load
    for i0 in range(0, len(idx), CHUNK):
      fa, fb = load(pa[i0:i0 + CHUNK]), load(pb[i0:i0 + CHUNK])
      for k, (x, y) in enumerate(zip(fa, fb)):
        if tuple(x.shape) != tuple(y.shape):
          raise SystemExit("compare_frames: frame %d is %s in %s and %s in %s" % (idx[i0 + k], tuple(x.shape), args.a, tuple(y.shape), args.b))
      at = 0
      while at < len(fa):                           # runs of one size go to the device together
        end = at
        while end < len(fa) and tuple(fa[end].shape) == tuple(fa[at].shape):
          end += 1
        rows += np.asarray(compare(_stack(fa[at:end]), _stack(fb[at:end]))).tolist()
        at = end
  frames = [dict({"index": int(i)}, **{k: float(v) for k, v in zip(COLUMNS, r)}) for i, r in zip(idx, rows)]
  for f in frames:
    print("frame %6d  L1 %9.5f  MSE %11.5f  PSNR %8.4f dB  SSIM %.6f" % (f["index"], f["L1"], f["MSE"], f["PSNR"], f["SSIM"]))
  s = summarise(rows)
  for k in COLUMNS:
    print("%-4s mean %.6f  min %.6f  max %.6f  worst frame %d" % (k, s[k]["mean"], s[k]["min"], s[k]["max"], idx[s[k]["worst"]]))
  for k in COLUMNS:
    s[k]["worst"] = int(idx[s[k]["worst"]])
  res = {"a": args.a, "b": args.b, "kind": kind, "frames": frames, "summary": s}
  if args.out:
    with open(args.out, "w") as f:
      json.dump(res, f, indent=1)
  return res


if __name__ == "__main__":
  main()

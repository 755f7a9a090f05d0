"""Decode rate of the device JPEG decoder (voicepuppet_amd.jpeg_dec.JpegDecoder) against the host expression it replaces: one JSON line
into profiles/jpeg_decode.json.  Needs an MI355X; no fallback.

  (a) 64 triptychs of 256 x 768 at quality 95, four forms alternating in one process, medians after warm-up: no restart markers and no
      index (one lane per file), the same files at first sight through a decoder with the index scan (scan_chunk_bytes=--scan_chunk: the
      scan kernel, then one lane per MCU row), the same files from their index (one lane per MCU row), and their restart_marker_rows=1
      re-saves (one lane per interval).  Three figures per form, each its own: host_parse_ms (reading nothing: jpeg_dec.parse of the 64 byte strings
      on one thread), host_pack_ms (JpegDecoder.pack: meta blobs, the per-file table, the copy into the pinned staging buffer) and
      device_ms (events around JpegDecoder.enqueue alone, parsed and packed before the first event: the H2D copy of the blob, the three
      kernels per 32 files, the copies of status and entries back).
      Content: 32 x 32 blocks of a random flat colour (smooth blocks) plus uniform noise of +-12 per channel, seeded per file.
  (b) host wall time per file of np.asarray(Image.open(path).convert("RGB"))[..., ::-1] copied, the decode expression of
      PixReferDataGenerator._frame_samples, on 1 thread and on a pool of 16.
  (c) sustained frames/s at batch 32, 256 x 256 on a folder of 3200 such files (hard links of the 64), flag off (PIL on the pool, the
      parent's behaviour), flag on in the first epoch (one lane per file) and flag on once files run from their index, the synthetic pool
      beside them: of the dataset iterator alone (PixReferDataGenerator.get_device_dataset, nothing consuming the batches but a stream
      wait), and of the train_pixrefer.py loop, each variant a child process, from the launcher's own log (its cumulative frames/s
      every 50 iterations, differenced into per-interval rates; an epoch is 100 iterations).
  --scan_out PATH merges the scan's figures (device_ms of one-lane, scan and indexed of this run and their ratios, the rounds, the
  first-epoch iterator rate with and without the scan) into PATH's "measured" key (profiles/jpeg_scan.json); --only picks the parts
  (iterator_scan: one more first epoch of the iterator, through the index scan).
"""
import argparse
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def triptych(seed, S=256):
  rng = np.random.default_rng(seed)
  flat = rng.integers(0, 256, (S // 32, 3 * S // 32, 3)).repeat(32, 0).repeat(32, 1)
  return (flat + rng.integers(-12, 13, (S, 3 * S, 3))).clip(0, 255).astype(np.uint8)


FOLDER_FILES = 3200


def make_folder(tmp, paths):
  folder = os.path.join(tmp, "clip")
  os.makedirs(folder)
  for i in range(FOLDER_FILES):
    dst = os.path.join(folder, "%d.jpg" % i)
    try:
      os.link(paths[i % len(paths)], dst)
    except OSError:
      shutil.copy(paths[i % len(paths)], dst)
  with open(os.path.join(tmp, "train.txt"), "w") as f:
    f.write("%s|%d\n" % (folder, FOLDER_FILES))


def loop_rates(tmp, N=32, S=256):
  """train_pixrefer.py as a child process per variant -> frames/s per 50-iteration interval from its own log"""
  cfg = open(os.path.join(ROOT, "config", "params.yml")).read()

  def run(name, dataset, flag, steps):
    work = os.path.join(tmp, "run_" + name)
    os.makedirs(work)
    with open(os.path.join(work, "params.yml"), "w") as f:
      f.write(cfg.replace("train_dataset_path: config/train.txt", "train_dataset_path: " + dataset))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "voicepuppet_amd.pixrefer.train_pixrefer", "--config_path", "params.yml", "--steps", str(steps),
           "--batch_size", str(N), "--img_size", str(S)] + (["--device_jpeg_decode"] if flag else [])
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
      raise RuntimeError("train_pixrefer.py (%s) failed: %s" % (name, (r.stdout + r.stderr)[-2000:]))
    cum = [float(x) for x in re.findall(r"([0-9.]+) frames/s", r.stdout + r.stderr)]
    t = [50 * (k + 1) * N / c for k, c in enumerate(cum)]
    return [50 * N / (t[k] - (t[k - 1] if k else 0.0)) for k in range(len(t))]
  lst = os.path.join(tmp, "train.txt")
  off = run("off", lst, False, 300)
  on = run("on", lst, True, 400)
  syn = run("synthetic", os.path.join(tmp, "absent.txt"), False, 300)
  return {"flag_off_pil": float(np.median(off[2:])), "flag_on_first_epoch_iterations_51_100": on[1],
          "flag_on_indexed_iterations_151_on": float(np.median(on[3:])), "synthetic_pool": float(np.median(syn[2:])),
          "intervals": {"flag_off": off, "flag_on": on, "synthetic": syn}, "batch": N, "img_size": S, "files": FOLDER_FILES}


def iterator_rates(tmp, paths, N=32, S=256, scan_chunk=128, plain=True, scan=True):
  import torch
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  lst, count = os.path.join(tmp, "train.txt"), FOLDER_FILES
  def run(dataset_path, on, spans, scan=0):
    g = PixReferDataGenerator(os.path.join(ROOT, "config", "params.yml"))
    p = g.params
    p.dataset_path, p.batch_size, p.img_size = dataset_path, N, S
    amd = dict(p.get("amd") or {})
    amd["device_jpeg_decode"], amd["device_jpeg_scan"] = on, scan
    p.amd = amd
    g.set_params(p)
    it = g.get_device_dataset().make_one_shot_iterator()
    rates, k = [], 0
    for skip, batches in spans:
      for _ in range(skip):
        it.next_batch()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(batches):
        it.next_batch()
      torch.cuda.synchronize()
      rates.append(N * batches / (time.perf_counter() - t0))
    return rates, (list(it._pf.segments_used[:2]) if on else None)
  epoch = count // N
  res = {"batch": N, "img_size": S, "files": count}
  if plain:
    off, _ = run(lst, False, [(4, 40)])
    on, segs = run(lst, True, [(4, epoch - 8), (epoch + 8, 40)])
    syn, _ = run(os.path.join(tmp, "absent.txt"), False, [(4, 40)])
    res.update({"flag_off_pil": off[0], "flag_on_first_epoch": on[0], "flag_on_indexed": on[1], "flag_on_indexed_segments_per_file": segs,
                "synthetic_pool": syn[0]})
  if scan:
    rates, scan_segs = run(lst, True, [(4, epoch - 8)], scan_chunk)
    res.update({"flag_on_scan_first_epoch": rates[0], "flag_on_scan_first_epoch_segments_per_file": scan_segs, "scan_chunk_bytes": scan_chunk})
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--files", type=int, default=64)
  ap.add_argument("--repeats", type=int, default=30)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.json"))
  ap.add_argument("--scan_chunk", type=int, default=128)
  ap.add_argument("--scan_out", default=None)
  ap.add_argument("--only", default="decode,host,iterator,iterator_scan,loop",
                  help="comma list of: decode (always), host, iterator, iterator_scan, loop")
  a = ap.parse_args()
  import torch
  from PIL import Image
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  if not torch.cuda.is_available():
    raise SystemExit("jpeg_decode_rate.py needs a GPU")

  def save(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=95, **kw)
    return b.getvalue()
  imgs = [triptych(i) for i in range(a.files)]
  plain, marked = [save(i) for i in imgs], [save(i, restart_marker_rows=1) for i in imgs]
  dec = JpegDecoder(a.files, 256, 768, bgr=True)
  out = torch.empty(a.files, 256, 768, 3, dtype=torch.uint8, device="cuda")
  _, st = dec.decode(plain, out=out)
  want = out.cpu().numpy().copy()
  assert st.cpu().tolist() == [0] * a.files
  index = [e.cpu().numpy().copy() for e in dec.tensor("entries")[:a.files, :16]]
  dec_scan = JpegDecoder(a.files, 256, 768, bgr=True, scan_chunk_bytes=a.scan_chunk)      # byte strings have no key: always first sight
  forms = {"one_lane_per_file": (plain, None), "scan": (plain, None), "indexed": (plain, index), "restart_markers": (marked, None)}
  base, scan_rounds = dec, None
  times = {k: {"device": [], "parse": [], "pack": []} for k in forms}
  segs = {}
  status = torch.empty(a.files, dtype=torch.int32, device="cuda")
  for r in range(a.warmup + a.repeats):
    for name, (files, idx) in forms.items():          # alternating
      dec = dec_scan if name == "scan" else base
      t0 = time.perf_counter()
      items = dec.items(files, idx)                   # host: parse the headers
      t1 = time.perf_counter()
      packed = dec.pack(items)                        # host: metas, table, the pinned staging buffer
      t2 = time.perf_counter()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record()
      dec.enqueue(packed, out, out.stride(1), out.stride(0), status, raise_bad=False)
      e1.record()
      torch.cuda.synchronize()
      if r >= a.warmup:
        times[name]["device"].append(e0.elapsed_time(e1))
        times[name]["parse"].append((t1 - t0) * 1e3)
        times[name]["pack"].append((t2 - t1) * 1e3)
      elif r == 0:
        assert status.cpu().tolist() == [0] * a.files
        segs[name] = dec.last_segments[0]
        if name == "scan":
          assert dec.tensor("scan_ok")[:a.files].cpu().tolist() == [1] * a.files
          scan_rounds = dec.tensor("scan_rounds")[:a.files].cpu().tolist()
        if files is plain:
          assert np.array_equal(out.cpu().numpy(), want)
  res = {"metric": "jpeg_decode", "device": torch.cuda.get_device_name(0), "files": a.files, "shape": [256, 768, 3], "quality": 95,
         "mean_file_bytes": float(np.mean([len(f) for f in plain])), "raw_bytes_per_file": 256 * 768 * 3,
         "decode": {k: {"segments_per_file": segs[k], "device_ms_median": float(np.median(v["device"])),
                        "device_ms_p90": float(np.percentile(v["device"], 90)), "host_parse_ms_median": float(np.median(v["parse"])),
                        "host_pack_ms_median": float(np.median(v["pack"])),
                        "files_per_second_device": a.files / (float(np.median(v["device"])) * 1e-3)} for k, v in times.items()},
         "note": "device_ms: events around JpegDecoder.enqueue alone (H2D copy of the blob, kernels, status / entries copies back); "
                 "parse and pack are host wall time on one thread, outside the events"}

  dec = base
  med = {k: res["decode"][k]["device_ms_median"] for k in res["decode"]}
  res["scan"] = {"chunk_bytes": a.scan_chunk, "max_rounds": dec_scan.scan_max_rounds, "rounds_per_file_max": max(scan_rounds), "rounds_per_file_median": float(np.median(scan_rounds)),
                 "device_ms_scan_over_one_lane": med["scan"] / med["one_lane_per_file"], "device_ms_scan_over_indexed": med["scan"] / med["indexed"]}
  only = set(a.only.split(","))
  tmp = tempfile.mkdtemp(prefix="jpeg_decode_rate_")
  paths = []
  for i, f in enumerate(plain):
    paths.append(os.path.join(tmp, "%d.jpg" % i))
    with open(paths[-1], "wb") as fh:
      fh.write(f)

  def host(p):
    return np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[..., ::-1])
  if "host" in only:
    one, pool = [], []
    with ThreadPoolExecutor(16) as ex:
      for r in range(3 + 10):
        t0 = time.perf_counter()
        for p in paths:
          host(p)
        t1 = time.perf_counter()
        list(ex.map(host, paths))
        t2 = time.perf_counter()
        if r >= 3:
          one.append((t1 - t0) / len(paths) * 1e3)
          pool.append((t2 - t1) / len(paths) * 1e3)
    res["host_pil"] = {"one_thread_ms_per_file": float(np.median(one)), "pool16_wall_ms_per_file": float(np.median(pool))}
  make_folder(tmp, paths)
  if only & {"iterator", "iterator_scan"}:
    res["iterator_frames_per_second"] = iterator_rates(tmp, paths, scan_chunk=a.scan_chunk, plain="iterator" in only, scan="iterator_scan" in only)
  del dec, base, dec_scan, out
  torch.cuda.empty_cache()
  if "loop" in only:
    res["train_loop_frames_per_second"] = loop_rates(tmp)
  shutil.rmtree(tmp)
  line = json.dumps(res)
  print(line)
  with open(a.out, "w") as f:
    f.write(line + "\n")
  if a.scan_out:
    rec = json.load(open(a.scan_out)) if os.path.exists(a.scan_out) else {}
    it = res.get("iterator_frames_per_second", {})
    rec.pop("note", None)
    rec["measured"] = {"device": res["device"], "files": a.files, "shape": [256, 768, 3], "quality": 95, "mean_file_bytes": res["mean_file_bytes"],
                       "repeats": a.repeats, "warmup": a.warmup, "device_ms_median": med, "segments_per_file": segs, "scan": res["scan"],
                       "iterator_first_epoch_frames_per_second": {"scan": it.get("flag_on_scan_first_epoch"), "one_lane": it.get("flag_on_first_epoch"),
                                                                  "indexed": it.get("flag_on_indexed"), "pil": it.get("flag_off_pil")}}
    with open(a.scan_out, "w") as f:
      f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
  main()

"""Frame-side latency of stream groups (voicepuppet_amd.stream.PuppetStreamGroup) on one GPU: prints one JSON line.

For S = 1, 4, 16, 64 slots, frame_batch 8 and 32, f32 and bf16 audio trunks, 1-frame chunks: every slot receives 640 samples per group
push, so every steady push emits one frame per slot.  Per push, after warm-up (medians of --pushes pushes):
  device_ms   HIP-event span of the push on the caller's stream (the host is synchronised before each push: the span is the push alone)
  enqueue_ms  host wall time of the push call (no device wait inside it)
Beside each, in the same process, S independent single-talker pushes in the style of PuppetStream before stream groups (`ParentStyle`
below: an AudioStream each, coeff.cpu() for the host splice, render_faces with its host-built tables and stream wait, framework
pointwise conditioning, Session.run and a host copy of the frames): their device span and wall time for one round of all S.  Group and
singles alternate push by push, so both see the same device state; `spread` is the relative difference between the medians of the even
and the odd measured pushes of one series, the run-to-run spread to judge the S = 1 comparison by.
realtime_talkers = S x 40 ms / device_ms.  Synthetic face model, photos and weights as in tests/test_gpu_puppet_group.py.
Usage: python scripts/puppet_group_latency.py [--pushes 100] [--warmup 10] [--slots 1,4,16,64] [--out profiles/puppet_group_latency.json]
Every GPU step of a longer job runs under its own limit and the steps are chained, e.g.
  timeout -k 10 900 python scripts/puppet_group_latency.py --slots 1,4 --out a.json && timeout -k 10 900 python scripts/puppet_group_latency.py --slots 16,64 --out b.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = os.path.join(ROOT, "config", "params.yml")
H = 512


def assets(S):
  from PIL import Image
  from scipy.io import savemat
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.pixrefer import infer_bfmvid as ib
  os.chdir(tempfile.mkdtemp())
  fm = br.synthetic_facemodel(3)
  os.makedirs("BFM")
  savemat(os.path.join("BFM", "BFM_model_front.mat"),
          {"meanshape": fm.meanshape, "idBase": fm.idBase, "exBase": fm.exBase, "meantex": fm.meantex, "texBase": fm.texBase,
           "point_buf": fm.point_buf, "tri": fm.tri, "keypoints": (fm.keypoints + 1).reshape(1, -1)})
  os.makedirs("ckpt_bfmnet")
  np.savez(ib.BFMNET_CKPT + ".npz", **random_variables(seed=11))
  os.makedirs("background")
  rng = np.random.default_rng(1)
  for i in range(1, 101):
    Image.fromarray((rng.uniform(size=(H, H, 3)) * 255).astype(np.uint8)).save(os.path.join("background", "%d.jpg" % i))
  photos = []
  for s in range(S):
    coeff, _ = br.synthetic_coeffs(1, 5 + s)
    photos.append({"bfmcoeff": coeff.reshape(1, 257), "transform_params": np.array([512, 512, 1.0, 0.0, 0.0], np.float32),
                   "center_x": 256, "center_y": 256, "ratio": 0.9})
  image = rng.uniform(size=(H, 3 * H, 3)).astype(np.float32)
  return image, photos


class ParentStyle:
  """One talker as PuppetStream ran it before stream groups (the comparison): see the module docstring."""

  def __init__(self, image, photo, nb, dtype):
    import torch
    from voicepuppet_amd.pixrefer import infer_bfmvid as ib
    from voicepuppet_amd.runtime import Session
    from voicepuppet_amd.stream import AudioStream, HeadSway, load_bfmnet_params
    self.ib, self.nb, self.photo = ib, nb, photo
    self.audio = AudioStream(load_bfmnet_params(ib.BFMNET_CKPT + ".npz"), max_chunk_frames=1, dtype=dtype)
    self.net, self.inputs_holder, self.fg_holder, self.targets_holder, self.nodes = ib.load_generator(CFG, nb, H)
    self.sess, self.renderer = Session(), ib.clip_renderer()
    self.inputs = torch.zeros([nb, H, H, 6], dtype=torch.float32, device="cuda")
    self.fg_inputs = torch.zeros([nb, H, H, 3], dtype=torch.float32, device="cuda")
    self.targets = torch.full([nb, H, H, 3], 0.5, dtype=torch.float32, device="cuda")
    self.inputs[:, ..., 0:3] = torch.as_tensor(np.ascontiguousarray(image[:, H:2 * H], dtype=np.float32)).to("cuda")
    self.fg_inputs[:, ..., 0:3] = torch.as_tensor(np.ascontiguousarray(image[:, :H] * image[:, 2 * H:], dtype=np.float32)).to("cuda")
    self.sway, self.frame = HeadSway(), 0

  def push(self, pcm, ears):
    import torch
    ib, p = self.ib, self.photo
    coeff = self.audio.push(pcm, ears=ears)
    k = int(coeff.shape[0])
    if k == 0:
      return 0
    g0 = self.frame
    self.frame += k
    angles = self.sway.next(k)
    seq = ib.splice_coeff(p['bfmcoeff'].reshape(1, 257), coeff.cpu().numpy()[np.newaxis])[0]
    face3d = ib.render_faces(self.renderer, int(p['center_x']), int(p['center_y']), float(p['ratio']), seq, (H, H, 3), p['transform_params'],
                             on_device=True, angles=angles)
    for i0 in range(0, k, self.nb):
      idx = [min(i0 + j, k - 1) for j in range(self.nb)]
      self.inputs[:, ..., 3:6] = face3d[idx].flip(-1).to(torch.float32) / 255.0
      for j, i in enumerate(idx):
        bg = ib.background_target(g0 + i, H)
        if bg is not None:
          self.targets[j] = torch.as_tensor(bg).to("cuda")
        else:
          self.targets[j] = 0.5
      self.sess.run([self.nodes['Outputs_u8']], feed_dict={self.inputs_holder: self.inputs, self.fg_holder: self.fg_inputs, self.targets_holder: self.targets})
    return k


def _stats(v):
  v = np.array(v)
  even, odd = np.median(v[0::2]), np.median(v[1::2])
  return {"median": float(np.median(v)), "p90": float(np.percentile(v, 90)), "spread": float(abs(even - odd) / max(np.median(v), 1e-9))}


def measure(S, nb, dtype, pushes, warmup, singles, image, photos):
  import torch
  from voicepuppet_amd.stream import PuppetStreamGroup
  g = PuppetStreamGroup(CFG, S, frame_batch=nb, max_chunk_frames=1, dtype=dtype)
  for s in range(S):
    g.attach(s, image, photos[s])
  par = [ParentStyle(image, photos[s], nb, dtype) for s in range(S)] if singles else []
  rng = np.random.default_rng(0)
  total = pushes + warmup + 40
  pcm = (0.3 * rng.standard_normal((total, S, 640))).astype(np.float32)
  one = np.full((1, 1), 0.005, np.float32)
  st = torch.cuda.current_stream()
  series = {"g_dev": [], "g_enq": [], "p_dev": [], "p_wall": []}
  for i in range(total):
    if len(series["g_dev"]) >= pushes:
      break
    k = g.audio.ready({s: 640 for s in range(S)})
    ears = {s: np.full((k[s], 1), 0.005, np.float32) for s in range(S) if k[s]}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    t = time.perf_counter()
    g.push({s: pcm[i, s] for s in range(S)}, ears=ears)
    t = time.perf_counter() - t
    e1.record(st)
    e1.synchronize()
    p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    p0.record(st)
    tp = time.perf_counter()
    for s, ps in enumerate(par):
      ps.push(pcm[i, s], ears.get(s, one[:0]))
    tp = time.perf_counter() - tp
    p1.record(st)
    p1.synchronize()
    if list(k) != [1] * S:
      continue                                         # (the first pushes fill the lookahead, one catches up)
    if warmup > 0:
      warmup -= 1
      continue
    series["g_dev"].append(e0.elapsed_time(e1))
    series["g_enq"].append(1000.0 * t)
    series["p_dev"].append(p0.elapsed_time(p1))
    series["p_wall"].append(1000.0 * tp)
  if len(series["g_dev"]) < pushes:
    raise RuntimeError("ran out of audio")
  gd, ge = _stats(series["g_dev"]), _stats(series["g_enq"])
  row = {"slots": S, "frame_batch": nb, "trunk": dtype, "pushes": pushes,
         "group": {"device_ms_median": gd["median"], "device_ms_p90": gd["p90"], "device_ms_spread": gd["spread"],
                   "enqueue_ms_median": ge["median"], "enqueue_ms_p90": ge["p90"], "realtime_talkers": S * 40.0 / gd["median"]}}
  if par:
    pd, pw = _stats(series["p_dev"]), _stats(series["p_wall"])
    row["singles"] = {"device_ms_median": pd["median"], "device_ms_p90": pd["p90"], "device_ms_spread": pd["spread"],
                      "wall_ms_median": pw["median"], "realtime_talkers": S * 40.0 / pd["median"]}
    row["group_over_singles_device"] = gd["median"] / pd["median"]
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pushes", type=int, default=100)
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--slots", default="1,4,16,64")
  ap.add_argument("--frame_batch", default="8,32")
  ap.add_argument("--trunks", default="f32,bf16")
  ap.add_argument("--no_singles", action="store_true", help="measure the group alone")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import torch
  out = os.path.abspath(a.out) if a.out else None
  slots = [int(x) for x in a.slots.split(",")]
  image, photos = assets(max(slots))
  rows = []
  for d in a.trunks.split(","):
    for nb in [int(x) for x in a.frame_batch.split(",")]:
      for S in slots:
        rows.append(measure(S, nb, d, a.pushes, a.warmup, not a.no_singles, image, photos))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
  line = json.dumps({"metric": "puppet_group_push_latency", "device": torch.cuda.get_device_name(0), "runs": rows})
  print(line)
  if out:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()

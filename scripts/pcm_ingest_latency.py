"""What the stream ingest (voicepuppet_amd.pcm.PcmIngest, csrc/pcm_in.hip) costs on one GPU: prints one JSON line.

Part 1, the push it sits in front of: a 64-slot PuppetStreamGroup (frame_batch 32, 1-frame chunks, f32 and bf16 audio trunks), one and the
same group fed alternately, push by push and in one process,
  plain   16 kHz float32, 640 samples per slot (PuppetStreamGroup.push, the path before the ingest existed)
  ingest  48 kHz stereo int16, 1920 frames per slot (PuppetStreamGroup.push_raw: ingest, then the same push)
Both advance every slot by 40 ms, so every steady push of either kind emits one frame per slot.  Per push, after warm-up (medians of
--pushes pushes of each kind): device_ms, the HIP-event span of the push on the caller's stream (the host is synchronised before each
push), and enqueue_ms, the host wall time of the call.  `spread` is the relative difference between the medians of the even and the odd
measured pushes of one series.
Part 2, the ingest launch alone (PcmIngest.push from a device tensor, so no copy is in the span): 1, 8 and 64 slots pushing 40 ms of
48 kHz stereo int16 each, one slot pushing a 10 s clip of it, and the same for 44.1 kHz (160 phases).
Synthetic face model, photos and weights as in scripts/puppet_group_latency.py.
Usage: python scripts/pcm_ingest_latency.py [--pushes 60] [--warmup 10] [--slots 64] [--out profiles/pcm_ingest.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CFG = os.path.join(ROOT, "config", "params.yml")


def _stats(v):
  v = np.array(v)
  even, odd = np.median(v[0::2]), np.median(v[1::2])
  return {"median": float(np.median(v)), "p90": float(np.percentile(v, 90)), "spread": float(abs(even - odd) / max(np.median(v), 1e-9))}


def _timed(fn):
  import torch
  st = torch.cuda.current_stream()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record(st)
  t = time.perf_counter()
  fn()
  t = time.perf_counter() - t
  e1.record(st)
  e1.synchronize()
  return e0.elapsed_time(e1), 1000.0 * t


def group_push(S, nb, dtype, pushes, warmup, image, photos):
  from voicepuppet_amd.stream import PuppetStreamGroup
  g = PuppetStreamGroup(CFG, S, frame_batch=nb, max_chunk_frames=1, dtype=dtype, ingest_rates=(48000,))
  for s in range(S):
    g.attach(s, image, photos[s], 48000, 2, "s16")
  rng = np.random.default_rng(0)
  series = {"plain_dev": [], "plain_enq": [], "ingest_dev": [], "ingest_enq": []}
  i = 0
  while len(series["ingest_dev"]) < pushes:
    i += 1
    if i > 2 * pushes + 2 * warmup + 200:
      raise RuntimeError("the pushes never became steady")
    for kind in ("plain", "ingest"):
      if kind == "plain":
        n = {s: 640 for s in range(S)}
        chunk = {s: (0.3 * rng.standard_normal(640)).astype(np.float32) for s in range(S)}
      else:
        n = dict(enumerate(g.ingest.ready({s: 1920 for s in range(S)})))
        chunk = {s: (0.3 * 32767 * rng.standard_normal((1920, 2))).clip(-32768, 32767).astype(np.int16) for s in range(S)}
      k = g.audio.ready(n)
      ears = {s: np.full((k[s], 1), 0.005, np.float32) for s in range(S) if k[s]}
      dev, enq = _timed(lambda: (g.push if kind == "plain" else g.push_raw)(chunk, ears=ears))
      if list(k) != [1] * S or i <= warmup:
        continue                                         # (the first pushes fill the lookahead)
      series[kind + "_dev"].append(dev)
      series[kind + "_enq"].append(enq)
  row = {"slots": S, "frame_batch": nb, "trunk": dtype, "pushes": pushes}
  for kind in ("plain", "ingest"):
    d, e = _stats(series[kind + "_dev"][:pushes]), _stats(series[kind + "_enq"][:pushes])
    row[kind] = {"device_ms_median": d["median"], "device_ms_p90": d["p90"], "device_ms_spread": d["spread"], "enqueue_ms_median": e["median"]}
  row["ingest_over_plain_device"] = row["ingest"]["device_ms_median"] / row["plain"]["device_ms_median"]
  row["ingest_minus_plain_device_ms"] = row["ingest"]["device_ms_median"] - row["plain"]["device_ms_median"]
  return row


def ingest_alone(rate, S, frames, pushes, warmup):
  import torch
  from voicepuppet_amd.pcm import PcmIngest
  ing = PcmIngest(S, rates=(rate,), max_in_frames=max(frames, 1 << 16))
  for s in range(S):
    ing.open_slot(s, rate, 2, "s16")
  rng = np.random.default_rng(1)
  raw = {s: torch.from_numpy((0.3 * 32767 * rng.standard_normal((frames, 2))).clip(-32768, 32767).astype(np.int16)).to("cuda") for s in range(S)}
  dev, enq = [], []
  for i in range(pushes + warmup):
    d, e = _timed(lambda: ing.push(raw))
    if i >= warmup:
      dev.append(d)
      enq.append(e)
  d, e = _stats(dev), _stats(enq)
  # the span includes the packing copies of the wrapper's device path (one per slot); launch_ms is the C call alone, packed input
  import ctypes
  from voicepuppet_amd import _lib
  from voicepuppet_amd._handle import slot_arrays
  packed = torch.zeros(S * ((frames * 4 + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
  n, fin = slot_arrays(S, {s: frames for s in range(S)}, ())
  out = torch.empty(sum(ing.ready({s: frames for s in range(S)})), dtype=torch.float32, device="cuda")
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  launch = []
  for i in range(pushes + warmup):
    t, _ = _timed(lambda: _lib.check(ing.L.vp_pcmin_push(ing.h, ctypes.c_void_p(packed.data_ptr()), n, fin, ctypes.c_void_p(out.data_ptr()), st)))
    if i >= warmup:
      launch.append(t)
  return {"rate": rate, "slots": S, "frames_per_slot": frames, "out_samples": int(out.numel()), "device_ms_median": d["median"],
          "device_ms_p90": d["p90"], "enqueue_ms_median": e["median"], "launch_device_ms_median": _stats(launch)["median"],
          "launch_device_ms_p90": _stats(launch)["p90"]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pushes", type=int, default=60)
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--slots", type=int, default=64)
  ap.add_argument("--frame_batch", type=int, default=32)
  ap.add_argument("--trunks", default="f32,bf16")
  ap.add_argument("--no_group", action="store_true", help="part 2 alone")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import torch
  out = os.path.abspath(a.out) if a.out else None
  alone = []
  for rate in (48000, 44100):
    for S, frames in ((1, rate * 40 // 1000), (8, rate * 40 // 1000), (64, rate * 40 // 1000), (1, 10 * rate)):
      alone.append(ingest_alone(rate, S, frames, a.pushes, a.warmup))
      print(json.dumps(alone[-1]), file=sys.stderr, flush=True)
  rows = []
  if not a.no_group:
    import puppet_group_latency as pgl
    image, photos = pgl.assets(a.slots)
    for d in a.trunks.split(","):
      rows.append(group_push(a.slots, a.frame_batch, d, a.pushes, a.warmup, image, photos))
      print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
  line = json.dumps({"metric": "pcm_ingest_latency", "device": torch.cuda.get_device_name(0), "group_push": rows, "ingest_alone": alone})
  print(line)
  if out:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()

"""Streaming-group latency (voicepuppet_amd.stream.AudioStreamGroup) on one GPU: prints one JSON line.

For S = 1, 4, 16, 64 slots, windows of 1 and 5 frames, f32 and bf16 trunks: every slot receives a chunk of exactly that many frames
(640 samples each) per group push, so every push after the first ones emits one window per slot - one round of the shared chain at
batch S.  Per push, after warm-up:
  device_ms   HIP-event span of the push on the stream (the host is synchronised before each push: the span is the push alone)
  enqueue_ms  host wall time of the push call (no device wait inside it)
plus realtime_streams = S x chunk audio ms / device_ms: how many real-time streams of that chunking one GPU sustains at that group size.
Usage: python scripts/stream_group_latency.py [--pushes 100] [--warmup 10] [--slots 1,4,16,64] [--out profiles/stream_group_latency.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(S, chunk, dtype, pushes, warmup):
  import torch
  from oracle import audio_ref
  from voicepuppet_amd import _lib
  from voicepuppet_amd.stream import AudioStreamGroup
  params = {k: v.astype(np.float32) for k, v in audio_ref.init_bfmnet_params(seed=0).items()}
  g = AudioStreamGroup(params, slots=S, max_chunk_frames=chunk, dtype=dtype)
  rng = np.random.default_rng(0)
  n = 640 * chunk
  total = pushes + warmup + 40
  pcm = torch.from_numpy((0.3 * rng.standard_normal(total * S * n)).astype(np.float32)).cuda()     # [push][slot][n]
  ears = torch.full((S * chunk, 1), 0.005, device="cuda")
  out = torch.empty(S * chunk, 64, device="cuda")
  L = g.L
  s = torch.cuda.current_stream()
  sp = ctypes.c_void_p(s.cuda_stream)
  nn = (ctypes.c_longlong * S)(*([n] * S))
  k = (ctypes.c_int * S)()
  dev, enq, i = [], [], 0
  while len(dev) < pushes:
    if i >= total:
      raise RuntimeError("ran out of audio")
    K = L.vp_bfmstream_group_ready(g.h, nn, None, k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    t = time.perf_counter()
    _lib.check(L.vp_bfmstream_group_push(g.h, ctypes.c_void_p(pcm.data_ptr() + 4 * i * S * n), nn, None, ctypes.c_void_p(ears.data_ptr()),
                                         ctypes.c_void_p(out.data_ptr()), sp), "vp_bfmstream_group_push")
    t = time.perf_counter() - t
    e1.record(s)
    e1.synchronize()
    i += 1
    if K != S * chunk:
      continue                                         # (the first pushes fill the lookahead, one catches up)
    if warmup > 0:
      warmup -= 1
      continue
    dev.append(e0.elapsed_time(e1))
    enq.append(1000.0 * t)
  dev, enq = np.array(dev), np.array(enq)
  chunk_ms = 40.0 * chunk
  return {"slots": S, "chunk_frames": chunk, "trunk": dtype, "window_frames": g.window_frames,
          "device_ms_median": float(np.median(dev)), "device_ms_p90": float(np.percentile(dev, 90)),
          "enqueue_ms_median": float(np.median(enq)), "enqueue_ms_p90": float(np.percentile(enq, 90)),
          "device_ms_per_stream": float(np.median(dev) / S),
          "realtime_streams": float(S * chunk_ms / np.median(dev)), "pushes": int(len(dev))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pushes", type=int, default=100)
  ap.add_argument("--warmup", type=int, default=10)
  ap.add_argument("--slots", default="1,4,16,64")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import torch
  rows = []
  for d in ("f32", "bf16"):
    for c in (1, 5):
      for S in [int(x) for x in a.slots.split(",")]:
        rows.append(measure(S, c, d, a.pushes, a.warmup))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
  line = json.dumps({"metric": "stream_group_push_latency", "device": torch.cuda.get_device_name(0), "runs": rows})
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()

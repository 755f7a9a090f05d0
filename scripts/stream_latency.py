"""Streaming inference latency (voicepuppet_amd.stream.AudioStream) on one GPU: prints one JSON line.

For windows of 1 and 5 frames, f32 and bf16 trunks: a 20 s clip is pushed in chunks of exactly that many frames (640 samples each), so
every push after the first emits one window.  Per push, after warm-up:
  device_ms   HIP-event span of the push on the stream (start event before the first launch, end event behind the last; the host is
              synchronised before each push, so the span is the push alone)
  enqueue_ms  host wall time of the push call (no device wait inside it)
plus the recompute factor T_win / chunk, the algorithmic lookahead and the real-time factor device_ms / chunk audio ms.
Usage: python scripts/stream_latency.py [--pushes 200] [--warmup 20] [--out profiles/stream_latency.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(chunk, dtype, pushes, warmup):
  import torch
  from oracle import audio_ref
  from voicepuppet_amd.stream import AudioStream
  params = {k: v.astype(np.float32) for k, v in audio_ref.init_bfmnet_params(seed=0).items()}
  st = AudioStream(params, max_chunk_frames=chunk, dtype=dtype)
  rng = np.random.default_rng(0)
  n = 640 * chunk
  pcm = torch.from_numpy((0.3 * rng.standard_normal(n * (pushes + warmup + 40))).astype(np.float32)).cuda()
  ears = torch.full((chunk, 1), 0.005, device="cuda")
  out = torch.empty(chunk, 64, device="cuda")
  import ctypes
  from voicepuppet_amd import _lib
  L = st.L
  s = torch.cuda.current_stream()
  sp = ctypes.c_void_p(s.cuda_stream)
  dev, enq, at = [], [], 0
  while len(dev) < pushes:
    k = st.ready(n)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    t = time.perf_counter()
    _lib.check(L.vp_bfmstream_push(st.h, ctypes.c_void_p(pcm.data_ptr() + 4 * at), n, ctypes.c_void_p(ears.data_ptr()),
                                   ctypes.c_void_p(out.data_ptr()), sp), "vp_bfmstream_push")
    t = time.perf_counter() - t
    e1.record(s)
    e1.synchronize()
    at += n
    if k != chunk:
      continue                                         # (the first pushes fill the lookahead, one catches up)
    if warmup > 0:
      warmup -= 1
      continue
    dev.append(e0.elapsed_time(e1))
    enq.append(1000.0 * t)
  dev, enq = np.array(dev), np.array(enq)
  chunk_ms = 40.0 * chunk
  return {"chunk_frames": chunk, "trunk": dtype, "window_frames": st.window_frames,
          "recompute_factor": st.window_frames / chunk,
          "device_ms_median": float(np.median(dev)), "device_ms_p90": float(np.percentile(dev, 90)),
          "enqueue_ms_median": float(np.median(enq)), "enqueue_ms_p90": float(np.percentile(enq, 90)),
          "real_time_factor": float(np.median(dev) / chunk_ms),
          "lookahead_ms": st.lookahead_ms, "pushes": int(len(dev))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pushes", type=int, default=200)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import torch
  rows = [measure(c, d, a.pushes, a.warmup) for d in ("f32", "bf16") for c in (1, 5)]
  line = json.dumps({"metric": "stream_push_latency", "device": torch.cuda.get_device_name(0), "runs": rows})
  print(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()

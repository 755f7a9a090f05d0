"""Cost of the device frame metrics (voicepuppet_amd.metrics, libvp_hip.so vp_frame_metrics_*) on one GPU: writes profiles/frame_metrics.json.

  compare   device time of one FrameMetrics.compare (HIP events around its two launches, warm, median of 50) for 1, 8 and 64 pairs of
            512 x 512 frames and 64 pairs of 256 x 256, uint8 and float32, the bytes the call reads
  copy      alternating with it, a plain device-to-device copy of the same bytes (one operand's onto the other's size: read n, write n,
            the bytes compare reads): the HBM yardstick.  ratio_to_copy = compare / copy
No threshold is set: the figures and the ratio are what is recorded.
Usage: python scripts/frame_metrics_latency.py [--out profiles/frame_metrics.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, st, rounds=60, warm=10):
  import torch
  ms = []
  for i in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    if i >= warm:
      ms.append(e0.elapsed_time(e1))
  return ms


def compare_times():
  import torch
  from voicepuppet_amd.metrics import FrameMetrics
  fm = FrameMetrics(64, 512, 512)
  st = torch.cuda.current_stream()
  out = torch.empty(64, 4, dtype=torch.float64, device="cuda")
  rows = []
  for dtype in ("uint8", "float32"):
    for n, size in ((1, 512), (8, 512), (64, 512), (64, 256)):
      g = torch.Generator(device="cuda").manual_seed(n + size)
      if dtype == "uint8":
        a = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, device="cuda", generator=g)
        b = (a.int() + torch.randint(-12, 13, a.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
      else:
        a = torch.rand((n, size, size, 3), device="cuda", generator=g) * 2 - 1
        b = (a + 0.05 * torch.randn(a.shape, device="cuda", generator=g)).clamp(-1, 1)
      dst = torch.empty_like(a)
      cmp_ms, copy_ms = [], []
      for _ in range(5):                           # alternate: both see the same clocks
        cmp_ms += timed(lambda: fm.compare(a, b, out=out), st, rounds=14, warm=4)
        copy_ms += timed(lambda: dst.copy_(a), st, rounds=14, warm=4)
      nbytes = 2 * a.numel() * a.element_size()
      c, y = float(np.median(cmp_ms)), float(np.median(copy_ms))
      rows.append({"dtype": dtype, "pairs": n, "height": size, "width": size, "bytes_read": nbytes, "compare_ms_median": c,
                   "compare_ms_p90": float(np.percentile(cmp_ms, 90)), "copy_ms_median": y, "copy_ms_p90": float(np.percentile(copy_ms, 90)),
                   "ratio_to_copy": c / y, "pairs_per_second": n * 1000.0 / c, "mean_psnr_db": float(out[:n, 2].mean())})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_metrics.json"))
  a = ap.parse_args()
  out = os.path.abspath(a.out)
  import torch
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  rec = {"metric": "frame_metrics", "device": torch.cuda.get_device_name(0), "commit": commit, "timing": "hip events, median of 50 warm calls",
         "compare": compare_times()}
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

"""Cost of the device key matte (voicepuppet_amd.matte, libvp_hip.so vp_keymatte_*) on one GPU: writes profiles/key_matte.json.

  fit     device time of one KeyMatte.fit (HIP events around its fill and four launches, warm, median of 50) for 1, 8 and 64 frames of
          256 x 256 and 512 x 512 of the synthetic studio scene, next to the border bytes it must read (twice: two passes)
  matte   the same for KeyMatte.matte at radius 0, 4 and 16.  bytes_min is what any implementation must move (3 bytes read and 1 written
          per pixel); bytes_moved adds what this one stages in its workspace at radius > 0 (a_k and b_k, float64: 16 bytes written per
          pixel, read back with the tile's halo, and the frame read a second time for the guide); the achieved bytes per second are
          given for both
No threshold is set: the figures are what is recorded.
Usage: python scripts/key_matte_latency.py [--out profiles/key_matte.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE = 32


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


def measure():
  import torch
  import key_matte_ref as kr
  from voicepuppet_amd.matte import KeyMatte, default_band
  st = torch.cuda.current_stream()
  fits, mattes = [], []
  for size in (256, 512):
    one, _ = kr.scene(size, size, seed=size, n=8)
    km = KeyMatte(64, size, size)
    out = torch.empty(64, size, size, dtype=torch.uint8, device="cuda")
    for n in (1, 8, 64):
      frames = torch.from_numpy(np.concatenate([one] * 8)[:n]).cuda()
      ms = timed(lambda: km.fit(frames), st)
      band = default_band(size)
      samples = n * (band * size + (size // 2 - band) * 2 * band)
      rep = km.report()
      t = float(np.median(ms))
      fits.append({"frames": n, "height": size, "width": size, "samples": samples, "bytes_read": 2 * 3 * samples, "fit_ms_median": t,
                   "fit_ms_p90": float(np.percentile(ms, 90)), "kept": rep["kept"], "residual_rms": rep["residual_rms"], "status": rep["status"]})
      for radius in (0, 4, 16):
        ms = timed(lambda: km.matte(frames, radius=radius, out=out), st)
        pixels = n * size * size
        halo = ((TILE + 2 * radius) / float(TILE)) ** 2
        bytes_min = 4 * pixels
        bytes_moved = bytes_min if radius == 0 else int(pixels * (3 * halo + 16 + 16 * halo + 3 + 1))
        t = float(np.median(ms))
        mattes.append({"frames": n, "height": size, "width": size, "radius": radius, "matte_ms_median": t, "matte_ms_p90": float(np.percentile(ms, 90)),
                       "bytes_min": bytes_min, "bytes_moved": bytes_moved, "gb_per_s_of_bytes_min": bytes_min / t / 1e6,
                       "gb_per_s_of_bytes_moved": bytes_moved / t / 1e6, "frames_per_second": n * 1000.0 / t,
                       "foreground_share": float((out[:n] >= 128).float().mean())})
  return fits, mattes


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_matte.json"))
  a = ap.parse_args()
  out = os.path.abspath(a.out)
  import torch
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  fits, mattes = measure()
  rec = {"metric": "key_matte", "device": torch.cuda.get_device_name(0), "commit": commit, "timing": "hip events, median of 50 warm calls",
         "fit": fits, "matte": mattes}
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

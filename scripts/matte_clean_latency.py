"""Cost of the matte clean-up and of the foreground estimate (voicepuppet_amd.matte_clean, voicepuppet_amd.matte; libvp_hip.so
vp_matteclean_*, vp_key_foreground) on one GPU: writes profiles/matte_clean.json.

  clean       device time of one MatteCleaner.clean (HIP events around its fill and launches, warm, median of 50) with the hole pass
              (twelve launches) and without it (max_hole=0: seven) for 1, 8 and 64 frames of 256 x 256 and 512 x 512 of the synthetic
              scene's key matte with its 68 anchors.  bytes_min is what any implementation must move: the matte read, the cleaned matte
              and the int32 labels written, 6 bytes per pixel.  bytes_moved is what this one's launches read and write per pixel, counted
              from the kernels' arguments (neighbour and column reads that hit the cache left out): local 7 (matte, parents, the pair
              records), merge 1 (the tiles' border pixels and their neighbours), gather 10, decide 6, the row pass 9 (parents, records,
              the bit plane), apply 3: 36; the hole pass local 7, merge 1, gather 10, decide 6, fill 9: 33 more
  foreground  the same for KeyMatte.foreground: 3 bytes of frame and 1 of matte read, 3 written per pixel, which is also all it moves
No threshold is set: the figures are what is recorded.
Usage: python scripts/matte_clean_latency.py [--out profiles/matte_clean.json]
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

from key_matte_latency import timed  # noqa: E402

COMPONENT_BYTES, HOLE_BYTES = 36, 33


def measure():
  import torch
  import matte_clean_ref as mr
  from voicepuppet_amd.matte import KeyMatte
  from voicepuppet_amd.matte_clean import MatteCleaner
  st = torch.cuda.current_stream()
  cleans, fores = [], []
  for size in (256, 512):
    one, _, _ = mr.scene(size, size, seed=size, n=8)
    lm = mr.landmarks(size, size, 8)
    km = KeyMatte(64, size, size).fit(torch.from_numpy(one).cuda())
    mc = MatteCleaner(64, size, size)
    out = torch.empty(64, size, size, dtype=torch.uint8, device="cuda")
    fout = torch.empty(64, size, size, 3, dtype=torch.uint8, device="cuda")
    for n in (1, 8, 64):
      frames = torch.from_numpy(np.concatenate([one] * 8)[:n]).cuda()
      anchors = torch.from_numpy(np.concatenate([lm] * 8)[:n]).cuda()
      matte = km.matte(frames).clone()
      pixels = n * size * size
      for holes in (True, False):
        kw = dict(anchors=anchors, out=out, max_hole=None if holes else 0)
        ms = timed(lambda: mc.clean(matte, **kw), st)
        rep = mc.report().astype(np.int64).sum(0)
        t = float(np.median(ms))
        moved = pixels * (COMPONENT_BYTES + (HOLE_BYTES if holes else 0))
        cleans.append({"frames": n, "height": size, "width": size, "hole_pass": holes, "launches": 12 if holes else 7, "clean_ms_median": t,
                       "clean_ms_p90": float(np.percentile(ms, 90)), "bytes_min": 6 * pixels, "bytes_moved": moved,
                       "gb_per_s_of_bytes_min": 6 * pixels / t / 1e6, "gb_per_s_of_bytes_moved": moved / t / 1e6, "frames_per_second": n * 1000.0 / t,
                       "components": int(rep[0]), "kept": int(rep[1]), "pixels_removed": int(rep[2]), "holes_filled": int(rep[4]),
                       "pixels_filled": int(rep[5]), "status_or": int(np.bitwise_or.reduce(mc.report()[:, 6]))})
      cleaned = mc.clean(matte, anchors=anchors).clone()
      for despill in (0.0, 1.0):
        ms = timed(lambda: km.foreground(frames, cleaned, despill=despill, out=fout), st)
        t = float(np.median(ms))
        fores.append({"frames": n, "height": size, "width": size, "despill": despill, "foreground_ms_median": t,
                      "foreground_ms_p90": float(np.percentile(ms, 90)), "bytes_min": 7 * pixels, "gb_per_s_of_bytes_min": 7 * pixels / t / 1e6,
                      "frames_per_second": n * 1000.0 / t})
  return cleans, fores


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matte_clean.json"))
  a = ap.parse_args()
  out = os.path.abspath(a.out)
  import torch
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  cleans, fores = measure()
  rec = {"metric": "matte_clean", "device": torch.cuda.get_device_name(0), "commit": commit, "timing": "hip events, median of 50 warm calls",
         "clean": cleans, "foreground": fores}
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

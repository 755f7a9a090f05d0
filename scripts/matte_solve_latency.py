"""Cost of the trimap and the closed-form matting solve (voicepuppet_amd.matte_solve; libvp_hip.so vp_mattesolve_*) on one GPU: writes
profiles/matte_solve.json.

For 1 and 64 frames of 512 x 512 of the synthetic scene (key, clean, then the trimap with its default squares), at radius 1 and 2, eps 1:
  trimap      device time of one MatteSolver.trimap (HIP events, warm, median of 50)
  iteration   device time of one conjugate-gradient iteration (its two launches): the difference between solves of 24 and of 8 iterations at
              tol = 0, where no frame stops, divided by 16.  bytes_min is what the iteration's launches must move for the tiles that hold
              an unknown pixel, 99 bytes per pixel of such a tile: launch P reads r, 1 / diag, the old p and the frame's three bytes and
              writes p and L p (43); launch U reads x, p, r, L p and 1 / diag and writes x and r (56).  Halo reads, the partial sums and
              the flags are left out
  solve       device time of one whole MatteSolver.solve at tol = 1e-6 with 256 iterations enqueued (2 fills, 514 launches;
              the launches behind a frame's stop return at once), the iterations the frames took, and the solve with exactly as many
              iterations enqueued as the slowest frame took
  active      the share of 32 x 32 tiles that hold an unknown pixel
No threshold is set: the figures are what is recorded.  The A/B of the two forms of the product: the shipped library forms the window
moments again in every iteration; `make -C voicepuppet_amd/csrc one FILE=matte_solve VAR=stored DEFS=-DVP_MS_STORED=1` builds
libvp_stored.so, which keeps them as nine float64 planes, and VP_LIB=.../libvp_stored.so with --out profiles/matte_solve_stored.json
records it ("library" in the record says which one ran).
Usage: python scripts/matte_solve_latency.py [--out profiles/matte_solve.json]
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

ITERATION_BYTES = 99


def measure(size=512):
  import torch
  import matte_clean_ref as mr
  from voicepuppet_amd.matte import KeyMatte
  from voicepuppet_amd.matte_clean import MatteCleaner
  from voicepuppet_amd.matte_solve import MatteSolver
  st = torch.cuda.current_stream()
  one, _, _ = mr.scene(size, size, seed=size, n=8, spill_levels=10.0)
  lm = mr.landmarks(size, size, 8)
  km = KeyMatte(64, size, size).fit(torch.from_numpy(one).cuda())
  mc = MatteCleaner(64, size, size)
  ms = MatteSolver(64, size, size, max_radius=2)
  tri_out = torch.empty(64, size, size, dtype=torch.uint8, device="cuda")
  out = torch.empty(64, size, size, dtype=torch.uint8, device="cuda")
  rows = []
  for n in (1, 64):
    frames = torch.from_numpy(np.concatenate([one] * 8)[:n]).cuda()
    anchors = torch.from_numpy(np.concatenate([lm] * 8)[:n]).cuda()
    cleaned = mc.clean(km.matte(frames), anchors=anchors).clone()
    t_tri = timed(lambda: ms.trimap(cleaned, out=tri_out), st)
    tri = ms.trimap(cleaned, out=tri_out)
    active = float(ms.tensor("tiles")[:n].float().mean().item())
    tiles = n * ((size + 31) // 32) ** 2
    for radius in (1, 2):
      t8 = float(np.median(timed(lambda: ms.solve(frames, tri, radius=radius, iters=8, tol=0.0, out=out), st, rounds=24, warm=4)))
      t24 = float(np.median(timed(lambda: ms.solve(frames, tri, radius=radius, iters=24, tol=0.0, out=out), st, rounds=24, warm=4)))
      t_it = (t24 - t8) / 16.0
      t_full = timed(lambda: ms.solve(frames, tri, radius=radius, iters=256, out=out), st, rounds=14, warm=4)
      rep = ms.report()
      most = int(rep["iterations"].max())
      t_exact = timed(lambda: ms.solve(frames, tri, radius=radius, iters=most, out=out), st, rounds=14, warm=4)
      moved = active * tiles * 1024 * ITERATION_BYTES
      rows.append({"frames": n, "height": size, "width": size, "radius": radius, "eps": 1.0, "tol": 1e-6,
                   "trimap_ms_median": float(np.median(t_tri)), "trimap_ms_p90": float(np.percentile(t_tri, 90)),
                   "active_tile_share": active, "unknown_pixels_mean": float(rep["unknown"].mean()),
                   "iteration_ms": t_it, "solve_8_iterations_ms": t8, "solve_24_iterations_ms": t24,
                   "iteration_bytes_min": moved, "iteration_gb_per_s_of_bytes_min": moved / t_it / 1e6,
                   "solve_ms_median_256_enqueued": float(np.median(t_full)), "solve_ms_p90_256_enqueued": float(np.percentile(t_full, 90)),
                   "iterations_mean": float(rep["iterations"].mean()), "iterations_max": most, "residual_max": float(rep["residual"].max()),
                   "status_or": int(np.bitwise_or.reduce(rep["status"])),
                   "solve_ms_median_iterations_max_enqueued": float(np.median(t_exact)), "frames_per_second": n * 1000.0 / float(np.median(t_full))})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matte_solve.json"))
  a = ap.parse_args()
  out = os.path.abspath(a.out)
  import torch
  from voicepuppet_amd import _lib
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  rec = {"metric": "matte_solve", "device": torch.cuda.get_device_name(0), "commit": commit,
         "timing": "hip events, medians of warm calls (trimap 50, solves 10 to 20)", "library": os.path.basename(_lib.LIB_PATH),
         "solve": measure()}
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

"""Device time of the photometric fit on one GPU (voicepuppet_amd.bfmfit.FaceFitter.observe / fit_appearance): writes
profiles/bfm_appearance.json.

  measured, at 1 / 16 / 128 frames:
    observe        FaceFitter.observe (shape, face normals, per-vertex kernel)
    accumulate     ONE accumulate stage of the chain (vp_bfmfit_appearance with stages = 1, max_trials = 1: the Gram launch and the launch
                   that adds the slabs' partials; includes the 1-block-per-frame initialisation launch in front of them)
    step           ONE step launch with its factorisation: the time of two step launches (stages = 2, max_trials = 2) minus `step_last`
    step_last      the step launch that ends a chain (stages = 2, max_trials = 1: accept / reject and the outputs, no factorisation; same
                   initialisation launch in front)
    fit            a whole fit_appearance from a ready observation (defaults: 32 rounds, finished frames return at once)
    trials_used    the smallest max_trials at which no frame ends with status 1 (found by bisection: nothing is read back by a fit)
  derived, for the accumulate launch:
    texbase_GBps   one pass over texBase (80 x 3N float64) divided by the launch time: at 1 frame the HBM rate, at more frames what the
                   Infinity Cache and L2 add (the other frames re-read the slab from there)
    fp64_TFLOPs    executed: frames x 3N rows x 105 tiles x 64 fused multiply-adds x 2; `useful` counts only the 4094 products per row that
                   the block structure of A needs (the dense 108-column Gram multiplies the other channels' zero lighting columns too)
Model: oracle.bfm_ref.synthetic_facemodel(seed=3, nlat=189, nlon=189, smooth=True), 35721 vertices (the size profiles/r01_render_path.jsonl
used).  Its normals point away from the camera over most of the face, so the observation's weight is replaced by |n_z| x inside (every
vertex inside the photo takes part, as on a real face's front).  A 480 x 640 smooth synthetic photo; every frame its own expression and
affine.  HIP events on the current stream, warm, median of 20 repetitions after 5 warm-up ones.  No threshold is set: nothing did this job
before.
Usage: python scripts/bfm_appearance_latency.py [--out profiles/bfm_appearance.json] [--frames 1 16 128]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bfm_fit_latency import timed  # noqa: E402


def photo(h=480, w=640, seed=0):
  rng = np.random.default_rng(seed)
  y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
  img = np.stack([128 + sum(rng.uniform(10, 30) * np.sin(2 * np.pi * (rng.uniform(0.3, 1.5) * x + rng.uniform(0.3, 1.5) * y) + rng.uniform(0, 6.28))
                            for _ in range(3)) for _ in range(3)], axis=2)
  return np.clip(np.round(img), 0, 255).astype(np.uint8)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfm_appearance.json"))
  ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 128])
  a = ap.parse_args()
  import torch
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmfit import FaceFitter
  fm = br.synthetic_facemodel(seed=3, nlat=189, nlon=189, smooth=True)
  fitter = FaceFitter(fm)
  N = fitter.model.nver
  img = torch.from_numpy(photo()).cuda()
  rec = {"metric": "bfm_appearance", "device": torch.cuda.get_device_name(0), "face_model": "synthetic, %d vertices" % N,
         "timing": "hip events, median of 20 warm repetitions", "texbase_bytes": 80 * 3 * N * 8}
  for n in a.frames:
    coeff, _ = br.synthetic_coeffs(n, 7)
    coeff[:, 144:224] = 0
    coeff[:, 227:254] = 0
    aff = np.stack([2.0 + 0.002 * np.arange(n), 96.0 + 0.1 * np.arange(n), 16.0 - 0.05 * np.arange(n)], axis=1)
    r = {"observe": timed(lambda: fitter.observe(coeff, img, aff))}
    sh, w, obs = fitter.observe(coeff, img, aff)
    w = (sh[:, :, 2] / float(fitter.model.c.sh[1])).abs() * (obs.sum(dim=2) > 0)
    c = torch.from_numpy(coeff).cuda()
    observation = (sh, w, obs)
    fitter.fit_appearance(c, observation=observation)                      # (sizes the workspace, leaves valid partials behind)
    r["accumulate"] = timed(lambda: fitter.fit_appearance(c, observation=observation, max_trials=1, _stages=1))
    r["step_last"] = timed(lambda: fitter.fit_appearance(c, observation=observation, max_trials=1, _stages=2))
    two = timed(lambda: fitter.fit_appearance(c, observation=observation, max_trials=2, _stages=2))
    r["step"] = {"ms_median": two["ms_median"] - r["step_last"]["ms_median"], "repetitions": two["repetitions"]}
    r["fit"] = timed(lambda: fitter.fit_appearance(c, observation=observation))
    _, report = fitter.fit_appearance(c, observation=observation)
    report = report.cpu().numpy()
    r["fit"].update(statuses={str(int(s)): int((report[:, 0] == s).sum()) for s in np.unique(report[:, 0])},
                    accepted_mean=float(report[:, 1].mean()), E_mean=float(report[:, 2].mean()))
    lo, hi = 1, 32                                                         # smallest max_trials without a status 1
    if np.any(report[:, 0] == 1):
      lo = hi = None
    while lo is not None and lo < hi:
      mid = (lo + hi) // 2
      if np.any(fitter.fit_appearance(c, observation=observation, max_trials=mid)[1][:, 0].cpu().numpy() == 1):
        lo = mid + 1
      else:
        hi = mid
    r["trials_used"] = lo
    t = r["accumulate"]["ms_median"] * 1e-3
    r["accumulate"].update(texbase_GBps=rec["texbase_bytes"] / t / 1e9, fp64_TFLOPs=n * 3 * N * 105 * 64 * 2 / t / 1e12,
                           fp64_TFLOPs_useful=n * 3 * N * 4094 * 2 / t / 1e12)
    rec["frames_%d" % n] = r
  line = json.dumps(rec, indent=1)
  print(line)
  out = os.path.abspath(a.out)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

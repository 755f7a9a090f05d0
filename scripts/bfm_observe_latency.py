"""Device time of FaceFitter.observe with and without its two options on one GPU (vp_bfmfit_observe against vp_bfmfit_observe_ex):
writes profiles/bfm_observe.json.

  measured, at 1 / 64 / 250 frames, in the same run:
    observe            the plain call at a = 1 (shape, face normals, the per-vertex kernel: one bilinear tap)
    visibility_ss{1,2,4}   visibility=True at raster_scale 1, 2, 4 and a = 1: + per chunk of 8 frames two clears, the dense rasteriser
                       (three launches), the vertex test; + one mask launch
    observe_a{4,16}    the plain call at a = 4 and a = 16 (the same work as at a = 1; its taps are further apart in memory)
    prefilter_a{1,4,16}    prefilter=True at a = 1 (k = 1: the single tap), a = 4 (k = 4: 16 taps) and a = 16 (k = 16: 256 taps)
  and per option `ratio` = its median over the plain call's at the same a.
Model: oracle.bfm_ref.synthetic_facemodel(seed=3, nlat=189, nlon=189, smooth=True), 35721 vertices, as scripts/bfm_appearance_latency.py;
the triangle winding does not matter to the time.  A 3600 x 3600 uint8 noise photo on the device, the face centred in it at every a; every
frame its own expression.  The times include observe's host work (the rotation matrices are made on the host from coeff's angles; coeff is
uploaded), the same for every variant.  HIP events on the current stream, median of 10 repetitions after 3 warm-up ones.  No threshold is
set: the call is off the streaming path and runs once per enrolment or clip.
Usage: python scripts/bfm_observe_latency.py [--out profiles/bfm_observe.json] [--frames 1 64 250]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bfm_fit_latency import timed  # noqa: E402

SIDE = 3600


def affine(a, n):
  """The 224 image's centre on the photo's, every frame a little further along."""
  return np.stack([np.full(n, float(a)), SIDE / 2 - 112.0 * a + 0.1 * np.arange(n), SIDE / 2 - 112.0 * a - 0.05 * np.arange(n)], axis=1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfm_observe.json"))
  ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 250])
  a = ap.parse_args()
  import torch
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmfit import FaceFitter
  fm = br.synthetic_facemodel(seed=3, nlat=189, nlon=189, smooth=True)
  fitter = FaceFitter(fm)
  N = fitter.model.nver
  img = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
  rec = {"metric": "bfm_observe", "device": torch.cuda.get_device_name(0), "face_model": "synthetic, %d vertices, %d triangles" % (N, fitter.model.ntri),
         "photo": "%d x %d noise" % (SIDE, SIDE), "timing": "hip events, median of 10 warm repetitions"}
  t = lambda fn: timed(fn, rounds=13, warm=3)
  for n in a.frames:
    coeff, _ = br.synthetic_coeffs(n, 7)
    r = {"observe": t(lambda: fitter.observe(coeff, img, affine(1, n)))}
    base = {1: r["observe"]["ms_median"]}
    for ss in (1, 2, 4):
      r["visibility_ss%d" % ss] = t(lambda: fitter.observe(coeff, img, affine(1, n), visibility=True, raster_scale=ss))
      r["visibility_ss%d" % ss]["ratio"] = r["visibility_ss%d" % ss]["ms_median"] / base[1]
    _, w, _, vis = fitter.observe(coeff, img, affine(1, n), visibility=True, return_visible=True)
    r["visibility_ss2"]["hidden_share"] = float(1.0 - vis.double().mean().item())
    for s in (4, 16):
      r["observe_a%d" % s] = t(lambda: fitter.observe(coeff, img, affine(s, n)))
      base[s] = r["observe_a%d" % s]["ms_median"]
    for s in (1, 4, 16):
      r["prefilter_a%d" % s] = t(lambda: fitter.observe(coeff, img, affine(s, n), prefilter=True))
      r["prefilter_a%d" % s]["ratio"] = r["prefilter_a%d" % s]["ms_median"] / base[s]
      inside = fitter.observe(coeff, img, affine(s, n), prefilter=True)[2].sum(dim=2) > 0
      r["prefilter_a%d" % s]["inside_share"] = float(inside.double().mean().item())
    rec["frames_%d" % n] = r
  line = json.dumps(rec, indent=1)
  print(line)
  out = os.path.abspath(a.out)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

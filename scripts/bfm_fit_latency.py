"""Device time of the landmark fit on one GPU (voicepuppet_amd.bfmfit.FaceFitter): writes profiles/bfm_fit.json.

  fit_N        FaceFitter.fit of N = 1, 64, 250 frames from zeros (full fit, defaults): one workgroup per frame
  sequence     one round of fit_sequence's schedule for 250 frames: 3 identity steps + a tracking fit from the previous values
Frames: the six of tests/golden/bfm_fit.npz repeated, each with landmark noise of its own (0.05 px) so that no two workgroups do the same
work; 252-vertex synthetic face model (the fit reads 68 keypoint rows of the model, whatever its size).  HIP events on the current stream,
warm, median of 20 repetitions after 5 warm-up ones.  No threshold is set: nothing did this job before, on the host or on the device.
Usage: python scripts/bfm_fit_latency.py [--out profiles/bfm_fit.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, rounds=25, warm=5):
  import torch
  st = torch.cuda.current_stream()
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
  return {"ms_median": float(np.median(ms)), "ms_p90": float(np.percentile(ms, 90)), "repetitions": len(ms)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfm_fit.json"))
  a = ap.parse_args()
  import torch
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmfit import FaceFitter
  gold = np.load(os.path.join(ROOT, "tests", "golden", "bfm_fit.npz"))
  fitter = FaceFitter(br.synthetic_facemodel(seed=int(gold["model_seed"]), smooth=True))
  rng = np.random.default_rng(0)
  rec = {"metric": "bfm_fit", "device": torch.cuda.get_device_name(0), "face_model": "synthetic, 252 vertices",
         "commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
         "timing": "hip events, median of 20 warm repetitions"}
  for n in (1, 64, 250):
    lm = torch.from_numpy(np.stack([gold["landmarks_2d"][i % 6] for i in range(n)]) + rng.normal(0, 0.05, size=(n, 68, 2))).cuda()
    rec["fit_%d" % n] = timed(lambda: fitter.fit(lm))
    _, report = fitter.fit(lm)
    report = report.cpu().numpy()
    rec["fit_%d" % n].update(statuses={str(int(s)): int((report[:, 0] == s).sum()) for s in np.unique(report[:, 0])},
                             iterations_mean=float(report[:, 1].mean()), iterations_max=int(report[:, 1].max()))
  coeff, _ = fitter.fit(lm)
  p = fitter.last_params.clone()

  def one_round():
    q, c = p.clone(), coeff.clone()
    for _ in range(3):
      fitter.identity_step(lm, q, c)
    fitter.fit(lm, init=c, params=q, free="tracking")
  rec["sequence_round_250"] = timed(one_round)
  line = json.dumps(rec, indent=1)
  print(line)
  out = os.path.abspath(a.out)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

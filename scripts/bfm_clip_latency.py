"""Device time of the joint clip fit on one GPU (voicepuppet_amd.bfmfit.FaceFitter.fit_clip; csrc/bfm_clip.hip): writes profiles/bfm_clip.json.

  trial_T{40,250}_{uncoupled,coupled}   one round of the chain (the clip step's launch + the frame systems' launch) for ONE clip of T frames:
                                        (time of fit_clip with max_trials = 9) - (with max_trials = 1), divided by 8; from the start
                                        fit_sequence(rounds=0) gives, which 9 trials do not carry to a status (the report is checked)
  trial_16x40_coupled                   the same for 16 clips of 40 frames in one call: the clip steps run side by side
  fit_T40_coupled                       a whole fit_clip(max_trials=64) of the T = 40 clip, lam_smooth = (200, 20000, 20000), with its report
Clips: tests/bfm_clip_ref.synthetic_clip(T, sigma = 1 px) on the 252-vertex synthetic face model (the fit reads 68 keypoint rows of the model,
whatever its size).  HIP events on the current stream, warm, median of 10 repetitions after 3 warm-up ones.  No threshold is set: nothing
did this job before, on the host or on the device.
Usage: python scripts/bfm_clip_latency.py [--out profiles/bfm_clip.json]
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
SMOOTH = (200.0, 20000.0, 20000.0)


def timed(fn, rounds=13, warm=3):
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
  return float(np.median(ms))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfm_clip.json"))
  a = ap.parse_args()
  import torch
  import bfm_clip_ref as cr
  from voicepuppet_amd.bfmfit import FaceFitter
  rec = {"metric": "bfm_clip", "device": torch.cuda.get_device_name(0), "face_model": "synthetic, 252 vertices",
         "commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
         "timing": "hip events, median of 10 warm repetitions; a trial = (9 trials - 1 trial) / 8"}
  fitter = None

  def per_trial(lm, start, smooth, lengths=None):
    t1 = timed(lambda: fitter.fit_clip(lm, clip_lengths=lengths, params=start, lam_smooth=smooth, max_trials=1))
    t9 = timed(lambda: fitter.fit_clip(lm, clip_lengths=lengths, params=start, lam_smooth=smooth, max_trials=9))
    _, report = fitter.fit_clip(lm, clip_lengths=lengths, params=start, lam_smooth=smooth, max_trials=9)
    status = report[:, 0].cpu().numpy()
    return {"ms_per_trial": (t9 - t1) / 8, "ms_1_trial": t1, "ms_9_trials": t9, "all_clips_still_running_after_9": bool(np.all(status == 1))}

  for T in (40, 250):
    fm, _, _, _, noisy = cr.synthetic_clip(T, 1.0)
    if fitter is None:
      fitter = FaceFitter(fm)
    lm = torch.from_numpy(noisy).cuda()
    fitter.fit_sequence(lm, rounds=0)
    start = fitter.last_params.clone()
    for name, smooth in (("uncoupled", (0.0, 0.0, 0.0)), ("coupled", SMOOTH)):
      rec["trial_T%d_%s" % (T, name)] = per_trial(lm, start, smooth)
    if T == 40:
      rec["trial_16x40_coupled"] = per_trial(lm.repeat(16, 1, 1), start.repeat(16, 1), SMOOTH, lengths=[40] * 16)
      ms = timed(lambda: fitter.fit_clip(lm, params=start, lam_smooth=SMOOTH, max_trials=64))
      _, report = fitter.fit_clip(lm, params=start, lam_smooth=SMOOTH, max_trials=64)
      r = report.cpu().numpy()[0]
      rec["fit_T40_coupled"] = {"ms": ms, "status": int(r[0]), "accepted_steps": int(r[1]), "E": float(r[2]), "g_inf": float(r[3])}
  line = json.dumps(rec, indent=1)
  print(line)
  out = os.path.abspath(a.out)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

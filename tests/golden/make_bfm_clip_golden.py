"""Regenerates tests/golden/bfm_clip.npz: the inputs of the joint clip fit's tests and the solutions of the float64 restatement
tests/bfm_clip_ref.py (numpy only; about a minute on a CPU).

  python tests/golden/make_bfm_clip_golden.py

Two clips of bfm_clip_ref.synthetic_clip (oracle.bfm_ref.synthetic_facemodel(3), synthetic_coeffs(T, 5) as the base, a random walk of
expression and angles and the landmark noise from np.random.default_rng(0)):
  T = 8,  sigma = 0.5 px   clean8, noisy8, start8 = bfm_fit_ref.fit_sequence(rounds=0), seq8 = fit_sequence's default schedule,
                           sol8 / rep8 = fit_clip from start8 with zero smoothing (status 0), star8 = the same run until it stalls (gtol = 0)
  T = 40, sigma = 1.0 px   clean40, noisy40, start40, and fit_clip from start40 with lam_smooth = (0, 0, 0) -> sol40_zero / rep40_zero (stalls:
                           status 2, not a converged case) and SMOOTH = (200, 20000, 20000) -> sol40_smooth / rep40_smooth (status 0),
                           star40_smooth (gtol = 0)
errors40 rows = (noise, start, zero smoothing, SMOOTH), columns = bfm_clip_ref.point_errors: mean distance to the clean landmarks and mean
distance between the first differences in time, px.  The fixture holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
MODEL_SEED, COEFF_SEED, SEED = 3, 5, 0
SMOOTH = (200.0, 20000.0, 20000.0)


def main():
  import bfm_clip_ref as cr
  import bfm_fit_ref as fr
  d = {"model_seed": MODEL_SEED, "coeff_seed": COEFF_SEED, "seed": SEED, "smooth": np.array(SMOOTH)}
  fm, tbl, truth, clean, noisy = cr.synthetic_clip(8, 0.5, SEED, MODEL_SEED, COEFF_SEED)
  start, _ = fr.fit_sequence(tbl, noisy, rounds=0)
  seq, _ = fr.fit_sequence(tbl, noisy)
  sol, rep, trials = cr.fit_clip(tbl, noisy, start)
  star, srep, _ = cr.fit_clip(tbl, noisy, start, gtol=0.0, max_trials=300)
  print("T = 8: fit_sequence %.6f, joint %.6f, report %s, %d trials; stalled at |g| %.3e" % (cr.clip_cost(tbl, seq, noisy), rep[2], rep, trials, srep[3]))
  assert rep[0] == 0 and srep[0] == 2 and srep[3] < 1e-6
  d.update(truth8=truth, clean8=clean, noisy8=noisy, start8=start, seq8=seq, sol8=sol, rep8=rep, star8=star)
  fm, tbl, truth, clean, noisy = cr.synthetic_clip(40, 1.0, SEED, MODEL_SEED, COEFF_SEED)
  start, _ = fr.fit_sequence(tbl, noisy, rounds=0)
  zero, zrep, ztr = cr.fit_clip(tbl, noisy, start)
  smooth, rep, trials = cr.fit_clip(tbl, noisy, start, lam_smooth=SMOOTH)
  star, srep, _ = cr.fit_clip(tbl, noisy, start, lam_smooth=SMOOTH, gtol=0.0, max_trials=300)
  assert rep[0] == 0 and srep[0] == 2 and srep[3] < 1e-6
  errors = np.array([cr.point_errors(noisy, clean), cr.landmark_errors(tbl, start, clean), cr.landmark_errors(tbl, zero, clean),
                     cr.landmark_errors(tbl, smooth, clean)])
  print("T = 40: zero smoothing %s (%d trials), SMOOTH %s (%d trials), stalled at |g| %.3e" % (zrep, ztr, rep, trials, srep[3]))
  print("errors (to clean, first differences), px: noise, start, zero, SMOOTH\n", errors)
  d.update(truth40=truth, clean40=clean, noisy40=noisy, start40=start, sol40_zero=zero, rep40_zero=zrep, sol40_smooth=smooth, rep40_smooth=rep,
           star40_smooth=star, errors40=errors)
  d["model_checksum"] = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.meanshape.sum(), float(fm.keypoints.sum())])
  path = os.path.join(HERE, "bfm_clip.npz")
  np.savez_compressed(path, **d)
  print(path, os.path.getsize(path), "bytes")
  assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
  main()

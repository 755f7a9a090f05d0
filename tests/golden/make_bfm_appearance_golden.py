"""Regenerates tests/golden/bfm_appearance.npz (run in the build container only, like make_bfmfit_golden.py: it imports the REFERENCE's own
utils/reconstruct_mesh.py from /root/reference; numpy only).

  python tests/golden/make_bfm_appearance_golden.py

Contents, for oracle.bfm_ref.synthetic_facemodel(seed=3, smooth=True) (252 vertices): the seed and the model checksum; coeff [6,257]
float32 = synthetic_coeffs (non-zero texture, lighting and pose) with the pose jittered, rows 4 and 5 with a yaw of +0.6 / -0.6 rad so that
back-facing vertices exist; face_texture, face_color [6,252,3] and face_projection [6,252,2] float64 = what the reference's own
`Reconstruction` returned for each row, handed to it as float64 (so that its sines and cosines are float64, as in make_bfmfit_golden.py).
The fixture holds data only.

The seeds are chosen so that, with the photo and affines of tests/bfm_appearance_ref.py (smooth_photo, test_affines), (a) no vertex has
|(n . R)_z| < 1e-9, (b) no vertex lies within 1e-6 px of the photo's border, (c) the float64 helper reaches gtol = 1e-6 on every frame
within 32 trials and its gtol = 0 floor of |g|_inf / E is at least 3x below gtol.  The figures are printed; tests/test_bfm_appearance_host.py
asserts them again."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
MODEL_SEED, COEFF_SEED, JITTER_SEED, FRAMES, GTOL = 3, 11, 111, 6, 1e-6


def make_coeff():
  from oracle import bfm_ref as br
  coeff, _ = br.synthetic_coeffs(FRAMES, COEFF_SEED)
  rng = np.random.default_rng(JITTER_SEED)
  coeff[:, 144:224] = rng.normal(0, 1.0, size=(FRAMES, 80)).astype(np.float32)
  coeff[:, 227:254] = rng.normal(0, 0.15, size=(FRAMES, 27)).astype(np.float32)
  coeff[:, 224:227] += rng.normal(0, 0.1, size=(FRAMES, 3)).astype(np.float32)
  coeff[:, 254:257] += rng.normal(0, 0.05, size=(FRAMES, 3)).astype(np.float32)
  coeff[4, 225], coeff[5, 225] = 0.6, -0.6
  return coeff.astype(np.float32)


def conditions(fm, coeff, verbose=True):
  """The three figures of the module docstring: (min |n_z|, min border distance, worst trials, worst floor)."""
  import bfm_appearance_ref as ar
  photo = ar.smooth_photo()
  H, W = photo.shape[:2]
  aff = ar.test_affines(len(coeff))
  nz_min, border, trials, floor = np.inf, np.inf, 0, 0.0
  for f in range(len(coeff)):
    nr, proj = ar.geometry(fm, coeff[f], ar.rotation(coeff[f, 224:227]))
    px, py = aff[f, 0] * proj[:, 0] + aff[f, 1], aff[f, 0] * proj[:, 1] + aff[f, 2]
    nz_min = min(nz_min, np.abs(nr[:, 2]).min())
    border = min(border, np.abs(np.stack([px, px - (W - 1), py, py - (H - 1)])).min())
    obs = ar.observe(fm, coeff[f], photo, aff[f], R=ar.rotation(coeff[f, 224:227]))
    p, rep, info = ar.fit(fm, obs, init=ar.coeff_to_p(coeff[f]), gtol=GTOL, max_trials=32)
    ps, reps, infos = ar.fit(fm, obs, init=ar.coeff_to_p(coeff[f]), gtol=0.0, max_trials=400)
    fl = reps[3] / reps[2]
    if verbose:
      print("frame %d: visible %d of %d, back-facing %d; gtol run status %d after %d trials (%d rejects), E %.6g; gtol = 0 run status %d after %d "
            "trials, floor |g|/E %.3e" % (f, int((obs[1] > 0).sum()), len(nr), int((nr[:, 2] < 0).sum()), rep[0], info["trials"], info["rejects"], rep[2],
                                          reps[0], infos["trials"], fl))
    assert rep[0] == 0, rep
    trials, floor = max(trials, info["trials"]), max(floor, fl)
  return nz_min, border, trials, floor


def main():
  from oracle import bfm_ref as br
  sys.path.insert(0, os.path.join(REF, "utils"))
  import reconstruct_mesh as rm                        # the reference module itself
  fm = br.synthetic_facemodel(seed=MODEL_SEED, smooth=True)
  coeff = make_coeff()
  d = {"model_seed": MODEL_SEED, "coeff": coeff}
  d["model_checksum"] = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(),
                                  float(fm.tri.sum()), float(fm.point_buf.sum()), float(fm.keypoints.sum())])
  outs = [rm.Reconstruction(coeff[i:i + 1].astype(np.float64), fm) for i in range(FRAMES)]
  d["face_texture"] = np.stack([np.array(o[1][0], np.float64) for o in outs])
  d["face_color"] = np.stack([np.array(o[2][0], np.float64) for o in outs])
  d["face_projection"] = np.stack([np.array(o[3][0], np.float64) for o in outs])
  nz_min, border, trials, floor = conditions(fm, coeff)
  print("min |(n.R)_z| %.3e (>= 1e-9); min distance to the photo border %.3e px (>= 1e-6); worst trials %d (<= 32); worst floor %.3e (<= %.3e)"
        % (nz_min, border, trials, floor, GTOL / 3))
  assert nz_min >= 1e-9 and border >= 1e-6 and trials <= 32 and 3 * floor <= GTOL
  path = os.path.join(HERE, "bfm_appearance.npz")
  np.savez_compressed(path, **d)
  print(path, os.path.getsize(path), "bytes")
  assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
  main()

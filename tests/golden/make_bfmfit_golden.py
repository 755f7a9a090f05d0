"""Regenerates tests/golden/bfm_fit.npz (run in the build container only, like make_bfm_visual_golden.py: it imports the REFERENCE's own
utils/reconstruct_mesh.py and utils/bfm_load_data.py from /root/reference; numpy, scipy and PIL only).

  python tests/golden/make_bfmfit_golden.py

Contents, for oracle.bfm_ref.synthetic_facemodel(seed=3, smooth=True) (252 vertices): the seed and the model checksum (as bfm_recon.npz);
coeff [6,257] float32 = synthetic_coeffs with the pose jittered by N(0, 0.1 rad) in the angles and N(0, 0.05) in the translation;
landmarks_2d [6,68,2] float64 = what the reference's own `Reconstruction` returned for each row (this pins the forward model of the fit).
The rows are handed to it as float64 arrays: with float32 angles its Compute_rotation_matrix takes float32 sines and cosines (:74-82), and
a fit's unknowns are float64.
The two seeds: about one frame in five of this family stalls at |g|_inf = 1e-6 .. 2e-6, where a step's gain in E (1e-13 of E = 50) falls
below the float64 rounding of E itself, so "E(p+d) < E(p)" rejects every step.  Of the seed pairs (s, s + 100),
s = 0 .. 9, three have six frames that all reach gtol = 1e-6 in the float64 helper; s = 7 is the one whose frames stall lowest when run
with gtol = 0 (3e-7 at the worst), i.e. with the widest margin between the default gtol and that floor.
pre_lm68 [68,2] = frame 0's landmarks under a similarity (scale 0.9, shift), lm3d68 [68,3] = the centred mean shape at the keypoints, and
pre_lm_new [5,2] / pre_trans_params [5] = what the reference's own `POS` and `process_img` (the two halves of `Preprocess`, called as it
calls them) returned for the five points of pre_lm68 (load_lm3d's selection, :122-127) on a blank 224 x 224 PIL image.  The fixture holds data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
MODEL_SEED, COEFF_SEED, JITTER_SEED, FRAMES = 3, 7, 107, 6


def main():
  from oracle import bfm_ref as br
  import bfm_fit_ref as fr
  sys.path.insert(0, os.path.join(REF, "utils"))
  import reconstruct_mesh as rm                        # the reference modules themselves
  import bfm_load_data as bl
  from PIL import Image
  fm = br.synthetic_facemodel(seed=MODEL_SEED, smooth=True)
  coeff, _ = br.synthetic_coeffs(FRAMES, COEFF_SEED)
  rng = np.random.default_rng(JITTER_SEED)
  coeff[:, 224:227] += rng.normal(0, 0.1, size=(FRAMES, 3)).astype(np.float32)
  coeff[:, 254:257] += rng.normal(0, 0.05, size=(FRAMES, 3)).astype(np.float32)
  d = {"model_seed": MODEL_SEED, "coeff": coeff.astype(np.float32)}
  d["model_checksum"] = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(),
                                  float(fm.tri.sum()), float(fm.point_buf.sum()), float(fm.keypoints.sum())])
  d["landmarks_2d"] = np.stack([np.array(rm.Reconstruction(coeff[i:i + 1].astype(np.float64), fm)[5][0], np.float64) for i in range(FRAMES)])
  mean = fm.meanshape.reshape(-1, 3)
  lm3d68 = (mean - mean.mean(axis=0, keepdims=True))[fm.keypoints]
  pre_lm68 = 0.9 * d["landmarks_2d"][0] + np.array([7.25, -5.5])
  img = Image.new("RGB", (224, 224))
  # Preprocess (:197-212) itself stops at its last line under this numpy (:210 builds an array from a mix of scalars and [1] arrays), so
  # its two halves, the reference's own POS and process_img, are called as it calls them and the five numbers are put together here
  lm5 = fr.five_points(pre_lm68)
  lm5 = np.stack([lm5[:, 0], 224 - 1 - lm5[:, 1]], axis=1)
  t, s = bl.POS(lm5.transpose(), fr.five_points(lm3d68).transpose())
  _, lm_new, t0, t1 = bl.process_img(img, lm5, t, s)
  lm_new = np.stack([lm_new[:, 0], 223 - lm_new[:, 1]], axis=1)
  trans_params = np.array([224.0, 224.0, float(102.0 / s), float(t0[0]), float(t1[0])])
  d["pre_lm68"], d["lm3d68"] = pre_lm68, lm3d68
  d["pre_lm_new"], d["pre_trans_params"] = np.asarray(lm_new, np.float64), np.asarray(trans_params, np.float64).reshape(5)
  path = os.path.join(HERE, "bfm_fit.npz")
  np.savez_compressed(path, **d)
  print(path, os.path.getsize(path), "bytes")
  assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
  main()

"""CPU checks of the landmark fit (voicepuppet_amd/bfmfit.py, csrc/bfm_fit.hip): the float64 restatement tests/bfm_fit_ref.py against the
reference-captured fixture tests/golden/bfm_fit.npz, its Jacobian and its convergence, the host alignment arithmetic of bfmfit.py against the
reference's captured values, the enrolment closed loop, and the C ABI.  The device fit itself: tests/test_gpu_bfm_fit.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_fit_ref as fr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")


@pytest.fixture(scope="module")
def gold():
  g = dict(np.load(GOLDEN))
  fm = br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True)
  chk = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(), float(fm.tri.sum()),
                  float(fm.point_buf.sum()), float(fm.keypoints.sum())])
  assert np.allclose(chk, g["model_checksum"], rtol=1e-12, atol=0), "the synthetic face model is not the fixture's"
  g["fm"], g["tbl"] = fm, fr.table(fm)
  return g


@pytest.fixture(scope="module")
def fits(gold):
  """The helper's fit of the six frames from zeros, once."""
  return fr.fit_frames(gold["tbl"], gold["landmarks_2d"])


def test_fixture_shape(gold):
  assert gold["fm"].meanshape.size == 3 * 252 and gold["tbl"].shape == (204, 145)
  assert gold["coeff"].shape == (6, 257) and gold["coeff"].dtype == np.float32 and gold["landmarks_2d"].shape == (6, 68, 2)


def test_forward_model_matches_reference(gold):
  """project() against landmarks_2d of the reference's own Reconstruction: both float64, so 1e-9 px (rounding of a 224 px coordinate is
  about 1e-13; the bound is far below anything a fit resolves)."""
  for f in range(6):
    got = fr.project(gold["tbl"], fr.coeff_to_p(gold["coeff"][f]))
    err = np.abs(got - gold["landmarks_2d"][f]).max()
    print("frame %d forward error %.3e px" % (f, err))
    assert err <= 1e-9


def test_jacobian_matches_central_differences(gold):
  """h = 1e-6: the rounding of a difference of two 224 px coordinates over 2h is 2 * 224 * 2^-53 / 2e-6 = 2.5e-8 per entry, the
  truncation h^2 f'''/6 = 1e-12 * O(1e3); 1e-6 stands a factor 10 above both and 1e-8 of the largest entry (1e2)."""
  tbl = gold["tbl"]
  for f in (0, 3):
    p = fr.coeff_to_p(gold["coeff"][f])
    _, J = fr.project(tbl, p, want_jac=True)
    num = np.zeros_like(J)
    for j in range(fr.NP):
      e = np.zeros(fr.NP)
      e[j] = 1e-6
      num[:, j] = ((fr.project(tbl, p + e) - fr.project(tbl, p - e)) / 2e-6).reshape(-1)
    err = np.abs(J - num).max()
    print("frame %d Jacobian error %.3e (largest entry %.3e)" % (f, err, np.abs(J).max()))
    assert err <= 1e-6


def test_helper_converges(gold, fits):
  ps, reps = fits
  print(reps)
  assert np.all(reps[:, 0] == 0) and np.all(reps[:, 1] <= 100) and np.all(reps[:, 3] <= 1e-6)
  for f in range(6):
    d = np.sqrt(((fr.project(gold["tbl"], ps[f]) - gold["landmarks_2d"][f]) ** 2).sum(axis=1))
    assert d.mean() < 0.5, d.mean()                   # (the regularised fit of lam = 1 leaves a fraction of a pixel)


def test_helper_masks_and_status(gold, fits):
  tbl, lm = gold["tbl"], gold["landmarks_2d"][0]
  start = fits[0][0].astype(np.float32).astype(np.float64)        # the fitted shape, the pose to be found again from zero
  start[144:] = 0
  p, rep = fr.fit(tbl, lm, init=start, free="pose")
  assert rep[0] == 0 and np.array_equal(p[:144], start[:144]) and not np.array_equal(p[144:], start[144:])
  p, rep = fr.fit(tbl, lm, max_iters=2)
  assert rep[0] == 1 and rep[1] == 2
  bad = lm.copy()
  bad[5, 1] = np.nan
  p, rep = fr.fit(tbl, bad, init=start)
  assert rep[0] == 3 and np.array_equal(p, start)
  w = np.ones(68)
  w[5] = 0                                                        # ... unless its weight drops it?  No: non-finite input is refused as a whole
  assert fr.fit(tbl, bad, weights=w)[1][0] == 3


def test_preprocess_landmarks_matches_reference(gold):
  from voicepuppet_amd import bfmfit
  lm_new, tp = bfmfit.preprocess_landmarks(gold["pre_lm68"], gold["lm3d68"])
  assert lm_new.shape == (68, 2) and tp.shape == (5,)
  # the reference was handed the five points; the map is affine, so the five points of the 68 mapped landmarks are the mapped five points
  e1, e2 = np.abs(bfmfit.five_points(lm_new) - gold["pre_lm_new"]).max(), np.abs(tp - gold["pre_trans_params"]).max()
  print("lm_new error %.3e, trans_params error %.3e" % (e1, e2))
  assert e1 <= 1e-9 and e2 <= 1e-9
  lm5, tp5 = bfmfit.preprocess_landmarks(gold["pre_lm68"], fr.five_points(gold["lm3d68"]))
  assert np.array_equal(lm5, lm_new) and np.array_equal(tp5, tp)
  assert np.array_equal(bfmfit.five_points(gold["pre_lm68"]), fr.five_points(gold["pre_lm68"]))


def test_crop_alignment_arithmetic():
  """utils/utils.py:78-110 on a case worked by hand: box x 100..300, y 50..350 in a 480 x 640 image."""
  from voicepuppet_amd import bfmfit
  xy = np.zeros((68, 2))
  xy[:, 0] = np.linspace(100, 300, 68)
  xy[:, 1] = np.linspace(50, 350, 68)
  out, cx, cy, ratio = bfmfit.crop_alignment(xy, 480, 640)
  # centre (200, 200); width = height = 200; ratio 1.3 fits; width = 260; left = top = 70
  assert (cx, cy) == (200, 200) and ratio == 224.0 / 260
  assert np.allclose(out[:, 0], (xy[:, 0] - 70) * 224 / 260, rtol=0, atol=1e-12) and np.allclose(out[:, 1], (xy[:, 1] - 70) * 224 / 260, rtol=0, atol=1e-12)
  # near the border the expansion shrinks: centre_y = 200 -> max_ratio = min(280/100, 440/100, 2, 2) stays 1.3; at the top it does not
  out, cx, cy, ratio = bfmfit.crop_alignment(xy - np.array([0.0, 50.0]), 480, 640)
  assert cy == 150 and ratio == 224.0 / int(200 * 1.3)
  out, cx, cy, ratio = bfmfit.crop_alignment(xy - np.array([0.0, 120.0]), 480, 640)      # centre_y = 80 -> max_ratio 0.8
  assert cy == 80 and ratio == 224.0 / int(200 * 0.8)


def closed_loop(photo, landmarks_xy, project224):
  """Distance of every input landmark from where its reconstructed landmark is pasted (infer_bfmvid.paste_geometry)."""
  from voicepuppet_amd.pixrefer.infer_bfmvid import paste_geometry
  side, y0, x0 = paste_geometry(int(photo["center_x"]), int(photo["center_y"]), float(photo["ratio"]), photo["transform_params"])
  back = fr.paste_map(project224, side, y0, x0)
  return np.sqrt(((back - landmarks_xy) ** 2).sum(axis=1))


PLACEMENTS = ((1.7, (130.0, 60.0)), (1.0, (200.0, 100.0)), (2.0, (100.0, 40.0)))     # a face of 260, 150 and 300 px in a 480 x 640 photo


def unit_scale_lm3d(gold, xy):
  """The standard landmarks scaled so that Preprocess's scale 102/s is 1 for this photo.  render_face divides the translation, which is in
  crop pixels, by ratio * (102/s) where the crop's own scale is `ratio` (infer_bfmvid.py:80-82): an approximation of the reference's that
  is exact at 102/s = 1 and moves the paste by t (1 - s/102) / ratio otherwise (3 px in these photos with the unscaled lm3d68, whatever
  the fit does).  The closed loop is about this project's chain, so it is run where the reference's own arithmetic closes."""
  from voicepuppet_amd import bfmfit
  crop = bfmfit.crop_alignment(xy, 480, 640)[0]
  return gold["lm3d68"] / bfmfit.preprocess_landmarks(crop, gold["lm3d68"])[1][2]


def test_enroll_closed_loop_host(gold):
  """crop_alignment + preprocess_landmarks (the product's host arithmetic) with the helper's fit in place of the device's: the fitted
  landmarks, pasted as render_face pastes the 224 image, land on the input within the fit's own residual (in photo pixels) + 2 px.
  The 2 px: tx, ty and side are truncated to integers (<= 1 px each on the paste corner) and the resize rounds half a pixel.
  Measured worst (error - residual) for the three placements: 1.87, 0.90, 1.00 px."""
  from voicepuppet_amd import bfmfit
  tbl = gold["tbl"]
  for scale, shift in PLACEMENTS:
    xy = fr.photo_landmarks(gold["landmarks_2d"][0], scale, shift)
    crop, cx, cy, ratio = bfmfit.crop_alignment(xy, 480, 640)
    lm_new, tp = bfmfit.preprocess_landmarks(crop, unit_scale_lm3d(gold, xy))
    assert abs(tp[2] - 1) < 0.01
    p, rep = fr.fit(tbl, lm_new)
    proj = fr.project(tbl, p)
    photo = {"center_x": cx, "center_y": cy, "ratio": ratio, "transform_params": tp}
    resid = np.sqrt(((proj - lm_new) ** 2).sum(axis=1)) / (ratio * tp[2])           # the fit's residual in photo pixels
    err = closed_loop(photo, xy, proj)
    print("closed loop at scale %.1f: worst error - residual %.3f px, worst residual %.3f px" % (scale, (err - resid).max(), resid.max()))
    assert np.all(err <= resid + 2.0)


def test_abi_exports_and_refusals(gold):
  from voicepuppet_amd import _lib
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header))
  new = {"vp_bfmfit_workspace_bytes", "vp_bfmfit_fit", "vp_bfmfit_identity_step"}
  assert new <= declared and new <= set(_lib.exported_symbols())
  lib = _lib.lib()
  for name in new:
    assert getattr(lib, name).argtypes is not None, name
  assert lib.vp_bfmfit_workspace_bytes(0) == 0
  assert lib.vp_bfmfit_workspace_bytes(65) - lib.vp_bfmfit_workspace_bytes(64) == 8 * (81 * 82 // 2 + 1)      # one more 64-frame partial
  # refused on the host, before anything is enqueued (no device is touched): a keypoint outside the model, a bad mask
  buf = (ctypes.c_ubyte * 4096)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  m = _lib.BfmModel()
  m.nver, m.ntri = 252, 1
  for k in ("meanshape", "idBase", "exBase"):
    setattr(m, k, ctypes.addressof(buf))
  kp = np.arange(68, dtype=np.int32)
  big = 1 << 30
  args = lambda kpa, free: (ctypes.byref(m), kpa.ctypes.data_as(ctypes.c_void_p), 0, p, None, 0, p, None, 0, 1, 1.0, 1.0, 1e-6, 100, free, p, p, p, big, None)
  bad = kp.copy()
  bad[67] = 252
  assert lib.vp_bfmfit_fit(*args(bad, 15)) == -1 and b"keypoint 67" in lib.vp_last_error()
  bad[67] = -1
  assert lib.vp_bfmfit_fit(*args(bad, 15)) == -1
  assert lib.vp_bfmfit_fit(*args(kp, 0)) == -1 and lib.vp_bfmfit_fit(*args(kp, 16)) == -1
  assert lib.vp_bfmfit_identity_step(ctypes.byref(m), bad.ctypes.data_as(ctypes.c_void_p), 0, p, None, 0, p, None, 1, 1.0, p, big, None) == -1


def test_cli_options():
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  opts, _ = fl.parse_options(["--clip", "lm.txt", "--size", "480", "640", "--out", "bfmcoeff.txt"])
  assert (opts.clip, opts.photo, tuple(opts.size), opts.out, opts.rounds, opts.id_steps) == ("lm.txt", None, (480, 640), "bfmcoeff.txt", 3, 3)
  launcher = open(os.path.join(ROOT, "voicepuppet", "bfmnet", "fit_landmarks.py")).read()
  assert "voicepuppet_amd.bfmnet.fit_landmarks" in launcher and len(launcher.splitlines()) == 14

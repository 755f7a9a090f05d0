"""CPU checks of the photometric fit's float64 helper (tests/bfm_appearance_ref.py) and of the host arithmetic around it: the helper
against the reference's own Reconstruction (tests/golden/bfm_appearance.npz), its Jacobian, `photo_affine`, the bilinear sampling rule, the
conditions the fixture was chosen for, and the C ABI's host-side refusals.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import bfm_appearance_ref as ar  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_appearance.npz")
FIT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")


@pytest.fixture(scope="module")
def gold():
  g = dict(np.load(GOLDEN))
  fm = br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True)
  chk = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(), float(fm.tri.sum()),
                  float(fm.point_buf.sum()), float(fm.keypoints.sum())])
  assert np.allclose(chk, g["model_checksum"], rtol=1e-12, atol=0), "the synthetic face model changed: regenerate the fixture"
  g["fm"] = fm
  return g


def test_helper_matches_reference(gold):
  """T, T L and the projection against face_texture, face_color, face_projection of the reference's own Reconstruction: float64 sums of
  about 100 terms of magnitude <= 255 on both sides, so 1e-9."""
  fm = gold["fm"]
  assert gold["coeff"].shape == (6, 257) and gold["coeff"].dtype == np.float32
  assert sum(abs(float(gold["coeff"][f, 225])) > 0.5 for f in range(6)) >= 2
  for f in range(6):
    c = gold["coeff"][f].astype(np.float64)
    nr, proj = ar.geometry(fm, c)
    p = ar.coeff_to_p(c)
    tex = ar.texture(fm, p[:80])
    col = ar.face_color(fm, ar.sh_terms(nr), p)
    errs = (np.abs(tex - gold["face_texture"][f]).max(), np.abs(col - gold["face_color"][f]).max(), np.abs(proj - gold["face_projection"][f]).max())
    print("frame %d: texture %.3e, colour %.3e, projection %.3e" % ((f,) + errs))
    assert max(errs) <= 1e-9
    assert np.any(nr[:, 2] < 0) and np.any(nr[:, 2] > 0)


def test_jacobian_matches_central_differences(gold):
  """r is bilinear in (delta, gamma): a central difference has no truncation error beyond rounding, 2 * 255 * 2^-53 / 2h = 6e-8 at h = 1e-6
  on entries up to |L B| ~ 10 and |Y T| ~ 700; 1e-5 stands above that."""
  fm = gold["fm"]
  photo = ar.smooth_photo()
  obs = ar.observe(fm, gold["coeff"][1], photo, ar.test_affines(6)[1])
  p = ar.coeff_to_p(gold["coeff"][1])
  _, J = ar.residual(fm, obs, p, want_jac=True)
  h = 1e-6
  num = np.zeros_like(J)
  for j in range(ar.NA):
    e = np.zeros(ar.NA)
    e[j] = h
    num[:, j] = (ar.residual(fm, obs, p + e) - ar.residual(fm, obs, p - e)) / (2 * h)
  print("J: largest entry %.3e, largest difference %.3e" % (np.abs(J).max(), np.abs(J - num).max()))
  assert np.abs(J - num).max() <= 1e-5
  # A and g are J's: the gradient of E by central differences (E ~ 600, rounding 600 * 2^-53 / 2e-6 = 3e-8 ... times a few: 1e-5)
  A, g, E = ar.normal_equations(fm, obs, p)
  gn = np.array([(ar.cost(fm, obs, p + h * np.eye(ar.NA)[j]) - ar.cost(fm, obs, p - h * np.eye(ar.NA)[j])) / (2 * h) for j in range(ar.NA)])
  print("g: |g| %.3e, largest difference from dE/dp / 2 %.3e" % (np.abs(g).max(), np.abs(g - gn / 2).max()))
  assert np.abs(g - gn / 2).max() <= 1e-5 * max(1.0, np.abs(g).max())
  assert abs(E - ar.cost(fm, obs, p)) <= 1e-12 * E and np.allclose(A, A.T, rtol=0, atol=1e-12 * np.abs(A).max())


def test_photo_affine_inverts_the_alignment():
  """a (u, v) + b gives back the photo's landmarks from preprocess_landmarks(crop_alignment(.)) to 1e-9 px, for random landmark sets;
  the second placement's crop is clipped by the image edge (its expansion ratio is below 1.3)."""
  from voicepuppet_amd import bfmfit
  g = dict(np.load(FIT_GOLDEN))
  rng = np.random.default_rng(4)
  clipped = 0
  for scale, shift in ((1.7, (130.0, 60.0)), (2.0, (-40.0, 20.0)), (0.8, (40.3, 200.7))):
    for _ in range(3):
      xy = scale * (g["landmarks_2d"][int(rng.integers(6))] + rng.normal(0, 1.5, size=(68, 2))) + np.asarray(shift)
      crop, cx, cy, ratio = bfmfit.crop_alignment(xy, 480, 640)
      width = xy[:, 0].max() - xy[:, 0].min()
      clipped += int(round(224.0 / ratio)) < int(width * 1.3)
      lm_new, _ = bfmfit.preprocess_landmarks(crop, g["lm3d68"])
      a, bx, by = bfmfit.photo_affine(xy, 480, 640, g["lm3d68"])
      back = np.stack([a * lm_new[:, 0] + bx, a * lm_new[:, 1] + by], axis=1)
      print("scale %.1f: a %.6f, b (%.3f, %.3f), worst %.3e px" % (scale, a, bx, by, np.abs(back - xy).max()))
      assert np.abs(back - xy).max() <= 1e-9
  assert clipped >= 1


def test_bilinear_known_answers():
  rng = np.random.default_rng(2)
  img = rng.integers(0, 256, size=(5, 7, 3)).astype(np.uint8)
  H, W = 5, 7
  v, inside = ar.bilinear(img, np.array([3.0, 2.5, 2.5, W - 1.0, W - 1 + 1e-3, 0.0, -1e-3, 4.0]), np.array([2.0, 1.0, 1.5, H - 1.0, 2.0, 0.0, 1.0, H - 1 + 1e-3]))
  assert inside.tolist() == [True, True, True, True, False, True, False, False]
  assert np.array_equal(v[0], img[2, 3].astype(np.float64))                                        # a pixel centre returns the pixel
  assert np.array_equal(v[1], (img[1, 2].astype(np.float64) + img[1, 3]) / 2)                      # a midpoint the mean
  assert np.allclose(v[2], img[1:3, 2:4].astype(np.float64).mean(axis=(0, 1)), rtol=0, atol=1e-12)
  assert np.array_equal(v[3], img[H - 1, W - 1].astype(np.float64))                                # px = W-1 is inside
  assert np.array_equal(v[5], img[0, 0].astype(np.float64))
  assert np.all(v[4] == 0) and np.all(v[6] == 0) and np.all(v[7] == 0)


def test_fixture_conditions(gold):
  """What the fixture's seeds were chosen for (tests/golden/make_bfm_appearance_golden.py), asserted again."""
  import make_bfm_appearance_golden as mk
  assert np.array_equal(mk.make_coeff(), gold["coeff"])
  nz_min, border, trials, floor = mk.conditions(gold["fm"], gold["coeff"])
  print("min |(n.R)_z| %.3e; min border distance %.3e px; worst trials %d; worst floor %.3e" % (nz_min, border, trials, floor))
  assert nz_min >= 1e-9 and border >= 1e-6 and trials <= 32 and 3 * floor <= mk.GTOL


def test_helper_statuses(gold):
  fm = gold["fm"]
  obs = ar.observe(fm, gold["coeff"][0], ar.smooth_photo(), ar.test_affines(6)[0])
  p, rep, info = ar.fit(fm, obs, max_trials=2)
  assert rep[0] == 1 and info["trials"] == 2
  bad = (obs[0], obs[1], obs[2].copy())
  bad[2][5, 1] = np.nan
  assert ar.fit(fm, bad)[1][0] == 3
  assert ar.fit(fm, (obs[0], np.zeros_like(obs[1]), obs[2]))[1][0] == 3


def test_abi_exports_and_refusals():
  from voicepuppet_amd import _lib
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header))
  new = {"vp_bfmfit_observe_workspace_bytes", "vp_bfmfit_observe", "vp_bfmfit_appearance_workspace_bytes", "vp_bfmfit_appearance"}
  assert new <= declared and new <= set(_lib.exported_symbols())
  lib = _lib.lib()
  for name in new:
    assert getattr(lib, name).argtypes is not None, name
  assert lib.vp_bfmfit_observe_workspace_bytes(0, 1, 1) == 0 and lib.vp_bfmfit_appearance_workspace_bytes(252, 0) == 0
  assert lib.vp_bfmfit_observe_workspace_bytes(252, 442, 2) - lib.vp_bfmfit_observe_workspace_bytes(252, 442, 1) == 8 * 3 * (252 + 443)
  # the slab partition is a function of nver alone: the workspace is linear in frames, and bounded at the BFM's size
  one = lib.vp_bfmfit_appearance_workspace_bytes(35709, 2) - lib.vp_bfmfit_appearance_workspace_bytes(35709, 1)
  assert lib.vp_bfmfit_appearance_workspace_bytes(35709, 128) - lib.vp_bfmfit_appearance_workspace_bytes(35709, 127) == one
  assert one <= 8 * (6120 + 128 * 5888)
  # refused on the host, before anything is enqueued (no device is touched)
  buf = (ctypes.c_ubyte * 4096)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  m = _lib.BfmModel()
  m.nver, m.ntri = 252, 442
  for k in ("meanshape", "idBase", "exBase", "meantex", "texBase", "tri", "point_buf"):
    setattr(m, k, ctypes.addressof(buf))
  big = 1 << 30
  obs = lambda frames=1, photo=p, pf=1, h=96, w=128, ws=big: lib.vp_bfmfit_observe(ctypes.byref(m), p, p, frames, photo, pf, h, w, p, None, p, p, p, p, ws, None)
  assert obs(frames=65536) == -1 and b"65535" in lib.vp_last_error()
  assert obs(frames=0) == -1 and obs(photo=None) == -1 and obs(h=1) == -1 and obs(w=1) == -1 and obs(pf=2) == -1
  assert obs(ws=64) == -1 and b"workspace" in lib.vp_last_error()
  app = lambda frames=1, sh=p, trials=32, stages=3, lam=1.0, gtol=1e-6, ws=big, params_in=0: lib.vp_bfmfit_appearance(
      ctypes.byref(m), sh, p, p, p, None, params_in, frames, lam, 1.0, gtol, trials, stages, p, p, p, ws, None)
  assert app(frames=0) == -1 and app(sh=None) == -1 and app(trials=0) == -1 and app(stages=0) == -1 and app(stages=4) == -1
  assert app(lam=-1.0) == -1 and app(gtol=float("nan")) == -1 and app(params_in=1) == -1
  assert app(ws=64) == -1 and b"workspace" in lib.vp_last_error()


def test_cli_options():
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  opts, _ = fl.parse_options(["--photo", "lm.txt", "--image", "face.jpg", "--out", "photo.npz", "--lam_tex", "2", "--lam_gamma", "0.5"])
  assert (opts.photo, opts.image, opts.size, opts.out, opts.lam_tex, opts.lam_gamma) == ("lm.txt", "face.jpg", None, "photo.npz", 2.0, 0.5)
  opts, _ = fl.parse_options(["--photo", "lm.txt", "--size", "480", "640", "--out", "photo.npz"])
  assert opts.image is None and tuple(opts.size) == (480, 640) and opts.lam_tex == 1.0 and opts.lam_gamma == 1.0

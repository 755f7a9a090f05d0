"""Device fit of BFM texture and lighting to a photo's pixels (voicepuppet_amd.bfmfit.FaceFitter.observe / fit_appearance / enroll(image=);
csrc/bfm_appear.hip: vp_bfmfit_observe, vp_bfmfit_appearance) against the float64 restatement tests/bfm_appearance_ref.py, which is pinned
to the reference's own `Reconstruction` (tests/test_bfm_appearance_host.py).  Two synthetic models: 252 vertices (4 slabs of 64, the last
with 60) and 1200 vertices (19 slabs, the last with 48); frames in {1, 3, 7}, the six rows of tests/golden/bfm_appearance.npz repeated; a
smooth 96 x 128 photo under affines with a != 1 that push some vertices outside it.

How a fit is judged (gtol = 1e-6, the default), per frame, in float64 on the host, as tests/test_gpu_bfm_fit.py judges:
  stationarity  |g|_inf of the HELPER at the device's p  <= 1.01 gtol E     (the stopping rule is relative; 1 %: float64 rounding of g)
  agreement     |p_dev - p*|_inf <= 2 |H^-1|_inf gtol E                     p* = the helper run until it stalls (gtol = 0), H = A at p*:
                H (p_dev - p*) = g(p_dev) - g(p*) to first order; the factor 2 covers the second-order term
The bounds follow from the stopping rule, not from what the device gives; the figures are printed before they are asserted."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_appearance_ref as ar  # noqa: E402
import bfm_fit_ref as fr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GTOL = 1e-6
MODELS = {252: dict(nlat=14, nlon=18), 1200: dict(nlat=30, nlon=40)}
# test_start_that_rejects: delta = 5 N(0,1) from np.random.default_rng(REJECT_SEED) on fixture row REJECT_FRAME.  Gauss-Newton on this
# bilinear problem rarely overshoots: of the seeds 0 .. 199 on the six rows, the helper rejects a trial from three (row 0 seed 83: 28 trials,
# 7 rejects; row 4 seed 40: 22 trials, 2 rejects; row 5 seed 60: 30 trials, 3 rejects).  The one that leaves most of the 32 trials is taken.
REJECT_FRAME, REJECT_SEED = 4, 40


class Case:
  """One model: its fitter, and per fixture row the helper's observation (once) and p* (once per key)."""

  def __init__(self, nver, coeff, photo):
    from voicepuppet_amd.bfmfit import FaceFitter
    self.fm = br.synthetic_facemodel(seed=3, smooth=True, **MODELS[nver])
    assert self.fm.meanshape.size == 3 * nver
    self.fitter = FaceFitter(self.fm)
    self.coeff, self.photo, self.aff = coeff, photo, ar.test_affines(6)
    self.obs = [ar.observe(self.fm, coeff[f], photo, self.aff[f], R=ar.rotation(coeff[f, 224:227])) for f in range(6)]
    self.star = {}


@pytest.fixture(scope="module")
def ctx():
  import torch
  coeff = np.load(os.path.join(GOLDEN, "bfm_appearance.npz"))["coeff"]
  photo = ar.smooth_photo()
  return {"torch": torch, "coeff": coeff, "photo": photo, 252: Case(252, coeff, photo), 1200: Case(1200, coeff, photo)}


def batch(a, frames):
  return np.stack([a[i % 6] for i in range(frames)])


def judge(case, key, f, obs, p_dev, init):
  """The two bounds of the module docstring for one frame."""
  fm = case.fm
  if (key, f) not in case.star:
    ps, rep, info = ar.fit(fm, obs, init=init, gtol=0.0, max_trials=400)
    assert rep[0] == 2 and rep[3] < GTOL * rep[2], rep                # it went below gtol E before the float64 floor stopped it
    case.star[(key, f)] = ps
  p_star = case.star[(key, f)]
  _, g, E = ar.normal_equations(fm, obs, p_dev)
  gmax = np.abs(g).max()
  A, _, _ = ar.normal_equations(fm, obs, p_star)
  hinv = np.abs(np.linalg.inv(A)).sum(axis=1).max()
  dp = np.abs(p_dev - p_star).max()
  print("%s frame %d: helper |g| %.3e (<= %.3e); |p - p*| %.3e (<= %.3e); E %.6g" % (key, f, gmax, 1.01 * GTOL * E, dp, 2 * hinv * GTOL * E, E))
  assert gmax <= 1.01 * GTOL * E
  assert dp <= 2 * hinv * GTOL * E


def check_rows_repeat(coeff, report, p):
  for i in range(6, coeff.shape[0]):
    assert np.array_equal(coeff[i], coeff[i % 6]) and np.array_equal(report[i], report[i % 6]) and np.array_equal(p[i], p[i % 6]), i


def run(case, *args, **kw):
  coeff, report = case.fitter.fit_appearance(*args, **kw)
  return coeff.cpu().numpy(), report.cpu().numpy(), case.fitter.last_appearance.cpu().numpy()


@pytest.mark.parametrize("frames", [1, 3, 7])
@pytest.mark.parametrize("nver", [252, 1200])
def test_observe(ctx, nver, frames):
  """sh, weight, observed within 1e-10 of the helper (a handful of float64 operations on values <= 255, the normalisation included);
  weight exactly 0 where the helper's is; a shared photo and a per-frame photo give the same bits."""
  case = ctx[nver]
  c, aff = batch(ctx["coeff"], frames), batch(case.aff, frames)
  sh, w, obs = (t.cpu().numpy() for t in case.fitter.observe(c, ctx["photo"], aff))
  assert sh.shape == (frames, nver, 9) and w.shape == (frames, nver) and obs.shape == (frames, nver, 3)
  for i in range(frames):
    hs, hw, ho = case.obs[i % 6]
    errs = (np.abs(sh[i] - hs).max(), np.abs(w[i] - hw).max(), np.abs(obs[i] - ho).max())
    print("%d vertices, frame %d: sh %.3e, weight %.3e, observed %.3e; %d visible, %d outside the photo" %
          (nver, i, errs[0], errs[1], errs[2], int((hw > 0).sum()), int((np.abs(ho).sum(axis=1) == 0).sum())))
    assert max(errs) <= 1e-10
    assert np.all(w[i][hw == 0] == 0) and np.all(w[i][hw > 0] > 0)
    assert np.any(np.abs(ho).sum(axis=1) == 0) and np.any(hw > 0)
  per = case.fitter.observe(c, np.tile(ctx["photo"], (frames, 1, 1, 1)), aff)
  for a, b in zip((sh, w, obs), per):
    assert np.array_equal(a, b.cpu().numpy())
  if frames == 3:                                              # a mask scales the weight; one affine row serves every frame
    mask = np.linspace(0.0, 2.0, nver)
    _, wm, _ = case.fitter.observe(c, ctx["photo"], aff, vertex_weights=mask)
    assert np.abs(wm.cpu().numpy() - w * mask).max() <= 1e-12
    one = case.fitter.observe(c[:1], ctx["photo"], aff[0])
    assert np.array_equal(one[2].cpu().numpy()[0], obs[0])


def test_observe_photo_border(ctx):
  """The device's own border rule, at the right and the bottom edge: a vertex placed exactly on px = W-1 (py = H-1) is inside and takes
  the last column's (row's) pixels, the clamp to the last cell with fraction 1; 1e-3 px further out it is outside: observed 0, weight 0.
  a = 1 and an offset found so that the device's projection + offset IS W-1 (H-1) in float64."""
  from voicepuppet_amd.utils.reconstruct_mesh import reconstruct_view
  case = ctx[252]
  photo = ctx["photo"]
  H, W = photo.shape[:2]
  c = ctx["coeff"][:1]
  proj = reconstruct_view(c, case.fitter.model)["face_projection"].cpu().numpy()[0]          # the projection observe computes (same device code)
  v = int(np.flatnonzero(case.obs[0][1] > 0)[0])                                              # a vertex that faces the camera

  def offset(x, target):
    b = target - x
    for _ in range(4):
      if x + b == target:
        return b
      b = np.nextafter(b, b + np.sign(target - (x + b)))
    raise AssertionError("no offset puts %r on %r" % (x, target))

  for axis, edge in ((0, W - 1.0), (1, H - 1.0)):
    mid = 40.0 - np.floor(proj[v, 1 - axis])                                                  # the other coordinate well inside
    aff = np.array([1.0, 0.0, 0.0])
    aff[1 + axis], aff[2 - axis] = offset(proj[v, axis], edge), mid
    px, py = proj[v, 0] + aff[1], proj[v, 1] + aff[2]
    assert (px, py)[axis] == edge
    sh, w, obs = (t.cpu().numpy()[0] for t in case.fitter.observe(c, photo, aff))
    want, inside = ar.bilinear(photo, np.array([px]), np.array([py]))
    print("axis %d: vertex %d at (%.6f, %.6f): observed %s, helper %s, weight %.3e" % (axis, v, px, py, obs[v], want[0], w[v]))
    assert inside[0] and w[v] > 0 and np.abs(obs[v] - want[0]).max() <= 1e-10
    q = np.floor((py, px)[axis])                                                              # on the edge itself: the two edge pixels only
    f = (py, px)[axis] - q
    line = photo[int(q):int(q) + 2, W - 1] if axis == 0 else photo[H - 1, int(q):int(q) + 2]
    assert np.abs(obs[v] - ((1 - f) * line[0].astype(np.float64) + f * line[1])).max() <= 1e-10
    aff[1 + axis] += 1e-3
    sh, w, obs = (t.cpu().numpy()[0] for t in case.fitter.observe(c, photo, aff))
    assert w[v] == 0 and np.all(obs[v] == 0)


@pytest.mark.parametrize("frames", [1, 3, 7])
@pytest.mark.parametrize("nver", [252, 1200])
def test_fit(ctx, nver, frames):
  case = ctx[nver]
  c, aff = batch(ctx["coeff"], frames), batch(case.aff, frames)
  coeff, report, p = run(case, c, photo=ctx["photo"], affine=aff)
  print(report[:6])
  assert coeff.shape == (frames, 257) and coeff.dtype == np.float32 and report.shape == (frames, 4) and p.shape == (frames, 107)
  assert np.all(report[:, 0] == 0) and np.all(report[:, 3] <= GTOL * report[:, 2])
  check_rows_repeat(coeff, report, p)
  for f in range(min(frames, 6)):
    judge(case, "fit", f, case.obs[f], p[f], ar.coeff_to_p(c[f]))
    want = ar.p_to_coeff(p[f], c[f]).astype(np.float32)           # float32 of the float64 solution; every other column the input's bits
    assert np.array_equal(coeff[f].view(np.uint32), want.view(np.uint32))
    E = ar.cost(case.fm, case.obs[f], p[f])
    assert abs(report[f, 2] - E) <= 1e-9 * E                       # (the observation itself differs by 1e-10 of 255)


def test_fit_with_given_observation(ctx):
  """observation = (sh, weight, observed) handed in, with a weight on EVERY vertex inside the photo (|n_z|: the synthetic mesh's normals
  point away from the camera over most of the face), so that every slab of the 1200-vertex model carries rows."""
  case = ctx[1200]
  c = batch(ctx["coeff"], 3)
  obs = [(o[0], np.where(np.abs(o[2]).sum(axis=1) > 0, np.abs(ar.geometry(case.fm, c[f], ar.rotation(c[f, 224:227]))[0][:, 2]), 0.0), o[2])
         for f, o in enumerate(case.obs[:3])]
  assert all((o[1] > 0).sum() > 800 for o in obs)
  coeff, report, p = run(case, c, observation=tuple(np.stack([o[k] for o in obs]) for k in range(3)))
  print(report)
  assert np.all(report[:, 0] == 0)
  for f in range(3):
    judge(case, "dense", f, obs[f], p[f], ar.coeff_to_p(c[f]))


def test_batch_invariance(ctx):
  """A frame's coefficients, report and float64 solution are the same bits alone, first and last of 7."""
  case = ctx[1200]
  c, aff = batch(ctx["coeff"], 7), batch(case.aff, 7)
  c[0] = c[6] = ctx["coeff"][2]
  aff[0] = aff[6] = case.aff[2]
  c1, r1, p1 = run(case, ctx["coeff"][2:3], photo=ctx["photo"], affine=case.aff[2:3])
  c7, r7, p7 = run(case, c, photo=ctx["photo"], affine=aff)
  for row in (0, 6):
    assert np.array_equal(c7[row].view(np.uint32), c1[0].view(np.uint32))
    assert np.array_equal(r7[row].view(np.uint64), r1[0].view(np.uint64))
    assert np.array_equal(p7[row].view(np.uint64), p1[0].view(np.uint64))


def test_start_that_rejects(ctx):
  """A start (delta = 5 N(0,1)) from which the HELPER rejects at least one trial before it converges; the device passes the same judgement."""
  case = ctx[252]
  f = REJECT_FRAME
  start = ctx["coeff"][f:f + 1].copy()
  start[0, 144:224] = (5.0 * np.random.default_rng(REJECT_SEED).normal(size=80)).astype(np.float32)
  init = ar.coeff_to_p(start[0])
  ph, rep, info = ar.fit(case.fm, case.obs[f], init=init, gtol=GTOL, max_trials=32)
  print("helper from the far start: status %d, %d trials, %d rejects" % (rep[0], info["trials"], info["rejects"]))
  assert rep[0] == 0 and info["rejects"] >= 1
  coeff, report, p = run(case, ctx["coeff"][f:f + 1], photo=ctx["photo"], affine=case.aff[f:f + 1], init=start)
  print(report)
  assert report[0, 0] == 0
  judge(case, "far", f, case.obs[f], p[0], init)


def test_statuses(ctx):
  torch = ctx["torch"]
  case = ctx[252]
  c, aff = batch(ctx["coeff"], 3), batch(case.aff, 3)
  coeff, report, p = run(case, c, photo=ctx["photo"], affine=aff, max_trials=2)
  assert np.all(report[:, 0] == 1)
  for f in range(3):                                                # the report is that of the returned point
    A, g, E = ar.normal_equations(case.fm, case.obs[f], p[f])
    assert abs(report[f, 2] - E) <= 1e-9 * E and abs(report[f, 3] - np.abs(g).max()) <= 1e-7 * np.abs(g).max()
  clean = run(case, c, photo=ctx["photo"], affine=aff)
  sh, w, obs = case.fitter.observe(c, ctx["photo"], aff)
  visible = int(torch.nonzero(w[1] > 0)[0])
  obs = obs.clone()
  obs[1, visible, 2] = float("nan")
  coeff, report, p = run(case, c, observation=(sh, w, obs))
  assert report[1, 0] == 3 and report[1, 1] == 0 and np.isnan(report[1, 2]) and np.isnan(report[1, 3])
  assert np.array_equal(coeff[1].view(np.uint32), c[1].view(np.uint32)) and np.array_equal(p[1], ar.coeff_to_p(c[1]))
  for f in (0, 2):
    assert np.array_equal(coeff[f], clean[0][f]) and np.array_equal(report[f], clean[1][f]) and np.array_equal(p[f], clean[2][f])
  away = aff.copy()
  away[2, 1] = 1000.0                                               # frame 2's face lies wholly outside the photo
  coeff, report, p = run(case, c, photo=ctx["photo"], affine=away)
  assert report[2, 0] == 3 and np.array_equal(coeff[2].view(np.uint32), c[2].view(np.uint32))
  for f in (0, 1):
    assert np.array_equal(coeff[f], clean[0][f]) and np.array_equal(report[f], clean[1][f])


def test_against_reconstruction_kernel(ctx):
  """With the fitted float32 coefficients, reconstruct_view's face_color against `observed` under `weight` reproduces the report's data
  term to 1e-4 relative: the float32 rounding of delta, 6e-8 x sum |B| ~ 100, moves a colour by about 1e-5 grey levels."""
  from voicepuppet_amd.utils.reconstruct_mesh import reconstruct_view
  case = ctx[1200]
  c, aff = batch(ctx["coeff"], 3), batch(case.aff, 3)
  sh, w, obs = case.fitter.observe(c, ctx["photo"], aff)
  coeff, report = case.fitter.fit_appearance(c, observation=(sh, w, obs))
  p = case.fitter.last_appearance
  col = reconstruct_view(coeff, case.fitter.model)["face_color"]
  data = (w[:, :, None] * (col - obs) ** 2).sum(dim=(1, 2)) / (3.0 * w.sum(dim=1))
  want = report[:, 2] - (p ** 2).sum(dim=1)                          # lam_tex = lam_gamma = 1
  rel = ((data - want).abs() / want).cpu().numpy()
  print("data term: reconstruction %s, report %s, relative difference %s" % (data.cpu().numpy(), want.cpu().numpy(), rel))
  assert np.all(rel <= 1e-4)


def test_enroll(ctx):
  from voicepuppet_amd import bfmfit
  case = ctx[252]
  g = dict(np.load(os.path.join(GOLDEN, "bfm_fit.npz")))
  xy = fr.photo_landmarks(g["landmarks_2d"][0], 1.7, (130.0, 60.0))
  image = ar.smooth_photo(480, 640, seed=5)
  plain = case.fitter.enroll(xy, 480, 640, g["lm3d68"])
  assert set(plain) == {"bfmcoeff", "transform_params", "center_x", "center_y", "ratio"}
  assert np.all(plain["bfmcoeff"][:, 144:224] == 0) and np.all(plain["bfmcoeff"][:, 227:254] == 0)
  got = case.fitter.enroll(xy, 480, 640, g["lm3d68"], image=image)
  rep = case.fitter.last_appearance_report.cpu().numpy()
  print("enroll: appearance report", rep)
  assert set(got) == set(plain) and rep.shape == (1, 4) and rep[0, 0] in (0, 1, 2)
  lm_new, _ = bfmfit.preprocess_landmarks(bfmfit.crop_alignment(xy, 480, 640)[0], g["lm3d68"])
  coeff, _ = case.fitter.fit(lm_new.reshape(1, 68, 2))
  coeff, _ = case.fitter.fit_appearance(coeff, photo=image, affine=bfmfit.photo_affine(xy, 480, 640, g["lm3d68"]))
  assert np.array_equal(got["bfmcoeff"].view(np.uint32), coeff.cpu().numpy().view(np.uint32))
  assert np.any(got["bfmcoeff"][:, 144:224] != 0) and np.any(got["bfmcoeff"][:, 227:254] != 0)
  for k in ("transform_params", "center_x", "center_y", "ratio"):
    assert np.array_equal(got[k], plain[k])
  assert np.array_equal(got["bfmcoeff"][:, :144], plain["bfmcoeff"][:, :144])


def test_cli_with_image(ctx, tmp_path, monkeypatch, capsys):
  """fit_landmarks.py --photo LANDMARKS --image FILE (no --size): the npz holds fitted texture and lighting columns, bit-equal to
  enroll(image=) on the decoded pixels, and the summary line gains the appearance status and the RMS colour residual, which is the square
  root of the helper's data term at the returned point."""
  from PIL import Image
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  from test_gpu_bfm_fit import write_bfm_assets
  case = ctx[252]
  monkeypatch.chdir(tmp_path)
  g = dict(np.load(os.path.join(GOLDEN, "bfm_fit.npz")))
  xy = fr.photo_landmarks(g["landmarks_2d"][0], 1.7, (130.0, 60.0))
  write_bfm_assets(case.fm, g["lm3d68"])
  np.savetxt("landmarks.txt", xy.reshape(1, 136), delimiter=",", fmt="%.10f")
  image = ar.smooth_photo(480, 640, seed=5)
  Image.fromarray(image).save("photo.png")
  fl.main(["--photo", "landmarks.txt", "--image", "photo.png", "--out", "photo.npz", "--lam_tex", "2", "--lam_gamma", "0.5"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  assert "1 frames" in line and "appearance status " in line and "grey levels" in line
  got = np.load("photo.npz")
  want = case.fitter.enroll(np.loadtxt("landmarks.txt", delimiter=",").reshape(68, 2), 480, 640, g["lm3d68"], image=image, lam_tex=2.0, lam_gamma=0.5)
  assert set(got.files) == set(want) and np.array_equal(got["bfmcoeff"].view(np.uint32), want["bfmcoeff"].view(np.uint32))
  assert "appearance status %d," % int(case.fitter.last_appearance_report.cpu().numpy()[0, 0]) in line
  from voicepuppet_amd import bfmfit
  aff = bfmfit.photo_affine(np.loadtxt("landmarks.txt", delimiter=",").reshape(68, 2), 480, 640, g["lm3d68"])
  obs = ar.observe(case.fm, want["bfmcoeff"][0], image, aff, R=ar.rotation(want["bfmcoeff"][0, 224:227]))
  rms = np.sqrt(ar.data_term(case.fm, obs, case.fitter.last_appearance.cpu().numpy()[0]))
  shown = float(line.split("colour RMS ")[1].split(" ")[0])
  print("colour RMS: line %.2f, helper %.4f" % (shown, rms))
  assert abs(shown - rms) <= 0.006                                  # two printed decimals

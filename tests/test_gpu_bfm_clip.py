"""Device joint fit of a clip (voicepuppet_amd.bfmfit.FaceFitter.fit_clip; csrc/bfm_clip.hip: vp_bfmfit_clip) against the float64
restatement tests/bfm_clip_ref.py.  252 vertices; inputs and the restatement's solutions from tests/golden/bfm_clip.npz
(tests/golden/make_bfm_clip_golden.py).

One clip step (max_trials = 1 from given params: the point returned is the first trial point, accepted): the step d and the trial E
against the restatement at the same point and mu = 1e-3, within 1e-9 relative (the float64-sum tolerance of test_gpu_bfm_appearance.py),
for T in {1, 2, 3, 17} (17: one frame past a 16-row slice), without and with coupling.
Full fits are judged as tests/test_gpu_bfm_fit.py judges its own (gtol = 1e-6), in float64 on the host:
  stationarity  |g|_inf of the RESTATEMENT at the device's parameters <= 1.01 gtol
  agreement     |p_dev - p*|_inf <= 2 |H^-1|_inf gtol, p* = the restatement run until it stalls (gtol = 0), H the dense clip matrix at p*
  E             the reported E within 1e-9 relative of the restatement's cost at the device's parameters
Only a case the restatement itself carries to status 0 with a margin is asserted as converged: T = 8 without coupling (its floor, run with
gtol = 0, is 3.0e-7).  T = 40 with (200, 20000, 20000) is not: test_golden_clip_coupled says why."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_clip_ref as cr  # noqa: E402
import bfm_fit_ref as fr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_clip.npz")
GTOL = 1e-6
SMOOTH = (200.0, 20000.0, 20000.0)
ZERO = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def ctx():
  import torch
  from voicepuppet_amd.bfmfit import FaceFitter
  g = dict(np.load(GOLDEN))
  fm = br.synthetic_facemodel(seed=int(g["model_seed"]))
  assert tuple(g["smooth"]) == SMOOTH
  return {"torch": torch, "fm": fm, "tbl": fr.table(fm), "g": g, "fitter": FaceFitter(fm)}


def run(ctx, lm, **kw):
  coeff, report = ctx["fitter"].fit_clip(lm, **kw)
  return coeff.cpu().numpy(), report.cpu().numpy(), ctx["fitter"].last_params.cpu().numpy()


@pytest.mark.parametrize("smooth", [ZERO, SMOOTH], ids=["uncoupled", "coupled"])
@pytest.mark.parametrize("T", [1, 2, 3, 17])
def test_one_clip_step(ctx, T, smooth):
  g, tbl = ctx["g"], ctx["tbl"]
  lm, start = g["noisy40"][:T], g["start40"][:T].copy()
  start[:, :80] = start[0, :80]
  want = cr.clip_step(tbl, start, lm, 1e-3, lam_smooth=smooth)
  e0, e1 = cr.clip_cost(tbl, start, lm, lam_smooth=smooth), cr.clip_cost(tbl, want, lm, lam_smooth=smooth)
  assert e1 < e0                                            # the restatement accepts this step: the device must return it
  coeff, report, p = run(ctx, lm, params=start, lam_smooth=smooth, max_trials=1)
  d_dev, d_ref = p - start, want - start
  err = np.abs(d_dev - d_ref).max() / np.abs(d_ref).max()
  print("T %d %s: |d| %.3e, step error %.3e relative; E %.12g against %.12g; report %s" % (T, smooth, np.abs(d_ref).max(), err, report[0, 2], e1, report[0]))
  assert report.shape == (1, 4) and report[0, 0] in (0, 1) and report[0, 1] == 1
  assert err <= 1e-9
  assert abs(report[0, 2] - e1) <= 1e-9 * e1
  assert np.all(p[:, :80] == p[0, :80])
  assert np.array_equal(coeff, fr.p_to_coeff(p).astype(np.float32))


def judge(ctx, name, lm, p_dev, report, p_star, smooth):
  tbl = ctx["tbl"]
  gmax = np.abs(cr.clip_gradient(tbl, p_dev, lm, lam_smooth=smooth)).max()
  A, _ = cr.clip_system(tbl, p_star, lm, lam_smooth=smooth)
  hinv = np.abs(np.linalg.inv(A)).sum(axis=1).max()
  dp = np.abs(p_dev - p_star).max()
  e = cr.clip_cost(tbl, p_dev, lm, lam_smooth=smooth)
  print("%s: report %s; restatement |g| %.3e (<= %.3e); |p - p*| %.3e (<= %.3e); E %.12g against %.12g"
        % (name, report, gmax, 1.01 * GTOL, dp, 2 * hinv * GTOL, report[2], e))
  assert report[0] == 0 and report[3] <= GTOL
  assert gmax <= 1.01 * GTOL
  assert dp <= 2 * hinv * GTOL
  assert abs(report[2] - e) <= 1e-9 * e


def test_full_fit_uncoupled(ctx):
  """T = 8, sigma = 0.5: converges; the cost is not above that of fit_sequence's schedule nor of the start."""
  g, tbl = ctx["g"], ctx["tbl"]
  coeff, report, p = run(ctx, g["noisy8"], params=g["start8"])
  judge(ctx, "T = 8", g["noisy8"], p, report[0], g["star8"], ZERO)
  assert np.all(p[:, :80] == p[0, :80])
  assert np.array_equal(coeff, fr.p_to_coeff(p).astype(np.float32))
  assert report[0, 2] <= cr.clip_cost(tbl, g["seq8"], g["noisy8"]) and report[0, 2] <= cr.clip_cost(tbl, g["start8"], g["noisy8"])


def test_golden_clip_coupled(ctx):
  """T = 40, sigma = 1.0, lam_smooth = (200, 20000, 20000): the first-difference error to the clean landmarks is below the restatement's
  with zero smoothing and below the noise's own (the condition of tests/test_bfm_clip_host.py, on the device's solution).
  NOT asserted: status 0.  The restatement reports status 0 here, but by a coin toss: its 25th accepted step has a predicted gain of
  1.4e-14 in E = 8110 while its measured dE scatters by +-3e-12 (ten rejections at +1.5e-12 .. +3.8e-12, then -1.4e-12 and the step is
  taken; traced on the CPU).  That is the float64 floor of "E falls" (DESIGN.md section 9), and a case the helper carries to gtol only by
  the sign of its rounding tests nothing.  Measured on the device: status 2 after 24 accepted steps at |g|_inf = 3.35e-6 (the angle rows),
  E = 8110.50072, the restatement's E.  What holds at the floor, and is asserted: status 0 or 2; E within 1e-9 relative of the
  restatement's cost at the device's parameters and of the restatement's own minimum (both lie within g^T H^-1 g, below 1e-12 relative,
  of the minimum); and H (p_dev - p*) = g(p_dev) - g(p*) to first order: |p_dev - p*|_inf <= 2 |H^-1|_inf max(|g(p_dev)|_inf, gtol)."""
  g, tbl = ctx["g"], ctx["tbl"]
  lm = g["noisy40"]
  coeff, report, p = run(ctx, lm, params=g["start40"], lam_smooth=SMOOTH)
  gmax = np.abs(cr.clip_gradient(tbl, p, lm, lam_smooth=SMOOTH)).max()
  A, _ = cr.clip_system(tbl, g["star40_smooth"], lm, lam_smooth=SMOOTH)
  hinv = np.abs(np.linalg.inv(A)).sum(axis=1).max()
  dp, e = np.abs(p - g["star40_smooth"]).max(), cr.clip_cost(tbl, p, lm, lam_smooth=SMOOTH)
  print("T = 40: report %s; restatement |g| %.3e; |p - p*| %.3e (<= %.3e); E %.12g against %.12g, restatement's minimum %.12g"
        % (report[0], gmax, dp, 2 * hinv * max(gmax, GTOL), report[0, 2], e, g["rep40_smooth"][2]))
  assert report[0, 0] in (0, 2) and report[0, 1] >= 1
  assert abs(report[0, 2] - e) <= 1e-9 * e and abs(report[0, 2] - g["rep40_smooth"][2]) <= 1e-9 * e
  assert abs(report[0, 3] - gmax) <= 1e-9                     # 136 terms |J| |r| <= 1e3 each per row: 1e-11 is g's float64 rounding
  assert dp <= 2 * hinv * max(gmax, GTOL)
  assert np.all(p[:, :80] == p[0, :80])
  err, fd = cr.landmark_errors(tbl, p, g["clean40"])
  _, fd_zero = cr.landmark_errors(tbl, g["sol40_zero"], g["clean40"])
  _, fd_noise = cr.point_errors(g["noisy40"], g["clean40"])
  print("first-difference error %.4f px (zero smoothing %.4f, noise %.4f); error to clean %.4f px" % (fd, fd_zero, fd_noise, err))
  assert fd < fd_zero and fd < fd_noise


def test_default_start_is_fit_sequence_rounds_0(ctx):
  """Without params the start is fit_sequence(rounds=0)'s: the same bits as handing that in; and E does not rise from it."""
  g, tbl, fitter = ctx["g"], ctx["tbl"], ctx["fitter"]
  lm = g["noisy8"][:5]
  fitter.fit_sequence(lm, rounds=0)
  start = fitter.last_params.cpu().numpy()
  c1, r1, p1 = run(ctx, lm, max_trials=6)
  c2, r2, p2 = run(ctx, lm, params=start, max_trials=6)
  assert np.array_equal(p1, p2) and np.array_equal(r1, r2) and np.array_equal(c1, c2)
  assert r1[0, 2] <= cr.clip_cost(tbl, start, lm)


def test_batch_invariance(ctx):
  """Clips of lengths (1, 2, 5, 3) in one call give the bits of each clip alone."""
  g = ctx["g"]
  lengths = (1, 2, 5, 3)
  lm, start = g["noisy40"][:11], g["start40"][:11]
  w = np.ones((11, 68))
  w[3, 10] = w[7, 40] = 0.0
  kw = dict(lam_smooth=SMOOTH, max_trials=5)
  coeff, report, p = run(ctx, lm, clip_lengths=lengths, params=start, weights=w, **kw)
  assert report.shape == (4, 4)
  a = 0
  for c, n in enumerate(lengths):
    c1, r1, p1 = run(ctx, lm[a:a + n], params=start[a:a + n], weights=w[a:a + n], **kw)
    assert np.array_equal(coeff[a:a + n].view(np.uint32), c1.view(np.uint32)), c
    assert np.array_equal(report[c].view(np.uint64), r1[0].view(np.uint64)), c
    assert np.array_equal(p[a:a + n].view(np.uint64), p1.view(np.uint64)), c
    a += n


def test_statuses_1_and_3(ctx):
  g, tbl = ctx["g"], ctx["tbl"]
  lm, start = g["noisy40"][:5].copy(), g["start40"][:5].copy()
  coeff, report, p = run(ctx, lm, clip_lengths=(3, 2), params=start, max_trials=2)
  assert np.all(report[:, 0] == 1) and np.all(report[:, 1] <= 2)
  for a, b, c in ((0, 3, 0), (3, 5, 1)):
    e = cr.clip_cost(tbl, p[a:b], lm[a:b])
    gm = np.abs(cr.clip_gradient(tbl, p[a:b], lm[a:b])).max()
    assert abs(report[c, 2] - e) <= 1e-9 * e and abs(report[c, 3] - gm) <= 1e-9 * gm
  # max_trials = 0: E and |g| at the start values, nothing moves
  c0, r0, p0 = run(ctx, lm[:3], params=start[:3], max_trials=0)
  s3 = start[:3].copy()
  s3[:, :80] = s3[0, :80]
  assert r0[0, 0] == 1 and r0[0, 1] == 0 and np.array_equal(p0, s3)
  assert abs(r0[0, 2] - cr.clip_cost(tbl, s3, lm[:3])) <= 1e-9 * r0[0, 2]
  # a NaN landmark: that clip alone gets status 3, its start values and template go back
  bad = lm.copy()
  bad[4, 30, 0] = np.nan
  tmpl = np.random.default_rng(9).normal(size=(5, 257)).astype(np.float32)
  cb, rb, pb = run(ctx, bad, clip_lengths=(3, 2), params=start, init=tmpl, max_trials=2)
  cg, rg, pg = run(ctx, lm, clip_lengths=(3, 2), params=start, init=tmpl, max_trials=2)
  assert rb[1, 0] == 3 and rb[1, 1] == 0 and np.isnan(rb[1, 2]) and np.isnan(rb[1, 3])
  assert np.array_equal(cb[3:].view(np.uint32), tmpl[3:].view(np.uint32)) and np.array_equal(pb[3:], start[3:])
  assert np.array_equal(cb[:3], cg[:3]) and np.array_equal(rb[0], rg[0]) and np.array_equal(pb[:3], pg[:3])
  untouched = np.ones(257, bool)
  untouched[:144] = untouched[224:227] = untouched[254:] = False
  assert np.array_equal(cg[:, untouched].view(np.uint32), tmpl[:, untouched].view(np.uint32))


def test_refusals(ctx):
  """Python refuses what it can see; the library refuses the rest on the host, before anything is enqueued."""
  from voicepuppet_amd import _lib
  g, fitter = ctx["g"], ctx["fitter"]
  lm = g["noisy8"]
  for kw in (dict(clip_lengths=(3, 4)), dict(clip_lengths=(8, 0)), dict(clip_lengths=()), dict(lam_smooth=(1, 2)), dict(lam_smooth=(0, -1, 0)),
             dict(lam_smooth=(0, float("nan"), 0))):
    with pytest.raises(ValueError):
      fitter.fit_clip(lm, **kw)
  with pytest.raises(RuntimeError, match="vp_bfmfit_clip"):
    fitter.fit_clip(lm, params=g["start8"], max_trials=-1)
  with pytest.raises(RuntimeError, match="vp_bfmfit_clip"):
    fitter.fit_clip(lm, params=g["start8"], lam_id=-1.0)
  assert _lib.lib().vp_bfmfit_clip_workspace_bytes(8, 9) == 0


def test_cli_joint(ctx, tmp_path, monkeypatch, capsys):
  """fit_landmarks.py --clip ... --joint --smooth ...: a bfmcoeff.txt that BFMCoeffLoader reads back, one identity for the clip; without
  --joint the file is what it was (fit_sequence's)."""
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  from voicepuppet_amd.generator.loader import BFMCoeffLoader
  import test_bfm_fit_host as host
  from test_gpu_bfm_fit import write_bfm_assets
  monkeypatch.chdir(tmp_path)
  g6 = dict(np.load(os.path.join(os.path.dirname(GOLDEN), "bfm_fit.npz")))
  fm = br.synthetic_facemodel(seed=int(g6["model_seed"]), smooth=True)
  xy = np.stack([fr.photo_landmarks(g6["landmarks_2d"][f], 2.0, (100.0, 40.0)) for f in range(6)])
  write_bfm_assets(fm, host.unit_scale_lm3d(g6, xy[0]))
  np.savetxt("landmarks.txt", xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  fl.main(["--clip", "landmarks.txt", "--size", "480", "640", "--out", "joint.txt", "--joint", "--smooth", "10", "100", "100", "--max_trials", "16"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  assert "6 frames" in line and "joint status" in line and "reprojection mean" in line
  rows = BFMCoeffLoader().get_data("joint.txt")
  assert rows.shape == (6, 257) and rows.dtype == np.float32 and np.all(np.isfinite(rows))
  assert np.all(rows[:, :80] == rows[0, :80]) and np.all(rows[:, 144:224] == 0) and np.all(rows[:, 227:254] == 0)
  fl.main(["--clip", "landmarks.txt", "--size", "480", "640", "--out", "plain.txt", "--rounds", "1", "--id_steps", "1"])
  assert "joint" not in capsys.readouterr().out.strip().splitlines()[-1]
  plain = BFMCoeffLoader().get_data("plain.txt")
  assert plain.shape == (6, 257) and not np.array_equal(plain, rows)

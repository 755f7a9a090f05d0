"""CPU checks of the joint clip fit's definition (tests/bfm_clip_ref.py, the float64 restatement of vp_bfmfit_clip) and of the C ABI's host
side: the gradient against finite differences, the arrowhead elimination against the dense solve, T = 1 against the per-frame fit, the cost
property, the smoothing condition on tests/golden/bfm_clip.npz, and what the library refuses before anything is enqueued.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_clip_ref as cr  # noqa: E402
import bfm_fit_ref as fr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_clip.npz")
SMOOTH = (200.0, 20000.0, 20000.0)
NEW = {"vp_bfmfit_clip_workspace_bytes", "vp_bfmfit_clip"}


@pytest.fixture(scope="module")
def ctx():
  g = dict(np.load(GOLDEN))
  fm = br.synthetic_facemodel(seed=int(g["model_seed"]))
  return {"g": g, "fm": fm, "tbl": fr.table(fm)}


def test_golden_is_the_generator_s_case(ctx):
  g = ctx["g"]
  fm, tbl, truth, clean, noisy = cr.synthetic_clip(8, 0.5, int(g["seed"]), int(g["model_seed"]), int(g["coeff_seed"]))
  assert np.array_equal(noisy, g["noisy8"]) and np.array_equal(clean, g["clean8"])
  assert np.allclose(g["model_checksum"], [fm.idBase.sum(), fm.exBase.sum(), fm.meanshape.sum(), float(fm.keypoints.sum())], rtol=1e-12)
  assert tuple(g["smooth"]) == SMOOTH


def test_gradient_is_the_finite_difference_of_clip_cost(ctx):
  """g = half the gradient of E (the convention g = J^T W r): central differences, h = 1e-6, on 40 of the 290 unknowns of a 3-frame clip."""
  g, tbl = ctx["g"], ctx["tbl"]
  lm, ps = g["noisy40"][:3], g["start40"][:3].copy()
  ps[:, :80] = ps[0, :80]
  grad = cr.clip_gradient(tbl, ps, lm, lam_smooth=SMOOTH)
  _, gd = cr.clip_system(tbl, ps, lm, lam_smooth=SMOOTH)
  assert np.array_equal(grad, gd)
  h = 1e-6
  rng = np.random.default_rng(1)
  picks = np.concatenate([rng.choice(80, 8, replace=False), 80 + rng.choice(210, 26, replace=False), [80 + 64, 80 + 69, 80 + 70 + 66, 80 + 140 + 67, 80 + 209, 80]])
  for i in picks:
    def at(delta):
      q = ps.copy()
      if i < 80:
        q[:, i] += delta
      else:
        q[(i - 80) // 70, 80 + (i - 80) % 70] += delta
      return cr.clip_cost(tbl, q, lm, lam_smooth=SMOOTH)
    fd = (at(h) - at(-h)) / (4 * h)
    assert abs(fd - grad[i]) <= 1e-5 * max(1.0, abs(grad[i])), (i, fd, grad[i])


@pytest.mark.parametrize("T", [1, 2, 3, 9])
@pytest.mark.parametrize("smooth", [(0.0, 0.0, 0.0), SMOOTH, (3.0, 0.0, 50.0)])
def test_elimination_is_the_dense_solve(ctx, T, smooth):
  g, tbl = ctx["g"], ctx["tbl"]
  lm, ps = g["noisy40"][:T], g["start40"][:T].copy()
  ps[:, :80] = ps[0, :80]
  s = cr.smooth_vector(smooth)
  As, gs, _ = cr.frame_systems(tbl, ps, lm)
  cg = cr.coupling_gradient(ps, s)
  for mu in (1e-3, 1e-9):
    a1, q1 = cr.dense_solve(As, gs, cg, s, mu)
    a2, q2 = cr.arrowhead_solve(As, gs, cg, s, mu)
    A, gg = cr.assemble(As, gs, cg, s)
    d = -np.linalg.solve(A + mu * np.diag(np.diag(A)), gg)
    want = np.concatenate([a2, q2.reshape(-1)])
    err = np.abs(want - d).max() / np.abs(d).max()
    print("T %d smooth %s mu %g: elimination against np.linalg.solve %.3e relative" % (T, smooth, mu, err))
    assert err <= 1e-10
    assert np.abs(np.concatenate([a1, q1.reshape(-1)]) - d).max() <= 1e-10 * np.abs(d).max()


def test_one_frame_without_coupling_is_the_per_frame_fit(ctx):
  g, tbl = ctx["g"], ctx["tbl"]
  lm = g["noisy8"][:1]
  p1, rep1 = fr.fit(tbl, lm[0], free="all", max_iters=100)
  # with the dense solver the arithmetic is the per-frame fit's own (the same matrix, the same Cholesky): the same iterates
  pc, repc, trials = cr.fit_clip(tbl, lm, np.zeros((1, 150)), max_trials=200, solver=cr.dense_solve)
  print(rep1, repc, trials)
  assert rep1[0] == 0 and repc[0] == 0 and repc[1] == rep1[1]
  assert np.array_equal(pc[0], p1) and abs(repc[2] - rep1[2]) <= 1e-12 * rep1[2]
  assert cr.clip_cost(tbl, pc, lm) == fr.total_cost(tbl, pc, lm)


def test_cost_does_not_rise_from_the_fit_sequence_result(ctx):
  """The accept rule only takes steps that lower E: from fit_sequence's own result (its default schedule) and from rounds = 0."""
  g, tbl = ctx["g"], ctx["tbl"]
  lm = g["noisy8"]
  for name in ("seq8", "start8"):
    e0 = fr.total_cost(tbl, g[name], lm)
    ps, rep, trials = cr.fit_clip(tbl, lm, g[name], max_trials=64)
    print("%s: E %.6f -> %.6f, report %s, %d trials" % (name, e0, rep[2], rep, trials))
    assert rep[0] == 0 and rep[2] <= e0 and abs(rep[2] - cr.clip_cost(tbl, ps, lm)) <= 1e-12 * rep[2]
  assert np.array_equal(ps, g["sol8"]) and np.array_equal(rep, g["rep8"])


def test_smoothing_lowers_the_first_difference_error(ctx):
  """T = 40, sigma = 1.0: with lam_smooth = (200, 20000, 20000) the first-difference error to the clean landmarks is below that with zeros
  and below the noise's own.  Measured: noise 1.781 px, zeros 1.264 px, (200, 20000, 20000) 0.915 px; error to the
  clean landmarks 1.264, 0.928, 0.765 px.  The solutions are the golden file's; one LM step from each confirms it is the restatement's
  (stationary: the converged one within gtol)."""
  g, tbl = ctx["g"], ctx["tbl"]
  clean, noisy = g["clean40"], g["noisy40"]
  _, fd_noise = cr.point_errors(noisy, clean)
  e_zero, fd_zero = cr.landmark_errors(tbl, g["sol40_zero"], clean)
  e_s, fd_s = cr.landmark_errors(tbl, g["sol40_smooth"], clean)
  print("first-difference error, px: noise %.4f, zero smoothing %.4f, %s %.4f; to clean: %.4f, %.4f" % (fd_noise, fd_zero, SMOOTH, fd_s, e_zero, e_s))
  assert fd_s < fd_zero and fd_s < fd_noise
  assert np.allclose(g["errors40"][[0, 2, 3], 1], [fd_noise, fd_zero, fd_s], rtol=1e-9)
  assert g["rep40_smooth"][0] == 0 and g["rep40_zero"][0] == 2
  assert np.abs(cr.clip_gradient(tbl, g["sol40_smooth"], noisy, lam_smooth=SMOOTH)).max() <= 1e-6
  assert np.all(g["sol40_smooth"][:, :80] == g["sol40_smooth"][0, :80])


def test_abi_exports_and_refusals():
  """The header declares the two names, the library exports them and the binding knows them; every refusal happens on the host (the
  pointers are host dummies: nothing is launched)."""
  from voicepuppet_amd import _lib
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header))
  assert NEW <= declared and NEW <= set(_lib.exported_symbols())
  assert "bfm_clip.hip" in open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  lib = _lib.lib()
  for name in NEW:
    assert getattr(lib, name).argtypes is not None, name
  size = lib.vp_bfmfit_clip_workspace_bytes
  assert size(0, 1) == 0 and size(5, 0) == 0 and size(2, 3) == 0
  assert size(11, 4) > size(11, 1) > size(10, 1) > 10 * 70 * 151 * 8
  buf = (ctypes.c_ubyte * 4096)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  m = _lib.BfmModel()
  m.nver, m.ntri = 252, 442
  for k in ("meanshape", "idBase", "exBase", "meantex", "texBase", "tri", "point_buf"):
    setattr(m, k, ctypes.addressof(buf))
  kp = (ctypes.c_int * 68)(*range(68))

  def call(offsets=(0, 3, 5), clips=2, smooth=(0.0, 0.0, 0.0), lam_id=1.0, gtol=1e-6, max_trials=4, ws=1 << 40, keypoints=kp, lm=p, model=m):
    off = (ctypes.c_int * len(offsets))(*offsets)
    sm = (ctypes.c_double * 3)(*smooth)
    return lib.vp_bfmfit_clip(ctypes.byref(model), keypoints, 0, lm, None, 0, off, clips, p, p, lam_id, 1.0, sm, gtol, max_trials, p, p, p, ws, None)

  def refused(what, **kw):
    assert call(**kw) == -1, what
    msg = lib.vp_last_error()
    assert b"vp_bfmfit_clip" in msg, (what, msg)
    return msg

  assert b"increase" in refused("a clip of 0 frames", offsets=(0, 3, 3))
  assert b"increase" in refused("offsets that fall", offsets=(0, 3, 2))
  assert b"clip_offsets[0]" in refused("first offset", offsets=(1, 3, 5))
  assert b"lam_smooth[1]" in refused("negative smoothing weight", smooth=(0.0, -1.0, 0.0))
  refused("nan smoothing weight", smooth=(float("nan"), 0.0, 0.0))
  refused("negative lam", lam_id=-1.0)
  refused("negative gtol", gtol=-1.0)
  refused("max_trials", max_trials=-1)
  refused("clips", clips=0)
  refused("no landmarks", lm=None)
  assert b"workspace too small" in refused("short workspace", ws=size(5, 2) - 1)
  bad_kp = (ctypes.c_int * 68)(*range(68))
  bad_kp[5] = 252
  assert b"keypoint 5" in refused("keypoint", keypoints=bad_kp)
  empty = _lib.BfmModel()
  empty.nver = 252
  refused("empty model", model=empty)


def test_python_surface_and_docs():
  """fit_clip's signature is the documented one; the documents state the energy, that lam_smooth is untuned, and the cost of a step."""
  import inspect
  from voicepuppet_amd import bfmfit
  sig = inspect.signature(bfmfit.FaceFitter.fit_clip)
  assert list(sig.parameters)[1:] == ["landmarks", "clip_lengths", "init", "params", "weights", "lam_id", "lam_ex", "lam_smooth", "gtol", "max_trials"]
  assert sig.parameters["lam_smooth"].default == (0, 0, 0) and sig.parameters["max_trials"].default == 64
  for path in ("README.md", "DESIGN.md", "voicepuppet_amd/bfmfit.py", "include/vp_hip.h"):
    text = open(os.path.join(ROOT, path)).read()
    assert "lam_smooth" in text and re.search(r"untuned", text, flags=re.I), path
  for path in ("README.md", "DESIGN.md"):
    text = open(os.path.join(ROOT, path)).read()
    assert "fit_clip" in text and ("bfm_clip.json" in text or "unmeasured" in text), path

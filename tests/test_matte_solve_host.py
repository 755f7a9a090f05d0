"""The trimap's and the matting solve's definitions and host layer, without a GPU: the numpy restatement (tests/matte_solve_ref.py) the
device kernels are compared with in tests/test_gpu_matte_solve.py - its trimap against the definition pixel by pixel, its Laplacian as a
dense matrix (symmetric, annihilates constants, no negative eigenvalue, the stated diagonal) with bounds taken from a numpy.longdouble
run, conjugate gradients against numpy.linalg.solve, every clause of the stopping rule, what the solve buys on the synthetic scenes;
the C ABI's surface, sizing and refusals; the dataset tool's options."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import key_matte_ref as kr  # noqa: E402
import matte_clean_ref as mr  # noqa: E402
import matte_solve_ref as sr  # noqa: E402


# ---- trimap -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (33, 47), (64, 17)])
def test_trimap_equals_the_definition(size):
  """brute-force min / max over the stated offsets; even and odd squares, 1, and squares larger than the image"""
  H, W = size
  mattes = [mr.blobs(H, W, seed=H + W), mr.blobs(H, W, seed=1, smooth=1), np.where(mr.blobs(H, W, seed=2) >= 128, 255, 0).astype(np.uint8)]
  for m in mattes:
    for erode, dilate in ((1, 1), (2, 3), (3, 2), (4, 4), (5, 7), (8, 5), (17, 18), (64, 63), (63, 64)):
      for support, core in ((32, 224), (100, 101), (1, 255)):
        got = sr.trimap(m[None], support, core, erode, dilate)[0]
        assert np.array_equal(got, sr.trimap_brute(m, support, core, erode, dilate)), (size, erode, dilate, support, core)
  m = mattes[0]
  assert np.array_equal(sr.trimap(m[None])[0], sr.trimap(m[None], erode=sr.default_erode(H, W), dilate=sr.default_dilate(H, W))[0])
  assert (sr.default_erode(576, 720), sr.default_dilate(576, 720)) == (30, 19) and (sr.default_erode(16, 16), sr.default_dilate(1024, 1024)) == (5, 35)
  one = np.zeros((16, 16), np.uint8)
  one[8, 8] = 255                                                    # the offsets of an even square: -(k / 2) .. k - 1 - (k / 2)
  t = sr.trimap(one[None], erode=1, dilate=4)[0]
  assert t[8, 8] == 255 and np.array_equal(np.argwhere(t == 127).min(0), [7, 7]) and np.array_equal(np.argwhere(t >= 127).max(0), [10, 10])


# ---- the Laplacian as a matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
def test_dense_laplacian_properties_with_bounds_from_the_long_double_run(radius):
  """On a 20 x 16 frame.  u is the largest difference between an entry of the float64 matrix and of the numpy.longdouble one: what
  float64 rounding does to an entry.  A symmetric exact matrix then bounds the asymmetry by 2 u; a row has at most (4 r + 1)^2 entries
  that are not 0, so its sum is within (4 r + 1)^2 u of the long-double row sum; an eigenvalue moves by at most the perturbation's
  norm, at most N u (N = 320); the diagonal by u plus diag()'s own float64 error, measured the same way.  The long-double matrix
  itself carries 2^-11 of these errors (a 64-bit mantissa against 53 bits)."""
  H, W = 20, 16
  frames, alpha, _ = sr.clutter_scene(H, W, seed=3)
  L64, L80 = sr.Laplacian(frames[0], radius, 1.0), sr.Laplacian(frames[0], radius, 1.0, np.longdouble)
  A, B = L64.dense(), L80.dense()
  N, taps = H * W, (4 * radius + 1) ** 2
  u = float(np.abs(A - B).max())
  tiny = u / 1024                                                    # the long-double run's own error: 11 more bits, with a factor of 2
  du = float(np.abs(L64.diag() - L80.diag()).max())
  print("radius %d: u %.3e, asymmetry %.3e (long double %.3e), row sums %.3e (%.3e), min eigenvalue %.3e, diagonal %.3e (diag() itself %.3e)"
        % (radius, u, np.abs(A - A.T).max(), float(np.abs(B - B.T).max()), np.abs(A.sum(1)).max(), float(np.abs(B.sum(1)).max()),
           np.linalg.eigvalsh((A + A.T) / 2).min(), np.abs(np.diag(A) - L64.diag().ravel()).max(), du))
  assert 0 < u <= 1e-8      # a window's 3 x 3 inverse: condition at most (255^2 + eps / n) / (eps / n) = 6e5 at eps 1, n 9, times 2^-53, times |A| <= 25
  assert float(np.abs(B - B.T).max()) <= tiny and float(np.abs(B.sum(1)).max()) <= tiny        # the exact matrix has both properties
  assert np.abs(A - A.T).max() <= 2 * u + tiny
  assert np.abs(A.sum(1)).max() <= taps * u + tiny
  assert np.linalg.eigvalsh((A + A.T) / 2).min() >= -N * u
  assert np.abs(np.diag(A) - L64.diag().ravel()).max() <= u + du + tiny
  assert (L64.diag() > 0).all() and A[0, 1] < 0
  far = np.abs(np.arange(N)[:, None] // W - np.arange(N)[None] // W) > 2 * radius
  assert not A[far].any()                                            # pixels more than 2 r rows apart share no window


def test_cg_equals_the_dense_solve():
  """tol 1e-12 on the 20 x 16 frame.  The bound: a relative residual of 1e-12 leaves an error of at most cond(L_UU) * 1e-12 * |x|, and
  numpy.linalg.solve itself cond * 2^-52 * |x|; both measured here (cond is about 50)."""
  H, W = 20, 16
  frames, alpha, _ = sr.clutter_scene(H, W, seed=3)
  tri = sr.trimap((alpha * 255).astype(np.uint8), erode=3, dilate=3)
  U = ((tri[0] != 0) & (tri[0] != 255))
  A = sr.Laplacian(frames[0], 1, 1.0).dense()
  cond = np.linalg.cond(A[np.ix_(U.ravel(), U.ravel())])
  want = sr.solve_dense(frames[0], tri[0])
  for name, dot in sr.DOTS.items():
    res = sr.solve_frame(frames[0], tri[0], 1, 1.0, 1000, 1e-12, dot=dot)
    err = np.abs(res["alpha"] - want).max()
    print("%s: %d unknown, cond %.1f, %d iterations, residual %.2e, max |cg - dense| %.3e" % (name, U.sum(), cond, res["iterations"], res["residual"], err))
    assert res["status"] == 0 and res["residual"] <= 1e-12 and res["unknown"] == U.sum() > 100
    assert err <= cond * (1e-12 + 2.0 ** -52) * np.abs(want).max()
  assert np.array_equal(want[~U], (tri[0][~U] == 255).astype(np.float64)) and -0.1 < want.min() and want.max() < 1.1


def test_clauses_of_the_stopping_rule():
  H, W = 33, 47
  frames, alpha, _ = sr.clutter_scene(H, W, seed=5)
  seg = np.where(alpha > 0.5, 255, 0).astype(np.uint8)
  tri = sr.trimap(seg)
  full = sr.solve_frame(frames[0], tri[0], tol=1e-6)
  assert full["status"] == 0 and 1 < full["iterations"] < 200 and full["residual"] <= 1e-6
  # all known: nothing to solve
  res = sr.solve_frame(frames[0], seg[0])
  assert (res["status"], res["iterations"], res["unknown"], res["residual"]) == (1, 0, 0, 0.0) and np.array_equal(res["matte"], seg[0])
  # a band and no known-1 pixel: k = 0, b = 0
  none = np.where(tri[0] == 255, 127, tri[0]).astype(np.uint8)
  res = sr.solve_frame(frames[0], none)
  assert (res["status"], res["iterations"]) == (1, 0) and res["unknown"] > 0 and not res["alpha"].any() and not res["matte"].any()
  # the same with known-1 pixels only: L annihilates constants, so b = -(L 1)_U is rounding at most and x stays at most that
  ones = np.where(tri[0] == 0, 127, tri[0]).astype(np.uint8)
  L = sr.Laplacian(frames[0])
  assert np.abs(L.apply(np.ones((H, W)))).max() <= 1e-10
  # a band that touches the frame's edge (the torso leaves through the bottom; and a stripe through the whole frame)
  U = (tri[0] != 0) & (tri[0] != 255)
  assert U[H - 1].any()
  stripe = np.array(tri[0])
  stripe[:, 20:27] = 127
  stripe[10:14, :] = 127
  res = sr.solve_frame(frames[0], stripe, tol=1e-9, iters=1000)
  assert res["status"] == 0 and res["residual"] <= 1e-9 and np.abs(res["alpha"] - sr.solve_dense(frames[0], stripe)).max() <= 1e-6
  # iters = 1: one step of steepest descent in the preconditioned norm, the residual falls and is reported
  one = sr.solve_frame(frames[0], tri[0], iters=1)
  assert (one["status"], one["iterations"]) == (0, 1) and 1e-6 < one["residual"] < 1.0 and one["alpha"][U].any()
  # tol = 1: r = b satisfies it before the first iteration
  res = sr.solve_frame(frames[0], tri[0], tol=1.0)
  assert (res["status"], res["iterations"], res["residual"]) == (0, 0, 1.0) and not res["alpha"][U].any()
  # unknown is anything but 0 and 255
  odd = np.where(U, 1 + (np.arange(H * W).reshape(H, W) % 253), tri[0]).astype(np.uint8)
  assert np.array_equal(sr.solve_frame(frames[0], odd)["alpha"], full["alpha"])
  # the matte's rounding
  x = np.array([-0.2, 0.0, 0.5 / 255, 0.4999 / 255, 1.0, 1.3, 0.5])
  assert np.floor(np.minimum(np.maximum(x, 0), 1) * 255 + 0.5).astype(np.uint8).tolist() == [0, 0, 1, 0, 255, 255, 128]


# ---- what the solve buys ------------------------------------------------------------------------------------------------------------------
# measured with the restatement, one frame of seed 1, 10 levels of spill, all defaults (radius 1, eps 1, tol 1e-6): matte MAE cleaned and
# solved, edge colour error of foreground() with the cleaned and with the solved matte, iterations
MEASURED = {(96, 80): (0.0217, 0.0025, 14.35, 4.97, 63), (256, 256): (0.0066, 0.0012, 13.99, 4.91, 109)}
# the cluttered scene (clutter_scene, seed 1), input the 0 / 255 segmentation alpha > 0.5: MAE of KeyMatte's matte, of the segmentation, solved
MEASURED_CLUTTER = {(96, 80): (0.3509, 0.0208, 0.0096, 78), (256, 256): (0.3537, 0.0071, 0.0046, 135)}


@pytest.mark.parametrize("size", [(96, 80), (256, 256)])
def test_the_solve_on_the_studio_scene(size):
  """key, clean, trimap, solve against the scene's known alpha and foreground: the solved matte's MAE is at most a third of the cleaned
  matte's, foreground()'s edge colour error at most half, and the trimap takes no pixel as known that is not (alpha < 0.98 as 1 or
  alpha > 0.02 as 0)."""
  H, W = size
  frames, alpha, fore = mr.scene(H, W, seed=1, n=1, spill_levels=10.0)
  _, model = kr.fit(frames)
  _, matte = kr.matte(model, frames)
  cleaned, _, _ = mr.clean(matte, mr.landmarks(H, W, 1))
  tri = sr.trimap(cleaned)
  _, solved, rep = sr.solve(frames, tri)
  mae_c, mae_s = kr.quality(cleaned, alpha)[0], kr.quality(solved, alpha)[0]
  ec, es = (mr.edge_colour_error(mr.foreground(model, frames, m), fore, alpha) for m in (cleaned, solved))
  print("%d x %d: %d unknown, %d iterations; matte MAE %.4f -> %.4f; edge colour error %.2f -> %.2f" % (W, H, rep[0]["unknown"], rep[0]["iterations"], mae_c, mae_s, ec, es))
  assert sr.wrongly_known(tri, alpha) == 0
  assert rep[0]["status"] == 0 and rep[0]["residual"] <= 1e-6 and rep[0]["iterations"] < 256
  assert mae_s <= mae_c / 3 and es <= ec / 2
  want = MEASURED[size]
  assert mae_s <= 1.5 * want[1] and es <= 1.5 * want[3] and rep[0]["iterations"] <= 1.5 * want[4]


@pytest.mark.parametrize("size", [(96, 80), (256, 256)])
def test_the_solve_on_the_cluttered_scene(size):
  """Three sine textures of 50 and 20 grey levels per channel plus noise behind the subject, where KeyMatte reports its failure (the
  backdrop's residual is far above a studio wall's few levels and its matte's MAE is a third of the frame); the input is the 0 / 255
  segmentation alpha > 0.5.  This generator's textures have periods down to 20 pixels, shorter than a (2 r + 1) window can model as a colour
  line at the torso's edge: the solve halves the segmentation's error at 96 x 80 (0.0208 -> 0.0096) and takes a third off at 256 x 256
  (0.0071 -> 0.0046), not the half of a smoother backdrop.  Asserted: better than the segmentation, and the measured values at 1.5
  times."""
  H, W = size
  frames, alpha, _ = sr.clutter_scene(H, W, seed=1)
  rep_key, model = kr.fit(frames)
  _, keyed = kr.matte(model, frames)
  seg = np.where(alpha > 0.5, 255, 0).astype(np.uint8)
  tri = sr.trimap(seg)
  _, solved, rep = sr.solve(frames, tri)
  mae_k, mae_g, mae_s = (kr.quality(m, alpha)[0] for m in (keyed, seg, solved))
  print("%d x %d cluttered: key residual %.1f levels; matte MAE key %.4f, segmentation %.4f, solved %.4f; %d iterations" % (W, H, model[17], mae_k, mae_g, mae_s, rep[0]["iterations"]))
  assert model[17] > 20.0 and mae_k > 0.2                                        # KeyMatte's report: no plain backdrop
  assert sr.wrongly_known(tri, alpha) == 0 and rep[0]["status"] == 0 and rep[0]["residual"] <= 1e-6
  want = MEASURED_CLUTTER[size]
  assert mae_s < mae_g and mae_s <= 1.5 * want[2] and rep[0]["iterations"] <= 1.5 * want[3]
  if size == (96, 80):
    assert mae_s <= mae_g / 2


def test_dot_product_orders_agree():
  """The two quantities behind the device tolerance S of tests/test_gpu_matte_solve.py, on the scene of that file that sets it (five
  frames of 33 x 47): the spread of alpha over three dot-product orders, and the fsum run's distance from the tol = 1e-12 solution."""
  n, H, W = 5, 33, 47
  frames, alpha, _ = mr.scene(H, W, seed=H * 1000 + W, n=n, spill_levels=10.0)
  _, model = kr.fit(frames)
  cleaned, _, _ = mr.clean(kr.matte(model, frames)[1], mr.landmarks(H, W, n))
  tri = sr.trimap(cleaned)
  spread = dist = 0.0
  for f in range(n):
    runs = [sr.solve_frame(frames[f], tri[f], dot=d) for d in sr.DOTS.values()]
    fine = sr.solve_frame(frames[f], tri[f], iters=1024, tol=1e-12)
    spread = max([spread] + [np.abs(r["alpha"] - runs[1]["alpha"]).max() for r in runs])
    dist = max(dist, np.abs(runs[1]["alpha"] - fine["alpha"]).max())
    assert all(np.array_equal(r["matte"], runs[1]["matte"]) for r in runs) and len(set(r["iterations"] for r in runs)) == 1
  print("spread %.3e, distance from the tol 1e-12 solution %.3e" % (spread, dist))
  assert spread <= dist <= 1.25 * 3.221e-5       # the recorded value with a margin for another numpy build's rounding; S itself is the record
  assert sr.summary([1742, 1742], [65, 65], [9e-7, 9e-7]) == "solve: 1742 px unknown, 65 iterations, residual 9e-07"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
NAMES = ("vp_mattesolve_desc_size", "vp_mattesolve_workspace_bytes", "vp_mattesolve_create", "vp_mattesolve_destroy", "vp_mattesolve_trimap",
         "vp_mattesolve_solve", "vp_mattesolve_laplacian", "vp_mattesolve_tensor")


def test_c_abi_surface():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.matte_solve as vs
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  assert sorted(n for n in _lib.exported_symbols() if n.startswith("vp_mattesolve_")) == sorted(NAMES)
  body = hdr[hdr.index("typedef struct vp_mattesolve_desc {"):hdr.index("} vp_mattesolve_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.MatteSolveDesc._fields_] == ["struct_bytes", "max_frames", "max_height", "max_width", "max_radius"]
  assert ctypes.sizeof(_lib.MatteSolveDesc) == 20 and _lib.DESC_SIZE_QUERIES["vp_mattesolve_desc_size"] is _lib.MatteSolveDesc
  for macro, value in (("MAX_FRAMES", _lib.MATTESOLVE_MAX_FRAMES), ("MAX_SIZE", _lib.MATTESOLVE_MAX_SIZE), ("MAX_RADIUS", _lib.MATTESOLVE_MAX_RADIUS),
                       ("MAX_SQUARE", _lib.MATTESOLVE_MAX_SQUARE), ("MAX_ITERS", _lib.MATTESOLVE_MAX_ITERS), ("REPORT_INTS", _lib.MATTESOLVE_REPORT_INTS)):
    assert "#define VP_MATTESOLVE_%s %d\n" % (macro, value) in hdr
  assert (3, 64, 1024, 8) == (_lib.MATTESOLVE_MAX_RADIUS, _lib.MATTESOLVE_MAX_SQUARE, _lib.MATTESOLVE_MAX_ITERS, _lib.MATTESOLVE_REPORT_INTS) and sr.REPORT_INTS == 8
  assert "vp_mattesolve_*    replaces  datasets/make_data_from_GRID.py:654-672" in hdr and hdr.count("UNTUNED on real footage") >= 3
  for word in ("TRIMAP", "MOMENTS", "LAPLACIAN", "DIAGONAL", "SYSTEM", "REPORT", "48 bytes per pixel", "No floating-point atomics"):
    assert word in hdr[hdr.index("Trimap and closed-form matting solve"):], word
  # the Makefile builds the object without FMA contraction, in both object lists
  mk = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  assert "matte_solve.hip" in mk and "matte_solve.o:" in mk.replace("matte_solve.o ", "matte_solve.o") and "matte_solve.$(VAR).o" in mk
  src = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "matte_solve.hip")).read()
  assert "atomicAdd(&g.part" not in src and not re.search(r"atomicAdd\(\s*\(?(double|float)", src) and "hipMalloc" not in src and "Synchronize" not in src
  # the Python layer's defaults and rules
  sig = inspect.signature(vs.MatteSolver.solve).parameters
  assert (sig["radius"].default, sig["eps"].default, sig["iters"].default, sig["tol"].default, sig["out"].default) == (1, 1.0, 512, 1e-6, None)
  sig = inspect.signature(vs.MatteSolver.trimap).parameters
  assert (sig["support"].default, sig["core"].default, sig["erode"].default, sig["dilate"].default) == (32, 224, None, None)
  assert inspect.signature(vs.MatteSolver.__init__).parameters["max_radius"].default == 2
  for size in ((16, 16), (96, 80), (256, 256), (576, 720), (1024, 1024)):
    assert (vs.default_erode(*size), vs.default_dilate(*size)) == (sr.default_erode(*size), sr.default_dilate(*size))
  assert "untuned on real footage" in vs.__doc__ and "untuned on real footage" in vs.MatteSolver.solve.__doc__ and "untuned on real footage" in vs.MatteSolver.trimap.__doc__
  rep = {"unknown": np.array([1742, 1742]), "iterations": np.array([65, 256]), "status": np.array([0, 0]), "residual": np.array([9e-7, 3e-4])}
  assert vs.summary(rep, 256, 1e-6) == (sr.summary(rep["unknown"], rep["iterations"], rep["residual"]), 0, 1)
  rep["status"][0] = 2
  assert vs.summary(rep, 256, 1e-6)[1:] == (1, 1) and vs.summary(rep)[1:] == (1, 0)


def test_matte_solver_needs_a_gpu(monkeypatch):
  import torch
  from voicepuppet_amd.matte_solve import MatteSolver
  monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    MatteSolver(1, 64, 64)


def test_descriptor_sizing_and_refusals_before_anything_is_enqueued():
  from voicepuppet_amd import _lib
  L = _lib.lib()
  D = _lib.MatteSolveDesc
  n = ctypes.sizeof(D)
  assert L.vp_mattesolve_desc_size() == n == 20
  sizes = {}
  for shape in ((1, 16, 16, 1), (2, 64, 48, 2), (4, 256, 256, 3), (64, 512, 512, 2), (1, 1024, 1024, 3)):
    ws = L.vp_mattesolve_workspace_bytes(ctypes.byref(D(n, *shape)))
    f, h, w, _ = shape
    tiles = f * ((h + 31) // 32) * ((w + 31) // 32)
    need = 48 * f * h * w + 44 * tiles + 36 * f
    assert need <= ws <= need + 4096 and ws % 256 == 0, (shape, ws, need)
    sizes[shape] = ws
  assert L.vp_mattesolve_workspace_bytes(ctypes.byref(D(n, 2, 64, 48, 1))) == sizes[(2, 64, 48, 2)]       # the radius costs no memory
  h = ctypes.c_void_p()
  for what, d in [("struct_bytes", D(n - 4, 1, 64, 64, 1)), ("max_frames", D(n, 0, 64, 64, 1)), ("max_frames", D(n, 4097, 64, 64, 1)),
                  ("max_height", D(n, 1, 15, 64, 1)), ("max_height", D(n, 1, 1025, 64, 1)), ("max_width", D(n, 1, 64, 15, 1)),
                  ("max_width", D(n, 1, 64, 1025, 1)), ("max_radius", D(n, 1, 64, 64, 0)), ("max_radius", D(n, 1, 64, 64, 4))]:
    assert L.vp_mattesolve_workspace_bytes(ctypes.byref(d)) == 0 and what in L.vp_last_error().decode(), what
    h.value = 1
    assert L.vp_mattesolve_create(ctypes.byref(d), ctypes.c_void_p(4096), 1 << 30, ctypes.byref(h)) == -1 and not h.value
  assert L.vp_mattesolve_workspace_bytes(None) == 0
  good = D(n, 2, 64, 48, 2)
  ws = sizes[(2, 64, 48, 2)]
  assert L.vp_mattesolve_create(ctypes.byref(good), ctypes.c_void_p(4096), ws - 1, ctypes.byref(h)) == -3 and not h.value
  assert "workspace too small" in L.vp_last_error().decode()
  assert L.vp_mattesolve_create(ctypes.byref(good), None, ws, ctypes.byref(h)) == -3 and L.vp_mattesolve_create(ctypes.byref(good), ctypes.c_void_p(4096), ws, None) == -1
  assert L.vp_mattesolve_create(ctypes.byref(good), ctypes.c_void_p(4096), ws, ctypes.byref(h)) == 0 and h.value     # host only: no device memory is touched
  p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

  def trimap(handle=h, matte=p, cnt=1, hh=64, ww=48, support=32, core=224, erode=0, dilate=0, out=q):
    return L.vp_mattesolve_trimap(handle, matte, cnt, hh, ww, support, core, erode, dilate, out, None)
  for what, kw in [("handle", dict(handle=None)), ("matte", dict(matte=None)), ("out", dict(out=None)), ("n 3", dict(cnt=3)), ("n 0", dict(cnt=0)),
                   ("height 15", dict(hh=15)), ("max_height", dict(hh=65)), ("width 15", dict(ww=15)), ("max_width", dict(ww=49)),
                   ("support", dict(support=0)), ("support", dict(support=256)), ("core", dict(core=0)), ("core", dict(core=256)),
                   ("erode", dict(erode=-1)), ("erode", dict(erode=65)), ("dilate", dict(dilate=-1)), ("dilate", dict(dilate=65)),
                   ("overlaps", dict(out=p)), ("overlaps", dict(out=ctypes.c_void_p((1 << 20) + 64 * 48 - 1)))]:
    assert trimap(**kw) == -1 and what in L.vp_last_error().decode(), (what, L.vp_last_error())

  def solve(handle=h, frames=p, cnt=1, hh=64, ww=48, pitch=None, stride=None, tri=q, radius=1, eps=1.0, iters=10, tol=1e-6, matte=q):
    pitch = 3 * ww if pitch is None else pitch
    return L.vp_mattesolve_solve(handle, frames, pitch, pitch * hh if stride is None else stride, cnt, hh, ww, tri, radius, eps, iters, tol, matte, None)
  for what, kw in [("handle", dict(handle=None)), ("frames", dict(frames=None)), ("n 3", dict(cnt=3)), ("n 0", dict(cnt=0)), ("height 15", dict(hh=15)),
                   ("max_height", dict(hh=65)), ("width 15", dict(ww=15)), ("max_width", dict(ww=49)), ("row_pitch", dict(pitch=3 * 48 - 1)),
                   ("frame_stride", dict(stride=3 * 48 * 64 - 1)), ("trimap", dict(tri=None)), ("matte", dict(matte=None)), ("radius 0", dict(radius=0)),
                   ("max_radius", dict(radius=3)), ("eps", dict(eps=0.0)), ("eps", dict(eps=float("inf"))), ("eps", dict(eps=float("nan"))),
                   ("overlaps", dict(matte=ctypes.c_void_p((1 << 24) + 64 * 48 - 1))), ("overlaps", dict(matte=ctypes.c_void_p((1 << 24) - 1))),
                   ("iters", dict(iters=0)), ("iters", dict(iters=1025)), ("tol", dict(tol=-1e-9)), ("tol", dict(tol=float("nan")))]:
    assert solve(**kw) == -1 and what in L.vp_last_error().decode(), (what, L.vp_last_error())

  def lap(handle=h, frames=p, cnt=1, hh=64, ww=48, pitch=3 * 48, radius=1, eps=1.0, src=q, out=ctypes.c_void_p(1 << 26)):
    return L.vp_mattesolve_laplacian(handle, frames, pitch, pitch * hh, cnt, hh, ww, radius, eps, src, out, None)
  for what, kw in [("handle", dict(handle=None)), ("n 3", dict(cnt=3)), ("row_pitch", dict(pitch=100)), ("radius", dict(radius=3)), ("eps", dict(eps=-1.0)),
                   ("device p", dict(src=None)), ("device p", dict(out=None)), ("8-byte", dict(src=ctypes.c_void_p((1 << 24) + 4))), ("overlaps", dict(out=q))]:
    assert lap(**kw) == -1 and what in L.vp_last_error().decode(), (what, L.vp_last_error())
  ptr, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
  assert L.vp_mattesolve_tensor(h, b"alpha", ctypes.byref(ptr), shp) == 0 and list(shp) == [2, 64, 48, 1] and ptr.value % 256 == 0
  assert L.vp_mattesolve_tensor(h, b"report", ctypes.byref(ptr), shp) == 0 and list(shp[:2]) == [2, 8] and 4096 <= ptr.value < 4096 + ws
  assert L.vp_mattesolve_tensor(h, b"tiles", ctypes.byref(ptr), shp) == 0 and list(shp[:3]) == [2, 2, 2]
  assert L.vp_mattesolve_tensor(h, b"nothing", ctypes.byref(ptr), shp) == -1 and b"alpha, report, tiles" in L.vp_last_error()
  assert L.vp_mattesolve_tensor(None, b"alpha", ctypes.byref(ptr), shp) == -1
  L.vp_mattesolve_destroy(h)
  L.vp_mattesolve_destroy(None)


# ---- the dataset tool's options -----------------------------------------------------------------------------------------------------------
def test_make_triptychs_options(capsys):
  from voicepuppet_amd.datasets.make_triptychs import parse_options
  o, _ = parse_options([])
  assert (o.solve_matte, o.solve_erode, o.solve_dilate, o.solve_radius, o.solve_eps, o.solve_iters, o.solve_tol) == (False, None, None, 1, 1.0, 512, 1e-6)
  o, _ = parse_options(["--alpha_dir", "a", "--solve_matte", "--solve_erode", "9", "--solve_dilate", "6", "--solve_radius", "2", "--solve_eps", "0.5",
                        "--solve_iters", "40", "--solve_tol", "1e-4", "--key_foreground"])
  assert (o.solve_matte, o.solve_erode, o.solve_dilate, o.solve_radius, o.solve_eps, o.solve_iters, o.solve_tol) == (True, 9, 6, 2, 0.5, 40, 1e-4)
  o, _ = parse_options(["--key_matte", "--clean_matte", "--solve_matte", "--key_foreground", "--write_alpha", "m"])
  assert o.key_matte and o.clean_matte and o.solve_matte and o.key_foreground and o.write_alpha == "m"
  for argv, word in ((["--solve_matte"], "--alpha_dir"), (["--key_matte", "--solve_matte", "--solve_erode", "0"], "--solve_erode"),
                     (["--key_matte", "--solve_matte", "--solve_dilate", "65"], "--solve_dilate"), (["--key_matte", "--solve_matte", "--solve_radius", "4"], "--solve_radius"),
                     (["--key_matte", "--solve_matte", "--solve_eps", "0"], "--solve_eps"), (["--key_matte", "--solve_matte", "--solve_iters", "1025"], "--solve_iters"),
                     (["--key_matte", "--solve_matte", "--solve_tol", "-1"], "--solve_tol"), (["--key_matte", "--alpha_dir", "a", "--solve_matte"], "--key_matte")):
    with pytest.raises(SystemExit) as e:
      parse_options(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err, argv
  import voicepuppet_amd.datasets.make_triptychs as mt
  assert "--solve_matte" in mt.__doc__ and "CLUTTERED" in mt.__doc__ and "matte, clean, solve, foreground, build" in mt.__doc__
  assert mt.__doc__.count("untuned on real footage") >= 3

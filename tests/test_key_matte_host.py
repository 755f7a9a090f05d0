"""The key matte's definition and host layer, without a GPU: known answers of the numpy restatement (tests/key_matte_ref.py) the device
kernels are compared with in tests/test_gpu_key_matte.py; vp_keymatte_solve_host against the restatement bit for bit; the quality of the
definition on the synthetic studio scene; the C ABI's surface, sizing and refusals; the dataset tool's options; and the refusals through
the sanitizer build of the host layer from a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import key_matte_ref as kr  # noqa: E402

CSRC = os.path.join(ROOT, "voicepuppet_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "key_matte.npz")


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- known answers of the restatement ---------------------------------------------------------------------------------------------------
def test_constant_backdrop():
  frames = np.empty((2, 32, 40, 3), np.uint8)
  frames[...] = (60, 140, 90)
  S, model = kr.fit(frames)
  assert model[kr.STATUS] == 0 and model[kr.N] == S[0, 20] == S[1, 20] and model[kr.KEPT] == 1.0 and model[kr.RESIDUAL_RMS] == 0.0
  assert model[[1, 2, 4, 5, 7, 8]].tolist() == [0.0] * 6 and model[[0, 3, 6]].tolist() == [60.0, 140.0, 90.0]
  # R = 0: sigma_min alone keeps Sigma invertible
  assert model[9:15].tolist() == [0.25, 0.0, 0.0, 0.25, 0.0, 0.25]
  raw, matte = kr.matte(model, frames)
  assert not raw.any() and not matte.any()


def test_noiseless_plane_is_recovered():
  H, W = 64, 48
  yy, xx = np.mgrid[0:H, 0:W]
  frames = np.stack([40 + 2 * xx + yy, 200 - xx - 2 * yy, 10 + 3 * yy], -1).astype(np.uint8)[None]
  S, model = kr.fit(frames)
  assert model[kr.STATUS] == 0
  assert np.abs(model[:9] - [40, 2, 1, 200, -1, -2, 10, 0, 3]).max() <= 1e-9
  assert model[kr.RESIDUAL_RMS] <= 1e-4 and not kr.matte(model, frames)[1].any()


def test_one_repeated_border_colour_and_sigma_min():
  frames = np.random.default_rng(0).integers(0, 256, (1, 48, 48, 3), dtype=np.uint8)
  frames[0][kr.sample_mask(48, 48)] = (17, 99, 201)
  for sigma_min in (0.5, 2.0, 3.0):
    _, model = kr.fit(frames, sigma_min=sigma_min)
    inv = 1.0 / (sigma_min * sigma_min)
    assert model[kr.STATUS] == 0 and model[kr.RESIDUAL_RMS] == 0.0 and np.all(np.isfinite(model))
    assert np.abs(model[9:15] - [inv, 0, 0, inv, 0, inv]).max() <= 1e-12 * inv


def test_fewer_than_16_samples_and_none():
  S = kr.moments(np.full((1, 16, 16, 3), 50, np.uint8), np.arange(256).reshape(16, 16) < 15)
  assert S[20] == 15
  model = kr.solve(S)
  assert model[kr.STATUS] == 1 and model[kr.N] == 15 and model[[1, 2, 4, 5, 7, 8]].tolist() == [0.0] * 6 and model[0] == 50.0
  # 16 samples, but one row: no spread in y, the 2 x 2 determinant is 0
  assert kr.solve(kr.moments(np.full((1, 16, 16, 3), 50, np.uint8), np.arange(256).reshape(16, 16) < 16))[kr.STATUS] == 1
  empty = kr.solve([0] * 21)
  assert empty[kr.STATUS] == 1 and empty[kr.N] == 0 and empty[9:15].tolist() == [0.25, 0.0, 0.0, 0.25, 0.0, 0.25] and not empty[:9].any()
  # a single column has no spread in x: the 2 x 2 determinant is 0
  col = np.zeros((16, 16), bool)
  col[:, 3] = True
  assert kr.solve(kr.moments(np.full((1, 16, 16, 3), 50, np.uint8), col))[kr.STATUS] == 1


def test_pass_2_rejects_a_bright_object_in_the_top_band():
  """A lamp of 4 x 8 pixels among 984 samples.  (Under pass 1's model an outlier group that is a share f of the samples sits at a d2 of
  about 1 / f, because it inflates the covariance it is measured with: one trimming pass at trim = 16 removes objects below about 1 / 17
  of the border, and keeps larger ones - kept and residual_rms then show it.)"""
  frames, _ = kr.scene(96, 80, seed=3, n=1)
  clean_S, clean = kr.fit(frames)
  lamp = frames.copy()
  lamp[0, 0:4, 30:38] = (255, 250, 240)
  S, model = kr.fit(lamp)
  first = kr.solve(S[0])
  assert S[0, 20] == clean_S[0, 20] and S[0, 20] - 4 * 8 - 10 <= S[1, 20] <= S[0, 20] - 4 * 8 and model[kr.KEPT] == S[1, 20] / S[0, 20] < 1.0
  assert first[kr.RESIDUAL_RMS] > 3 * clean[kr.RESIDUAL_RMS]                                  # pass 1 is spoilt by the lamp ...
  assert abs(model[kr.RESIDUAL_RMS] - clean[kr.RESIDUAL_RMS]) < 0.5                            # ... pass 2 is not
  assert np.abs(model[[0, 3, 6]] - clean[[0, 3, 6]]).max() < 1.0
  assert np.all(kr.raw_key(model, lamp)[0, 0:4, 30:38] == 255)


def test_radius_0_returns_the_raw_key():
  frames, _ = kr.scene(48, 40, seed=5, n=2)
  _, model = kr.fit(frames)
  raw, matte = kr.matte(model, frames, radius=0)
  assert np.array_equal(raw, matte) and 0 < (raw == 255).mean() < 1 and (raw == 0).any()
  assert not np.array_equal(kr.matte(model, frames, radius=1)[1], raw)
  # the sample set: the top band and the upper sides
  m = kr.sample_mask(48, 40)
  assert m[:3].all() and m[3:24, :3].all() and m[3:24, -3:].all() and not m[3:, 3:-3].any() and not m[24:].any() and kr.default_band(16) == 2


def test_golden_scene_has_not_drifted():
  """tests/golden/key_matte.npz (tests/golden/make_key_matte_golden.py): three 96 x 80 frames with their moments, model, raw key and matte"""
  g = np.load(GOLDEN)
  frames, _ = kr.scene(96, 80, seed=1, n=3)
  assert np.array_equal(frames, g["frames"])
  S, model = kr.fit(g["frames"])
  assert np.array_equal(S, g["moments"]) and np.array_equal(_bits(model), _bits(g["model"]))
  raw, matte = kr.matte(model, g["frames"])
  assert np.array_equal(raw, g["raw"]) and np.array_equal(matte, g["matte"])


# ---- vp_keymatte_solve_host ---------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
  from voicepuppet_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libvp_hip.so is not built")
  return _lib, _lib.lib()


def _solve_host(L, S, sigma_min=2.0):
  out = (ctypes.c_double * kr.MODEL_DOUBLES)()
  assert L.vp_keymatte_solve_host((ctypes.c_int64 * 21)(*[int(v) for v in S]), sigma_min, out) == 0
  return np.array(out[:], np.float64)


def test_solve_host_equals_the_restatement_bit_for_bit():
  _lib, L = _lib_or_skip()
  cases = []
  for (H, W), n, seed in (((96, 80), 3, 1), ((256, 256), 2, 2), ((33, 47), 5, 3)):
    frames, _ = kr.scene(H, W, seed=seed, n=n)
    S, _ = kr.fit(frames)
    cases += [S[0], S[1]]
  frames, _ = kr.scene(96, 80, seed=1, n=1)
  cases.append(kr.moments(frames, kr.sample_mask(96, 80, 40, 96)))                 # most of the frame: the subject is in the samples
  cases.append(kr.moments(np.full((1, 16, 16, 3), 50, np.uint8), np.arange(256).reshape(16, 16) < 15))
  cases.append([0] * 21)
  for S in cases:
    for sigma_min in (2.0, 0.75):
      got, want = _solve_host(L, S, sigma_min), kr.solve(S, sigma_min)
      assert np.array_equal(_bits(got), _bits(want)), (got, want)
  out = (ctypes.c_double * kr.MODEL_DOUBLES)()
  S = (ctypes.c_int64 * 21)()
  for bad in (0.0, -1.0, float("nan"), float("inf")):
    assert L.vp_keymatte_solve_host(S, bad, out) == -1 and b"sigma_min" in L.vp_last_error()
  assert L.vp_keymatte_solve_host(None, 2.0, out) == -1 and L.vp_keymatte_solve_host(S, 2.0, None) == -1


# ---- quality of the definition ------------------------------------------------------------------------------------------------------------
# measured with the restatement at the defaults: (mean absolute error, share of pixels off by more than 0.25) with the guided filter
MEASURED = {(96, 80): (0.022922, 0.006293), (256, 256): (0.007166, 0.000148)}


@pytest.mark.parametrize("size", sorted(MEASURED))
def test_quality_against_the_known_alpha(size):
  """Against the scene's known alpha, three frames, all defaults.  Measured: 96 x 80: MAE 0.0229, share off by more than 0.25 0.63 % (raw
  key, radius 0: 0.0280 and 4.90 %); 256 x 256: MAE 0.0072, share 0.015 % (raw key: 0.0093 and 1.55 %).  Asserted at 1.5 times the
  measured values: the margin only guards the restatement against an accidental change.  What holds without a measurement: the guided
  filter's share is strictly below the raw key's."""
  frames, alpha = kr.scene(*size, seed=1, n=3)
  _, model = kr.fit(frames)
  raw, matte = kr.matte(model, frames)
  mae, share = kr.quality(matte, alpha)
  raw_mae, raw_share = kr.quality(raw, alpha)
  print("%d x %d: MAE %.6f, share %.6f; raw key: MAE %.6f, share %.6f" % (size + (mae, share, raw_mae, raw_share)))
  assert share < raw_share
  assert mae <= 1.5 * MEASURED[size][0] and share <= 1.5 * MEASURED[size][1]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_keymatte_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.matte as vm  # importable without a GPU
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  names = ("vp_keymatte_desc_size", "vp_keymatte_workspace_bytes", "vp_keymatte_create", "vp_keymatte_destroy", "vp_keymatte_fit",
           "vp_keymatte_apply", "vp_keymatte_get_model", "vp_keymatte_set_model", "vp_keymatte_tensor", "vp_keymatte_solve_host")
  for name in names:
    assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols(), name
  assert sorted(n for n in _lib.exported_symbols() if n.startswith("vp_keymatte_")) == sorted(names)
  body = hdr[hdr.index("typedef struct vp_keymatte_desc {"):hdr.index("} vp_keymatte_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.KeyMatteDesc._fields_]
  assert [n for n, _ in _lib.KeyMatteDesc._fields_] == ["struct_bytes", "max_frames", "max_height", "max_width", "max_radius"]
  assert ctypes.sizeof(_lib.KeyMatteDesc) == 20 and _lib.DESC_SIZE_QUERIES["vp_keymatte_desc_size"] is _lib.KeyMatteDesc
  for macro, value in (("MAX_FRAMES", _lib.KEYMATTE_MAX_FRAMES), ("MAX_SIZE", _lib.KEYMATTE_MAX_SIZE), ("MAX_RADIUS", _lib.KEYMATTE_MAX_RADIUS),
                       ("MODEL_DOUBLES", _lib.KEYMATTE_MODEL_DOUBLES)):
    assert "#define VP_KEYMATTE_%s %d" % (macro, value) in hdr
  assert vm.MODEL_DOUBLES == kr.MODEL_DOUBLES == 19 and (vm.N, vm.KEPT, vm.RESIDUAL_RMS, vm.STATUS) == (kr.N, kr.KEPT, kr.RESIDUAL_RMS, kr.STATUS)
  assert "vp_keymatte_*      replaces" in hdr and "UNTUNED on real footage" in hdr
  mk = open(os.path.join(CSRC, "Makefile")).read()
  assert "key_matte.hip" in mk.split("SRCS =")[1].split("\n")[0]
  contract = [l for l in mk.splitlines() if "-ffp-contract=off" in l and "CXXFLAGS +=" in l]
  assert len(contract) == 2 and "key_matte.o" in contract[0] and "key_matte.$(VAR).o" in contract[1]
  import inspect
  sig = inspect.signature(vm.KeyMatte.matte).parameters
  assert [(k, sig[k].default) for k in ("lo", "hi", "radius", "eps")] == [("lo", 4.0), ("hi", 10.0), ("radius", 4), ("eps", 25.0)]
  sig = inspect.signature(vm.KeyMatte.fit).parameters
  assert [(k, sig[k].default) for k in ("band", "side_rows", "trim", "sigma_min")] == [("band", None), ("side_rows", None), ("trim", 16.0), ("sigma_min", 2.0)]


def test_keymatte_needs_a_gpu(monkeypatch):
  import torch
  from voicepuppet_amd.matte import KeyMatte
  monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    KeyMatte(1, 64, 64)


def test_library_sizes_and_refuses_with_the_field_named():
  _lib, L = _lib_or_skip()
  n = ctypes.sizeof(_lib.KeyMatteDesc)
  D = _lib.KeyMatteDesc
  assert L.vp_keymatte_desc_size() == n == 20
  # two float64 planes of max_frames x max_height x max_width with a radius, none without
  assert 64 * 512 * 512 * 16 <= L.vp_keymatte_workspace_bytes(ctypes.byref(D(n, 64, 512, 512, 16))) <= 64 * 512 * 512 * 16 + 4096
  assert 0 < L.vp_keymatte_workspace_bytes(ctypes.byref(D(n, 64, 512, 512, 0))) <= 4096
  assert L.vp_keymatte_workspace_bytes(ctypes.byref(D(n, 4096, 1024, 1024, 16))) >= 4096 * 1024 * 1024 * 16       # no 32-bit product
  for what, d in [("max_frames", D(n, 0, 64, 64, 4)), ("max_frames", D(n, -1, 64, 64, 4)), ("max_frames", D(n, 4097, 64, 64, 4)),
                  ("max_height", D(n, 1, 0, 64, 4)), ("max_height", D(n, 1, 15, 64, 4)), ("max_height", D(n, 1, 1025, 64, 4)),
                  ("max_width", D(n, 1, 64, -5, 4)), ("max_width", D(n, 1, 64, 15, 4)), ("max_width", D(n, 1, 64, 1025, 4)),
                  ("max_radius", D(n, 1, 64, 64, 17)), ("max_radius", D(n, 1, 64, 64, -1)), ("struct_bytes", D(n - 4, 1, 64, 64, 4))]:
    assert L.vp_keymatte_workspace_bytes(ctypes.byref(d)) == 0 and what in L.vp_last_error().decode(), what
    h = ctypes.c_void_p()
    assert L.vp_keymatte_create(ctypes.byref(d), ctypes.c_void_p(4096), 1 << 30, ctypes.byref(h)) == -1 and not h.value
    assert what in L.vp_last_error().decode()
  # create is host only: with a workspace address that is never touched, the call-time refusals answer without a GPU
  good = D(n, 2, 64, 48, 4)
  ws = L.vp_keymatte_workspace_bytes(ctypes.byref(good))
  h = ctypes.c_void_p()
  assert L.vp_keymatte_create(ctypes.byref(good), ctypes.c_void_p(4096), ws - 1, ctypes.byref(h)) == -3 and not h.value
  assert b"workspace too small" in L.vp_last_error()
  assert L.vp_keymatte_create(ctypes.byref(good), ctypes.c_void_p(4096), ws, ctypes.byref(h)) == 0 and h.value
  p = ctypes.c_void_p(1 << 20)

  def apply(cnt=1, hh=64, ww=48, pitch=None, stride=None, lo=4.0, hi=10.0, radius=4, eps=25.0, matte=p):
    pitch = 3 * ww if pitch is None else pitch
    return L.vp_keymatte_apply(h, p, pitch, pitch * hh if stride is None else stride, cnt, hh, ww, lo, hi, radius, eps, None, matte, None)

  def fit(cnt=1, hh=64, ww=48, band=0, side_rows=0, trim=16.0, sigma_min=2.0):
    return L.vp_keymatte_fit(h, p, 3 * ww, 3 * ww * hh, cnt, hh, ww, band, side_rows, trim, sigma_min, None)
  for what, kw in [("n 3", dict(cnt=3)), ("n 0", dict(cnt=0)), ("height 15", dict(hh=15)), ("max_height", dict(hh=65)), ("width 15", dict(ww=15)),
                   ("max_width", dict(ww=49)), ("row_pitch", dict(pitch=3 * 48 - 1)), ("frame_stride", dict(stride=3 * 48 * 64 - 1)),
                   ("lo", dict(lo=10.0, hi=10.0)), ("lo", dict(lo=-1.0)), ("hi", dict(hi=float("inf"))), ("radius 5", dict(radius=5)),
                   ("radius -1", dict(radius=-1)), ("eps", dict(eps=0.0)), ("eps", dict(eps=float("nan"))), ("matte", dict(matte=None))]:
    assert apply(**kw) == -1 and what in L.vp_last_error().decode(), (what, L.vp_last_error())
  for what, kw in [("n 3", dict(cnt=3)), ("max_height", dict(hh=65)), ("band 25", dict(band=25)), ("band -1", dict(band=-1)),
                   ("side_rows 65", dict(side_rows=65)), ("side_rows 3", dict(band=4, side_rows=3)), ("trim", dict(trim=-1.0)),
                   ("trim", dict(trim=float("nan"))), ("sigma_min", dict(sigma_min=0.0))]:
    assert fit(**kw) == -1 and what in L.vp_last_error().decode(), (what, L.vp_last_error())
  assert L.vp_keymatte_get_model(h, None, None) == -1 and L.vp_keymatte_set_model(h, ctypes.c_void_p((1 << 20) + 4), None) == -1
  assert b"8-byte" in L.vp_last_error()
  q, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
  assert L.vp_keymatte_tensor(h, b"moments", ctypes.byref(q), shp) == 0 and list(shp[:2]) == [2, 21] and q.value % 256 == 0
  assert L.vp_keymatte_tensor(h, b"model", ctypes.byref(q), shp) == 0 and shp[0] == 19 and 4096 <= q.value < 4096 + ws
  assert L.vp_keymatte_tensor(h, b"nothing", ctypes.byref(q), shp) == -1 and b"moments, model" in L.vp_last_error()
  L.vp_keymatte_destroy(h)
  L.vp_keymatte_destroy(None)


# ---- the dataset tool's options ------------------------------------------------------------------------------------------------------------
def test_make_triptychs_options(capsys):
  from voicepuppet_amd.datasets.make_triptychs import parse_options
  o, _ = parse_options([])
  assert (o.key_matte, o.key_frames, o.key_thresholds, o.key_radius, o.key_eps, o.key_band, o.write_alpha) == (False, None, (4.0, 10.0), 4, 25.0, None, None)
  assert (o.alpha_dir, o.frame_batch, o.appearance, o.size, o.crop, o.joint, o.smooth) == (None, 32, "first", None, None, False, None)   # as before
  o, _ = parse_options(["--key_matte", "--key_frames", "8", "--key_thresholds", "3", "9.5", "--key_radius", "0", "--key_eps", "100", "--key_band", "6",
                        "--write_alpha", "mattes"])
  assert (o.key_matte, o.key_frames, o.key_thresholds, o.key_radius, o.key_eps, o.key_band, o.write_alpha) == (True, 8, (3.0, 9.5), 0, 100.0, 6, "mattes")
  for argv, word in ((["--key_matte", "--alpha_dir", "a"], "--alpha_dir"), (["--write_alpha", "a"], "--key_matte"),
                     (["--key_matte", "--key_thresholds", "5", "5"], "LO < HI"), (["--key_matte", "--key_radius", "17"], "--key_radius"),
                     (["--key_matte", "--key_eps", "0"], "--key_eps")):
    with pytest.raises(SystemExit) as e:
      parse_options(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err, argv
  import voicepuppet_amd.datasets.make_triptychs as mt
  assert "enrolment photo" in mt.__doc__ and "--key_matte" in mt.__doc__ and "PLAIN" in mt.__doc__


# ---- the host layer under sanitizers -------------------------------------------------------------------------------------------------------
def test_refusals_through_the_host_build_under_sanitizers():
  """tests/key_matte_badargs.cpp, a stand-alone program with its own main, against the `make host-asan` build of the C-ABI layer
  (AddressSanitizer + UBSan, kernels reduced to launch stubs): sizing, every refusal of create, fit, apply, the model copies and the
  tensor query, and vp_keymatte_solve_host on ordinary, degenerate and extreme moments, with the sanitizers silent.  Nothing is loaded
  into Python."""
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  clang = "/opt/rocm/lib/llvm/bin/clang++"
  if not (os.path.exists(hipcc) and os.path.exists(clang)):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", CSRC, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  libdir = os.path.join(ROOT, "voicepuppet_amd")
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "key_matte_badargs")
    c = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "key_matte_badargs.cpp"),
                        "-L", libdir, "-l:libvp_host_asan.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "all refused" in r.stdout and "NOT-" not in r.stdout and r.stdout.count("refused ") >= 25 and r.stdout.count("solved ") >= 4
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]

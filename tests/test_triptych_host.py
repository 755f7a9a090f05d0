"""The triptych stages' definitions and host layer, without a GPU: the numpy restatement (tests/triptych_ref.py) that the device kernels are
compared with byte for byte in tests/test_gpu_triptych.py is pinned here, independently of the kernels - its hole fill against
scipy.ndimage.binary_fill_holes, its integer blur against a float64 Gaussian with the same border - together with ear.txt's formula, the C
ABI's surface and the refused descriptors."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triptych_ref as tr  # noqa: E402


# ---- the masks of the fill tests (shared with tests/test_gpu_triptych.py) ---------------------------------------------------------------
def ring(h=40, w=52):
  m = np.zeros((h, w), np.uint8)
  m[5:h - 5, 7:w - 7] = 1
  m[12:h - 12, 15:w - 15] = 0
  return m


def letter_c(h=40, w=52):
  m = ring(h, w)
  m[h // 2 - 2:h // 2 + 2, w - 15:] = 0          # the ring opened to the right: the hole is joined to the outside
  return m


def hole_at_border(h=40, w=52):
  m = np.zeros((h, w), np.uint8)
  m[0:20, 10:30] = 1
  m[0:12, 15:25] = 0                             # a notch whose open side is the image border itself
  return m


def diagonal_leak(h=40, w=52):
  """a hole whose only link to the outside is a diagonal step: 4-connectivity does not pass it, the hole stays filled"""
  m = ring(h, w)
  m[12:h - 12, 15:w - 15] = 1
  m[5:h - 5, 7:w - 7] = 1
  m[20, 20] = 0                                  # the hole
  m[19, 19] = 0                                  # diagonal neighbour ...
  m[5:19, 19] = 0                                # ... joined to the outside by a straight corridor
  return m


def spiral(size=224, pitch=4, open_to_border=False):
  """a one-pixel-wide corridor of zeros wound inwards through a block of ones; returns (mask, turns)"""
  m = np.ones((size, size), np.uint8)
  y, x, dy, dx, turns = 1, 1, 0, 1, 0

  def blocked(y, x, dy, dx):
    for k in range(1, pitch + 1):
      ny, nx = y + k * dy, x + k * dx
      if k == 1 and not (1 <= ny <= size - 2 and 1 <= nx <= size - 2):
        return True
      if 0 <= ny < size and 0 <= nx < size and m[ny, nx] == 0:
        return True
    return False
  while True:
    m[y, x] = 0
    if blocked(y, x, dy, dx):
      dy, dx = dx, -dy                           # turn clockwise
      turns += 1
      if blocked(y, x, dy, dx):
        break
    y, x = y + dy, x + dx
  if open_to_border:
    m[0, 1] = 0
  return m, turns


def random_mask(h, w, seed, density=0.6):
  return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def fill_cases():
  sp_closed, turns = spiral()
  sp_open, _ = spiral(open_to_border=True)
  assert turns >= 8
  return [("ring", ring()), ("c", letter_c()), ("hole_at_border", hole_at_border()), ("diagonal", diagonal_leak()),
          ("spiral_open", sp_open), ("spiral_closed", sp_closed), ("ones", np.ones((33, 47), np.uint8)), ("zeros", np.zeros((33, 47), np.uint8)),
          ("random_37x45", random_mask(37, 45, 1)), ("random_224", random_mask(224, 224, 2))]


def disc_with_holes(size=224):
  yy, xx = np.mgrid[0:size, 0:size]
  m = ((yy - 110) ** 2 + (xx - 116) ** 2 <= 90 ** 2).astype(np.uint8)
  m[(yy - 90) ** 2 + (xx - 90) ** 2 <= 12 ** 2] = 0
  m[(yy - 150) ** 2 + (xx - 120) ** 2 <= 3 ** 2] = 0
  m[100:104, 140:190] = 0
  return m


# ---- stage a ---------------------------------------------------------------------------------------------------------------------------
def test_fill_equals_scipy_on_the_mask_set():
  ndimage = pytest.importorskip("scipy.ndimage")
  for name, m in fill_cases():
    want = ndimage.binary_fill_holes(m > 0).astype(np.uint8)
    assert np.array_equal(tr.fill_holes(m), want), name
    assert np.array_equal(tr.fill_holes(m * 200), want), name          # any nonzero value is mask


def test_fill_known_answers():
  assert tr.fill_holes(ring()).sum() == 30 * 38                        # the hole is filled
  assert np.array_equal(tr.fill_holes(letter_c()), letter_c())         # open: nothing is filled
  assert np.array_equal(tr.fill_holes(hole_at_border()), hole_at_border())
  d = tr.fill_holes(diagonal_leak())
  assert d[20, 20] == 1 and d[19, 19] == 0                             # the diagonal step does not leak
  closed, turns = spiral()
  opened, _ = spiral(open_to_border=True)
  assert turns >= 8 and (closed == 0).sum() > 224 * 20
  assert tr.fill_holes(closed).all() and np.array_equal(tr.fill_holes(opened), opened)


# ---- stage b ---------------------------------------------------------------------------------------------------------------------------
def test_linear_table_known_answers():
  s, c0, c1 = tr.linear_table(224, 224)
  assert np.array_equal(s, np.arange(224)) and np.all(c0 == 1) and np.all(c1 == 0)
  s, c0, c1 = tr.linear_table(4, 8)                                    # f = d / 2 - 0.25
  assert s.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and c1.tolist() == [0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0]
  assert c0.dtype == c1.dtype == np.float32 and np.all(c0 + c1 == 1)
  s, c0, c1 = tr.linear_table(8, 2)                                    # f = 4 d + 1.5
  assert s.tolist() == [1, 5] and c1.tolist() == [0.5, 0.5]
  m = disc_with_holes()
  assert np.array_equal(tr.resize_mask(m, 224), m.astype(np.float32))


def test_erode_is_the_minimum_of_the_window_inside_the_image():
  m = np.ones((9, 9), np.float32)
  m[4, 4] = 0.25
  e = tr.erode5(m)
  assert np.all(e[2:7, 2:7] == 0.25) and e.sum() == 81 - 25 * 0.75
  assert np.all(tr.erode5(np.ones((3, 3), np.float32)) == 1)          # the border adds nothing


# ---- stage d ---------------------------------------------------------------------------------------------------------------------------
def _float_blur(u):
  k = np.arange(tr.TAPS, dtype=np.float64)
  g = np.exp(-((k - tr.RADIUS) ** 2) / 32.0)
  g /= g.sum()
  h, w = u.shape
  x, y = np.arange(w), np.arange(h)
  hor = sum(g[i] * u[:, tr.reflect101(x + i - tr.RADIUS, w)].astype(np.float64) for i in range(tr.TAPS))
  return sum(g[i] * hor[tr.reflect101(y + i - tr.RADIUS, h), :] for i in range(tr.TAPS))


def test_integer_blur_within_one_level_of_the_float64_gaussian():
  q = tr.blur_taps()
  assert q.sum() == 65536 and q.shape == (21,) and np.array_equal(q, q[::-1]) and q[10] == q.max()
  rng = np.random.default_rng(3)
  step = np.zeros((40, 53), np.uint8)
  step[:, 20:] = 255
  images = [rng.integers(0, 256, (11, 11), dtype=np.uint8), rng.integers(0, 256, (37, 45), dtype=np.uint8),
            rng.integers(0, 256, (64, 64), dtype=np.uint8), step, step.T.copy(), np.full((12, 30), 255, np.uint8)]
  for u in images:
    got, want = tr.blur(u).astype(np.float64), _float_blur(u)
    worst = np.abs(got - want).max()
    print("blur %s: worst |integer - float64| %.4f grey levels" % (u.shape, worst))
    assert worst <= 1.0
    assert np.abs(got - np.rint(want)).max() <= 1
  assert np.all(tr.blur(np.full((12, 30), 255, np.uint8)) == 255) and np.all(tr.blur(np.zeros((11, 11), np.uint8)) == 0)


def test_geometry_status():
  assert tr.geometry_status(100, 156, 0, 256, 256) == 0 and tr.geometry_status(100, 157, 0, 256, 256) == 3
  assert tr.geometry_status(100, 0, -1, 256, 256) == 3 and tr.geometry_status(10, 0, 0, 256, 256) == 1
  assert tr.geometry_status(11, 0, 0, 256, 256) == 0 and tr.geometry_status(201, 0, 0, 256, 200) == 2


# ---- ear.txt ---------------------------------------------------------------------------------------------------------------------------
def test_ear_formula_on_hand_values():
  from voicepuppet_amd.datasets.make_triptychs import ear_value
  lm = np.zeros((68, 2))
  lm[36], lm[39] = (0, 0), (4, 0)                      # eye 1: width 4, both heights 2 -> 1.0
  lm[37], lm[41] = (1, 1), (1, -1)
  lm[38], lm[40] = (3, 1), (3, -1)
  lm[42], lm[45] = (10, 5), (20, 5)                    # eye 2: width 10, heights 3 and 4 -> 0.7
  lm[43], lm[47] = (12, 6), (12, 3)
  lm[44], lm[46] = (18, 7), (18, 3)
  assert abs(ear_value(lm.reshape(-1).tolist()) - 0.85) < 1e-15
  lm[42:48] += 100.0                                   # a shift changes nothing
  assert abs(ear_value(lm.reshape(-1).tolist()) - 0.85) < 1e-12


def test_launcher_options():
  from voicepuppet_amd.datasets.make_triptychs import parse_options
  o, _ = parse_options(["--clip_dir", "c", "--landmarks", "l.txt", "--out_dir", "o"])
  assert (o.size, o.crop, o.alpha_dir, o.bfmcoeff, o.appearance, o.frame_batch, o.list) == (None, None, None, None, "first", 32, None)
  o, _ = parse_options(["--clip_dir", "c", "--landmarks", "l.txt", "--out_dir", "o", "--size", "256", "--crop", "10", "20", "300", "--appearance",
                        "none", "--frame_batch", "8", "--list", "train.txt", "--alpha_dir", "a", "--bfmcoeff", "b.txt"])
  assert (o.size, o.crop, o.alpha_dir, o.bfmcoeff, o.appearance, o.frame_batch, o.list) == (256, (10, 20, 300), "a", "b.txt", "none", 8, "train.txt")
  shim = open(os.path.join(ROOT, "voicepuppet", "datasets", "make_triptychs.py")).read()
  assert "from voicepuppet_amd.datasets.make_triptychs import main" in shim


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NAMES = ("vp_triptych_desc_size", "vp_triptych_workspace_bytes", "vp_triptych_create", "vp_triptych_build", "vp_triptych_mask",
         "vp_triptych_fill_holes", "vp_triptych_blur_taps", "vp_triptych_tensor", "vp_triptych_destroy")


def test_header_declares_the_triptych_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.triptych as vt  # importable without a GPU
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  for name in NAMES:
    assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols(), name
  assert sorted(n for n in _lib.exported_symbols() if n.startswith("vp_triptych_")) == sorted(NAMES)
  body = hdr[hdr.index("typedef struct vp_triptych_desc {"):hdr.index("} vp_triptych_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.TriptychDesc._fields_]
  assert ctypes.sizeof(_lib.TriptychDesc) == 20 and _lib.DESC_SIZE_QUERIES["vp_triptych_desc_size"] is _lib.TriptychDesc
  assert "#define VP_TRIPTYCH_MAX_FRAMES %d" % _lib.TRIPTYCH_MAX_FRAMES in hdr and "#define VP_TRIPTYCH_MAX_SIZE %d" % _lib.TRIPTYCH_MAX_SIZE in hdr
  for cited in ("make_data_from_GRID.py:430-469", ":690-695", "binary_fill_holes", "REFLECT_101", "paste_geometry", "int(round())"):
    assert cited in hdr, cited
  mk = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  assert "triptych.hip" in mk.split("SRCS =")[1].split("\n")[0]
  assert "triptych.o" in [l for l in mk.splitlines() if "-ffp-contract=off" in l][0]      # no contraction in the float32 stages
  assert sorted(vt.STATUS) == [0, 1, 2, 3]
  d = vt.triptych_desc(256, 4)
  assert (d.struct_bytes, d.max_frames, d.size, d.face_size, d.max_side) == (20, 4, 256, 224, 256)


def test_library_answers_and_refuses_with_the_field_named():
  from voicepuppet_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libvp_hip.so is not built: desc_size, workspace_bytes, the taps and the refusals are unexercised")
  L = _lib.lib()
  for name in NAMES:
    assert hasattr(L, name), name
  n = ctypes.sizeof(_lib.TriptychDesc)
  assert L.vp_triptych_desc_size() == n
  q = (ctypes.c_int * 21)()
  assert L.vp_triptych_blur_taps(q) == 0 and list(q) == tr.blur_taps().tolist()
  assert L.vp_triptych_blur_taps(None) == -1
  # the planes of a 64-frame builder at 512: two of bytes, one of 32-bit sums, and the filled masks
  assert L.vp_triptych_workspace_bytes(ctypes.byref(_lib.TriptychDesc(n, 64, 512, 224, 512))) >= 64 * (512 * 512 * 6 + 224 * 224)
  for what, d in [("max_frames", _lib.TriptychDesc(n, 0, 256, 224, 256)), ("max_frames", _lib.TriptychDesc(n, 4097, 256, 224, 256)),
                  ("size", _lib.TriptychDesc(n, 1, 10, 224, 10)), ("size", _lib.TriptychDesc(n, 1, 1025, 224, 256)),
                  ("face_size", _lib.TriptychDesc(n, 1, 256, 1, 256)), ("face_size", _lib.TriptychDesc(n, 1, 256, 257, 256)),
                  ("max_side", _lib.TriptychDesc(n, 1, 256, 224, 10)), ("max_side", _lib.TriptychDesc(n, 1, 256, 224, 257)),
                  ("struct_bytes", _lib.TriptychDesc(n - 4, 1, 256, 224, 256))]:
    assert L.vp_triptych_workspace_bytes(ctypes.byref(d)) == 0 and what in L.vp_last_error().decode(), what
    h = ctypes.c_void_p()
    assert L.vp_triptych_create(ctypes.byref(d), None, 0, None, ctypes.byref(h)) == -1 and not h.value
    assert what in L.vp_last_error().decode()
  good = _lib.TriptychDesc(n, 2, 64, 224, 64)
  ws = L.vp_triptych_workspace_bytes(ctypes.byref(good))
  h = ctypes.c_void_p()
  assert L.vp_triptych_create(ctypes.byref(good), ctypes.c_void_p(4096), ws - 1, None, ctypes.byref(h)) == -3 and not h.value
  # the calls without a handle refuse what the host can check before anything is enqueued
  p = ctypes.c_void_p(1 << 20)
  for what, args in [("n ", (0, 8, 8)), ("height", (1, 257, 8)), ("height", (1, 0, 8)), ("width", (1, 8, 257)), ("width", (1, 8, 0))]:
    assert L.vp_triptych_fill_holes(p, args[0], args[1], args[2], p, None) == -1 and what in L.vp_last_error().decode(), what
  assert L.vp_triptych_fill_holes(None, 1, 8, 8, p, None) == -1
  assert L.vp_triptych_build(None, p, p, p, p, None, 1, p, p, None) == -1 and L.vp_triptych_mask(None, p, p, 1, 1, None) == -1
  assert L.vp_triptych_tensor(None, b"mask", ctypes.byref(ctypes.c_void_p()), None) == -1

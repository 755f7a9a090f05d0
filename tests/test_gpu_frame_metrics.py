"""The device frame metrics (libvp_hip.so vp_frame_metrics_*, voicepuppet_amd.metrics.FrameMetrics) against the float64 numpy restatement
(tests/frame_metrics_ref.py, pinned in tests/test_frame_metrics_host.py): integer sums exactly, L1 and MSE to 1 ulp, PSNR and SSIM within
1e-9, batch rows and repeated calls bit for bit, padded and poisoned layouts, the float32 entry, refusals.

Shapes: the smallest that can still go wrong - one window, one row / column of windows across tile edges, exactly one tile and ragged
tiles both for tiles of 32 and for the 16 x 16 windows (26 x 26 values) the kernel uses, whole tiles, and one 256 x 768 frame."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_metrics_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(11, 11), (11, 43), (43, 11), (26, 26), (27, 59), (42, 42), (43, 75), (64, 96)]
KINDS = ["noise", "ramp", "identical", "extremes", "corner"]
TOL = 1e-9
_CACHE = {}


def _pair(kind, h, w, seed):
  """one uint8 frame pair [h, w, 3]"""
  rng = np.random.default_rng(seed)
  noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
  if kind == "noise":
    return noise, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
  if kind == "ramp":                                   # a smooth ramp and its copy with +-12 of noise (the JPEG tests' content)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 5) % 256], -1).astype(np.int64)
    return a.astype(np.uint8), (a + rng.integers(-12, 13, a.shape)).clip(0, 255).astype(np.uint8)
  if kind == "identical":
    return noise, noise.copy()
  if kind == "extremes":
    return np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
  b = noise.copy()                                     # "corner": one value of one corner pixel differs; the corner turns with the seed
  y, x = [(h - 1, w - 1), (0, 0), (h - 1, 0), (0, w - 1)][seed % 4]
  b[y, x, seed % 3] ^= 0x80
  return noise, b


def _case(kind, h, w, n=3):
  """(a, b uint8 [n, h, w, 3], restatement [n, 4], integer sums [n, 2]) - computed once and shared"""
  key = (kind, h, w, n)
  if key not in _CACHE:
    pairs = [_pair(kind, h, w, 100 * h + w + i) for i in range(n)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want, sums = fr.batch(a, b), np.array([fr.sums(x, y) for x, y in zip(a, b)], np.int64)
    for arr in (a, b, want, sums):
      arr.setflags(write=False)
    _CACHE[key] = (a, b, want, sums)
  return _CACHE[key]


def _fm():
  from voicepuppet_amd.metrics import FrameMetrics
  if "fm" not in _CACHE:
    _CACHE["fm"] = FrameMetrics(4, 256, 768)
  return _CACHE["fm"]


def _dev(x):
  import torch
  return torch.tensor(np.asarray(x), device="cuda")


def _ulp_close(got, want):
  return np.all(np.abs(got - want) <= np.spacing(np.abs(want)))


def _check(got, want, exact_means):
  print("max |diff| L1 %.3g MSE %.3g SSIM %.3g" % tuple(np.abs(got[:, j] - want[:, j]).max() for j in (0, 1, 3)))
  if exact_means:
    assert _ulp_close(got[:, 0], want[:, 0]) and _ulp_close(got[:, 1], want[:, 1])
  else:
    assert np.abs(got[:, :2] - want[:, :2]).max() <= TOL
  inf = np.isinf(want[:, 2])
  assert np.array_equal(np.isinf(got[:, 2]), inf) and (got[inf, 2] > 0).all()
  assert np.abs(got[~inf, 2] - want[~inf, 2]).max(initial=0.0) <= TOL
  assert np.abs(got[:, 3] - want[:, 3]).max() <= TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_u8_equals_the_restatement(h, w, kind):
  a, b, want, sums = _case(kind, h, w)
  fm = _fm()
  da, db = _dev(a), _dev(b)
  got_t = fm.compare(da, db)
  got = got_t.cpu().numpy()
  assert np.array_equal(fm.tensor("abs_sum")[:3].cpu().numpy(), sums[:, 0]) and np.array_equal(fm.tensor("sq_sum")[:3].cpu().numpy(), sums[:, 1])
  _check(got, want, exact_means=True)
  # a frame's row does not depend on the batch around it, nor a call on the one before it: bit for bit
  for i in range(3):
    alone = fm.compare(da[i:i + 1], db[i:i + 1]).cpu().numpy()
    assert alone.tobytes() == got[i:i + 1].tobytes(), i
  assert fm.compare(da, db).cpu().numpy().tobytes() == got.tobytes()


def test_u8_one_large_frame():
  a, b, want, sums = _case("ramp", 256, 768, n=1)
  fm = _fm()
  got = fm.compare(_dev(a), _dev(b)).cpu().numpy()
  assert int(fm.tensor("abs_sum")[0]) == sums[0, 0] and int(fm.tensor("sq_sum")[0]) == sums[0, 1]
  _check(got, want, exact_means=True)
  assert fm.compare(_dev(a), _dev(b)).cpu().numpy().tobytes() == got.tobytes()


def _embed(x, pitch_extra, lead, slack, fill, frames_extra=1):
  """x [n, h, w, 3] inside a larger buffer full of `fill`: rows pitch_extra ELEMENTS longer than 3 w, `slack` rows behind every frame, `lead`
  rows in front of the first and frames_extra frames behind the last -> (the view of x's values, the whole buffer)"""
  import torch
  n, h, w, _ = x.shape
  row = 3 * w + pitch_extra
  buf = torch.full((lead + (n + frames_extra) * (h + slack), row), fill, dtype=torch.tensor(x[:0]).dtype, device="cuda")
  view = buf[lead:lead + n * (h + slack)].view(n, h + slack, row)[:, :h, :3 * w].unflatten(2, (w, 3))
  view.copy_(_dev(x))
  return view, buf


@pytest.mark.parametrize("h,w", [(11, 11), (43, 75), (27, 59)])
def test_padded_and_poisoned_layouts_change_nothing(h, w):
  """a's rows 16 bytes wider than 3 w with 2 rows of slack per frame, b's 32 bytes wider with 5: the values beyond W, H and n are 0xFF
  (uint8) or NaN (float32) and the results are the dense ones bit for bit - nothing outside the arguments is read."""
  a, b, want, sums = _case("noise", h, w)
  fm = _fm()
  dense = fm.compare(_dev(a), _dev(b)).cpu().numpy()
  va, _ = _embed(a, 16, 1, 2, 0xFF)
  vb, _ = _embed(b, 32, 3, 5, 0xFF)
  assert va.stride(1) == 3 * w + 16 and vb.stride(1) == 3 * w + 32 and va.stride(0) != vb.stride(0) and not va.is_contiguous()
  got = fm.compare(va, vb).cpu().numpy()
  assert got.tobytes() == dense.tobytes()
  assert np.array_equal(fm.tensor("abs_sum")[:3].cpu().numpy(), sums[:, 0])
  mixed = fm.compare(va, _dev(b)).cpu().numpy()                      # a padded decoder output against a dense tensor
  assert mixed.tobytes() == dense.tobytes()
  fa, fb = a.astype(np.float32), b.astype(np.float32)
  fdense = fm.compare(_dev(fa), _dev(fb), value_range=(0, 255)).cpu().numpy()
  wa, _ = _embed(fa, 4, 1, 2, float("nan"))                          # 16 bytes
  wb, _ = _embed(fb, 8, 3, 5, float("nan"))
  fgot = fm.compare(wa, wb, value_range=(0, 255)).cpu().numpy()
  assert fgot.tobytes() == fdense.tobytes() and np.isfinite(fgot[:, [0, 1, 3]]).all()


@pytest.mark.parametrize("h,w", SHAPES + [(256, 768)])
def test_f32_equals_the_restatement_on_the_mapped_doubles(h, w):
  """float32 in about [-1.2, 1.2] at value_range (-1, 1): values outside are clamped, the rest maps without rounding"""
  n = 1 if h == 256 else 3
  rng = np.random.default_rng(7 * h + w)
  xa = rng.uniform(-1.2, 1.2, (n, h, w, 3)).astype(np.float32)
  xb = (xa + rng.normal(0, 0.1, xa.shape)).astype(np.float32)
  xb[0, 0, 0, 0], xa[0, -1, -1, 2] = 7.0, -9.0                       # far outside: 255 and 0
  want = fr.batch(fr.map_f32(xa), fr.map_f32(xb))
  fm = _fm()
  got = fm.compare(_dev(xa), _dev(xb), value_range=(-1, 1)).cpu().numpy()
  _check(got, want, exact_means=False)
  clamped = fm.compare(_dev(np.clip(xa, -1, 1)), _dev(np.clip(xb, -1, 1))).cpu().numpy()
  assert np.abs(clamped - got).max() <= TOL
  for i in range(n):
    assert fm.compare(_dev(xa[i:i + 1]), _dev(xb[i:i + 1])).cpu().numpy().tobytes() == got[i:i + 1].tobytes()
  assert fm.compare(_dev(xa), _dev(xb)).cpu().numpy().tobytes() == got.tobytes()


def test_f32_of_uint8_values_gives_the_uint8_result():
  """u / 127.5 - 1 is a float32 exactly for u = 0 and 255 only: a frame pair of those two values gives the uint8 numbers within 1e-9 at
  value_range (-1, 1), and so does every u at (0, 255), where float32(u) is exact.  For the other u float32(u / 127.5 - 1) is off by up to
  2^-25 (half an ulp of values under 1), e = 127.5 * 2^-25 = 3.8e-6 after the mapping, which has no rounding to take it back: L1 then agrees
  within 2 e, and MSE, PSNR and SSIM within the bounds that follow from e (derived where they are asserted)."""
  import torch
  fm = _fm()
  rng = np.random.default_rng(3)
  a = (rng.integers(0, 2, (2, 43, 75, 3)) * 255).astype(np.uint8)
  b = (rng.integers(0, 2, (2, 43, 75, 3)) * 255).astype(np.uint8)
  a[:, 5:30, 5:60] = b[:, 5:30, 5:60]                                # some structure in common: SSIM away from 0
  want = fm.compare(_dev(a), _dev(b)).cpu().numpy()
  assert np.abs(want - fr.batch(a, b)).max() <= TOL
  to_f = lambda u: (u.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
  assert np.array_equal(fr.map_f32(to_f(a)), a.astype(np.float64))
  got = fm.compare(_dev(to_f(a)), _dev(to_f(b)), value_range=(-1, 1)).cpu().numpy()
  assert np.abs(got - want).max() <= TOL
  a, b, want, _ = _case("ramp", 43, 75)
  got = fm.compare(_dev(a.astype(np.float32)), _dev(b.astype(np.float32)), value_range=(0, 255)).cpu().numpy()
  assert np.abs(got - want).max() <= TOL
  near = fm.compare(_dev(to_f(a)), _dev(to_f(b)), value_range=(-1, 1)).cpu().numpy()
  print("uint8 values through (-1, 1): max |L1 diff| %.3g" % np.abs(near[:, 0] - want[:, 0]).max())
  e = 127.5 * 2.0 ** -25                                             # per value; a difference a - b moves by at most 2 e
  assert np.abs(near[:, 0] - want[:, 0]).max() <= 2 * e
  # (d + 2 e)^2 - d^2 with |d| <= 255; PSNR by its derivative 10 / (ln 10 MSE) at the smaller MSE
  mse_bound = 2 * 255 * 2 * e + 4 * e * e
  assert np.abs(near[:, 1] - want[:, 1]).max() <= mse_bound
  assert np.all(np.abs(near[:, 2] - want[:, 2]) <= 10 / np.log(10) * mse_bound / (want[:, 1] - mse_bound))
  # S = (A / C)(B / D), both factors at most 1 in size, C >= C1, D >= C2; means move by e, second moments by 2 * 255 e, so A and C by
  # 4 * 255 e and B and D by 8 * 255 e: |dS| <= (4 + 4) 255 e / C1 + (8 + 8) 255 e / C2
  assert np.abs(near[:, 3] - want[:, 3]).max() <= 255 * e * (8 / fr.C1 + 16 / fr.C2)
  assert isinstance(got, np.ndarray) and torch.is_tensor(fm.compare(_dev(a), _dev(b)))


def test_refusals_enqueue_nothing():
  """n > max_frames, a size over the descriptor's, width < 11, a pitch smaller than the row: an error with the reason, and `out` untouched"""
  import torch
  from voicepuppet_amd.metrics import FrameMetrics
  fm = FrameMetrics(2, 32, 48)
  L = fm.L
  buf = torch.zeros(3 * 32 * 48 * 3 + 64, dtype=torch.uint8, device="cuda")
  out = torch.full((4, 4), -7.0, dtype=torch.float64, device="cuda")
  p, o = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr())
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def u8(n, h, w, pitch=None, stride=None, b_pitch=None):
    pitch = 3 * w if pitch is None else pitch
    stride = h * pitch if stride is None else stride
    bp = pitch if b_pitch is None else b_pitch
    return L.vp_frame_metrics_u8(fm.h, p, pitch, stride, p, bp, max(stride, h * bp), n, h, w, o, st), L.vp_last_error().decode()

  for what, call in [("max_frames", lambda: u8(3, 32, 48)), ("max_height", lambda: u8(1, 33, 48)), ("max_width", lambda: u8(1, 32, 49)),
                     ("width 10", lambda: u8(1, 32, 10)), ("height 10", lambda: u8(1, 10, 48)),
                     ("a_row_pitch", lambda: u8(1, 32, 48, pitch=3 * 48 - 1, stride=32 * 3 * 48, b_pitch=3 * 48)),
                     ("b_row_pitch", lambda: u8(1, 32, 48, b_pitch=3 * 48 - 16)),
                     ("a_frame_stride", lambda: u8(2, 32, 48, stride=31 * 3 * 48))]:
    rc, err = call()
    assert rc == -1 and what in err, (what, rc, err)
  fp = ctypes.c_void_p(buf.data_ptr())
  rc = L.vp_frame_metrics_f32(fm.h, fp, 12 * 20 - 4, 12 * 20 * 16, fp, 12 * 20, 12 * 20 * 16, 1, 16, 20, 127.5, 127.5, o, st)
  assert rc == -1 and "a_row_pitch" in L.vp_last_error().decode()
  with pytest.raises(ValueError):
    fm.compare(buf[:32 * 48 * 3].view(1, 32, 48, 3), buf[:32 * 48 * 3].view(1, 32, 48, 3).float(), value_range=(0, 255))
  with pytest.raises(ValueError):
    fm.compare(buf[:32 * 48 * 3].view(1, 32, 48, 3).float(), buf[:32 * 48 * 3].view(1, 32, 48, 3).float(), value_range=(0, 2))
  with pytest.raises(ValueError):                                    # columns two pixels apart
    fm.compare(buf[:32 * 48 * 3].view(1, 32, 48, 3)[:, :, ::2], buf[:32 * 48 * 3].view(1, 32, 48, 3)[:, :, ::2])
  with pytest.raises(RuntimeError, match="max_frames"):
    fm.compare(buf[:3 * 32 * 48 * 3].view(3, 32, 48, 3), buf[:3 * 32 * 48 * 3].view(3, 32, 48, 3))
  torch.cuda.synchronize()
  assert (out == -7.0).all()
  good = fm.compare(buf[:2 * 32 * 48 * 3].view(2, 32, 48, 3), buf[:2 * 32 * 48 * 3].view(2, 32, 48, 3), out=out)
  assert good.data_ptr() == out.data_ptr() and good.cpu().numpy()[:, 0].tolist() == [0.0, 0.0] and (out[2:] == -7.0).all()

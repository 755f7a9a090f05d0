"""numpy restatement of the key matte (include/vp_hip.h, vp_keymatte_*), written from the header's text: the border moments in Python
integers, SOLVE in Python floats in the header's order, APPLY in float64 arrays in the header's order, the window sums by shifted-array
accumulation in increasing offset (for one pixel: the window's columns in increasing x from +0.0, then its rows in increasing y from
+0.0).  numpy contracts nothing into a fused multiply-add.  And the synthetic studio scene the tests and the quality figures use."""
import numpy as np

MODEL_DOUBLES = 19
N, KEPT, RESIDUAL_RMS, STATUS = 15, 16, 17, 18
DEFAULTS = dict(trim=16.0, sigma_min=2.0, lo=4.0, hi=10.0, radius=4, eps=25.0)


def default_band(H):
  return max(2, H // 16)


def sample_mask(H, W, band=None, side_rows=None):
  band = default_band(H) if band is None else band
  side_rows = H // 2 if side_rows is None else side_rows
  assert 1 <= band and 2 * band <= W and band <= side_rows <= H
  yy, xx = np.mgrid[0:H, 0:W]
  return (yy < band) | ((yy < side_rows) & ((xx < band) | (xx >= W - band)))


def moments(frames, mask):
  """frames uint8 [n, H, W, 3]; mask bool [H, W] or [n, H, W] -> the 21 moments as Python integers (exact)."""
  n, H, W, _ = frames.shape
  mask = np.broadcast_to(mask, (n, H, W))
  yy, xx = np.mgrid[0:H, 0:W]
  v = np.stack([np.broadcast_to(xx, (n, H, W)), np.broadcast_to(yy, (n, H, W)), frames[..., 0], frames[..., 1], frames[..., 2],
                np.ones((n, H, W), np.int64)], -1).astype(np.int64)[mask]
  out = []
  for i in range(6):
    for j in range(i, 6):
      out.append(int((v[:, i] * v[:, j]).sum(dtype=np.int64)))
  return out


def solve(S, sigma_min=2.0):
  """SOLVE: the 21 moments -> the model record, float64 [19]"""
  m = [0.0] * MODEL_DOUBLES
  s2 = float(sigma_min) * float(sigma_min)
  n = int(S[20])
  m[KEPT] = 1.0
  if n < 1:
    m[9] = m[12] = m[14] = 1.0 / s2
    m[STATUS] = 1.0
    return np.array(m, np.float64)
  Nd = float(n)
  nn = Nd * Nd
  f = lambda i: float(int(S[i])) / Nd                 # float(int) is the nearest double

  def cen(ab, a, b):
    """(double)(N Sab - Sa Sb) / (Nd Nd): the integer exact, converted by its magnitude's two 64-bit halves"""
    v = n * int(S[ab]) - int(S[a]) * int(S[b])
    u = abs(v)
    d = float(u >> 64) * 18446744073709551616.0 + float(u & 0xFFFFFFFFFFFFFFFF)
    return (-d if v < 0 else d) / nn
  mx, my = f(5), f(10)
  mc = [f(14), f(17), f(19)]
  Cxx, Cxy, Cyy = cen(0, 5, 5), cen(1, 5, 10), cen(6, 10, 10)
  Cxc = [cen(2, 5, 14), cen(3, 5, 17), cen(4, 5, 19)]
  Cyc = [cen(7, 10, 14), cen(8, 10, 17), cen(9, 10, 19)]
  C00, C01, C02 = cen(11, 14, 14), cen(12, 14, 17), cen(13, 14, 19)
  C11, C12, C22 = cen(15, 17, 17), cen(16, 17, 19), cen(18, 19, 19)
  det = Cxx * Cyy - Cxy * Cxy
  degenerate = n < 16 or not (det > 1e-9 * (Cxx * Cyy))
  px, py = [0.0] * 3, [0.0] * 3
  for c in range(3):
    if not degenerate:
      px[c] = (Cxc[c] * Cyy - Cyc[c] * Cxy) / det
      py[c] = (Cyc[c] * Cxx - Cxc[c] * Cxy) / det
    m[3 * c] = (mc[c] - px[c] * mx) - py[c] * my
    m[3 * c + 1], m[3 * c + 2] = px[c], py[c]
  R00 = (C00 - px[0] * Cxc[0]) - py[0] * Cyc[0]
  R01 = (C01 - px[0] * Cxc[1]) - py[0] * Cyc[1]
  R02 = (C02 - px[0] * Cxc[2]) - py[0] * Cyc[2]
  R11 = (C11 - px[1] * Cxc[1]) - py[1] * Cyc[1]
  R12 = (C12 - px[1] * Cxc[2]) - py[1] * Cyc[2]
  R22 = (C22 - px[2] * Cxc[2]) - py[2] * Cyc[2]
  R00, R11, R22 = max(R00, 0.0), max(R11, 0.0), max(R22, 0.0)
  m[RESIDUAL_RMS] = float(np.sqrt(np.float64(((R00 + R11) + R22) / 3.0)))
  a, b, c, d, e, f_ = R00 + s2, R01, R02, R11 + s2, R12, R22 + s2
  A00, A01, A02 = d * f_ - e * e, c * e - b * f_, b * e - c * d
  A11, A12, A22 = a * f_ - c * c, b * c - a * e, a * d - b * b
  D = (a * A00 + b * A01) + c * A02
  if D > 0.0:
    m[9:15] = [A00 / D, A01 / D, A02 / D, A11 / D, A12 / D, A22 / D]
  else:
    m[9:15] = [1.0 / s2, 0.0, 0.0, 1.0 / s2, 0.0, 1.0 / s2]
    degenerate = True
  m[N] = Nd
  m[STATUS] = 1.0 if degenerate else 0.0
  return np.array(m, np.float64)


def d2(model, frames):
  """-> float64 [n, H, W]"""
  m = [np.float64(v) for v in model]
  n, H, W, _ = frames.shape
  yy, xx = np.mgrid[0:H, 0:W]
  xd, yd = xx.astype(np.float64), yy.astype(np.float64)
  c = frames.astype(np.float64)
  r0 = c[..., 0] - ((m[0] + m[1] * xd) + m[2] * yd)
  r1 = c[..., 1] - ((m[3] + m[4] * xd) + m[5] * yd)
  r2 = c[..., 2] - ((m[6] + m[7] * xd) + m[8] * yd)
  q0 = (m[9] * r0 + m[10] * r1) + m[11] * r2
  q1 = (m[10] * r0 + m[12] * r1) + m[13] * r2
  q2 = (m[11] * r0 + m[13] * r1) + m[14] * r2
  return (r0 * q0 + r1 * q1) + r2 * q2


def fit(frames, band=None, side_rows=None, trim=16.0, sigma_min=2.0):
  """-> (moments int64 [2, 21], model float64 [19]) of the two passes"""
  n, H, W, _ = frames.shape
  mask = sample_mask(H, W, band, side_rows)
  S1 = moments(frames, mask)
  first = solve(S1, sigma_min)
  S2 = moments(frames, mask[None] & (d2(first, frames) <= trim))
  model = solve(S2, sigma_min)
  model[KEPT] = float(S2[20]) / float(S1[20]) if S1[20] > 0 else 0.0
  return np.array([S1, S2], np.int64), model


def raw_key(model, frames, lo=4.0, hi=10.0):
  lo2, den = float(lo) * float(lo), float(hi) * float(hi) - float(lo) * float(lo)
  with np.errstate(invalid="ignore"):
    t = np.fmin(np.fmax((d2(model, frames) - lo2) / den, 0.0), 1.0)
  a = (t * t) * (3.0 - 2.0 * t)
  return np.floor(255.0 * a + 0.5).astype(np.uint8)


def guide(frames):
  c = frames.astype(np.int64)
  return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def _box(a, r, axis):
  """sum over the window [i - r, i + r] clipped to the array, accumulated in increasing offset from zero"""
  out = np.zeros_like(a)
  size = a.shape[axis]
  for d in range(-r, r + 1):
    lo, hi = max(0, -d), min(size, size - d)
    if lo >= hi:
      continue
    dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
    out[tuple(dst)] += a[tuple(src)]
  return out


def _window(a, r):
  return _box(_box(a, r, -1), r, -2)              # per row over its columns first, then over the rows


def guided(I, p, radius=4, eps=25.0):
  """I int64 [n, H, W] the guide, p uint8 [n, H, W] the raw key -> the matte, uint8"""
  if radius == 0:
    return p.copy()
  I, p = I.astype(np.int64), p.astype(np.int64)
  nw = _window(np.ones_like(I), radius)
  sI, sp, sII, sIp = _window(I, radius), _window(p, radius), _window(I * I, radius), _window(I * p, radius)
  ak = (sIp * nw - sI * sp).astype(np.float64) / ((sII * nw - sI * sI).astype(np.float64) + float(eps) * (nw * nw).astype(np.float64))
  bk = (sp.astype(np.float64) - ak * sI.astype(np.float64)) / nw.astype(np.float64)
  sa, sb = _window(ak, radius), _window(bk, radius)
  nwd = nw.astype(np.float64)
  q = (sa / nwd) * I.astype(np.float64) + sb / nwd
  return np.floor(np.fmin(np.fmax(q, 0.0), 255.0) + 0.5).astype(np.uint8)


def matte(model, frames, lo=4.0, hi=10.0, radius=4, eps=25.0):
  """-> (raw key, matte), uint8 [n, H, W] each"""
  p = raw_key(model, frames, lo, hi)
  return p, guided(guide(frames), p, radius, eps)


# ---- the synthetic studio scene ---------------------------------------------------------------------------------------------------------
def scene(H, W, seed=0, n=1, noise=3.0):
  """A head (textured ellipse) and shoulders (textured trapezoid leaving through the bottom edge) in front of a backdrop that is a plane
  gradient per channel plus Gaussian noise of `noise` levels, composited with a known alpha whose edge ramp is 3 pixels wide.
  -> (frames uint8 [n, H, W, 3], alpha float64 [n, H, W]); the frames of a scene differ by noise and a small sway of the head."""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
  u, v = xx / W, yy / H
  back = np.stack([70.0 + 24.0 * u + 10.0 * v, 150.0 - 14.0 * u + 18.0 * v, 95.0 + 8.0 * u - 12.0 * v], -1)
  frames, alphas = [], []
  for k in range(n):
    cx, cy, ax, ay = W * (0.5 + 0.01 * k), H * 0.40, W * 0.20, H * 0.24
    ex, ey = (xx - cx) / ax, (yy - cy) / ay
    rho = np.sqrt(ex * ex + ey * ey) + 1e-12
    grad = np.sqrt((ex / ax) ** 2 + (ey / ay) ** 2) / rho + 1e-12
    head = np.clip(0.5 - ((rho - 1.0) / grad) / 3.0, 0.0, 1.0)
    top, half0, half1 = H * 0.68, W * 0.16, W * 0.46                    # the trapezoid: its top edge and its half widths at the top and at y = H
    slope = (half1 - half0) / (H - top)
    norm = np.sqrt(1.0 + slope * slope)
    side = (np.abs(xx - W * 0.5) - (half0 + slope * (yy - top))) / norm
    torso = np.clip(0.5 - np.maximum(top - yy, side) / 3.0, 0.0, 1.0)
    alpha = np.maximum(head, torso)
    tex = 12.0 * np.sin(xx * 0.9 + k) * np.cos(yy * 0.7)
    skin = np.stack([205.0 + tex, 160.0 + 0.8 * tex, 135.0 - 0.5 * tex], -1)
    cloth = np.stack([40.0 + 0.5 * tex, 45.0 + tex, 60.0 - tex], -1)
    fore = np.where((head >= torso)[..., None], skin, cloth) + rng.normal(0.0, 2.0, (H, W, 3))
    img = alpha[..., None] * fore + (1.0 - alpha[..., None]) * (back + rng.normal(0.0, noise, (H, W, 3)))
    frames.append(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8))
    alphas.append(alpha)
  return np.stack(frames), np.stack(alphas)


def quality(matte_u8, alpha):
  """(mean absolute error, share of pixels off by more than 0.25) of a uint8 matte against the known alpha"""
  err = np.abs(matte_u8.astype(np.float64) / 255.0 - alpha)
  return float(err.mean()), float((err > 0.25).mean())

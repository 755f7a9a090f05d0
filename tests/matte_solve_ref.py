"""numpy restatement of the trimap and the closed-form matting solve (include/vp_hip.h, vp_mattesolve_*), written from the header's text:
`trimap`, `Laplacian` (`apply`, `diag`) and `solve`, a Jacobi-preconditioned conjugate-gradient run with a pluggable dot product.  Every
float routine takes its number format (numpy.float64, or numpy.longdouble for the tolerance measurements).  And the cluttered-backdrop
variant of matte_clean_ref.scene the quality figures use."""
import math

import numpy as np

import matte_clean_ref as mr

REPORT_INTS = 8
STATUS_NO_CONSTRAINT, STATUS_BREAKDOWN = 1, 2


def default_erode(H, W):
  return max(5, min(64, min(H, W) // 19))


def default_dilate(H, W):
  return max(5, min(64, min(H, W) // 29))


# ---- trimap -------------------------------------------------------------------------------------------------------------------------------
def _square(B, k, erode):
  """B bool [H, W] -> the erosion (AND) or dilation (OR) over the offsets -(k // 2) .. k - 1 - (k // 2) on both axes, clipped to the image"""
  H, W = B.shape
  out = B
  for axis, size in ((1, W), (0, H)):
    src, acc = out, out.copy()
    for d in range(-(k // 2), k - (k // 2)):
      lo, hi = max(0, -d), min(size, size - d)
      if lo >= hi or d == 0:
        continue
      dst, s = [slice(None)] * 2, [slice(None)] * 2
      dst[axis], s[axis] = slice(lo, hi), slice(lo + d, hi + d)
      if erode:
        acc[tuple(dst)] &= src[tuple(s)]
      else:
        acc[tuple(dst)] |= src[tuple(s)]
    out = acc
  return out


def trimap(matte, support=32, core=224, erode=None, dilate=None):
  """matte uint8 [n, H, W] -> uint8 [n, H, W]: 255 on fg, else 127 on maybe, else 0"""
  n, H, W = matte.shape
  erode = default_erode(H, W) if erode is None else erode
  dilate = default_dilate(H, W) if dilate is None else dilate
  out = np.zeros(matte.shape, np.uint8)
  for f in range(n):
    fg = _square(matte[f] >= core, erode, True)
    maybe = _square(matte[f] >= support, dilate, False)
    out[f] = np.where(fg, 255, np.where(maybe, 127, 0))
  return out


def trimap_brute(m, support, core, erode, dilate):
  """the definition itself, pixel by pixel: m uint8 [H, W]"""
  H, W = m.shape
  out = np.zeros((H, W), np.uint8)
  for y in range(H):
    for x in range(W):
      def window(k):
        return m[max(0, y - k // 2):min(H, y + k - k // 2), max(0, x - k // 2):min(W, x + k - k // 2)]
      out[y, x] = 255 if window(erode).min() >= core else (127 if window(dilate).max() >= support else 0)
  return out


# ---- the matting Laplacian ----------------------------------------------------------------------------------------------------------------
def box(a, r):
  """a [H, W, ...] -> the sum over the (2 r + 1)^2 window clipped to the image, rows in increasing y, within a row increasing x"""
  H, W = a.shape[:2]
  P = np.zeros((H + 2 * r, W + 2 * r) + a.shape[2:], a.dtype)
  P[r:r + H, r:r + W] = a
  out = np.zeros(a.shape, a.dtype)
  for dy in range(2 * r + 1):
    for dx in range(2 * r + 1):
      out = out + P[dy:dy + H, dx:dx + W]
  return out


class Laplacian:
  """L of the header for one frame uint8 [H, W, 3]"""

  def __init__(self, frame, radius=1, eps=1.0, dtype=np.float64):
    self.r, self.dtype = int(radius), dtype
    I = frame.astype(np.int64)
    H, W = I.shape[:2]
    self.H, self.W = H, W
    n = box(np.ones((H, W), np.int64), self.r)
    S = box(I, self.r)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    S2 = box(np.stack([I[..., c] * I[..., d] for c, d in pairs], -1), self.r)
    nd = n.astype(dtype)
    self.n, self.I = nd, I.astype(dtype)
    self.mu = S.astype(dtype) / nd[..., None]
    C = [(n * S2[..., k] - S[..., c] * S[..., d]).astype(dtype) / (nd * nd) for k, (c, d) in enumerate(pairs)]
    reg = dtype(eps) / nd
    a, b, c, d, e, f = C[0] + reg, C[1], C[2], C[3] + reg, C[4], C[5] + reg
    A00, A01, A02, A11, A12, A22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
    D = (a * A00 + b * A01) + c * A02
    self.inv = [A00 / D, A01 / D, A02 / D, A11 / D, A12 / D, A22 / D]

  def _mul(self, v):
    """Inv v for v [H, W, 3] (or three planes)"""
    i = self.inv
    return [(i[0] * v[0] + i[1] * v[1]) + i[2] * v[2], (i[1] * v[0] + i[3] * v[1]) + i[4] * v[2], (i[2] * v[0] + i[4] * v[1]) + i[5] * v[2]]

  def apply(self, p):
    """p [H, W] -> L p, no masking"""
    p = p.astype(self.dtype)
    mp = box(p, self.r) / self.n
    mIp = box(self.I * p[..., None], self.r) / self.n[..., None]
    a = self._mul([mIp[..., c] - self.mu[..., c] * mp for c in range(3)])
    b = mp - ((a[0] * self.mu[..., 0] + a[1] * self.mu[..., 1]) + a[2] * self.mu[..., 2])
    sa, sb = box(np.stack(a, -1), self.r), box(b, self.r)
    return self.n * p - (((sa[..., 0] * self.I[..., 0] + sa[..., 1] * self.I[..., 1]) + sa[..., 2] * self.I[..., 2]) + sb)

  def diag(self):
    """diag(L)_i = sum over the windows j that hold i of 1 - (1 + (I_i - mu_j)' Inv_j (I_i - mu_j)) / n_j"""
    r, H, W = self.r, self.H, self.W
    pad = lambda a: np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2))
    inside, mu, n = pad(np.ones((H, W), bool)), pad(self.mu), pad(self.n)
    inv = [pad(v) for v in self.inv]
    out = np.zeros((H, W), self.dtype)
    one = self.dtype(1)
    for dy in range(2 * r + 1):
      for dx in range(2 * r + 1):
        s = (slice(dy, dy + H), slice(dx, dx + W))
        d = [self.I[..., c] - mu[s][..., c] for c in range(3)]
        i = [v[s] for v in inv]
        q = [(i[0] * d[0] + i[1] * d[1]) + i[2] * d[2], (i[1] * d[0] + i[3] * d[1]) + i[4] * d[2], (i[2] * d[0] + i[4] * d[1]) + i[5] * d[2]]
        m = (d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]
        with np.errstate(divide="ignore", invalid="ignore"):
          term = one - (one + m) / n[s]
        out = out + np.where(inside[s], term, 0)
    return out

  def dense(self):
    """[H W, H W]: column i is apply(e_i)"""
    N = self.H * self.W
    out = np.empty((N, N), self.dtype)
    for i in range(N):
      e = np.zeros(N, self.dtype)
      e[i] = 1
      out[:, i] = self.apply(e.reshape(self.H, self.W)).ravel()
    return out


# ---- dot products -------------------------------------------------------------------------------------------------------------------------
def dot_sum(a, b):
  return np.sum(a * b)


def dot_fsum(a, b):
  return a.dtype.type(math.fsum((a * b).tolist())) if a.dtype == np.float64 else np.sum(a * b)


def dot_running(a, b):
  s = a.dtype.type(0)
  for v in (a * b).tolist() if a.dtype == np.float64 else (a * b):
    s = s + v
  return a.dtype.type(s)


DOTS = {"sum": dot_sum, "fsum": dot_fsum, "running": dot_running}


# ---- the solve ----------------------------------------------------------------------------------------------------------------------------
def solve_frame(frame, tri, radius=1, eps=1.0, iters=200, tol=1e-6, dot=dot_fsum, dtype=np.float64):
  """frame uint8 [H, W, 3], tri uint8 [H, W] -> dict(alpha [H, W] unclamped with k on the known pixels, matte uint8, unknown, iterations,
  status, residual)"""
  L = Laplacian(frame, radius, eps, dtype)
  U = (tri != 0) & (tri != 255)
  k = (tri == 255).astype(dtype)
  x = np.zeros(tri.shape, dtype)
  res = dict(unknown=int(U.sum()), iterations=0, status=STATUS_NO_CONSTRAINT, residual=0.0)      # b.b = 0 without an unknown pixel too
  if U.any():
    res["status"] = 0
    b = np.where(U, -L.apply(k), 0).astype(dtype)
    dinv = np.where(U, 1 / np.where(U, L.diag(), 1), 0).astype(dtype)
    bb = dot(b[U], b[U])
    if bb == 0:
      res["status"] = STATUS_NO_CONSTRAINT
    else:
      r = b.copy()
      z = dinv * r
      p = z.copy()
      rz = dot(r[U], z[U])
      rr = bb
      limit = dtype(tol) * dtype(tol) * bb
      it = 0
      while it < iters and not rr <= limit:
        Ap = np.where(U, L.apply(p), 0)
        pAp = dot(p[U], Ap[U])
        if not (pAp > 0 and np.isfinite(pAp)):
          res["status"] = STATUS_BREAKDOWN
          break
        a = rz / pAp
        x = x + a * p
        r = r - a * Ap
        z = dinv * r
        rr = dot(r[U], r[U])
        rz_new = dot(r[U], z[U])
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
      res["iterations"], res["residual"] = it, float(np.sqrt(rr / bb))
  res["alpha"] = np.where(U, x, k)
  res["matte"] = np.where(U, np.floor(np.minimum(np.maximum(x, 0), 1) * 255 + dtype(0.5)), k * 255).astype(np.uint8)
  return res


def solve(frames, tri, **kw):
  """frames uint8 [n, H, W, 3], tri uint8 [n, H, W] -> (alpha [n, H, W], matte uint8 [n, H, W], report: list of the per-frame dicts)"""
  res = [solve_frame(frames[f], tri[f], **kw) for f in range(frames.shape[0])]
  return np.stack([r["alpha"] for r in res]), np.stack([r["matte"] for r in res]), res


def solve_dense(frame, tri, radius=1, eps=1.0):
  """numpy.linalg.solve on the unknown block -> alpha [H, W]"""
  L = Laplacian(frame, radius, eps)
  A = L.dense()
  U = ((tri != 0) & (tri != 255)).ravel()
  k = (tri == 255).astype(np.float64).ravel()
  x = k.copy()
  x[U] = np.linalg.solve(A[np.ix_(U, U)], -(A @ k)[U])
  return x.reshape(tri.shape)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def clutter_scene(H, W, seed=0, n=1, noise=3.0):
  """The subject of matte_clean_ref.scene (no prop, no logo) over a cluttered backdrop: three sine textures of about 50 grey levels per
  channel plus Gaussian noise.  -> (frames uint8 [n, H, W, 3], alpha float64 [n, H, W], fore float64 [n, H, W, 3])"""
  _, alpha, fore = mr.scene(H, W, seed=seed, n=n, prop=False, logo=False)
  rng = np.random.default_rng(seed + 1000)
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
  tex = [np.sin(xx * 0.23 + yy * 0.11), np.sin(xx * 0.07 - yy * 0.19 + 1.0), np.sin((xx + yy) * 0.31 + 2.0)]
  back = np.stack([120.0 + 50.0 * tex[0] + 20.0 * tex[1], 110.0 + 50.0 * tex[1] + 20.0 * tex[2], 100.0 + 50.0 * tex[2] + 20.0 * tex[0]], -1)
  frames = []
  for k in range(n):
    img = alpha[k][..., None] * fore[k] + (1.0 - alpha[k][..., None]) * (back + rng.normal(0.0, noise, (H, W, 3)))
    frames.append(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8))
  return np.stack(frames), alpha, fore


def wrongly_known(tri, alpha):
  """pixels the trimap takes as known against the true alpha: known 1 where alpha < 0.98, known 0 where alpha > 0.02"""
  return int(((tri == 255) & (alpha < 0.98)).sum() + ((tri == 0) & (alpha > 0.02)).sum())


def summary(unknown, iterations, residual):
  return "solve: %d px unknown, %d iterations, residual %.0e" % (round(float(np.mean(unknown))), round(float(np.mean(iterations))), float(np.mean(residual)))

"""numpy restatement of the matte clean-up (include/vp_hip.h, vp_matteclean_*) and of the foreground estimate (vp_key_foreground), written
from the header's text.  Labelling is min-propagation to a fixed point (every pixel takes the smallest label among itself and its
neighbours, then the label of its label), not scipy and not a union-find.  And the synthetic scene the tests and the quality figures
use: key_matte_ref's studio scene with the neck joined, a detached prop, a backdrop-coloured logo on the torso and a known spill term,
returned with its true alpha and its true foreground colours."""
import numpy as np

REPORT_INTS = 8
DEFAULTS = dict(support=32, core=224, grow=4, keep="anchored")


def default_min_area(H, W):
  return H * W // 1024


def default_max_hole(H, W):
  return H * W // 256


# ---- labelling ----------------------------------------------------------------------------------------------------------------------------
def label(in_set, eight):
  """in_set bool [H, W] -> int32 [H, W]: -1 outside the set, else the smallest y * W + x of the pixel's component (8- or 4-connected)"""
  H, W = in_set.shape
  big = H * W
  L = np.where(in_set, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
  steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if eight else [])
  while True:
    P = np.full((H + 2, W + 2), big, np.int64)
    P[1:-1, 1:-1] = L
    M = L.copy()
    for dy, dx in steps:
      np.minimum(M, P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], out=M)
    M = np.where(in_set, M, big)
    flat = np.append(M.ravel(), big)                     # the label of the label (the label big maps to itself)
    M = np.where(in_set, flat[M], big)
    if np.array_equal(M, L):
      break
    L = M
  return np.where(in_set, L, -1).astype(np.int32)


def _dilate(K, g):
  """K bool [H, W] -> true within Chebyshev distance g of a true pixel"""
  out = K.copy()
  H, W = K.shape
  for axis, size in ((1, W), (0, H)):
    src = out.copy()
    for d in range(-g, g + 1):
      lo, hi = max(0, -d), min(size, size - d)
      if lo >= hi or d == 0:
        continue
      dst, s = [slice(None)] * 2, [slice(None)] * 2
      dst[axis], s[axis] = slice(lo, hi), slice(lo + d, hi + d)
      out[tuple(dst)] |= src[tuple(s)]
  return out


def clean_frame(m, support=32, core=224, min_area=None, max_hole=None, grow=4, keep="anchored", anchors=()):
  """m uint8 [H, W], anchors: (x, y) pairs -> (cleaned uint8 [H, W], labels int32 [H, W], report int32 [8])"""
  H, W = m.shape
  min_area = default_min_area(H, W) if min_area is None else min_area
  max_hole = default_max_hole(H, W) if max_hole is None else max_hole
  assert keep in ("all", "anchored")
  m = m.astype(np.int64)
  S = m >= support
  L = label(S, True)
  roots = np.unique(L[S])
  area = np.bincount(L[S], minlength=H * W)
  bottom = set(L[H - 1][S[H - 1]].tolist())
  anchored = set(int(L[y, x]) for x, y in anchors if 0 <= x < W and 0 <= y < H and S[y, x])
  passed = [int(r) for r in roots if area[r] >= min_area and (keep == "all" or int(r) in bottom or int(r) in anchored)]
  status = 0
  kept = passed
  if keep == "anchored" and len(roots) > 0 and not passed:
    kept, status = [int(r) for r in roots], 1
  K = S & np.isin(L, kept)
  near = _dilate(K, grow)
  m1 = np.where(S, np.where(K, m, 0), np.where(near, m, 0))
  removed = int((S & ~K).sum())
  zeroed = int(((m > 0) & ~S & ~near).sum())
  holes = filled = 0
  if max_hole > 0:
    N = m1 < core
    LN = label(N, False)
    hole_area = np.bincount(LN[N], minlength=H * W)
    edge = set(LN[0][N[0]].tolist()) | set(LN[H - 1][N[H - 1]].tolist()) | set(LN[:, 0][N[:, 0]].tolist()) | set(LN[:, W - 1][N[:, W - 1]].tolist())
    fill = [int(r) for r in np.unique(LN[N]) if int(r) not in edge and hole_area[r] <= max_hole]
    F = N & np.isin(LN, fill)
    m1 = np.where(F, 255, m1)
    holes, filled = len(fill), int(F.sum())
  report = np.array([len(roots), len(kept), removed, zeroed, holes, filled, status, 0], np.int32)
  return m1.astype(np.uint8), L, report


def clean(matte, anchors=None, **kw):
  """matte uint8 [n, H, W], anchors None or int [n, k, 2] -> (cleaned [n, H, W], labels int32 [n, H, W], report int32 [n, 8])"""
  res = [clean_frame(matte[f], anchors=() if anchors is None else [tuple(int(v) for v in a) for a in anchors[f]], **kw) for f in range(matte.shape[0])]
  return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def summary(report):
  r = report.reshape(-1, REPORT_INTS).astype(np.int64).sum(0)
  removed = int(r[0] - r[1])
  return "removed %d component%s / %d px, filled %d hole%s / %d px" % (removed, "" if removed == 1 else "s", int(r[2]), int(r[4]),
                                                                      "" if r[4] == 1 else "s", int(r[5]))


# ---- the foreground estimate ------------------------------------------------------------------------------------------------------------
def planes(model, H, W):
  """b_c(x, y) -> float64 [H, W, 3]"""
  m = [np.float64(v) for v in model]
  yy, xx = np.mgrid[0:H, 0:W]
  xd, yd = xx.astype(np.float64), yy.astype(np.float64)
  return np.stack([(m[3 * c] + m[3 * c + 1] * xd) + m[3 * c + 2] * yd for c in range(3)], -1)


def spill(model, H, W):
  """(key channel, its lead over the larger of the other two) at (W // 2, H // 2)"""
  m = [np.float64(v) for v in model]
  x, y = np.float64(W // 2), np.float64(H // 2)
  v = [(m[3 * c] + m[3 * c + 1] * x) + m[3 * c + 2] * y for c in range(3)]
  k = 0 if v[0] >= v[1] and v[0] >= v[2] else (1 if v[1] >= v[2] else 2)
  return k, v[k] - max(v[c] for c in range(3) if c != k)


def foreground(model, frames, matte, despill=0.0):
  """frames uint8 [n, H, W, 3], matte uint8 [n, H, W] -> uint8 [n, H, W, 3]"""
  n, H, W, _ = frames.shape
  b = planes(model, H, W)[None]
  I = frames.astype(np.float64)
  m = matte.astype(np.float64)[..., None]
  with np.errstate(divide="ignore", invalid="ignore"):
    e = b + (I - b) * (np.float64(255.0) / m)
  e = np.fmin(np.fmax(e, 0.0), 255.0)
  e = np.where(m == 255.0, I, e)
  k, lead = spill(model, H, W)
  if lead >= 16.0 and despill > 0.0:
    i, j = [c for c in range(3) if c != k]
    e[..., k] = e[..., k] - np.float64(despill) * np.fmax(0.0, e[..., k] - (e[..., i] + e[..., j]) / 2.0)
  e = np.where(m == 0.0, 0.0, e)
  return np.floor(e + 0.5).astype(np.uint8)


# ---- worst cases of the labelling -----------------------------------------------------------------------------------------------------------
def blobs(H, W, seed=0, smooth=2):
  """random blobs with soft rims: box-smoothed noise, stretched to 0 .. 255 -> uint8 [H, W]"""
  rng = np.random.default_rng(seed)
  a = rng.random((H + 2 * smooth, W + 2 * smooth))
  c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), 0), 1)
  k = 2 * smooth + 1
  s = (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)
  s = (s - s.mean()) / s.std()
  return np.clip(np.floor(128.0 + 300.0 * s), 0, 255).astype(np.uint8)


def patterns(H, W):
  """name -> uint8 [H, W] of 0 / 255: what a tiled union-find finds hardest (paths that cross every tile border, many components,
  one component that spans the frame)"""
  yy, xx = np.mgrid[0:H, 0:W]
  out = {"zeros": np.zeros((H, W), bool), "ones": np.ones((H, W), bool), "checkerboard": (xx + yy) % 2 == 0}
  serp = yy % 2 == 0                                       # full rows joined alternately at the right and the left end
  serp |= (yy % 4 == 1) & (xx == W - 1)
  serp |= (yy % 4 == 3) & (xx == 0)
  out["serpentine"] = serp
  spiral = np.zeros((H, W), bool)                          # a one-pixel path from a corner inwards, one pixel of gap between the turns
  y, x, dy, dx, turns = 0, 0, 0, 1, 0
  spiral[0, 0] = True
  while turns < 2:
    ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
    if 0 <= ny < H and 0 <= nx < W and not spiral[ny, nx] and not (0 <= ay < H and 0 <= ax < W and spiral[ay, ax]):
      y, x, turns = ny, nx, 0
      spiral[y, x] = True
    else:
      dy, dx, turns = dx, -dy, turns + 1
  out["spiral"] = spiral
  out["comb"] = (yy == H - 1) | (xx % 2 == 0)              # teeth over the full height joined by the bottom row
  out["diagonal"] = (xx * (H - 1) // max(W - 1, 1)) == yy if W >= H else (yy * (W - 1) // max(H - 1, 1)) == xx
  return {k: (v * 255).astype(np.uint8) for k, v in out.items()}


# ---- the synthetic scene ------------------------------------------------------------------------------------------------------------------
def scene(H, W, seed=0, n=1, noise=3.0, spill_levels=0.0, prop=True, logo=True):
  """key_matte_ref.scene's head, shoulders and backdrop (a plane gradient per channel plus Gaussian noise), with a neck that joins head and
  shoulders, a detached prop left of the head, a logo on the torso that has the backdrop's own colour (alpha 1: a key sees a hole), and
  `spill_levels` grey levels of the backdrop's key channel (green) added to what the camera sees of the subject.
  -> (frames uint8 [n, H, W, 3], alpha float64 [n, H, W]: the subject's true alpha, which is 0 on the prop, fore float64 [n, H, W, 3]: the
  true foreground colours, without the spill)"""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
  u, v = xx / W, yy / H
  back = np.stack([70.0 + 24.0 * u + 10.0 * v, 150.0 - 14.0 * u + 18.0 * v, 95.0 + 8.0 * u - 12.0 * v], -1)
  frames, alphas, fores = [], [], []
  for k in range(n):
    cx, cy, ax, ay = W * (0.5 + 0.01 * k), H * 0.40, W * 0.20, H * 0.24
    ex, ey = (xx - cx) / ax, (yy - cy) / ay
    rho = np.sqrt(ex * ex + ey * ey) + 1e-12
    grad = np.sqrt((ex / ax) ** 2 + (ey / ay) ** 2) / rho + 1e-12
    head = np.clip(0.5 - ((rho - 1.0) / grad) / 3.0, 0.0, 1.0)
    top, half0, half1 = H * 0.68, W * 0.16, W * 0.46
    slope = (half1 - half0) / (H - top)
    side = (np.abs(xx - W * 0.5) - (half0 + slope * (yy - top))) / np.sqrt(1.0 + slope * slope)
    torso = np.clip(0.5 - np.maximum(top - yy, side) / 3.0, 0.0, 1.0)
    neck = np.clip(0.5 - np.maximum(np.abs(xx - cx) - W * 0.07, np.maximum(H * 0.5 - yy, yy - H * 0.72)) / 3.0, 0.0, 1.0)
    body = np.maximum(torso, neck)
    alpha = np.maximum(head, body)
    tex = 12.0 * np.sin(xx * 0.9 + k) * np.cos(yy * 0.7)
    skin = np.stack([205.0 + tex, 160.0 + 0.8 * tex, 135.0 - 0.5 * tex], -1)
    cloth = np.stack([40.0 + 0.5 * tex, 45.0 + tex, 60.0 - tex], -1)
    fore = np.where((head >= body)[..., None], skin, cloth)
    if logo:
      inside = ((xx - W * 0.5) / (W * 0.033)) ** 2 + ((yy - H * 0.86) / (H * 0.028)) ** 2 <= 1.0
      fore = np.where(inside[..., None], back, fore)
    if prop:
      pr = 0.5 - (np.sqrt((xx - W * 0.15) ** 2 + (yy - H * 0.52) ** 2) - min(H, W) * 0.05) / 3.0
      pa = np.clip(pr, 0.0, 1.0)
      fore = np.where((pa > alpha)[..., None], np.array([200.0, 60.0, 40.0]), fore)
      covered = np.maximum(alpha, pa)                      # what hides the backdrop; `alpha` stays the subject's: the prop is not the subject
    else:
      covered = alpha
    fore = fore + rng.normal(0.0, 2.0, (H, W, 3))
    seen = fore + np.array([0.0, spill_levels, 0.0])
    img = covered[..., None] * seen + (1.0 - covered[..., None]) * (back + rng.normal(0.0, noise, (H, W, 3)))
    frames.append(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8))
    alphas.append(alpha)
    fores.append(np.clip(fore, 0.0, 255.0))
  return np.stack(frames), np.stack(alphas), np.stack(fores)


def landmarks(H, W, n=1):
  """68 (x, y) anchors per frame on the scene's face: a ring inside the head ellipse -> int32 [n, 68, 2]"""
  t = np.arange(68) * (2.0 * np.pi / 68)
  out = np.empty((n, 68, 2), np.int32)
  for k in range(n):
    out[k, :, 0] = np.floor(W * (0.5 + 0.01 * k) + W * 0.12 * np.cos(t))
    out[k, :, 1] = np.floor(H * 0.40 + H * 0.15 * np.sin(t))
  return out


def edge_colour_error(colours, fore, alpha):
  """mean absolute error in grey levels of `colours` against the true foreground over the edge pixels 0.25 < alpha < 0.98"""
  edge = (alpha > 0.25) & (alpha < 0.98)
  return float(np.abs(colours.astype(np.float64) - fore)[edge].mean())

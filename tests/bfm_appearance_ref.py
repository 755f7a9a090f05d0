"""numpy float64 restatement of what voicepuppet_amd.bfmfit.FaceFitter.observe / fit_appearance and csrc/bfm_appear.hip compute: the
observation of a photo at the vertices of `Reconstruction` (utils/reconstruct_mesh.py:172-194), the photometric objective on texture and
lighting, its analytic Jacobian, A / g, and the Levenberg-Marquardt rule of DESIGN.md section 9 with its relative stopping test.  TEST
INFRASTRUCTURE ONLY: written from the stated rule, it does not import the product.  PINNED: tests/golden/bfm_appearance.npz holds
face_texture, face_color and face_projection of the reference's own Reconstruction (tests/golden/make_bfm_appearance_golden.py);
tests/test_bfm_appearance_host.py checks `texture`, `lighting`, `geometry` against them.

Unknowns p [107] = [delta(80) | gamma(27)] = coefficients 144:224, 227:254."""
import numpy as np

NA = 107
FOCAL, CENTER = 1015.0, 112.0
SH_A = (np.pi, 2 * np.pi / np.sqrt(3.0), 2 * np.pi / np.sqrt(8.0))
SH_C = (1 / np.sqrt(4 * np.pi), np.sqrt(3.0) / np.sqrt(4 * np.pi), 3 * np.sqrt(5.0) / np.sqrt(12 * np.pi))
INIT_LIT = np.array([0.8, 0, 0, 0, 0, 0, 0, 0, 0])


def coeff_to_p(coeff):
  c = np.asarray(coeff, np.float64)
  return np.concatenate([c[..., 144:224], c[..., 227:254]], axis=-1)


def p_to_coeff(p, template):
  c = np.array(template, np.float64)
  c[..., 144:224], c[..., 227:254] = p[..., :80], p[..., 80:]
  return c


def rotation(angles):
  """Compute_rotation_matrix (:68-93): (Rz Ry Rx)^T, float64; sines and cosines in the dtype of `angles`, as the reference takes them."""
  a = np.asarray(angles).reshape(3)
  c, s = np.cos(a), np.sin(a)
  rx = np.array([[1.0, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]], np.float64)
  ry = np.array([[c[1], 0, s[1]], [0, 1.0, 0], [-s[1], 0, c[1]]], np.float64)
  rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1.0]], np.float64)
  return np.ascontiguousarray(((rz @ ry) @ rx).T)


def geometry(fm, coeff, R=None):
  """One row of coefficients -> (rotated unit normals [N,3], face_projection [N,2]) as Reconstruction computes them (:175-186)."""
  c = np.asarray(coeff, np.float64).reshape(257)
  if R is None:
    R = rotation(c[224:227])
  shape = (np.asarray(fm.idBase, np.float64) @ c[:80] + np.asarray(fm.exBase, np.float64) @ c[80:144] + np.asarray(fm.meanshape, np.float64).reshape(-1))
  shape = shape.reshape(-1, 3) - np.asarray(fm.meanshape, np.float64).reshape(-1, 3).mean(axis=0, keepdims=True)
  tri = (np.asarray(fm.tri) - 1).astype(np.int64)
  pb = (np.asarray(fm.point_buf) - 1).astype(np.int64)
  fn = np.cross(shape[tri[:, 0]] - shape[tri[:, 1]], shape[tri[:, 1]] - shape[tri[:, 2]])
  fn = np.concatenate([fn, np.zeros((1, 3))], axis=0)
  vn = fn[pb].sum(axis=1)
  vn = vn / np.linalg.norm(vn, axis=1)[:, None]
  cam = (shape @ R + c[254:257]) * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 10.0])
  proj = np.stack([(FOCAL * cam[:, 0] + CENTER * cam[:, 2]) / cam[:, 2], 224.0 - (FOCAL * cam[:, 1] + CENTER * cam[:, 2]) / cam[:, 2]], axis=1)
  return vn @ R, proj


def sh_terms(n):
  """The nine SH terms of Illumination_layer (:137-155) for unit normals n [N,3]."""
  a0, a1, a2 = SH_A
  c0, c1, c2 = SH_C
  nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
  return np.stack([np.full_like(nx, a0 * c0), -a1 * c1 * ny, a1 * c1 * nz, -a1 * c1 * nx, a2 * c2 * nx * ny, -a2 * c2 * ny * nz,
                   a2 * c2 * 0.5 / np.sqrt(3.0) * (3 * np.square(nz) - 1), -a2 * c2 * nx * nz, a2 * c2 * 0.5 * (np.square(nx) - np.square(ny))], axis=1)


def bilinear(img, px, py):
  """img [H,W,3] uint8 sampled at (px, py), integer coordinates = pixel centres: (values [n,3] float64, inside [n] bool).  inside iff
  0 <= px <= W-1 and 0 <= py <= H-1; the values outside are 0."""
  H, W = img.shape[:2]
  px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
  inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
  qx, qy = np.where(inside, px, 0.0), np.where(inside, py, 0.0)
  x0 = np.minimum(np.floor(qx).astype(np.int64), W - 2)
  y0 = np.minimum(np.floor(qy).astype(np.int64), H - 2)
  fx, fy = (qx - x0)[:, None], (qy - y0)[:, None]
  I = img.astype(np.float64)
  top = (1.0 - fx) * I[y0, x0] + fx * I[y0, x0 + 1]
  bot = (1.0 - fx) * I[y0 + 1, x0] + fx * I[y0 + 1, x0 + 1]
  return np.where(inside[:, None], (1.0 - fy) * top + fy * bot, 0.0), inside


def observe(fm, coeff, photo, affine, vertex_weights=None, R=None):
  """(sh [N,9], weight [N], observed [N,3]) of one frame: weight = vertex_weights max(0, (n . R)_z) inside."""
  nr, proj = geometry(fm, coeff, R)
  a, bx, by = np.asarray(affine, np.float64)
  obs, inside = bilinear(photo, a * proj[:, 0] + bx, a * proj[:, 1] + by)
  vw = np.ones(len(nr)) if vertex_weights is None else np.asarray(vertex_weights, np.float64)
  return sh_terms(nr), np.where(inside, vw * np.maximum(0.0, nr[:, 2]), 0.0), obs


def texture(fm, delta):
  """Texture_formation (:58-62): [N,3]."""
  return (np.asarray(fm.texBase, np.float64) @ delta + np.asarray(fm.meantex, np.float64).reshape(-1)).reshape(-1, 3)


def lighting(Y, gamma):
  """[N,3]: sum_k Y_vk (gamma_ck + init_k)   (:133-135, :159-161)."""
  return Y @ (np.asarray(gamma, np.float64).reshape(3, 9) + INIT_LIT).T


def face_color(fm, Y, p):
  return texture(fm, p[:80]) * lighting(Y, p[80:])


def lam_vector(lam_tex, lam_gamma):
  return np.concatenate([np.full(80, float(lam_tex)), np.full(27, float(lam_gamma))])


def residual(fm, obs, p, want_jac=False):
  """r [3N] (row 3v+c) = T L - I, and with want_jac J [3N,107]: d r / d delta_j = L B[3v+c, j], d r / d gamma_ck = Y_vk T_vc."""
  Y, _, I = obs
  T, L = texture(fm, p[:80]), lighting(Y, p[80:])
  r = (T * L - I).reshape(-1)
  if not want_jac:
    return r
  N = Y.shape[0]
  J = np.zeros((N, 3, NA))
  J[:, :, :80] = L[:, :, None] * np.asarray(fm.texBase, np.float64).reshape(N, 3, 80)
  for c in range(3):
    J[:, c, 80 + 9 * c:89 + 9 * c] = Y * T[:, c:c + 1]
  return r, J.reshape(3 * N, NA)


def rows_weight(obs):
  w = np.where(obs[1] > 0, obs[1], 0.0)
  return np.repeat(w, 3), 3.0 * w.sum()


def cost(fm, obs, p, lam_tex=1.0, lam_gamma=1.0):
  w3, W = rows_weight(obs)
  r = residual(fm, obs, p)
  return float(np.sum(w3 * r * r) / W + np.sum(lam_vector(lam_tex, lam_gamma) * p * p))


def data_term(fm, obs, p):
  w3, W = rows_weight(obs)
  r = residual(fm, obs, p)
  return float(np.sum(w3 * r * r) / W)


def normal_equations(fm, obs, p, lam_tex=1.0, lam_gamma=1.0):
  """(A, g, E): A = J^T W J / W + Lambda, g = J^T W r / W + Lambda p."""
  w3, W = rows_weight(obs)
  r, J = residual(fm, obs, p, want_jac=True)
  lam = lam_vector(lam_tex, lam_gamma)
  A = J.T @ (w3[:, None] * J) / W + np.diag(lam)
  g = J.T @ (w3 * r) / W + lam * p
  return A, g, float(np.sum(w3 * r * r) / W + np.sum(lam * p * p))


def fit(fm, obs, init=None, lam_tex=1.0, lam_gamma=1.0, gtol=1e-6, max_trials=32):
  """One frame.  Returns (p [107], report [4] = status, accepted steps, E, |g|_inf, info = {trials, rejects}).  A trial is one evaluation of
  (A, g, E); the first is the start point.  Status 0 |g|_inf <= gtol E (or E = 0), 1 max_trials evaluations used up, 2 mu > 1e8,
  3 non-finite input or sum w = 0.  gtol = 0 runs until the acceptance test stalls (status 2) or max_trials."""
  p = np.zeros(NA) if init is None else np.array(init, np.float64)
  info = {"trials": 0, "rejects": 0}
  w3, W = rows_weight(obs)
  if not (all(np.all(np.isfinite(o)) for o in obs) and np.all(np.isfinite(p)) and W > 0):
    return p, np.array([3.0, 0.0, np.nan, np.nan]), info
  kw = dict(lam_tex=lam_tex, lam_gamma=lam_gamma)
  A, g, E = normal_equations(fm, obs, p, **kw)
  info["trials"] = 1
  if not np.isfinite(E):
    return p, np.array([3.0, 0.0, np.nan, np.nan]), info
  mu, iters = 1e-3, 0
  gmax = float(np.max(np.abs(g)))
  status = 0 if (gmax <= gtol * E or E == 0) else (1 if info["trials"] >= max_trials else -1)
  while status < 0:
    d = None
    while d is None:
      try:
        L = np.linalg.cholesky(A + mu * np.diag(np.diag(A)))
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.all(np.isfinite(p + d)):
          d = None
      except np.linalg.LinAlgError:
        d = None
      if d is None:
        mu *= 4.0
        if mu > 1e8:
          status = 2
          break
    if status >= 0:
      break
    with np.errstate(all="ignore"):
      At, gt, Et = normal_equations(fm, obs, p + d, **kw)
    info["trials"] += 1
    if Et < E:                                               # False for a non-finite cost
      p, A, g, E, mu, iters = p + d, At, gt, Et, max(mu / 3.0, 1e-9), iters + 1
      gmax = float(np.max(np.abs(g)))
      if gmax <= gtol * E or E == 0:
        status = 0
    else:
      info["rejects"] += 1
      mu *= 4.0
      if mu > 1e8:
        status = 2
    if status < 0 and info["trials"] >= max_trials:
      status = 1
  return p, np.array([float(status), iters, E, gmax]), info


def smooth_photo(h=96, w=128, seed=0):
  """A smooth synthetic uint8 RGB image: a few low-frequency waves per channel around mid grey."""
  rng = np.random.default_rng(seed)
  y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
  img = np.zeros((h, w, 3))
  for c in range(3):
    img[:, :, c] = 128 + sum(rng.uniform(10, 30) * np.sin(2 * np.pi * (rng.uniform(0.3, 1.5) * x + rng.uniform(0.3, 1.5) * y) + rng.uniform(0, 6.28))
                             for _ in range(3))
  return np.clip(np.round(img), 0, 255).astype(np.uint8)


def test_affines(frames):
  """[frames,3] (a, bx, by) for the 96 x 128 photo: a != 1, the face taller than the photo, so some vertices fall outside; every frame its own."""
  f = np.arange(frames, dtype=np.float64) % 6
  return np.stack([0.55 + 0.01 * f, 2.4 + 0.7 * f, -13.6 - 0.5 * f], axis=1)


test_affines.__test__ = False

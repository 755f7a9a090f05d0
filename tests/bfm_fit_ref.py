"""numpy float64 restatement of what voicepuppet_amd.bfmfit and csrc/bfm_fit.hip compute: the 68-landmark forward model of `Reconstruction`
(utils/reconstruct_mesh.py:172-194), its analytic Jacobian, the Levenberg-Marquardt rule of DESIGN.md section 9, the shared-identity
Gauss-Newton step and the fixed schedule of `fit_sequence`.  TEST INFRASTRUCTURE ONLY: written from the stated rule, it does not import the
product.  PINNED: tests/golden/bfm_fit.npz holds landmarks_2d of the reference's own reconstruct_mesh.Reconstruction
(tests/golden/make_bfmfit_golden.py); tests/test_bfm_fit_host.py checks `project` against them.

Parameters p [150] = [alpha(80) | beta(64) | angles(3) | t(3)] = coefficients 0:80, 80:144, 224:227, 254:257."""
import numpy as np

NP = 150
FREE_ID, FREE_EX, FREE_ANGLES, FREE_T = 1, 2, 4, 8
FREE = {"all": 15, "tracking": FREE_EX | FREE_ANGLES | FREE_T, "pose": FREE_ANGLES | FREE_T}
FOCAL, CENTER = 1015.0, 112.0


def coeff_to_p(coeff):
  c = np.asarray(coeff, np.float64)
  return np.concatenate([c[..., :144], c[..., 224:227], c[..., 254:257]], axis=-1)


def p_to_coeff(p, template=None):
  p = np.asarray(p, np.float64)
  c = np.zeros(p.shape[:-1] + (257,), np.float64) if template is None else np.array(template, np.float64)
  c[..., :144], c[..., 224:227], c[..., 254:257] = p[..., :144], p[..., 144:147], p[..., 147:150]
  return c


def free_index(free):
  bits = FREE[free] if isinstance(free, str) else int(free)
  idx = []
  for bit, lo, hi in ((FREE_ID, 0, 80), (FREE_EX, 80, 144), (FREE_ANGLES, 144, 147), (FREE_T, 147, 150)):
    if bits & bit:
      idx += list(range(lo, hi))
  return np.array(idx, np.int64)


def table(fm):
  """[204,145]: the keypoint rows of idBase | exBase | meanshape - centre (row 3k+c: landmark k, coordinate c)."""
  kp = np.asarray(fm.keypoints).astype(np.int64)
  rows = (3 * kp[:, None] + np.arange(3)[None, :]).reshape(-1)
  mean = np.asarray(fm.meanshape, np.float64).reshape(-1, 3)
  mean = (mean - mean.mean(axis=0, keepdims=True)).reshape(-1)
  return np.concatenate([np.asarray(fm.idBase, np.float64)[rows], np.asarray(fm.exBase, np.float64)[rows], mean[rows, None]], axis=1)


def rotation(angles):
  """M = Rz Ry Rx and its three derivatives; Compute_rotation_matrix (:68-93) returns M^T, and shape @ M^T = (M shape^T)^T."""
  ax, ay, az = angles
  cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
  rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
  ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  dx = np.array([[0.0, 0, 0], [0, -sx, -cx], [0, cx, -sx]])
  dy = np.array([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]])
  dz = np.array([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]])
  return rz @ ry @ rx, (rz @ ry @ dx, rz @ dy @ rx, dz @ ry @ rx)


def project(tbl, p, want_jac=False):
  """landmarks_2d [68,2] of Reconstruction at p, and with want_jac the Jacobian [136,150] (row 2k: x of landmark k, 2k+1: y)."""
  p = np.asarray(p, np.float64)
  S = (tbl[:, :144] @ p[:144] + tbl[:, 144]).reshape(68, 3)
  M, dM = rotation(p[144:147])
  cam = S @ M.T + p[147:150]
  qz = 10.0 - cam[:, 2]
  proj = np.stack([FOCAL * cam[:, 0] / qz + CENTER, 224.0 - (FOCAL * cam[:, 1] / qz + CENTER)], axis=1)
  if not want_jac:
    return proj
  G = np.zeros((68, 2, 3))                                   # d proj / d cam
  G[:, 0, 0] = FOCAL / qz
  G[:, 0, 2] = FOCAL * cam[:, 0] / (qz * qz)
  G[:, 1, 1] = -FOCAL / qz
  G[:, 1, 2] = -FOCAL * cam[:, 1] / (qz * qz)
  H = G @ M                                                  # d proj / d shape   [68,2,3]
  J = np.zeros((68, 2, NP))
  J[:, :, :144] = np.einsum("kic,kcj->kij", H, tbl[:, :144].reshape(68, 3, 144))
  for a in range(3):
    J[:, :, 144 + a] = np.einsum("kic,kc->ki", G, S @ dM[a].T)
  J[:, :, 147:150] = G
  return proj, J.reshape(136, NP)


def weights_rows(weights):
  w = np.ones(68) if weights is None else np.asarray(weights, np.float64).reshape(68)
  return np.repeat(w, 2)


def lam_vector(lam_id, lam_ex):
  return np.concatenate([np.full(80, float(lam_id)), np.full(64, float(lam_ex)), np.zeros(6)])


def cost(tbl, p, lm, weights=None, lam_id=1.0, lam_ex=1.0):
  r = (project(tbl, p) - lm).reshape(-1)
  return float(np.sum(weights_rows(weights) * r * r) + np.sum(lam_vector(lam_id, lam_ex) * p * p))


def normal_equations(tbl, p, lm, weights=None, lam_id=1.0, lam_ex=1.0):
  """(A, g, E) over all 150 parameters: A = J^T W J + Lambda, g = J^T W r + Lambda p."""
  proj, J = project(tbl, p, want_jac=True)
  r = (proj - lm).reshape(-1)
  w, lam = weights_rows(weights), lam_vector(lam_id, lam_ex)
  A = J.T @ (w[:, None] * J) + np.diag(lam)
  g = J.T @ (w * r) + lam * p
  return A, g, float(np.sum(w * r * r) + np.sum(lam * p * p))


def fit(tbl, lm, weights=None, init=None, free="all", lam_id=1.0, lam_ex=1.0, gtol=1e-6, max_iters=100):
  """One frame.  Returns (p [150], report [4] = status, accepted iterations, E, |g|_inf).  Status 0 converged, 1 max_iters, 2 stalled
  (mu > 1e8), 3 non-finite input.  "E(p+d) < E(p)" is evaluated without the regularisation of the blocks that are not free: it is the
  same number on both sides (d leaves those blocks alone), and left in it would only set the rounding of both (a fixed |alpha|^2 of 50
  hides a change of 1e-15 in the rest).  The reported E is the whole cost."""
  p = np.zeros(NP) if init is None else np.array(init, np.float64)
  lm = np.asarray(lm, np.float64)
  if not (np.all(np.isfinite(lm)) and np.all(np.isfinite(p))):
    return p, np.array([3.0, 0.0, np.nan, np.nan])
  idx = free_index(free)
  bits = FREE[free] if isinstance(free, str) else int(free)
  cmp_id, cmp_ex = (lam_id if bits & FREE_ID else 0.0), (lam_ex if bits & FREE_EX else 0.0)
  whole = lambda q: cost(tbl, q, lm, weights, lam_id, lam_ex)
  mu, iters = 1e-3, 0
  E = cost(tbl, p, lm, weights, cmp_id, cmp_ex)
  while True:
    A, g, _ = normal_equations(tbl, p, lm, weights, lam_id, lam_ex)
    A, g = A[np.ix_(idx, idx)], g[idx]
    gmax = float(np.max(np.abs(g)))
    if gmax <= gtol:
      return p, np.array([0.0, iters, whole(p), gmax])
    if iters >= max_iters:
      return p, np.array([1.0, iters, whole(p), gmax])
    while True:
      accepted = False
      try:
        L = np.linalg.cholesky(A + mu * np.diag(np.diag(A)))
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        trial = p.copy()
        trial[idx] += d
        with np.errstate(all="ignore"):
          Et = cost(tbl, trial, lm, weights, cmp_id, cmp_ex)
        accepted = bool(Et < E)                              # False for a non-finite cost on either side
      except np.linalg.LinAlgError:
        pass
      if accepted:
        p, E, mu, iters = trial, Et, max(mu / 3.0, 1e-9), iters + 1
        break
      mu *= 4.0
      if mu > 1e8:
        return p, np.array([2.0, iters, whole(p), gmax])


def fit_frames(tbl, lms, weights=None, init=None, **kw):
  ps, reps = [], []
  for f in range(len(lms)):
    w = None if weights is None else (weights[f] if np.ndim(weights) == 2 else weights)
    p, rep = fit(tbl, lms[f], w, None if init is None else init[f], **kw)
    ps.append(p)
    reps.append(rep)
  return np.stack(ps), np.stack(reps)


def identity_system(tbl, ps, lms, weights=None, lam_id=1.0):
  """A = sum_t J_a^T W J_a + T lam I, g = sum_t J_a^T W r + T lam alpha, summed in frame order; alpha is row 0's."""
  T = len(ps)
  A, g = np.zeros((80, 80)), np.zeros(80)
  for f in range(T):
    w = weights_rows(None if weights is None else (weights[f] if np.ndim(weights) == 2 else weights))
    proj, J = project(tbl, ps[f], want_jac=True)
    Ja = J[:, :80]
    A += Ja.T @ (w[:, None] * Ja)
    g += Ja.T @ (w * (proj - lms[f]).reshape(-1))
  return A + T * lam_id * np.eye(80), g + T * lam_id * ps[0][:80]


def identity_step(tbl, ps, lms, weights=None, lam_id=1.0):
  """One Gauss-Newton step on the shared alpha: solves A d = -g and writes alpha + d into every row."""
  A, g = identity_system(tbl, ps, lms, weights, lam_id)
  L = np.linalg.cholesky(A)
  d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
  out = np.array(ps, np.float64)
  out[:, :80] = ps[0][:80] + d
  return out


def total_cost(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0):
  return float(sum(cost(tbl, ps[f], lms[f], None if weights is None else (weights[f] if np.ndim(weights) == 2 else weights), lam_id, lam_ex)
                   for f in range(len(ps))))


def fit_sequence(tbl, lms, rounds=3, id_steps=3, weights=None, lam_id=1.0, lam_ex=1.0, gtol=1e-6, max_iters=100):
  """The fixed schedule: per-frame full fit from zeros, alpha <- mean of the per-frame identities, then `rounds` times
  (`id_steps` identity steps, one tracking fit of every frame from its previous values)."""
  kw = dict(lam_id=lam_id, lam_ex=lam_ex, gtol=gtol, max_iters=max_iters)
  ps, reps = fit_frames(tbl, lms, weights, None, free="all", **kw)
  ps[:, :80] = ps[:, :80].mean(axis=0, keepdims=True)
  for _ in range(rounds):
    for _ in range(id_steps):
      ps = identity_step(tbl, ps, lms, weights, lam_id)
    ps, reps = fit_frames(tbl, lms, weights, ps, free="tracking", **kw)
  return ps, reps


def five_points(lm):
  """The five points of load_lm3d (utils/bfm_load_data.py:122-127) from 68 rows: eyes (means of two corners), nose, mouth corners."""
  lm = np.asarray(lm, np.float64)
  idx = np.array([31, 37, 40, 43, 46, 49, 55]) - 1
  five = np.stack([lm[idx[0]], lm[idx[[1, 2]]].mean(0), lm[idx[[3, 4]]].mean(0), lm[idx[5]], lm[idx[6]]], axis=0)
  return five[[1, 2, 0, 3, 4]]


def photo_landmarks(lm224, scale=1.7, shift=(130.0, 60.0)):
  """Landmarks of a face somewhere in a 480 x 640 photo: a model projection (pixels of the 224 image) under a similarity."""
  return scale * np.asarray(lm224, np.float64) + np.asarray(shift, np.float64)


def paste_map(proj224, side, y0, x0, face_size=224):
  """Where render_face's resize + paste (infer_bfmvid.py:111-121) puts a point of the face_size image: canvas (x, y)."""
  p = np.asarray(proj224, np.float64)
  return np.stack([x0 + p[:, 0] * side / face_size, y0 + p[:, 1] * side / face_size], axis=1)

"""numpy float64 restatement of the joint clip fit (voicepuppet_amd.bfmfit.FaceFitter.fit_clip; csrc/bfm_clip.hip: vp_bfmfit_clip), built on
tests/bfm_fit_ref.py and written from the stated rule (include/vp_hip.h).  TEST INFRASTRUCTURE ONLY: it does not
import the product.

One clip: frames t = 1 .. T, unknowns x = [alpha (80) | q_1 | ... | q_T], q_t = [beta_t (64) | angles (3) | t (3)]; a frame's parameters are
bfm_fit_ref's p[150] = [alpha | q_t].

  E = sum_t bfm_fit_ref.cost(p_t)  +  sum_{t<T} sum_i s_i (q_t+1,i - q_t,i)^2        s = (s_ex x 64, s_ang x 3, s_t x 3)

Two solvers for (A + mu diag A) d = -g: `dense` (np.linalg on the (80 + 70 T)^2 matrix) and `arrowhead`, a separate statement of the block
elimination the device performs.  tests/test_bfm_clip_host.py checks one against the other."""
import numpy as np

import bfm_fit_ref as fr

NA, NQ = 80, 70


def smooth_vector(lam_smooth):
  s_ex, s_ang, s_t = (float(v) for v in lam_smooth)
  return np.concatenate([np.full(64, s_ex), np.full(3, s_ang), np.full(3, s_t)])


def frame_weights(weights, f):
  return None if weights is None else (weights[f] if np.ndim(weights) == 2 else weights)


def coupling_terms(ps, s):
  """[T-1]: s . (q_t+1 - q_t)^2 per pair of neighbours."""
  q = np.asarray(ps, np.float64)[:, NA:]
  return ((q[1:] - q[:-1]) ** 2 * s).sum(axis=1)


def frame_costs(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0):
  return np.array([fr.cost(tbl, ps[f], lms[f], frame_weights(weights, f), lam_id, lam_ex) for f in range(len(ps))])


def clip_cost(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0)):
  return float(frame_costs(tbl, ps, lms, weights, lam_id, lam_ex).sum() + coupling_terms(ps, smooth_vector(lam_smooth)).sum())


def frame_systems(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0):
  """Per frame (A_t [150,150], g_t [150], E_t) of bfm_fit_ref.normal_equations."""
  out = [fr.normal_equations(tbl, ps[f], lms[f], frame_weights(weights, f), lam_id, lam_ex) for f in range(len(ps))]
  return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def coupling_gradient(ps, s):
  """[T,70]: half the gradient of the coupling terms with respect to q_t (the convention of g = J^T W r)."""
  q = np.asarray(ps, np.float64)[:, NA:]
  g = np.zeros_like(q)
  g[1:] += s * (q[1:] - q[:-1])
  g[:-1] += s * (q[:-1] - q[1:])
  return g


def assemble(As, gs, cg, s):
  """Dense (A [(80+70T)^2], g) in the order [alpha | q_1 | ... | q_T] from the frames' systems and the coupling."""
  T = len(As)
  n = NA + NQ * T
  A, g = np.zeros((n, n)), np.zeros(n)
  for f in range(T):
    lo = NA + NQ * f
    A[:NA, :NA] += As[f][:NA, :NA]
    g[:NA] += gs[f][:NA]
    A[lo:lo + NQ, :NA] = As[f][NA:, :NA]
    A[:NA, lo:lo + NQ] = As[f][:NA, NA:]
    A[lo:lo + NQ, lo:lo + NQ] = As[f][NA:, NA:] + np.diag(s) * ((f > 0) + (f < T - 1))
    g[lo:lo + NQ] = gs[f][NA:] + cg[f]
    if f < T - 1:
      A[lo:lo + NQ, lo + NQ:lo + 2 * NQ] = -np.diag(s)
      A[lo + NQ:lo + 2 * NQ, lo:lo + NQ] = -np.diag(s)
  return A, g


def clip_system(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0)):
  s = smooth_vector(lam_smooth)
  As, gs, _ = frame_systems(tbl, ps, lms, weights, lam_id, lam_ex)
  return assemble(As, gs, coupling_gradient(ps, s), s)


def dense_solve(As, gs, cg, s, mu):
  """d of (A + mu diag A) d = -g: (d_alpha [80], d_q [T,70])."""
  A, g = assemble(As, gs, cg, s)
  L = np.linalg.cholesky(A + mu * np.diag(np.diag(A)))
  d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
  return d[:NA], d[NA:].reshape(len(As), NQ)


def arrowhead_solve(As, gs, cg, s, mu):
  """The same d by block elimination, forward over t:  S_t = L_t L_t^T;  [Y_t | z_t | W_t] = L_t^-1 [B~_t | r~_t | -diag(s)];
  S_t+1 = D_t+1 - W_t^T W_t;  [B~_t+1 | r~_t+1] = [B_t+1 | r_t+1] - W_t^T [Y_t | z_t];  corner -= [Y_t | z_t]^T [Y_t | z_t];  then the
  80x80 solve and, backward over t,  L_t^T x_t = z_t - Y_t x_alpha - W_t x_t+1."""
  T = len(As)
  C = sum(As[f][:NA, :NA] for f in range(T))
  C = C + mu * np.diag(np.diag(C))
  ra = -sum(gs[f][:NA] for f in range(T))
  Ls, Ys, zs, Ws = [], [], [], []
  carry_S, carry_B, carry_r = np.zeros((NQ, NQ)), np.zeros((NQ, NA)), np.zeros(NQ)
  for f in range(T):
    D = As[f][NA:, NA:] + np.diag(s) * ((f > 0) + (f < T - 1))
    D = D + mu * np.diag(np.diag(D))
    S = D - carry_S
    B = As[f][NA:, :NA] - carry_B
    r = -(gs[f][NA:] + cg[f]) - carry_r
    L = np.linalg.cholesky(S)
    Y, z = np.linalg.solve(L, B), np.linalg.solve(L, r)
    W = np.linalg.solve(L, -np.diag(s)) if f < T - 1 else np.zeros((NQ, NQ))
    C = C - Y.T @ Y
    ra = ra - Y.T @ z
    carry_S, carry_B, carry_r = W.T @ W, W.T @ Y, W.T @ z
    Ls.append(L); Ys.append(Y); zs.append(z); Ws.append(W)
  Lc = np.linalg.cholesky(C)
  xa = np.linalg.solve(Lc.T, np.linalg.solve(Lc, ra))
  xq = np.zeros((T, NQ))
  nxt = np.zeros(NQ)
  for f in range(T - 1, -1, -1):
    xq[f] = np.linalg.solve(Ls[f].T, zs[f] - Ys[f] @ xa - Ws[f] @ nxt)
    nxt = xq[f]
  return xa, xq


def clip_step(tbl, ps, lms, mu, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0), solver=arrowhead_solve):
  """One trial point: ps + d at damping mu."""
  s = smooth_vector(lam_smooth)
  As, gs, _ = frame_systems(tbl, ps, lms, weights, lam_id, lam_ex)
  xa, xq = solver(As, gs, coupling_gradient(ps, s), s, mu)
  trial = np.array(ps, np.float64)
  trial[:, :NA] += xa
  trial[:, NA:] += xq
  return trial


def clip_gradient(tbl, ps, lms, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0)):
  """g over [alpha | q_1 | ... | q_T], from the frames' gradients alone."""
  s = smooth_vector(lam_smooth)
  _, gs, _ = frame_systems(tbl, ps, lms, weights, lam_id, lam_ex)
  return np.concatenate([gs[:, :NA].sum(axis=0), (gs[:, NA:] + coupling_gradient(ps, s)).reshape(-1)])


def fit_clip(tbl, lms, ps0, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0), gtol=1e-6, max_trials=64, solver=arrowhead_solve):
  """Levenberg-Marquardt on the whole clip.  Returns (ps [T,150], report [4] = status, accepted steps, E, |g|_inf, trials used).  alpha is
  row 0's.  "E falls" is sum_t (E_t(trial) - E_t(current)) + sum (coupling(trial) - coupling(current)) < 0: differences, term by term."""
  ps = np.array(ps0, np.float64)
  ps[:, :NA] = ps[0, :NA]
  lms = np.asarray(lms, np.float64)
  if not (np.all(np.isfinite(lms)) and np.all(np.isfinite(ps))):
    return ps, np.array([3.0, 0.0, np.nan, np.nan]), 0
  s = smooth_vector(lam_smooth)
  kw = dict(weights=weights, lam_id=lam_id, lam_ex=lam_ex)
  mu, iters, trials = 1e-3, 0, 0
  Ef, Ec = frame_costs(tbl, ps, lms, **kw), coupling_terms(ps, s)
  total = lambda: float(Ef.sum() + Ec.sum())
  while True:
    As, gs, _ = frame_systems(tbl, ps, lms, **kw)
    cg = coupling_gradient(ps, s)
    gmax = float(max(np.abs(gs[:, :NA].sum(axis=0)).max(), np.abs(gs[:, NA:] + cg).max()))
    if gmax <= gtol:
      return ps, np.array([0.0, iters, total(), gmax]), trials
    while True:
      if trials >= max_trials:
        return ps, np.array([1.0, iters, total(), gmax]), trials
      try:
        xa, xq = solver(As, gs, cg, s, mu)
      except np.linalg.LinAlgError:                          # no factorisation: as a rejected trial, without an evaluation
        mu *= 4.0
        if mu > 1e8:
          return ps, np.array([2.0, iters, total(), gmax]), trials
        continue
      trial = ps.copy()
      trial[:, :NA] += xa
      trial[:, NA:] += xq
      trials += 1
      with np.errstate(all="ignore"):
        Eft, Ect = frame_costs(tbl, trial, lms, **kw), coupling_terms(trial, s)
        dE = float((Eft - Ef).sum() + (Ect - Ec).sum())
      if dE < 0.0:                                           # False for a non-finite cost on either side
        ps, Ef, Ec, mu, iters = trial, Eft, Ect, max(mu / 3.0, 1e-9), iters + 1
        break
      mu *= 4.0
      if mu > 1e8:
        return ps, np.array([2.0, iters, total(), gmax]), trials


def landmark_errors(tbl, ps, clean):
  """(mean distance to the clean landmarks, mean distance between the first differences in time of both), px."""
  proj = np.stack([fr.project(tbl, p) for p in ps])
  return point_errors(proj, clean)


def point_errors(proj, clean):
  err = np.sqrt(((proj - clean) ** 2).sum(axis=-1)).mean()
  if len(proj) < 2:
    return float(err), 0.0
  fd = np.sqrt((((proj[1:] - proj[:-1]) - (clean[1:] - clean[:-1])) ** 2).sum(axis=-1)).mean()
  return float(err), float(fd)


def synthetic_clip(T, sigma, seed=0, model_seed=3, coeff_seed=5, beta_step=0.05, angle_step=0.005):
  """A clip of one synthetic person: oracle.bfm_ref.synthetic_facemodel(model_seed), synthetic_coeffs(T, coeff_seed)'s first row as the base,
  expression and angles on a random walk (per-frame steps N(0, beta_step) and N(0, angle_step rad): about 1 px of landmark motion per
  frame, a talking head at 25 frames per second) drawn from np.random.default_rng(seed), then landmark noise N(0, sigma px) from the same
  generator.  Returns (fm, tbl, truth [T,150], clean [T,68,2], noisy [T,68,2])."""
  from oracle import bfm_ref as br
  fm = br.synthetic_facemodel(model_seed)
  tbl = fr.table(fm)
  coeff, _ = br.synthetic_coeffs(T, coeff_seed)
  truth = np.tile(fr.coeff_to_p(coeff[0]), (T, 1))
  rng = np.random.default_rng(seed)
  truth[:, 80:144] += np.cumsum(rng.normal(0, beta_step, size=(T, 64)), axis=0)
  truth[:, 144:147] += np.cumsum(rng.normal(0, angle_step, size=(T, 3)), axis=0)
  clean = np.stack([fr.project(tbl, p) for p in truth])
  noisy = clean + rng.normal(0, sigma, size=clean.shape)
  return fm, tbl, truth, clean, noisy

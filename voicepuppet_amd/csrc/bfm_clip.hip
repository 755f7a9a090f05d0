// Joint fit of a clip's BFM coefficients to its landmarks: ONE identity alpha for the clip, expression and pose per frame, with optional
// temporal coupling.  The joint counterpart of bfm_fit.hip's per-frame fit (same forward model, same reference functions: the inverse of
// `Reconstruction`, utils/reconstruct_mesh.py:172-194, for the landmarks it returns).  float64 throughout.
//
//   unknowns   alpha (80) and per frame q_t = [beta_t (64) | angles (3) | t (3)]: 80 + 70 T numbers; a frame's parameters are p_t[150]
//   cost       E = sum_t ( sum_k w_tk |pi_k(alpha, q_t) - l_tk|^2 + lam_id |alpha|^2 + lam_ex |beta_t|^2 )
//                + sum_{t<T} ( s_ex |beta_t+1 - beta_t|^2 + s_ang |ang_t+1 - ang_t|^2 + s_t |t_t+1 - t_t|^2 )
//   solver     the Levenberg-Marquardt rule of bfm_fit.hip on the whole clip: (A + mu diag A) d = -g; E falls: accept, mu <- max(mu/3, 1e-9);
//              else mu <- 4 mu; mu > 1e8 -> status 2; |g|_inf <= gtol -> status 0; max_trials trial points used up -> status 1;
//              non-finite input -> status 3.  mu0 = 1e-3.
//   A          block arrowhead: per-frame 70x70 blocks D_t on a chain whose off-diagonal blocks are -diag(s), bordered by the 70x80
//              blocks B_t (alpha coupling), corner C = sum_t (alpha, alpha) blocks.
//
// A fit is a fixed chain of launches, nothing is read back:  init, frames, (clip, frames) x max_trials, clip.
//   frames : one workgroup per frame: the full 150x150 (A_t, g_t, E_t) of ONE frame at its trial point (bfm_fit_device.h: the accumulation
//            of bfm_fit_kernel), written as a packed 151-row triangle (row 150 = [g | E]) to the buffer that is not the accepted one.
//   clip   : one workgroup per clip.  Accept / reject: sum_t (E_t(trial) - E_t(current)) + (coupling(trial) - coupling(current)) < 0, NOT a
//            difference of two clip totals (the float64 floor of the test stays at a frame's magnitude).  Then the block Cholesky sweep
//            forward over t:  S_t = L_t L_t^T,  [Y_t | z_t | W_t] = L_t^-1 [B~_t | r~_t | -diag(s)],  S_t+1 = D_t+1 - W_t^T W_t,
//            [B~_t+1 | r~_t+1] = [B_t+1 | r_t+1] - W_t^T [Y_t | z_t],  corner -= [Y_t | z_t]^T [Y_t | z_t] (held in registers),
//            the 80x80 solve (fit_device.h), the back substitution  L_t^T x_t = z_t - Y_t x_alpha + L_t^-1 (s x_t+1)  from the factors kept
//            in the workspace (70 x 151 doubles per frame), and the next trial point of every frame.
// Both leave a clip with a status alone.  Every sum has a fixed order and there are no atomics: a clip's result does not depend on the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "workspace.h"
#include "fit_device.h"
#include "bfm_fit_device.h"

namespace vp {

constexpr int CL_NA = 80;          // alpha
constexpr int CL_NQ = 70;          // unknowns per frame
constexpr int CL_SS = 71;          // LDS row stride of S
constexpr int CL_PC = 151;         // panel columns: border 80 | right-hand side | coupling 70
constexpr int CL_PS = 152;         // LDS row stride of the panel
constexpr int CL_NS = CL_NQ * (CL_NQ + 1) / 2;                   // 2485 elements of S's lower triangle
constexpr int CL_NU = CL_NS + CL_NQ * (CL_NA + 1);               // 8155 elements the coupling updates: S and [B | r]
constexpr int CL_UPD = (CL_NU + FIT_THREADS - 1) / FIT_THREADS;  // 32 per thread
constexpr int CL_CTRI = 81 * 82 / 2;                             // 3321: the corner's packed triangle, row 80 = the right-hand side
constexpr int CL_CR = (CL_CTRI + FIT_THREADS - 1) / FIT_THREADS; // 13 per thread
constexpr int CL_PB = (CL_PC + 15) / 16;                         // 10 panel columns per thread of a row of 16 threads
constexpr int CL_SB = (CL_NQ + 15) / 16;                         // 5 columns of S
constexpr int CL_EIDX = FIT_TRI - 1;                            // (150, 150) of a frame's triangle: E_t
// per-frame state in the workspace (doubles)
constexpr int FS_P = 0, FS_PT = 152, FS_BAD = 304, FS_SYS = 312, FS_FAC = FS_SYS + 2 * FIT_TRI;
constexpr int FS_LROWS = CL_NQ * CL_NQ;                          // L_t, 70 x 70 row-major; then [Y_t | z_t], 70 x 81
constexpr int FS_STRIDE = (FS_FAC + CL_NQ * CL_PC + 7) / 8 * 8;
// per-clip state
constexpr int CS_MU = 0, CS_STATUS = 1, CS_ITERS = 2, CS_TRIALS = 3, CS_GMAX = 4, CS_CUR = 5, CS_E = 6, CS_SIZE = 8;
constexpr size_t CL_LDS_BYTES = (size_t)(CL_NQ * CL_SS + CL_NQ * CL_PS + 3 * CL_NA + 3 * 72 + FIT_THREADS) * sizeof(double);

struct ClipArgs {
  const double* tbl; const double* tblT;
  const double* landmarks;      // [frames,68,2]
  const double* weights; int weights_per_frame;
  const int* offsets;           // device [clips+1]
  int clips, frames;
  double* cstate;               // [clips][CS_SIZE]
  double* fstate;               // [frames][FS_STRIDE]
  double lam_id, lam_ex, s_ex, s_ang, s_t, gtol;
  int max_trials;
  const float* coeff_in; float* coeff; double* params; double* report;
  double focal, center;
};

__device__ __forceinline__ double smooth_of(const ClipArgs& a, int i) { return i < 64 ? a.s_ex : i < 67 ? a.s_ang : a.s_t; }

// (i, j), j <= i, of the packed index e
__device__ __forceinline__ void tri_inv(int e, int& i, int& j) {
  i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

__global__ __launch_bounds__(FIT_THREADS) void bfm_clip_init_kernel(ClipArgs a) {
  const int t = threadIdx.x, b = blockIdx.x;
  if (b < a.frames) {
    double* FS = a.fstate + (size_t)b * FS_STRIDE;
    int lo = 0, hi = a.clips;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.offsets[mid] <= b) lo = mid; else hi = mid;
    }
    const int arow = a.offsets[lo];                  // alpha: the clip's first row's
    if (t < FIT_NPAD) {
      const double v = t < FIT_NP ? a.params[(size_t)(t < CL_NA ? arow : b) * FIT_NP + t] : 0.0;
      FS[FS_P + t] = v;
      FS[FS_PT + t] = v;
    }
    if (t == 0) FS[FS_BAD] = 0.0;
  } else if (t == 0) {
    double* CS = a.cstate + (size_t)(b - a.frames) * CS_SIZE;
    CS[CS_MU] = 1e-3; CS[CS_STATUS] = -1.0; CS[CS_ITERS] = 0.0; CS[CS_TRIALS] = 0.0; CS[CS_GMAX] = 0.0; CS[CS_CUR] = 0.0; CS[CS_E] = 0.0;
  }
}

// (A_t, g_t, E_t) of frame blockIdx.x at its trial point -> the buffer that does not hold the accepted system
__global__ __launch_bounds__(FIT_THREADS) void bfm_clip_frame_kernel(ClipArgs a) {
  __shared__ double jb[FIT_SLICE * FIT_NPAD];
  __shared__ double pv[FIT_NPAD];
  __shared__ double buf[FIT_FRAME_LDS];
  FrameLds L;
  frame_lds(buf, L);
  const int t = threadIdx.x, f = blockIdx.x;
  int lo = 0, hi = a.clips;                          // the clip: offsets[lo] <= f < offsets[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.offsets[mid] <= f) lo = mid; else hi = mid;
  }
  const double* CS = a.cstate + (size_t)lo * CS_SIZE;
  if (CS[CS_STATUS] >= 0.0) return;                  // a finished clip (the same value for every thread)
  const int cur = (int)CS[CS_CUR];
  double* FS = a.fstate + (size_t)f * FS_STRIDE;
  double* sys = FS + FS_SYS + (size_t)(1 - cur) * FIT_TRI;
  double bad = 0.0;
  if (t < FIT_NPAD) {
    const double v = FS[FS_PT + t];
    pv[t] = v;
    if (!isfinite(v)) bad = 1.0;
  }
  if (t < 2 * FIT_NL) {
    const double v = a.landmarks[(size_t)f * 2 * FIT_NL + t];
    L.lm[t] = v;
    if (!isfinite(v)) bad = 1.0;
  }
  if (t < FIT_NL) {
    const double w = a.weights ? a.weights[(a.weights_per_frame ? (size_t)f * FIT_NL : 0) + t] : 1.0;
    L.sw[t] = w > 0.0 ? sqrt(w) : 0.0;
  }
  if (t < 144) L.rw[t] = 0.0;
  if (block_sum(bad, L.red) != 0.0) {                // status 3 at the start; a rejected trial later
    if (t == 0) { FS[FS_BAD] = 1.0; sys[CL_EIDX] = __longlong_as_double(0x7ff8000000000000LL); }
    return;
  }
  const double lam = t < 80 ? a.lam_id : t < FIT_NQ ? a.lam_ex : 0.0;
  int bi, bj;
  tile_of(t, bi, bj);
  const bool has_tile = t < FIT_TILES;
  double acc[8][8];
  double gacc;
  eval_frame<true>(a.tblT, pv, L, a.focal, a.center);
  double term = t < 2 * FIT_NL ? L.rw[t] * L.rw[t] : 0.0;
  if (t < FIT_NQ) term += lam * pv[t] * pv[t];
  const double E = block_sum(term, L.red);
  accum_normal(a.tbl, L, 15, jb, bi, bj, has_tile, acc, gacc);
  if (has_tile) {
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        const int i = 8 * bi + x, j = 8 * bj + y;
        if (i < FIT_NP && j <= i) {
          double v = acc[x][y];
          if (i == j) v += i < 80 ? a.lam_id : i < FIT_NQ ? a.lam_ex : 0.0;
          sys[tri_idx(i, j)] = v;
        }
      }
  }
  if (t < FIT_NP) sys[tri_idx(FIT_NP, t)] = gacc + lam * pv[t];
  if (t == 0) sys[CL_EIDX] = E;
}

struct ClipLds { double *Sm, *Pn, *piv, *dv, *xa, *xn, *vv, *ww, *red; };

// In-place Cholesky of S (Sm, lower triangle; the pivots go to piv, the diagonal of Sm is left) with the forward substitution of the
// panel's first ncols columns: Pn <- L^-1 Pn.  False (for every thread) when a pivot is not > 0.
__device__ bool clip_factor(const ClipLds& D, int ncols) {
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  __syncthreads();
  for (int k = 0; k < CL_NQ; ++k) {
    const double akk = D.Sm[k * CL_SS + k];
    if (!(akk > 0.0)) return false;                  // the same value for every thread: a uniform exit
    const double pv = sqrt(akk), rpv = 1.0 / pv;     // (one division per column; the column and the panel's row are scaled by products)
    const int below = CL_NQ - 1 - k;
    for (int e = t; e < below + ncols; e += FIT_THREADS) {
      if (e < below) D.Sm[(k + 1 + e) * CL_SS + k] *= rpv;
      else D.Pn[k * CL_PS + (e - below)] *= rpv;
    }
    if (t == 0) D.piv[k] = pv;
    __syncthreads();
    // trailing update, 16 x 16 threads.  Every value a thread needs is read into registers before its first store: LDS loads cannot
    // be moved across LDS stores that might alias, and one workgroup on its CU has nothing else to hide their latency behind.
    double pk[CL_PB], sk[CL_SB];
#pragma unroll
    for (int j = 0; j < CL_PB; ++j) { const int c = tx + 16 * j; pk[j] = c < ncols ? D.Pn[k * CL_PS + c] : 0.0; }
#pragma unroll
    for (int j = 0; j < CL_SB; ++j) { const int c = k + 1 + tx + 16 * j; sk[j] = c < CL_NQ ? D.Sm[c * CL_SS + k] : 0.0; }
    for (int i = k + 1 + ty; i < CL_NQ; i += 16) {
      const double lik = D.Sm[i * CL_SS + k];
      double pi[CL_PB], si[CL_SB];
#pragma unroll
      for (int j = 0; j < CL_PB; ++j) { const int c = tx + 16 * j; pi[j] = c < ncols ? D.Pn[i * CL_PS + c] : 0.0; }
#pragma unroll
      for (int j = 0; j < CL_SB; ++j) { const int c = k + 1 + tx + 16 * j; si[j] = c <= i ? D.Sm[i * CL_SS + c] : 0.0; }
#pragma unroll
      for (int j = 0; j < CL_PB; ++j) { const int c = tx + 16 * j; if (c < ncols) D.Pn[i * CL_PS + c] = pi[j] - lik * pk[j]; }
#pragma unroll
      for (int j = 0; j < CL_SB; ++j) { const int c = k + 1 + tx + 16 * j; if (c <= i) D.Sm[i * CL_SS + c] = si[j] - lik * sk[j]; }
    }
    __syncthreads();
  }
  return true;
}

// The step d of (A + mu diag A) d = -g at the accepted point (systems `cur` of the T frames at F0): p + d goes to every frame's trial
// point.  False when a pivot is not > 0 (nothing usable has been written then).
__device__ bool clip_solve(const ClipArgs& a, const ClipLds& D, double* F0, int T, int cur, double mu, bool smooth) {
  const int t = threadIdx.x;
  const int ncols = smooth ? CL_PC : CL_NA + 1;
  const double s_i = t < CL_NQ ? smooth_of(a, t) : 0.0;
  int ci[CL_CR], cj[CL_CR];
  double cr[CL_CR];
#pragma unroll
  for (int k = 0; k < CL_CR; ++k) {
    const int e = t + FIT_THREADS * k;
    ci[k] = -1; cj[k] = 0; cr[k] = 0.0;
    if (e < CL_CTRI) tri_inv(e, ci[k], cj[k]);
  }
  for (int f = 0; f < T; ++f) {                      // the corner and its right-hand side, in frame order
    const double* sys = F0 + (size_t)f * FS_STRIDE + FS_SYS + (size_t)cur * FIT_TRI;
#pragma unroll
    for (int k = 0; k < CL_CR; ++k) {
      if (ci[k] < 0) continue;
      if (ci[k] < CL_NA) cr[k] += sys[tri_idx(ci[k], cj[k])];
      else if (cj[k] < CL_NA) cr[k] -= sys[tri_idx(FIT_NP, cj[k])];
    }
  }
#pragma unroll
  for (int k = 0; k < CL_CR; ++k)
    if (ci[k] == cj[k] && ci[k] < CL_NA) cr[k] += mu * cr[k];

  double upd[CL_UPD];
#pragma unroll
  for (int k = 0; k < CL_UPD; ++k) upd[k] = 0.0;
  for (int f = 0; f < T; ++f) {
    double* FS = F0 + (size_t)f * FS_STRIDE;
    const double* sys = FS + FS_SYS + (size_t)cur * FIT_TRI;
    const int nb = (f > 0 ? 1 : 0) + (f < T - 1 ? 1 : 0);
    __syncthreads();                                 // the previous frame's panel has been used
    // (all of a thread's global loads are issued before the first LDS store: the systems come from L2 or HBM, a microsecond away)
    double val[CL_UPD];
    int at[CL_UPD];
#pragma unroll
    for (int k = 0; k < CL_UPD; ++k) {
      const int e = t + FIT_THREADS * k;
      double v = 0.0;
      at[k] = -1;
      if (e < CL_NS) {
        int i, j;
        tri_inv(e, i, j);
        v = sys[tri_idx(CL_NA + i, CL_NA + j)];
        if (i == j) { v += (double)nb * smooth_of(a, i); v += mu * v; }
        at[k] = i * CL_SS + j;
      } else if (e < CL_NU) {
        const int r = e - CL_NS, i = r / (CL_NA + 1), c = r % (CL_NA + 1);
        if (c < CL_NA) {
          v = sys[tri_idx(CL_NA + i, c)];
        } else {                                     // -g of q_t: the frame's own and the coupling's
          const double q = FS[FS_P + CL_NA + i];
          double cg = 0.0;
          if (f > 0) cg += q - FS[FS_P + CL_NA + i - FS_STRIDE];
          if (f < T - 1) cg += q - FS[FS_P + CL_NA + i + FS_STRIDE];
          v = -(sys[tri_idx(FIT_NP, CL_NA + i)] + smooth_of(a, i) * cg);
        }
        at[k] = CL_NQ * CL_SS + i * CL_PS + c;         // Pn follows Sm in LDS
      }
      val[k] = v - upd[k];
    }
#pragma unroll
    for (int k = 0; k < CL_UPD; ++k)
      if (at[k] >= 0) D.Sm[at[k]] = val[k];
    if (smooth)
      for (int e = t; e < CL_NQ * CL_NQ; e += FIT_THREADS) {
        const int i = e / CL_NQ, j = e % CL_NQ;
        D.Pn[i * CL_PS + CL_NA + 1 + j] = (i == j && f < T - 1) ? -smooth_of(a, i) : 0.0;
      }
    if (!clip_factor(D, ncols)) return false;
    double* fac = FS + FS_FAC;
    for (int e = t; e < FS_LROWS; e += FIT_THREADS) {
      const int i = e / CL_NQ, j = e % CL_NQ;
      fac[e] = j < i ? D.Sm[i * CL_SS + j] : j == i ? D.piv[i] : 0.0;
    }
    for (int e = t; e < CL_NQ * (CL_NA + 1); e += FIT_THREADS) fac[FS_LROWS + e] = D.Pn[(e / (CL_NA + 1)) * CL_PS + e % (CL_NA + 1)];
#pragma unroll
    for (int k = 0; k < CL_CR; ++k) {
      if (ci[k] < 0) continue;
      double s = 0.0;
#pragma unroll 10
      for (int r = 0; r < CL_NQ; ++r) s = fma(D.Pn[r * CL_PS + ci[k]], D.Pn[r * CL_PS + cj[k]], s);
      cr[k] -= s;
    }
    const bool carry = smooth && f < T - 1;
#pragma unroll
    for (int k = 0; k < CL_UPD; ++k) {
      const int e = t + FIT_THREADS * k;
      double s = 0.0;
      if (carry && e < CL_NU) {
        int i, cb;                                   // W's column i against the panel column cb; W is lower triangular: rows r >= i
        if (e < CL_NS) { int j; tri_inv(e, i, j); cb = CL_NA + 1 + j; }
        else { const int r = e - CL_NS; i = r / (CL_NA + 1); cb = r % (CL_NA + 1); }
#pragma unroll 8
        for (int r = i; r < CL_NQ; ++r) s = fma(D.Pn[r * CL_PS + CL_NA + 1 + i], D.Pn[r * CL_PS + cb], s);
      }
      upd[k] = s;
    }
  }
  __syncthreads();
  double* tri = D.Pn;                                // the corner's Schur complement, packed, row 80 = its right-hand side
#pragma unroll
  for (int k = 0; k < CL_CR; ++k)
    if (ci[k] >= 0) tri[t + FIT_THREADS * k] = cr[k];
  if (!chol_solve(tri, D.piv, D.dv, CL_NA)) return false;
  if (t < CL_NA) D.xa[t] = D.dv[t];
  for (int f = T - 1; f >= 0; --f) {                 // back substitution
    double* FS = F0 + (size_t)f * FS_STRIDE;
    const double* fac = FS + FS_FAC;
    const bool coupled = smooth && f < T - 1;
    __syncthreads();
    for (int e0 = 0; e0 < CL_NQ * CL_PC; e0 += 8 * FIT_THREADS) {      // eight loads in flight per thread, then their LDS stores
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int e = e0 + t + FIT_THREADS * j; v[j] = e < CL_NQ * CL_PC ? fac[e] : 0.0; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + t + FIT_THREADS * j;
        if (e < FS_LROWS) D.Sm[(e / CL_NQ) * CL_SS + e % CL_NQ] = v[j];
        else if (e < CL_NQ * CL_PC) D.Pn[((e - FS_LROWS) / (CL_NA + 1)) * CL_PS + (e - FS_LROWS) % (CL_NA + 1)] = v[j];
      }
    }
    __syncthreads();
    if (t < CL_NQ) {
      double v = D.Pn[t * CL_PS + CL_NA];
      for (int c = 0; c < CL_NA; ++c) v = fma(-D.Pn[t * CL_PS + c], D.xa[c], v);
      D.vv[t] = v;
      D.ww[t] = coupled ? s_i * D.xn[t] : 0.0;
      D.dv[t] = 1.0 / D.Sm[t * CL_SS + t];           // the substitutions multiply by 1 / L_kk
    }
    if (coupled) {                                   // ww <- L^-1 (s x_t+1)
      for (int k = 0; k < CL_NQ; ++k) {
        __syncthreads();
        const double wk = D.ww[k] * D.dv[k];
        if (t > k && t < CL_NQ) D.ww[t] -= D.Sm[t * CL_SS + k] * wk;
      }
      __syncthreads();
      if (t < CL_NQ) D.vv[t] += D.ww[t] * D.dv[t];
    }
    for (int k = CL_NQ - 1; k >= 0; --k) {           // vv <- L^-T vv
      __syncthreads();
      const double xk = D.vv[k] * D.dv[k];
      if (t < k) D.vv[t] -= D.Sm[k * CL_SS + t] * xk;
    }
    __syncthreads();
    if (t < CL_NQ) {
      const double x = D.vv[t] * D.dv[t];
      D.xn[t] = x;
      FS[FS_PT + CL_NA + t] = FS[FS_P + CL_NA + t] + x;
    } else if (t >= 128 && t < 128 + CL_NA) {
      FS[FS_PT + t - 128] = FS[FS_P + t - 128] + D.xa[t - 128];
    }
  }
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(FIT_THREADS) void bfm_clip_step_kernel(ClipArgs a) {
  extern __shared__ double lds[];
  ClipLds D;
  D.Sm = lds; D.Pn = D.Sm + CL_NQ * CL_SS; D.piv = D.Pn + CL_NQ * CL_PS; D.dv = D.piv + CL_NA; D.xa = D.dv + CL_NA;
  D.xn = D.xa + CL_NA; D.vv = D.xn + 72; D.ww = D.vv + 72; D.red = D.ww + 72;
  const int t = threadIdx.x, c = blockIdx.x;
  double* CS = a.cstate + (size_t)c * CS_SIZE;
  if (CS[CS_STATUS] >= 0.0) return;
  const int f0 = a.offsets[c], T = a.offsets[c + 1] - f0;
  double* F0 = a.fstate + (size_t)f0 * FS_STRIDE;
  double mu = CS[CS_MU], gmax = CS[CS_GMAX], E = CS[CS_E];
  int iters = (int)CS[CS_ITERS], trials = (int)CS[CS_TRIALS], cur = (int)CS[CS_CUR], status = -1;
  const bool first = trials == 0;
  const bool smooth = a.s_ex != 0.0 || a.s_ang != 0.0 || a.s_t != 0.0;
  const double s_i = t < CL_NQ ? smooth_of(a, t) : 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  __syncthreads();

  // the trial point against the accepted one: differences frame by frame (thread j: frames j, j + 256, ... in order; then the fixed tree)
  double dE = 0.0, Et = 0.0, bad = 0.0;
  for (int f = t; f < T; f += FIT_THREADS) {
    const double* FS = F0 + (size_t)f * FS_STRIDE;
    const double et = FS[FS_SYS + (size_t)(1 - cur) * FIT_TRI + CL_EIDX];
    if (first) { if (FS[FS_BAD] != 0.0 || !isfinite(et)) bad = 1.0; }
    else dE += et - FS[FS_SYS + (size_t)cur * FIT_TRI + CL_EIDX];
    Et += et;
  }
  if (smooth && t < CL_NQ) {
    for (int f = 0; f + 1 < T; ++f) {
      const double* FS = F0 + (size_t)f * FS_STRIDE + CL_NA + t;
      const double dt = FS[FS_PT + FS_STRIDE] - FS[FS_PT], dc = FS[FS_P + FS_STRIDE] - FS[FS_P];
      if (!first) dE += s_i * (dt * dt - dc * dc);
      Et += s_i * dt * dt;
    }
  }
  dE = block_sum(dE, D.red);
  Et = block_sum(Et, D.red);
  if (first && block_sum(bad, D.red) != 0.0) {       // status 3: the start values go back
    for (int f = 0; f < T; ++f) {
      const size_t row = (size_t)(f0 + f);
      for (int i = t; i < 257; i += FIT_THREADS) a.coeff[row * 257 + i] = a.coeff_in[row * 257 + i];
    }
    if (t == 0) {
      double* r = a.report + (size_t)c * 4;
      r[0] = 3.0; r[1] = 0.0; r[2] = nan; r[3] = nan;
      CS[CS_STATUS] = 3.0;
    }
    return;
  }
  const bool accept = first || dE < 0.0;             // false for a non-finite cost
  if (accept) {
    if (t < FIT_NPAD)
      for (int f = 0; f < T; ++f) { double* FS = F0 + (size_t)f * FS_STRIDE; FS[FS_P + t] = FS[FS_PT + t]; }
    cur = 1 - cur;
    E = Et;
    if (!first) { mu = fmax(mu / 3.0, 1e-9); ++iters; }
    // |g|_inf over alpha (thread j < 80: the frames' rows added in frame order) and over every q_t (thread 128 + i)
    double gm = 0.0;
    if (t < CL_NA) {
      double g = 0.0;
      for (int f = 0; f < T; ++f) g += F0[(size_t)f * FS_STRIDE + FS_SYS + (size_t)cur * FIT_TRI + tri_idx(FIT_NP, t)];
      gm = fabs(g);
    } else if (t >= 128 && t < 128 + CL_NQ) {
      const int i = t - 128;
      const double si = smooth_of(a, i);
      for (int f = 0; f < T; ++f) {
        const double* FS = F0 + (size_t)f * FS_STRIDE;
        const double q = FS[FS_PT + CL_NA + i];
        double cg = 0.0;
        if (f > 0) cg += q - FS[FS_PT + CL_NA + i - FS_STRIDE];
        if (f < T - 1) cg += q - FS[FS_PT + CL_NA + i + FS_STRIDE];
        const double g = fabs(FS[FS_SYS + (size_t)cur * FIT_TRI + tri_idx(FIT_NP, CL_NA + i)] + si * cg);
        gm = (g > gm || g != g) ? g : gm;
      }
    }
    gmax = block_max(gm, D.red);
    if (gmax <= a.gtol) status = 0;
  } else {
    mu *= 4.0;
    if (mu > 1e8) status = 2;
  }
  if (status < 0 && trials >= a.max_trials) status = 1;
  if (status < 0) {
    for (;;) {                                       // at most 29 rounds: mu grows from >= 1e-9 by 4 to 1e8
      __syncthreads();
      if (clip_solve(a, D, F0, T, cur, mu, smooth)) break;
      mu *= 4.0;                                     // no factorisation: as a rejected trial, without an evaluation
      if (mu > 1e8) { status = 2; break; }
    }
  }
  __syncthreads();
  if (t == 0) {
    CS[CS_MU] = mu; CS[CS_STATUS] = (double)status; CS[CS_ITERS] = (double)iters; CS[CS_TRIALS] = (double)(trials + 1); CS[CS_GMAX] = gmax;
    CS[CS_CUR] = (double)cur; CS[CS_E] = E;
    double* r = a.report + (size_t)c * 4;
    r[0] = (double)status; r[1] = (double)iters; r[2] = E; r[3] = gmax;
  }
  if (accept || status >= 0) {                       // the accepted point of every frame
    for (int f = 0; f < T; ++f) {
      const size_t row = (size_t)(f0 + f);
      const double* P = F0 + (size_t)f * FS_STRIDE + FS_P;
      const float* in = a.coeff_in + row * 257;
      float* out = a.coeff + row * 257;
      for (int i = t; i < 257; i += FIT_THREADS) {
        const int j = i < FIT_NQ ? i : (i >= 224 && i < 227) ? FIT_NQ + (i - 224) : i >= 254 ? 147 + (i - 254) : -1;
        out[i] = j >= 0 ? (float)P[j] : in[i];
      }
      if (t < FIT_NP) a.params[row * FIT_NP + t] = P[t];
    }
  }
}

static size_t clip_offset_doubles(int clips) { return ((size_t)clips + 1 + 1) / 2 + 1; }

}  // namespace vp

extern "C" {

size_t vp_bfmfit_clip_workspace_bytes(int total_frames, int clips) {
  if (total_frames < 1 || clips < 1 || clips > total_frames) return 0;
  return (vp::FIT_TABLE_DOUBLES + vp::clip_offset_doubles(clips) + (size_t)clips * vp::CS_SIZE + (size_t)total_frames * vp::FS_STRIDE) * sizeof(double) +
         512;
}

int vp_bfmfit_clip(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights, int weights_per_frame,
                   const int* clip_offsets, int clips, const float* coeff_in, double* params, double lam_id, double lam_ex, const double* lam_smooth,
                   double gtol, int max_trials, float* coeff, double* report, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !keypoints || !landmarks || !clip_offsets || !coeff_in || !params || !lam_smooth || !coeff || !report || !workspace || clips < 1 ||
      m->nver < 1 || !m->meanshape || !m->idBase || !m->exBase) {
    vp::set_err("vp_bfmfit_clip: bad argument (null pointer, or clips < 1)");
    return VP_ERR_ARG;
  }
  for (int k = 0; k < vp::FIT_NL; ++k)
    if (keypoints[k] < 0 || keypoints[k] >= m->nver) {
      vp::set_err("vp_bfmfit_clip: bad argument (keypoint %d = %d outside 0 .. %d)", k, keypoints[k], m->nver - 1);
      return VP_ERR_ARG;
    }
  if (clip_offsets[0] != 0) {
    vp::set_err("vp_bfmfit_clip: bad argument (clip_offsets[0] = %d, must be 0)", clip_offsets[0]);
    return VP_ERR_ARG;
  }
  for (int c = 0; c < clips; ++c)
    if (clip_offsets[c + 1] <= clip_offsets[c]) {
      vp::set_err("vp_bfmfit_clip: bad argument (clip_offsets must increase: clip %d has %d frames)", c, clip_offsets[c + 1] - clip_offsets[c]);
      return VP_ERR_ARG;
    }
  const int frames = clip_offsets[clips];
  if (!(lam_id >= 0.0 && lam_id <= 1e12) || !(lam_ex >= 0.0 && lam_ex <= 1e12) || !(gtol >= 0.0) || max_trials < 0 || max_trials > 100000) {
    vp::set_err("vp_bfmfit_clip: bad argument (0 <= lam <= 1e12; gtol >= 0; 0 <= max_trials <= 100000)");
    return VP_ERR_ARG;
  }
  for (int k = 0; k < 3; ++k)
    if (!(lam_smooth[k] >= 0.0 && lam_smooth[k] <= 1e12)) {
      vp::set_err("vp_bfmfit_clip: bad argument (lam_smooth[%d] = %g outside 0 .. 1e12: weights are not negative)", k, lam_smooth[k]);
      return VP_ERR_ARG;
    }
  if (workspace_bytes < vp_bfmfit_clip_workspace_bytes(frames, clips)) {
    vp::set_err("vp_bfmfit_clip: workspace too small");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)vp::bfm_clip_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vp::CL_LDS_BYTES);
    attr_done = true;
  }
  double* tbl = vp::fit_tables(m, keypoints, table_ready, workspace, st);
  int* offsets = (int*)(tbl + vp::FIT_TABLE_DOUBLES);
  // (a pageable source: the runtime has staged the bytes when the call returns, so the caller's array is free again)
  VP_HIP_CHECK(hipMemcpyAsync(offsets, clip_offsets, ((size_t)clips + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  vp::ClipArgs a{};
  a.tbl = tbl; a.tblT = tbl + vp::FIT_NR * vp::FIT_TC;
  a.landmarks = landmarks; a.weights = weights; a.weights_per_frame = weights_per_frame ? 1 : 0;
  a.offsets = offsets; a.clips = clips; a.frames = frames;
  a.cstate = tbl + vp::FIT_TABLE_DOUBLES + vp::clip_offset_doubles(clips);
  a.fstate = a.cstate + (size_t)clips * vp::CS_SIZE;
  a.lam_id = lam_id; a.lam_ex = lam_ex; a.s_ex = lam_smooth[0]; a.s_ang = lam_smooth[1]; a.s_t = lam_smooth[2]; a.gtol = gtol;
  a.max_trials = max_trials;
  a.coeff_in = coeff_in; a.coeff = coeff; a.params = params; a.report = report;
  a.focal = m->focal; a.center = m->image_center;
  hipLaunchKernelGGL(vp::bfm_clip_init_kernel, dim3(frames + clips), dim3(vp::FIT_THREADS), 0, st, a);
  hipLaunchKernelGGL(vp::bfm_clip_frame_kernel, dim3(frames), dim3(vp::FIT_THREADS), 0, st, a);
  for (int k = 0; k < max_trials; ++k) {
    hipLaunchKernelGGL(vp::bfm_clip_step_kernel, dim3(clips), dim3(vp::FIT_THREADS), vp::CL_LDS_BYTES, st, a);
    hipLaunchKernelGGL(vp::bfm_clip_frame_kernel, dim3(frames), dim3(vp::FIT_THREADS), 0, st, a);
  }
  hipLaunchKernelGGL(vp::bfm_clip_step_kernel, dim3(clips), dim3(vp::FIT_THREADS), vp::CL_LDS_BYTES, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

// Fit BFM coefficients to 68 landmarks: the inverse of `Reconstruction` (utils/reconstruct_mesh.py:172-194) for the landmarks it returns.
// Replaces what the reference gets from FaceReconModel.pb (datasets/make_data_from_GRID.py:193-214, infer_bfmvid.py:47-74) for the
// identity, expression and pose blocks of the 257 coefficients; texture and lighting are not fitted.  float64 throughout.
//
//   unknowns   p[150] = [alpha(80) | beta(64) | angles(3) | t(3)] = coefficients 0:80, 80:144, 224:227, 254:257
//   forward    S = mean - centre + idBase alpha + exBase beta at the keypoints;  cam = (Rz Ry Rx) S + t;  qz = 10 - cam_z;
//              pi = (focal cam_x / qz + centre, 224 - (focal cam_y / qz + centre))
//   cost       E = sum_k w_k |pi_k - l_k|^2 + lam_id |alpha|^2 + lam_ex |beta|^2
//   solver     Levenberg-Marquardt: A = J^T W J + Lambda, g = J^T W r + Lambda p on the free parameters; |g|_inf <= gtol -> status 0;
//              (A + mu diag A) d = -g by Cholesky; E(p+d) < E(p): accept, mu <- max(mu/3, 1e-9); else mu <- 4 mu; mu > 1e8 -> status 2;
//              max_iters accepted steps -> status 1; non-finite input -> status 3.  mu0 = 1e-3.
//
//   table    : the keypoint rows of idBase | exBase | mean - centre as [204,145] and transposed [145,204], once per model (cached by the caller)
//   fit      : one workgroup per frame.  A's lower triangle is accumulated in registers (8x8 tiles, one per thread) from 16-row slices of J
//              staged in LDS, written with the damping to a packed triangle in LDS (151 rows: row 150 carries -g, so the factorisation
//              does the forward substitution) and factorised there.  Every sum has a fixed order: a frame's result does not depend on the batch.
//   identity : one Gauss-Newton step on an alpha shared by all frames: per-block partial systems over 64 consecutive frames (in frame
//              order), one block adds the partials in block order and solves, one launch writes alpha to every row.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "workspace.h"
#include "fit_device.h"
#include "bfm_fit_device.h"      // the frame's forward model, Jacobian slices and register-tile accumulation, shared with bfm_clip.hip

namespace vp {

constexpr int ID_N = 80;
constexpr int ID_TRI = 81 * 82 / 2;              // 3321: 80 rows + the -g row
constexpr int ID_PART = ID_TRI + 1;              // + the number of frames that took part
constexpr int ID_FRAMES = 64;      // frames per block of the identity accumulation

struct FitKeypoints { int v[FIT_NL]; };

__global__ __launch_bounds__(256) void bfm_fit_table_kernel(const double* __restrict__ meanshape, const double* __restrict__ idBase,
                                                            const double* __restrict__ exBase, int nver, double c0, double c1, double c2,
                                                            FitKeypoints kp, double* __restrict__ tbl, double* __restrict__ tblT) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= FIT_NR * FIT_TC) return;
  const int r = i / FIT_TC, j = i % FIT_TC;
  const int c = r % 3;
  const size_t rows = (size_t)3 * nver, row = (size_t)3 * kp.v[r / 3] + c;
  double v;
  if (j < 80) v = idBase[(size_t)j * rows + row];
  else if (j < FIT_NQ) v = exBase[(size_t)(j - 80) * rows + row];
  else v = meanshape[row] - (c == 0 ? c0 : c == 1 ? c1 : c2);
  tbl[r * FIT_TC + j] = v;
  tblT[j * FIT_NR + r] = v;
}

struct FitArgs {
  const double* tbl; const double* tblT;
  const double* landmarks;      // [frames,68,2]
  const double* weights;        // null, [68] or [frames,68]
  int weights_per_frame;
  const float* init;            // [frames,257]
  double* params;               // optional [frames,150]
  int params_in;
  float* coeff;                 // [frames,257]
  double* report;               // [frames,4]
  int frames;
  double lam_id, lam_ex, gtol;
  int max_iters, free_mask;
  double focal, center;
};

__global__ __launch_bounds__(FIT_THREADS) void bfm_fit_kernel(FitArgs a) {
  extern __shared__ double lds[];
  double* tri = lds;                                 // [FIT_TRI]
  double* jb = tri + FIT_TRI;                        // [16][152]
  double* p = jb + FIT_SLICE * FIT_NPAD;             // [152]
  double* ptry = p + FIT_NPAD;
  double* g = ptry + FIT_NPAD;
  double* d = g + FIT_NPAD;
  double* lam = d + FIT_NPAD;
  double* piv = lam + FIT_NPAD;
  FrameLds L;
  L.S = piv + FIT_NPAD;                              // [204]
  L.lm = L.S + FIT_NR;                               // [136]
  L.sw = L.lm + 2 * FIT_NL;                          // [68]
  L.rw = L.sw + FIT_NL;                              // [144]
  L.hh = L.rw + 144;                                 // [408]
  L.jp = L.hh + 6 * FIT_NL;                          // [816]
  L.red = L.jp + 12 * FIT_NL;                        // [256]

  const int t = threadIdx.x, f = blockIdx.x;
  const float* init = a.init + (size_t)f * 257;
  float* out = a.coeff + (size_t)f * 257;
  for (int i = t; i < 257; i += FIT_THREADS) out[i] = init[i];             // the template wherever nothing is fitted
  double bad = 0.0;
  if (t < FIT_NPAD) {
    double v = 0.0;
    if (t < FIT_NP) v = a.params_in ? a.params[(size_t)f * FIT_NP + t] : (double)init[coeff_index(t)];
    p[t] = v;
    lam[t] = t < 80 ? a.lam_id : t < FIT_NQ ? a.lam_ex : 0.0;
    if (!isfinite(v)) bad = 1.0;
  }
  if (t < 2 * FIT_NL) {
    const double v = a.landmarks[(size_t)f * 2 * FIT_NL + t];
    L.lm[t] = v;
    if (!isfinite(v)) bad = 1.0;
  }
  if (t < FIT_NL) {
    const double w = a.weights ? a.weights[(a.weights_per_frame ? (size_t)f * FIT_NL : 0) + t] : 1.0;
    L.sw[t] = w > 0.0 ? sqrt(w) : 0.0;               // (a negative or NaN weight drops the landmark)
  }
  if (t < 144) L.rw[t] = 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (block_sum(bad, L.red) != 0.0) {                // status 3: the start values go back
    if (a.params && t < FIT_NP && !a.params_in) a.params[(size_t)f * FIT_NP + t] = p[t];
    if (t == 0) { double* r = a.report + (size_t)f * 4; r[0] = 3.0; r[1] = 0.0; r[2] = nan; r[3] = nan; }
    return;
  }

  int bi, bj;
  tile_of(t, bi, bj);
  const bool has_tile = t < 19 * 20 / 2;
  double acc[8][8];

  // The cost that "E(p+d) < E(p)" compares leaves out the regularisation of the blocks that are not free: d does not touch them, so it
  // is the same number on both sides, and left in it would only set the rounding of both (a fixed |alpha|^2 of 50 hides a change of
  // 1e-15 in the rest: a pose-only fit could not see its last steps).  e_fixed is added back for the report.
  auto cost_at = [&](const double* pv) {
    double term = t < 2 * FIT_NL ? L.rw[t] * L.rw[t] : 0.0;
    if (t < FIT_NQ && (a.free_mask & free_bit(t))) term += lam[t] * pv[t] * pv[t];
    return block_sum(term, L.red);
  };
  const double e_fixed = block_sum((t < FIT_NQ && !(a.free_mask & free_bit(t))) ? lam[t] * p[t] * p[t] : 0.0, L.red);

  eval_frame<true>(a.tblT, p, L, a.focal, a.center);
  double E = cost_at(p);
  double mu = 1e-3, gmax = nan;
  int iters = 0, status = -1;
  while (status < 0) {
    // A (register tiles) and g at p; eval_frame<true>(p) has run
    double gacc;
    accum_normal(a.tbl, L, a.free_mask, jb, bi, bj, has_tile, acc, gacc);
    const bool is_free = t < FIT_NP && (a.free_mask & free_bit(t));
    if (t < FIT_NPAD) g[t] = is_free ? gacc + lam[t] * p[t] : 0.0;
    if (has_tile && bi == bj) {
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int i = 8 * bi + x;
        if (i < FIT_NP) acc[x][x] = (a.free_mask & free_bit(i)) ? acc[x][x] + lam[i] : 1.0;       // a fixed parameter: d = 0
      }
    }
    gmax = block_max(is_free ? fabs(g[t]) : 0.0, L.red);
    if (gmax <= a.gtol) { status = 0; break; }
    if (iters >= a.max_iters) { status = 1; break; }
    for (;;) {                                        // at most 29 rounds: mu grows from >= 1e-9 by 4 to 1e8
      __syncthreads();
      if (has_tile) {
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < 8; ++y) {
            const int i = 8 * bi + x, j = 8 * bj + y;
            if (i < FIT_NP && j <= i) tri[tri_idx(i, j)] = i == j ? acc[x][y] + mu * acc[x][y] : acc[x][y];
          }
      }
      if (t < FIT_NP) tri[tri_idx(FIT_NP, t)] = -g[t];
      bool accepted = false;
      double Et = nan;
      if (chol_solve(tri, piv, d, FIT_NP)) {
        if (t < FIT_NPAD) ptry[t] = (t < FIT_NP && is_free) ? p[t] + d[t] : p[t];
        __syncthreads();
        eval_frame<false>(a.tblT, ptry, L, a.focal, a.center);
        Et = cost_at(ptry);
        accepted = Et < E;                            // false for a non-finite cost on either side
      }
      if (accepted) {
        __syncthreads();
        if (t < FIT_NPAD) p[t] = ptry[t];
        E = Et;
        mu = fmax(mu / 3.0, 1e-9);
        ++iters;
        __syncthreads();
        eval_frame<true>(a.tblT, p, L, a.focal, a.center);
        break;
      }
      mu *= 4.0;
      if (mu > 1e8) { status = 2; break; }
    }
  }
  __syncthreads();
  if (t < FIT_NP) {
    if (a.params) a.params[(size_t)f * FIT_NP + t] = p[t];
    if (a.free_mask & free_bit(t)) out[coeff_index(t)] = (float)p[t];
  }
  if (t == 0) { double* r = a.report + (size_t)f * 4; r[0] = (double)status; r[1] = (double)iters; r[2] = E + e_fixed; r[3] = gmax; }
}

constexpr size_t FIT_LDS_BYTES = (size_t)(FIT_TRI + FIT_SLICE * FIT_NPAD + 6 * FIT_NPAD + FIT_NR + 2 * FIT_NL + FIT_NL + 144 + 6 * FIT_NL +
                                          12 * FIT_NL + FIT_THREADS) * sizeof(double);

struct IdArgs {
  const double* tbl; const double* tblT;
  const double* landmarks; const double* weights; int weights_per_frame;
  const double* params;         // [frames,150]
  int frames;
  double focal, center;
  double* part;                 // [blocks][ID_PART]
};

// partial system of frames 64 b .. 64 b + 63, in frame order: packed lower triangle of sum J_a^T W J_a, row 80 = - sum J_a^T W r, the frame count
__global__ __launch_bounds__(FIT_THREADS) void bfm_fit_identity_accum_kernel(IdArgs a) {
  __shared__ double jb[FIT_SLICE * ID_N];
  __shared__ double p[FIT_NPAD];
  __shared__ double buf[FIT_NR + 2 * FIT_NL + FIT_NL + 144 + 6 * FIT_NL + 12 * FIT_NL + FIT_THREADS];
  FrameLds L;
  L.S = buf; L.lm = L.S + FIT_NR; L.sw = L.lm + 2 * FIT_NL; L.rw = L.sw + FIT_NL; L.hh = L.rw + 144; L.jp = L.hh + 6 * FIT_NL; L.red = L.jp + 12 * FIT_NL;
  const int t = threadIdx.x;
  int bi, bj;
  tile_of(t, bi, bj);
  const bool has_tile = t < 20 * 21 / 2;             // 4x4 tiles of the 80 x 80 triangle
  double acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
  double gacc = 0.0;
  int used = 0;
  if (t < 144) L.rw[t] = 0.0;
  const int f0 = blockIdx.x * ID_FRAMES, f1 = min(f0 + ID_FRAMES, a.frames);
  for (int f = f0; f < f1; ++f) {
    __syncthreads();
    double bad = 0.0;
    if (t < FIT_NP) { const double v = a.params[(size_t)f * FIT_NP + t]; p[t] = v; if (!isfinite(v)) bad = 1.0; }
    if (t < 2 * FIT_NL) { const double v = a.landmarks[(size_t)f * 2 * FIT_NL + t]; L.lm[t] = v; if (!isfinite(v)) bad = 1.0; }
    if (t < FIT_NL) {
      const double w = a.weights ? a.weights[(a.weights_per_frame ? (size_t)f * FIT_NL : 0) + t] : 1.0;
      L.sw[t] = w > 0.0 ? sqrt(w) : 0.0;
    }
    if (block_sum(bad, L.red) != 0.0) continue;      // a frame the fit returned with status 3 takes no part
    ++used;
    eval_frame<true>(a.tblT, p, L, a.focal, a.center);
    for (int c = 0; c < (2 * FIT_NL + FIT_SLICE - 1) / FIT_SLICE; ++c) {
      __syncthreads();
      jac_slice<ID_N>(a.tbl, L, c, 1, jb);
      __syncthreads();
      if (has_tile) {
        for (int row = 0; row < FIT_SLICE; ++row) {
          double av[4], bv[4];
#pragma unroll
          for (int x = 0; x < 4; ++x) { av[x] = jb[row * ID_N + 4 * bi + x]; bv[x] = jb[row * ID_N + 4 * bj + x]; }
#pragma unroll
          for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = fma(av[x], bv[y], acc[x][y]);
        }
      }
      if (t < ID_N)
        for (int row = 0; row < FIT_SLICE; ++row) gacc = fma(jb[row * ID_N + t], L.rw[FIT_SLICE * c + row], gacc);
    }
  }
  double* part = a.part + (size_t)blockIdx.x * ID_PART;
  if (has_tile) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int i = 4 * bi + x, j = 4 * bj + y;
        if (j <= i) part[tri_idx(i, j)] = acc[x][y];
      }
  }
  if (t < ID_N) part[tri_idx(ID_N, t)] = -gacc;
  if (t == 0) { part[tri_idx(ID_N, ID_N)] = 0.0; part[ID_TRI] = (double)used; }
}

// adds the partials in block order, solves (A + T lam I) d = -(g + T lam alpha), alpha_new = alpha + d (alpha = row 0's)
__global__ __launch_bounds__(FIT_THREADS) void bfm_fit_identity_solve_kernel(const double* __restrict__ part, int blocks, const double* __restrict__ params,
                                                                             double lam_id, double* __restrict__ alpha_new) {
  __shared__ double tri[ID_PART];
  __shared__ double piv[ID_N], d[ID_N], alpha[ID_N];
  const int t = threadIdx.x;
  for (int e = t; e < ID_PART; e += FIT_THREADS) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(size_t)b * ID_PART + e];
    tri[e] = s;
  }
  if (t < ID_N) alpha[t] = params[t];
  __syncthreads();
  const double T = tri[ID_TRI];
  __syncthreads();
  if (t < ID_N) {
    tri[tri_idx(t, t)] += T * lam_id;
    tri[tri_idx(ID_N, t)] -= T * lam_id * alpha[t];
  }
  const bool ok = T > 0.0 && chol_solve(tri, piv, d, ID_N);
  if (t < ID_N) {
    const double v = alpha[t] + d[t];
    alpha_new[t] = (ok && isfinite(v)) ? v : alpha[t];           // no frame took part, or no solution: alpha stays
  }
}

__global__ __launch_bounds__(256) void bfm_fit_identity_write_kernel(const double* __restrict__ alpha_new, int frames, double* __restrict__ params,
                                                                     float* __restrict__ coeff) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)frames * ID_N) return;
  const size_t f = i / ID_N;
  const int j = (int)(i % ID_N);
  const double v = alpha_new[j];
  params[f * FIT_NP + j] = v;
  if (coeff) coeff[f * 257 + j] = (float)v;
}

// workspace: [tbl 204x145][tblT 145x204][alpha_new 80][partials blocks x ID_PART]
static size_t fit_table_doubles() { return (size_t)2 * FIT_NR * FIT_TC; }
static int id_blocks(int frames) { return (frames + ID_FRAMES - 1) / ID_FRAMES; }

static bool check_common(const char* who, const vp_bfm_model* m, const int* keypoints, const double* landmarks, int frames, const void* workspace,
                         size_t workspace_bytes) {
  if (!m || !keypoints || !landmarks || !workspace || frames < 1 || m->nver < 1 || !m->meanshape || !m->idBase || !m->exBase) {
    set_err("%s: bad argument", who);
    return false;
  }
  for (int k = 0; k < FIT_NL; ++k)
    if (keypoints[k] < 0 || keypoints[k] >= m->nver) {
      set_err("%s: bad argument (keypoint %d = %d outside 0 .. %d)", who, k, keypoints[k], m->nver - 1);
      return false;
    }
  if (workspace_bytes < vp_bfmfit_workspace_bytes(frames)) {
    set_err("%s: workspace too small", who);
    return false;
  }
  return true;
}

double* fit_tables(const vp_bfm_model* m, const int* keypoints, int table_ready, void* workspace, hipStream_t st) {
  double* tbl = vp::align256((double*)workspace);
  if (!table_ready) {
    FitKeypoints kp;
    for (int k = 0; k < FIT_NL; ++k) kp.v[k] = keypoints[k];
    hipLaunchKernelGGL(bfm_fit_table_kernel, dim3((FIT_NR * FIT_TC + 255) / 256), dim3(256), 0, st, m->meanshape, m->idBase, m->exBase, m->nver,
                       m->center[0], m->center[1], m->center[2], kp, tbl, tbl + FIT_NR * FIT_TC);
  }
  return tbl;
}

}  // namespace vp

extern "C" {

size_t vp_bfmfit_workspace_bytes(int frames) {
  if (frames < 1) return 0;
  return (vp::fit_table_doubles() + vp::ID_N + (size_t)vp::id_blocks(frames) * vp::ID_PART) * sizeof(double) + 512;
}

int vp_bfmfit_fit(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights, int weights_per_frame,
                  const float* init, double* params, int params_in, int frames, double lam_id, double lam_ex, double gtol, int max_iters, int free_mask,
                  float* coeff, double* report, void* workspace, size_t workspace_bytes, void* stream) {
  if (!vp::check_common("vp_bfmfit_fit", m, keypoints, landmarks, frames, workspace, workspace_bytes)) return VP_ERR_ARG;
  if (!init || !coeff || !report || (params_in && !params) || !(lam_id >= 0.0 && lam_id <= 1e12) || !(lam_ex >= 0.0 && lam_ex <= 1e12) ||
      !(gtol >= 0.0) || max_iters < 0 || max_iters > 100000 || free_mask < 1 || free_mask > 15) {
    vp::set_err("vp_bfmfit_fit: bad argument (init, coeff, report; 0 <= lam <= 1e12; gtol >= 0; 0 <= max_iters <= 100000; free 1 .. 15)");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)vp::bfm_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vp::FIT_LDS_BYTES);
    attr_done = true;
  }
  double* tbl = vp::fit_tables(m, keypoints, table_ready, workspace, st);
  vp::FitArgs a{};
  a.tbl = tbl; a.tblT = tbl + vp::FIT_NR * vp::FIT_TC;
  a.landmarks = landmarks; a.weights = weights; a.weights_per_frame = weights_per_frame ? 1 : 0;
  a.init = init; a.params = params; a.params_in = params_in ? 1 : 0; a.coeff = coeff; a.report = report; a.frames = frames;
  a.lam_id = lam_id; a.lam_ex = lam_ex; a.gtol = gtol; a.max_iters = max_iters; a.free_mask = free_mask;
  a.focal = m->focal; a.center = m->image_center;
  hipLaunchKernelGGL(vp::bfm_fit_kernel, dim3(frames), dim3(vp::FIT_THREADS), vp::FIT_LDS_BYTES, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_bfmfit_identity_step(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights,
                            int weights_per_frame, double* params, float* coeff, int frames, double lam_id, void* workspace, size_t workspace_bytes,
                            void* stream) {
  if (!vp::check_common("vp_bfmfit_identity_step", m, keypoints, landmarks, frames, workspace, workspace_bytes)) return VP_ERR_ARG;
  if (!params || !(lam_id >= 0.0 && lam_id <= 1e12)) {
    vp::set_err("vp_bfmfit_identity_step: bad argument (params; 0 <= lam_id <= 1e12)");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double* tbl = vp::fit_tables(m, keypoints, table_ready, workspace, st);
  double* alpha_new = tbl + vp::fit_table_doubles();
  const int blocks = vp::id_blocks(frames);
  vp::IdArgs a{};
  a.tbl = tbl; a.tblT = tbl + vp::FIT_NR * vp::FIT_TC;
  a.landmarks = landmarks; a.weights = weights; a.weights_per_frame = weights_per_frame ? 1 : 0; a.params = params; a.frames = frames;
  a.focal = m->focal; a.center = m->image_center; a.part = alpha_new + vp::ID_N;
  hipLaunchKernelGGL(vp::bfm_fit_identity_accum_kernel, dim3(blocks), dim3(vp::FIT_THREADS), 0, st, a);
  hipLaunchKernelGGL(vp::bfm_fit_identity_solve_kernel, dim3(1), dim3(vp::FIT_THREADS), 0, st, a.part, blocks, params, lam_id, alpha_new);
  hipLaunchKernelGGL(vp::bfm_fit_identity_write_kernel, dim3((unsigned)(((size_t)frames * vp::ID_N + 255) / 256)), dim3(256), 0, st, alpha_new, frames,
                     params, coeff);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

// One frame of the landmark fit on the device, shared by bfm_fit.hip (the per-frame fit) and bfm_clip.hip (the joint fit of a clip): the
// forward model at the keypoints, the per-landmark factors of its Jacobian, 16-row slices of J in LDS and the accumulation of J^T W J in
// 8x8 register tiles.  float64 throughout; workgroups of FIT_THREADS threads.  bfm_fit.hip's header states the model and the rule.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vp_hip.h"
#include "fit_device.h"

namespace vp {

constexpr int FIT_NP = 150;        // unknowns
constexpr int FIT_NPAD = 152;      // padded to a multiple of the 8x8 tile
constexpr int FIT_NQ = 144;        // alpha | beta
constexpr int FIT_NL = 68;         // landmarks
constexpr int FIT_NR = 204;        // table rows: 3 per landmark
constexpr int FIT_TC = 145;        // table columns: 144 bases + the centred mean
constexpr int FIT_SLICE = 16;      // rows of J per LDS slice (8 landmarks)
constexpr int FIT_TRI = 151 * 152 / 2;           // packed lower triangle of 151 rows
constexpr int FIT_FRAME_LDS = FIT_NR + 2 * FIT_NL + FIT_NL + 144 + 6 * FIT_NL + 12 * FIT_NL + FIT_THREADS;      // FrameLds, doubles

// LDS arrays one frame's evaluation works on
struct FrameLds {
  double* S;       // [204] shape at the keypoints
  double* lm;      // [136] target landmarks
  double* sw;      // [68]  sqrt(weight)
  double* rw;      // [144] sqrt(w) * residual, rows 136.. stay 0
  double* hh;      // [68][6]  d pi / d S for the x and the y row (already times M)
  double* jp;      // [68][12] d pi / d (angles, t) for the x and the y row
  double* red;     // [256]
};

__device__ __forceinline__ void frame_lds(double* buf, FrameLds& L) {
  L.S = buf; L.lm = L.S + FIT_NR; L.sw = L.lm + 2 * FIT_NL; L.rw = L.sw + FIT_NL; L.hh = L.rw + 144; L.jp = L.hh + 6 * FIT_NL; L.red = L.jp + 12 * FIT_NL;
}

// One coordinate of the shape: mean + sum_j base_j p_j as a compensated dot product (error-free product and sum, the small terms first,
// the mean last).  The plain 144-term sum leaves 1e-15 in the shape, 1e-13 px in every residual and 1e-12 in E, which is what a step
// taken at |g|_inf = 1e-6 gains: the acceptance test E(p+d) < E(p) would stall a fit there.  This keeps the shape to an ulp.
__device__ __forceinline__ double shape_row(const double* __restrict__ tblT, const double* pv, int row) {
#pragma clang fp contract(off)
  double s = 0.0, c = 0.0;
  for (int j = 0; j < FIT_NQ; ++j) {
    const double a = tblT[j * FIT_NR + row], b = pv[j];
    const double h = a * b, r = __builtin_fma(a, b, -h);          // a b = h + r exactly
    const double u = s + h, z = u - s;
    c += ((s - (u - z)) + (h - z)) + r;                             // s + h = u + (...) exactly
    s = u;
  }
  const double m = tblT[FIT_NQ * FIT_NR + row];
  const double u = s + m, z = u - s;
  c += (s - (u - z)) + (m - z);
  return u + c;
}

// residuals (and, with kJac, the per-landmark factors of the Jacobian) at the parameters pv [150] (LDS).  Ends with a barrier.
template <bool kJac>
__device__ void eval_frame(const double* __restrict__ tblT, const double* pv, const FrameLds& L, double focal, double center) {
  const int t = threadIdx.x;
  if (t < FIT_NR) L.S[t] = shape_row(tblT, pv, t);
  __syncthreads();
  if (t < FIT_NL) {
    double sx, cx, sy, cy, sz, cz;
    sincos(pv[144], &sx, &cx); sincos(pv[145], &sy, &cy); sincos(pv[146], &sz, &cz);
    // M = Rz Ry Rx
    const double m00 = cz * cy, m01 = cz * sy * sx - sz * cx, m02 = cz * sy * cx + sz * sx;
    const double m10 = sz * cy, m11 = sz * sy * sx + cz * cx, m12 = sz * sy * cx - cz * sx;
    const double m20 = -sy, m21 = cy * sx, m22 = cy * cx;
    const double X = L.S[3 * t], Y = L.S[3 * t + 1], Z = L.S[3 * t + 2];
    const double camx = m00 * X + m01 * Y + m02 * Z + pv[147];
    const double camy = m10 * X + m11 * Y + m12 * Z + pv[148];
    const double camz = m20 * X + m21 * Y + m22 * Z + pv[149];
    const double qz = 10.0 - camz;
    const double u = focal * camx / qz + center, v = 224.0 - (focal * camy / qz + center);
    const double w = L.sw[t];
    // a landmark of weight 0 is dropped: its residual does not enter, whatever it is
    L.rw[2 * t] = w == 0.0 ? 0.0 : w * (u - L.lm[2 * t]);
    L.rw[2 * t + 1] = w == 0.0 ? 0.0 : w * (v - L.lm[2 * t + 1]);
    if (kJac) {
      const double gx0 = focal / qz, gx2 = focal * camx / (qz * qz);          // d u / d cam = (gx0, 0, gx2)
      const double gy1 = -focal / qz, gy2 = -focal * camy / (qz * qz);        // d v / d cam = (0, gy1, gy2)
      double* h = L.hh + 6 * t;
      h[0] = gx0 * m00 + gx2 * m20; h[1] = gx0 * m01 + gx2 * m21; h[2] = gx0 * m02 + gx2 * m22;
      h[3] = gy1 * m10 + gy2 * m20; h[4] = gy1 * m11 + gy2 * m21; h[5] = gy1 * m12 + gy2 * m22;
      // d cam / d angle = (dM/d angle) S
      const double ax0 = (cz * sy * cx + sz * sx) * Y + (-cz * sy * sx + sz * cx) * Z;
      const double ax1 = (sz * sy * cx - cz * sx) * Y + (-sz * sy * sx - cz * cx) * Z;
      const double ax2 = (cy * cx) * Y + (-cy * sx) * Z;
      const double ay0 = (-cz * sy) * X + (cz * cy * sx) * Y + (cz * cy * cx) * Z;
      const double ay1 = (-sz * sy) * X + (sz * cy * sx) * Y + (sz * cy * cx) * Z;
      const double ay2 = (-cy) * X + (-sy * sx) * Y + (-sy * cx) * Z;
      const double az0 = -m10 * X - m11 * Y - m12 * Z;
      const double az1 = m00 * X + m01 * Y + m02 * Z;
      double* q = L.jp + 12 * t;
      q[0] = gx0 * ax0 + gx2 * ax2; q[1] = gx0 * ay0 + gx2 * ay2; q[2] = gx0 * az0; q[3] = gx0; q[4] = 0.0; q[5] = gx2;
      q[6] = gy1 * ax1 + gy2 * ax2; q[7] = gy1 * ay1 + gy2 * ay2; q[8] = gy1 * az1; q[9] = 0.0; q[10] = gy1; q[11] = gy2;
    }
  }
  __syncthreads();
}

// J rows 16c .. 16c+15 (landmarks 8c .. 8c+7), times sqrt(w), columns 0 .. kCols-1 -> jb [16][kCols]; columns not in free_mask are 0
template <int kCols>
__device__ void jac_slice(const double* __restrict__ tbl, const FrameLds& L, int c, int free_mask, double* jb) {
  for (int e = threadIdx.x; e < FIT_SLICE * kCols; e += FIT_THREADS) {
    const int row = e / kCols, j = e % kCols;
    const int k = 8 * c + (row >> 1), uv = row & 1;
    double v = 0.0;
    const int bit = j < 80 ? 1 : j < FIT_NQ ? 2 : j < 147 ? 4 : 8;
    if (k < FIT_NL && j < FIT_NP && (free_mask & bit) && L.sw[k] != 0.0) {
      if (j < FIT_NQ) {
        const double* h = L.hh + 6 * k + 3 * uv;
        const double* tr = tbl + (3 * k) * FIT_TC + j;
        v = h[0] * tr[0] + h[1] * tr[FIT_TC] + h[2] * tr[2 * FIT_TC];
      } else {
        v = L.jp[12 * k + 6 * uv + (j - FIT_NQ)];
      }
      v *= L.sw[k];
    }
    jb[e] = v;
  }
}

// tile (bi, bj), bj <= bi, of thread t in the lower triangle of kTs x kTs tiles
__device__ __forceinline__ void tile_of(int t, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= t && bi < 64) ++bi;
  bj = t - bi * (bi + 1) / 2;
}

constexpr int FIT_TILES = 19 * 20 / 2;           // 8x8 tiles in the lower triangle of 152 x 152: one per thread

// J^T W J (lower triangle, the 8x8 tile (bi, bj) of this thread in acc) and J^T W r (element threadIdx.x in gacc) over the free columns at
// the point eval_frame<true> has just run for.  jb: LDS [16][152].  Rows are added slice by slice, in row order.
__device__ __forceinline__ void accum_normal(const double* __restrict__ tbl, const FrameLds& L, int free_mask, double* jb, int bi, int bj,
                                             bool has_tile, double (&acc)[8][8], double& gacc) {
  const int t = threadIdx.x;
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int y = 0; y < 8; ++y) acc[x][y] = 0.0;
  gacc = 0.0;
  for (int c = 0; c < (2 * FIT_NL + FIT_SLICE - 1) / FIT_SLICE; ++c) {
    __syncthreads();
    jac_slice<FIT_NPAD>(tbl, L, c, free_mask, jb);
    __syncthreads();
    if (has_tile) {
      for (int row = 0; row < FIT_SLICE; ++row) {
        double av[8], bv[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) { av[x] = jb[row * FIT_NPAD + 8 * bi + x]; bv[x] = jb[row * FIT_NPAD + 8 * bj + x]; }
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < 8; ++y) acc[x][y] = fma(av[x], bv[y], acc[x][y]);
      }
    }
    if (t < FIT_NP)
      for (int row = 0; row < FIT_SLICE; ++row) gacc = fma(jb[row * FIT_NPAD + t], L.rw[FIT_SLICE * c + row], gacc);
  }
}

__device__ __forceinline__ int coeff_index(int j) { return j < FIT_NQ ? j : j < 147 ? 224 + (j - FIT_NQ) : 254 + (j - 147); }
__device__ __forceinline__ int free_bit(int j) { return j < 80 ? 1 : j < FIT_NQ ? 2 : j < 147 ? 4 : 8; }

// the keypoint tables [204,145] and [145,204] at the head of a workspace (bfm_fit.hip); gathers them first unless table_ready
constexpr size_t FIT_TABLE_DOUBLES = (size_t)2 * FIT_NR * FIT_TC;
double* fit_tables(const vp_bfm_model* m, const int* keypoints, int table_ready, void* workspace, hipStream_t st);

}  // namespace vp

// Trimap and closed-form matting solve (include/vp_hip.h, vp_mattesolve_*): the trimap from an erosion and a dilation of a matte, and
// alpha inside its unknown band from the matting Laplacian of Levin, Lischinski and Weiss, applied by window sums, solved by
// Jacobi-preconditioned conjugate gradients in float64.  The header defines every number; this translation unit is compiled with
// -ffp-contract=off.
//
// One workgroup of 256 lanes per 32 x 32 tile and frame in every launch.
//   trimap   the tile's matte bytes with a halo of 32 as two bits in LDS, the row pass, the column pass; and whether the tile holds an
//            unknown pixel.
//   product  (ms_apply) the frame's bytes and p for the tile with a halo of 2 r in LDS; then in two halves of 16 rows: a_j, b_j of
//            the windows of (16 + 2 r) x (32 + 2 r) centres into LDS, each window's moments formed again from the bytes (exact integer
//            sums, one 3 x 3 adjugate), and the sums of a_j, b_j over each pixel's window.  a and b never leave LDS, and no moment or
//            inverse is kept in memory.  Measured against the form that keeps them as nine float64 planes (VP_MS_STORED below; 64 frames
//            of 512 x 512): stored planes make an iteration 1.8 % faster at radius 1 and 5.7 % at radius 2 and the workspace 120 bytes
//            per pixel instead of 48; this form is the shipped one (profiles/matte_solve.json, matte_solve_stored.json).
//   solve    one fill, the init launch (b = -(L k)_U, 1 / diag(L), r, z, p, the partial sums of b.b and r.z; diag by its definition:
//            the windows that hold the pixel, each one's moments formed again), then per iteration two launches:
//              P   sums the tiles' partials of r.r, b.b and r.z in a fixed order (every workgroup of the frame does, and gets the same
//                  bits), stops the frame or forms the new direction p = z + beta p for tile and halo, writes it for the tile,
//                  L p and the tile's partial of p.Lp;
//              U   sums p.Lp and r.z, alpha, x += alpha p, r -= alpha L p, the tile's partials of r.r and r.z;
//            and the finish launch: the report of the frames that ran to `iters` and the matte's bytes.
//            The direction is double-buffered (a tile reads its neighbours' old p while they write the new one); r.z's partials are
//            too.  A stopped frame has its flag set by every workgroup that sees the stop (all see the same sums).  A workgroup reads the
//            flag through one lane and LDS (ms_idle), so all its waves take the same way; one that still reads it as clear in the launch
//            in which others set it forms the same sums and comes to the same decision.  No launch waits on another workgroup.
// LDS of a product launch: 3 x 44 x 44 bytes, 44 x 44 + 4 x 22 x 38 + 256 doubles: 49.6 KiB.  Every index is bounded by the call's height
// and width, checked against the descriptor, the pitch and the stride before anything is enqueued.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>

#include "frame_args.h"
#include "vp_common.h"
#include "workspace.h"

#pragma clang fp contract(off)

// Build-time A/B (make one FILE=matte_solve VAR=stored DEFS=-DVP_MS_STORED=1): the window's mean and inverse kept as nine float64 planes
// in the workspace, written once per solve, in place of forming them again in every product.  Same numbers, same bits; DESIGN.md 6 has
// the measurement.
#ifndef VP_MS_STORED
#define VP_MS_STORED 0
#endif

namespace vp {

constexpr int kMsLanes = 256;
constexpr int kMsTile = 32;
constexpr int kMsPer = kMsTile * kMsTile / kMsLanes;                  // 4 pixels per lane: two in each half
constexpr int kMsHalf = kMsTile / 2;
constexpr int kMsEdge = kMsTile + 4 * VP_MATTESOLVE_MAX_RADIUS;       // 44: p and the bytes
constexpr int kMsWinCols = kMsTile + 2 * VP_MATTESOLVE_MAX_RADIUS;    // 38: window centres of a half
constexpr int kMsWinRows = kMsHalf + 2 * VP_MATTESOLVE_MAX_RADIUS;    // 22
constexpr int kMsReport = VP_MATTESOLVE_REPORT_INTS;
constexpr int kMsHalo = VP_MATTESOLVE_MAX_SQUARE / 2;                 // 32: the trimap's
constexpr int kMsTriEdge = kMsTile + 2 * kMsHalo;                     // 96
enum { kPartBB = 0, kPartRR = 1, kPartPAP = 2, kPartRZ = 3, kPartCount = 5 };   // kPartRZ + parity

struct MsArgs {
  const unsigned char* frames;
  size_t pitch, stride;                      // bytes
  const unsigned char* tri;                  // [n][H][W]
  const double* pin;                         // the single op's plane
  double* pout;
  double *x, *r, *dinv, *p0, *p1, *ap;       // [n][H][W]
  double* part;                              // [5][pcap]: per frame and tile
  size_t pcap;
  double* mom;                               // VP_MS_STORED: [9][mcap]: mu 0 1 2, inv 00 01 02 11 12 22 per pixel
  size_t mcap;
  int *active, *flag, *report;               // [n][tiles], [n], [n][8]
  unsigned char* matte;
  double eps, tol2;
  int H, W, radius, it, iters, tiles;
};

// MOMENTS of the header for the window centred on (lx, ly) of the staged bytes (0 outside the image, so every sum is the clipped
// window's); nw its pixel count.  With kP also the sums of p and I p over it, rows in increasing y, within a row increasing x.
template <bool kP>
__device__ __forceinline__ void ms_window(const unsigned char* sI, const double* sp, int E, int lx, int ly, int r, int nw, double eps, double* mu,
                                          double* inv, double* sums) {
  int S[3] = {0, 0, 0}, S2[6] = {0, 0, 0, 0, 0, 0};
  double s = 0.0, sc[3] = {0.0, 0.0, 0.0};
  const int plane = E * E;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int at = (ly + dy) * E + lx + dx;
      const int c0 = sI[at], c1 = sI[plane + at], c2 = sI[2 * plane + at];
      S[0] += c0; S[1] += c1; S[2] += c2;
      S2[0] += c0 * c0; S2[1] += c0 * c1; S2[2] += c0 * c2; S2[3] += c1 * c1; S2[4] += c1 * c2; S2[5] += c2 * c2;
      if (kP) {
        const double pv = sp[at];
        s += pv;
        sc[0] += (double)c0 * pv; sc[1] += (double)c1 * pv; sc[2] += (double)c2 * pv;
      }
    }
  const double nd = (double)nw, nn = nd * nd, reg = eps / nd;
  for (int c = 0; c < 3; ++c) mu[c] = (double)S[c] / nd;
  // at most 49 * 49 * 255 * 255: an int
  const double a = (double)(nw * S2[0] - S[0] * S[0]) / nn + reg, b = (double)(nw * S2[1] - S[0] * S[1]) / nn, c = (double)(nw * S2[2] - S[0] * S[2]) / nn;
  const double d = (double)(nw * S2[3] - S[1] * S[1]) / nn + reg, e = (double)(nw * S2[4] - S[1] * S[2]) / nn, f = (double)(nw * S2[5] - S[2] * S[2]) / nn + reg;
  const double A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d, A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
  const double D = (a * A00 + b * A01) + c * A02;
  inv[0] = A00 / D; inv[1] = A01 / D; inv[2] = A02 / D; inv[3] = A11 / D; inv[4] = A12 / D; inv[5] = A22 / D;
  if (kP) { sums[0] = s; sums[1] = sc[0]; sums[2] = sc[1]; sums[3] = sc[2]; }
}

// the sums of p and I p over the window alone (the stored form of the product)
__device__ __forceinline__ void ms_psums(const unsigned char* sI, const double* sp, int E, int lx, int ly, int r, double* sums) {
  double s = 0.0, sc[3] = {0.0, 0.0, 0.0};
  const int plane = E * E;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int at = (ly + dy) * E + lx + dx;
      const double pv = sp[at];
      s += pv;
      sc[0] += (double)sI[at] * pv; sc[1] += (double)sI[plane + at] * pv; sc[2] += (double)sI[2 * plane + at] * pv;
    }
  sums[0] = s; sums[1] = sc[0]; sums[2] = sc[1]; sums[3] = sc[2];
}

// the frame's bytes for the tile with a halo of 2 r: three planes of E x E, 0 outside the image
__device__ __forceinline__ void ms_stage_bytes(const MsArgs& g, unsigned char* sI, int x0, int y0, int f) {
  const int r = g.radius, E = kMsTile + 4 * r;
  const unsigned char* frame = g.frames + (size_t)f * g.stride;
  for (int i = threadIdx.x; i < E * E; i += kMsLanes) {
    const int ly = i / E, lx = i - ly * E, gx = x0 - 2 * r + lx, gy = y0 - 2 * r + ly;
    int c0 = 0, c1 = 0, c2 = 0;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) {
      const unsigned char* px = frame + (size_t)gy * g.pitch + 3 * gx;
      c0 = px[0]; c1 = px[1]; c2 = px[2];
    }
    sI[i] = (unsigned char)c0; sI[E * E + i] = (unsigned char)c1; sI[2 * E * E + i] = (unsigned char)c2;
  }
}

// the lane's pixel q (0 .. 3) of the tile: q / 2 is the half
__device__ __forceinline__ void ms_pixel(int q, int* tx, int* ty) {
  const int li = threadIdx.x + (q & 1) * kMsLanes;
  *ty = (q >> 1) * kMsHalf + (li >> 5);
  *tx = li & 31;
}

// LAPLACIAN of the header for the lane's four pixels: sI and sp are staged and a barrier has passed.  Every lane of the workgroup calls it.
template <bool kStored>
__device__ __forceinline__ void ms_apply(const MsArgs& g, const unsigned char* sI, const double* sp, double* sab, int x0, int y0, double* lp, size_t plane0 = 0) {
  const int r = g.radius, E = kMsTile + 4 * r, cols = kMsTile + 2 * r, rows = kMsHalf + 2 * r, taps = 2 * r + 1;
  constexpr int kPlane = kMsWinRows * kMsWinCols;
  for (int half = 0; half < 2; ++half) {
    for (int i = threadIdx.x; i < rows * cols; i += kMsLanes) {
      const int wy = i / cols, wx = i - wy * cols;
      const int cx = wx - r, cy = half * kMsHalf - r + wy, gx = x0 + cx, gy = y0 + cy;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, b = 0.0;
      if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) {
        const int nw = window_extent(gx, r, g.W) * window_extent(gy, r, g.H);
        double mu[3], inv[6], s[4];
        if (kStored) {
          const double* m = g.mom + plane0 + (size_t)gy * g.W + gx;
          for (int c = 0; c < 3; ++c) mu[c] = m[c * g.mcap];
          for (int c = 0; c < 6; ++c) inv[c] = m[(3 + c) * g.mcap];
          ms_psums(sI, sp, E, cx + 2 * r, cy + 2 * r, r, s);
        } else {
          ms_window<true>(sI, sp, E, cx + 2 * r, cy + 2 * r, r, nw, g.eps, mu, inv, s);
        }
        const double nd = (double)nw, mp = s[0] / nd;
        const double v0 = s[1] / nd - mu[0] * mp, v1 = s[2] / nd - mu[1] * mp, v2 = s[3] / nd - mu[2] * mp;
        a0 = (inv[0] * v0 + inv[1] * v1) + inv[2] * v2;
        a1 = (inv[1] * v0 + inv[3] * v1) + inv[4] * v2;
        a2 = (inv[2] * v0 + inv[4] * v1) + inv[5] * v2;
        b = mp - ((a0 * mu[0] + a1 * mu[1]) + a2 * mu[2]);
      }
      sab[i] = a0; sab[kPlane + i] = a1; sab[2 * kPlane + i] = a2; sab[3 * kPlane + i] = b;
    }
    __syncthreads();
    for (int j = 0; j < 2; ++j) {
      int tx, ty;
      ms_pixel(2 * half + j, &tx, &ty);
      const int gx = x0 + tx, gy = y0 + ty;
      double out = 0.0;
      if (gx < g.W && gy < g.H) {
        double sa0 = 0.0, sa1 = 0.0, sa2 = 0.0, sb = 0.0;
        for (int dy = 0; dy < taps; ++dy)
          for (int dx = 0; dx < taps; ++dx) {
            const int at = (ty - half * kMsHalf + dy) * cols + tx + dx;
            sa0 += sab[at]; sa1 += sab[kPlane + at]; sa2 += sab[2 * kPlane + at]; sb += sab[3 * kPlane + at];
          }
        const int at = (ty + 2 * r) * E + tx + 2 * r;
        const double I0 = (double)sI[at], I1 = (double)sI[E * E + at], I2 = (double)sI[2 * E * E + at];
        const double nd = (double)(window_extent(gx, r, g.W) * window_extent(gy, r, g.H));
        out = nd * sp[at] - (((sa0 * I0 + sa1 * I1) + sa2 * I2) + sb);
      }
      lp[2 * half + j] = out;
    }
    __syncthreads();
  }
}

// the workgroup's sum of v in a fixed tree; every lane gets it
__device__ __forceinline__ double ms_tree(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kMsLanes / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// the frame's sum of one kind of partial over its tiles: lane t takes tiles t, t + 256, .. in that order, then the tree
__device__ __forceinline__ double ms_frame_sum(const MsArgs& g, int kind, int f, double* red) {
  const double* part = g.part + (size_t)kind * g.pcap + (size_t)f * g.tiles;
  double v = 0.0;
  for (int t = threadIdx.x; t < g.tiles; t += kMsLanes) v += part[t];
  return ms_tree(v, red);
}

// Whether this workgroup has nothing to do: its frame has stopped or its tile holds no unknown pixel.  One lane reads both words, a
// barrier follows, and every lane branches on the value in LDS: all waves of the workgroup take the same way whenever another
// workgroup's store of the flag lands.
__device__ __forceinline__ bool ms_idle(const MsArgs& g, int f, int tile, int* shared) {
  if (threadIdx.x == 0) *shared = g.flag[f] || !g.active[(size_t)f * g.tiles + tile];
  __syncthreads();
  return *shared != 0;
}

__device__ __forceinline__ void ms_stop(const MsArgs& g, int f, int iterations, int status, double residual) {
  if (threadIdx.x != 0) return;
  int* rep = g.report + f * kMsReport;
  rep[1] = iterations;
  rep[2] = status;
  *(double*)(rep + 4) = residual;
  g.flag[f] = 1;
}

#define MS_SHARED                                                    \
  __shared__ unsigned char sI[3 * kMsEdge * kMsEdge];                \
  __shared__ double sp[kMsEdge * kMsEdge];                           \
  __shared__ double sab[4 * kMsWinRows * kMsWinCols];                \
  __shared__ double red[kMsLanes]

// the single op: out = L p, no masking.  grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kMsLanes) void ms_laplacian_kernel(const MsArgs g) {
  MS_SHARED;
  (void)red;
  const int r = g.radius, E = kMsTile + 4 * r, x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile, f = blockIdx.z;
  const size_t plane = (size_t)f * g.H * g.W;
  ms_stage_bytes(g, sI, x0, y0, f);
  for (int i = threadIdx.x; i < E * E; i += kMsLanes) {
    const int ly = i / E, lx = i - ly * E, gx = x0 - 2 * r + lx, gy = y0 - 2 * r + ly;
    sp[i] = (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) ? g.pin[plane + (size_t)gy * g.W + gx] : 0.0;
  }
  __syncthreads();
  double lp[kMsPer];
  ms_apply<false>(g, sI, sp, sab, x0, y0, lp);
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    if (x0 + tx < g.W && y0 + ty < g.H) g.pout[plane + (size_t)(y0 + ty) * g.W + x0 + tx] = lp[q];
  }
}

// grid (tiles_x, tiles_y, n): every tile, with or without unknown pixels
__global__ __launch_bounds__(kMsLanes) void ms_init_kernel(const MsArgs g) {
  MS_SHARED;
  __shared__ int count;
  const int r = g.radius, E = kMsTile + 4 * r, x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile, f = blockIdx.z;
  const int tile = blockIdx.y * gridDim.x + blockIdx.x;
  const size_t plane = (size_t)f * g.H * g.W;
  const unsigned char* tri = g.tri + plane;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  int t[kMsPer], mine = 0;
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    t[q] = (x0 + tx < g.W && y0 + ty < g.H) ? tri[(size_t)(y0 + ty) * g.W + x0 + tx] : 0;
    mine += t[q] != 0 && t[q] != 255;
  }
  if (mine) atomicAdd(&count, mine);
  __syncthreads();
  const int unknown = count;
  double lp[kMsPer] = {0.0, 0.0, 0.0, 0.0};
  if (unknown) {
    ms_stage_bytes(g, sI, x0, y0, f);
    for (int i = threadIdx.x; i < E * E; i += kMsLanes) {
      const int ly = i / E, lx = i - ly * E, gx = x0 - 2 * r + lx, gy = y0 - 2 * r + ly;
      sp[i] = (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H && tri[(size_t)gy * g.W + gx] == 255) ? 1.0 : 0.0;
    }
    __syncthreads();
    ms_apply<false>(g, sI, sp, sab, x0, y0, lp);
  }
  double bb = 0.0, rz = 0.0;
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    const size_t o = plane + (size_t)gy * g.W + gx;
    double x = t[q] == 255 ? 1.0 : 0.0, b = 0.0, dinv = 0.0, z = 0.0;
    if (t[q] != 0 && t[q] != 255) {
      // DIAGONAL of the header: the windows j that hold this pixel, rows in increasing y, within a row increasing x
      const int at = (ty + 2 * r) * E + tx + 2 * r;
      const double I0 = (double)sI[at], I1 = (double)sI[E * E + at], I2 = (double)sI[2 * E * E + at];
      double diag = 0.0;
      for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
          const int jx = gx + dx, jy = gy + dy;
          if (jx < 0 || jx >= g.W || jy < 0 || jy >= g.H) continue;
          const int nw = window_extent(jx, r, g.W) * window_extent(jy, r, g.H);
          double mu[3], inv[6];
          ms_window<false>(sI, nullptr, E, tx + 2 * r + dx, ty + 2 * r + dy, r, nw, g.eps, mu, inv, nullptr);
          const double d0 = I0 - mu[0], d1 = I1 - mu[1], d2 = I2 - mu[2];
          const double q0 = (inv[0] * d0 + inv[1] * d1) + inv[2] * d2, q1 = (inv[1] * d0 + inv[3] * d1) + inv[4] * d2;
          const double q2 = (inv[2] * d0 + inv[4] * d1) + inv[5] * d2;
          diag += 1.0 - (1.0 + ((d0 * q0 + d1 * q1) + d2 * q2)) / (double)nw;
        }
      x = 0.0;
      b = -lp[q];
      dinv = 1.0 / diag;
      z = dinv * b;
      bb += b * b;
      rz += b * z;
    }
    g.x[o] = x; g.r[o] = b; g.dinv[o] = dinv; g.p0[o] = z; g.p1[o] = 0.0; g.ap[o] = 0.0;
  }
  bb = ms_tree(bb, red);
  rz = ms_tree(rz, red);
  if (threadIdx.x == 0) {
    const size_t at = (size_t)f * g.tiles + tile;
    g.part[kPartBB * g.pcap + at] = bb;
    g.part[kPartRR * g.pcap + at] = bb;                  // r = b before the first iteration
    g.part[kPartPAP * g.pcap + at] = 0.0;
    g.part[kPartRZ * g.pcap + at] = rz;
    g.part[(kPartRZ + 1) * g.pcap + at] = 0.0;
    g.active[at] = unknown > 0;
    if (unknown) atomicAdd(&g.report[f * kMsReport], unknown);    // an integer: any order gives the same count
  }
}

#if VP_MS_STORED
// the nine planes of the stored form: grid (tiles_x, tiles_y, n), every tile
__global__ __launch_bounds__(kMsLanes) void ms_moments_kernel(const MsArgs g) {
  __shared__ unsigned char sI[3 * kMsEdge * kMsEdge];
  const int r = g.radius, E = kMsTile + 4 * r, x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile, f = blockIdx.z;
  ms_stage_bytes(g, sI, x0, y0, f);
  __syncthreads();
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    double mu[3], inv[6];
    ms_window<false>(sI, nullptr, E, tx + 2 * r, ty + 2 * r, r, window_extent(gx, r, g.W) * window_extent(gy, r, g.H), g.eps, mu, inv, nullptr);
    double* m = g.mom + (size_t)f * g.H * g.W + (size_t)gy * g.W + gx;
    for (int c = 0; c < 3; ++c) m[c * g.mcap] = mu[c];
    for (int c = 0; c < 6; ++c) m[(3 + c) * g.mcap] = inv[c];
  }
}
#endif

// launch P of iteration g.it.  grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kMsLanes) void ms_product_kernel(const MsArgs g) {
  MS_SHARED;
  __shared__ int idle;
  const int f = blockIdx.z, tile = blockIdx.y * gridDim.x + blockIdx.x;
  if (ms_idle(g, f, tile, &idle)) return;
  const int r = g.radius, E = kMsTile + 4 * r, x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile;
  const size_t plane = (size_t)f * g.H * g.W;
  const double bb = ms_frame_sum(g, kPartBB, f, red), rr = ms_frame_sum(g, kPartRR, f, red);
  if (bb == 0.0) { ms_stop(g, f, 0, 1, 0.0); return; }
  if (rr <= g.tol2 * bb) { ms_stop(g, f, g.it, 0, sqrt(rr / bb)); return; }
  double beta = 0.0;
  if (g.it > 0) beta = ms_frame_sum(g, kPartRZ + (g.it & 1), f, red) / ms_frame_sum(g, kPartRZ + ((g.it - 1) & 1), f, red);
  const double* prev = ((g.it > 0 ? g.it - 1 : 0) & 1) ? g.p1 : g.p0;
  double* cur = (g.it & 1) ? g.p1 : g.p0;
  ms_stage_bytes(g, sI, x0, y0, f);
  for (int i = threadIdx.x; i < E * E; i += kMsLanes) {
    const int ly = i / E, lx = i - ly * E, gx = x0 - 2 * r + lx, gy = y0 - 2 * r + ly;
    double p = 0.0;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) {
      const size_t o = plane + (size_t)gy * g.W + gx;
      const double dv = g.dinv[o];
      if (dv != 0.0) p = g.it > 0 ? dv * g.r[o] + beta * prev[o] : prev[o];     // 0 on every known pixel
    }
    sp[i] = p;
  }
  __syncthreads();
  double lp[kMsPer];
  ms_apply<VP_MS_STORED != 0>(g, sI, sp, sab, x0, y0, lp, plane);
  double pap = 0.0;
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    const size_t o = plane + (size_t)gy * g.W + gx;
    if (g.dinv[o] == 0.0) continue;
    const double p = sp[(ty + 2 * r) * E + tx + 2 * r];
    if (g.it > 0) cur[o] = p;
    g.ap[o] = lp[q];
    pap += p * lp[q];
  }
  pap = ms_tree(pap, red);
  if (threadIdx.x == 0) g.part[kPartPAP * g.pcap + (size_t)f * g.tiles + tile] = pap;
}

// launch U of iteration g.it.  grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kMsLanes) void ms_update_kernel(const MsArgs g) {
  __shared__ double red[kMsLanes];
  __shared__ int idle;
  const int f = blockIdx.z, tile = blockIdx.y * gridDim.x + blockIdx.x;
  if (ms_idle(g, f, tile, &idle)) return;
  const int x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile;
  const size_t plane = (size_t)f * g.H * g.W;
  const double pap = ms_frame_sum(g, kPartPAP, f, red);
  if (!(pap > 0.0) || !(pap <= 1.7976931348623157e308)) {
    const double bb = ms_frame_sum(g, kPartBB, f, red), rr = ms_frame_sum(g, kPartRR, f, red);
    ms_stop(g, f, g.it, 2, sqrt(rr / bb));
    return;
  }
  const double alpha = ms_frame_sum(g, kPartRZ + (g.it & 1), f, red) / pap;
  const double* p = (g.it & 1) ? g.p1 : g.p0;
  double rr = 0.0, rz = 0.0;
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    const size_t o = plane + (size_t)gy * g.W + gx;
    const double dv = g.dinv[o];
    if (dv == 0.0) continue;
    g.x[o] = g.x[o] + alpha * p[o];
    const double rv = g.r[o] - alpha * g.ap[o];
    g.r[o] = rv;
    rr += rv * rv;
    rz += rv * (dv * rv);
  }
  rr = ms_tree(rr, red);
  rz = ms_tree(rz, red);
  if (threadIdx.x == 0) {
    const size_t at = (size_t)f * g.tiles + tile;
    g.part[kPartRR * g.pcap + at] = rr;
    g.part[(kPartRZ + ((g.it + 1) & 1)) * g.pcap + at] = rz;
  }
}

// grid (tiles_x, tiles_y, n): the report of a frame that ran all its iterations (its first tile's workgroup), and the matte
__global__ __launch_bounds__(kMsLanes) void ms_finish_kernel(const MsArgs g) {
  __shared__ double red[kMsLanes];
  const int f = blockIdx.z, x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile;
  const size_t plane = (size_t)f * g.H * g.W;
  __shared__ int stopped;
  if (threadIdx.x == 0) stopped = g.flag[f];                        // (no workgroup writes the flag in this launch)
  __syncthreads();
  if (blockIdx.x == 0 && blockIdx.y == 0 && !stopped) {
    const double bb = ms_frame_sum(g, kPartBB, f, red), rr = ms_frame_sum(g, kPartRR, f, red);
    if (threadIdx.x == 0) {
      int* rep = g.report + f * kMsReport;
      if (bb == 0.0) { rep[1] = 0; rep[2] = 1; *(double*)(rep + 4) = 0.0; }
      else { rep[1] = g.iters; rep[2] = 0; *(double*)(rep + 4) = sqrt(rr / bb); }
    }
  }
  for (int q = 0; q < kMsPer; ++q) {
    int tx, ty;
    ms_pixel(q, &tx, &ty);
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    const size_t o = plane + (size_t)gy * g.W + gx;
    const int t = g.tri[o];
    g.matte[o] = t == 0 || t == 255 ? (unsigned char)t : (unsigned char)(int)floor(fmin(fmax(g.x[o], 0.0), 1.0) * 255.0 + 0.5);
  }
}

struct MsTriArgs {
  const unsigned char* matte;
  unsigned char* out;
  int* active;
  int H, W, support, core, erode, dilate, tiles;
};

// TRIMAP of the header.  grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kMsLanes) void ms_trimap_kernel(const MsTriArgs g) {
  __shared__ unsigned char sm[kMsTriEdge][kMsTriEdge];   // bit 0: m >= core, or outside the image; bit 1: m >= support
  __shared__ unsigned char row[kMsTriEdge][kMsTile];
  __shared__ int count;
  const int x0 = blockIdx.x * kMsTile, y0 = blockIdx.y * kMsTile, f = blockIdx.z;
  const size_t plane = (size_t)f * g.H * g.W;
  const int elo = g.erode / 2, ehi = g.erode - 1 - elo, dlo = g.dilate / 2, dhi = g.dilate - 1 - dlo;   // at most 32 and 31
  if (threadIdx.x == 0) count = 0;
  for (int i = threadIdx.x; i < kMsTriEdge * kMsTriEdge; i += kMsLanes) {
    const int ly = i / kMsTriEdge, lx = i - ly * kMsTriEdge, gx = x0 - kMsHalo + lx, gy = y0 - kMsHalo + ly;
    int v = 1;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) {
      const int m = g.matte[plane + (size_t)gy * g.W + gx];
      v = (m >= g.core ? 1 : 0) | (m >= g.support ? 2 : 0);
    }
    sm[ly][lx] = (unsigned char)v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kMsTriEdge * kMsTile; i += kMsLanes) {
    const int ly = i / kMsTile, tx = i - ly * kMsTile;
    int all = 1, any = 0;
    for (int d = -elo; d <= ehi; ++d) all &= sm[ly][kMsHalo + tx + d];
    for (int d = -dlo; d <= dhi; ++d) any |= sm[ly][kMsHalo + tx + d];
    row[ly][tx] = (unsigned char)((all & 1) | (any & 2));
  }
  __syncthreads();
  int mine = 0;
  for (int q = 0; q < kMsPer; ++q) {
    const int li = threadIdx.x + q * kMsLanes, ty = li >> 5, tx = li & 31, gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    int all = 1, any = 0;
    for (int d = -elo; d <= ehi; ++d) all &= row[kMsHalo + ty + d][tx];
    for (int d = -dlo; d <= dhi; ++d) any |= row[kMsHalo + ty + d][tx];
    const int t = (all & 1) ? 255 : ((any & 2) ? 127 : 0);
    g.out[plane + (size_t)gy * g.W + gx] = (unsigned char)t;
    mine += t == 127;
  }
  if (mine) atomicAdd(&count, mine);
  __syncthreads();
  if (threadIdx.x == 0) g.active[(size_t)f * g.tiles + blockIdx.y * gridDim.x + blockIdx.x] = count > 0;
}

}  // namespace vp

struct vp_mattesolve {
  vp_mattesolve_desc d;
  double *x, *r, *dinv, *p0, *p1, *ap;       // [max_frames][max_height][max_width] each
  double* part;                              // [5][max_frames * max_tiles]
  int *active, *flag, *report;               // [max_frames * max_tiles], [max_frames], [max_frames][8]
  double* mom;                               // VP_MS_STORED builds only: [9][pixels]
  int max_tiles;
  int height, width;                         // of the last solve: the layout of "alpha"
  int tile_height, tile_width;               // of the last trimap or solve: the layout of "tiles"
};

using namespace vp;

static int ms_check(const vp_mattesolve_desc* d, vp_mattesolve* h) {
  if (const int rc = check_desc(d, "vp_mattesolve")) return rc;
  if (const int rc = check_extents_desc("vp_mattesolve", d->max_frames, VP_MATTESOLVE_MAX_FRAMES, d->max_height, d->max_width, 16, VP_MATTESOLVE_MAX_SIZE)) return rc;
  if (const int rc = check_radius_desc("vp_mattesolve", d->max_radius, 1, VP_MATTESOLVE_MAX_RADIUS)) return rc;
  h->d = *d;
  h->max_tiles = ((d->max_height + kMsTile - 1) / kMsTile) * ((d->max_width + kMsTile - 1) / kMsTile);
  h->height = h->tile_height = d->max_height;
  h->width = h->tile_width = d->max_width;
  return VP_OK;
}

static size_t ms_carve(vp_mattesolve* h, void* base) {
  Arena ar(base);
  const size_t pixels = (size_t)h->d.max_frames * h->d.max_height * h->d.max_width, tiles = (size_t)h->d.max_frames * h->max_tiles;
  h->x = ar.take<double>(pixels);
  h->r = ar.take<double>(pixels);
  h->dinv = ar.take<double>(pixels);
  h->p0 = ar.take<double>(pixels);
  h->p1 = ar.take<double>(pixels);
  h->ap = ar.take<double>(pixels);
  h->part = ar.take<double>(kPartCount * tiles);
  h->active = ar.take<int>(tiles);
  h->flag = ar.take<int>(h->d.max_frames);
  h->report = ar.take<int>((size_t)h->d.max_frames * kMsReport);
  h->mom = VP_MS_STORED ? ar.take<double>(9 * pixels) : nullptr;
  return align256(ar.total());
}

static int ms_size(const vp_mattesolve* h, const char* who, int n, int H, int W) {
  return check_batch(who, n, H, W, 16, h->d.max_frames, h->d.max_height, h->d.max_width);
}

// what solve and laplacian share: the handle, the frames and their layout, radius and eps
static int ms_frames(const vp_mattesolve* h, const char* who, const void* frames, size_t pitch, size_t stride, int n, int H, int W, int radius, double eps) {
  if (!h || !frames) { set_err("%s: bad argument (handle, device frames)", who); return VP_ERR_ARG; }
  if (const int rc = ms_size(h, who, n, H, W)) return rc;
  if (const int rc = check_pitch(who, "", pitch, stride, H, (size_t)W * 3)) return rc;
  if (radius < 1 || radius > h->d.max_radius) { set_err("%s: radius %d outside 1 .. max_radius %d", who, radius, h->d.max_radius); return VP_ERR_ARG; }
  if (!(std::isfinite(eps) && eps > 0.0)) { set_err("%s: eps must be finite and positive", who); return VP_ERR_ARG; }
  return VP_OK;
}

static dim3 ms_grid(int n, int H, int W) { return dim3((W + kMsTile - 1) / kMsTile, (H + kMsTile - 1) / kMsTile, n); }   // at most 32 x 32 x 4096

extern "C" {

size_t vp_mattesolve_desc_size(void) { return sizeof(vp_mattesolve_desc); }

size_t vp_mattesolve_workspace_bytes(const vp_mattesolve_desc* d) {
  vp_mattesolve h;
  return ms_check(d, &h) ? 0 : ms_carve(&h, nullptr);
}

int vp_mattesolve_create(const vp_mattesolve_desc* d, void* workspace, size_t bytes, vp_mattesolve_t** out) {
  return open_handle("vp_mattesolve_create", d, ms_check, ms_carve, workspace, bytes, out);
}

void vp_mattesolve_destroy(vp_mattesolve_t* h) { delete h; }

int vp_mattesolve_trimap(vp_mattesolve_t* h, const unsigned char* matte, int n, int height, int width, int support, int core, int erode,
                         int dilate, unsigned char* out, void* stream) {
  const char* who = "vp_mattesolve_trimap";
  if (!h || !matte || !out) { set_err("%s: bad argument (handle, device matte, device out)", who); return VP_ERR_ARG; }
  if (const int rc = ms_size(h, who, n, height, width)) return rc;
  if (support < 1 || support > 255) { set_err("%s: support %d outside 1 .. 255", who, support); return VP_ERR_ARG; }
  if (core < 1 || core > 255) { set_err("%s: core %d outside 1 .. 255", who, core); return VP_ERR_ARG; }
  const int side = height < width ? height : width;
  if (erode == 0) erode = side / 19 < 5 ? 5 : (side / 19 > VP_MATTESOLVE_MAX_SQUARE ? VP_MATTESOLVE_MAX_SQUARE : side / 19);
  if (dilate == 0) dilate = side / 29 < 5 ? 5 : (side / 29 > VP_MATTESOLVE_MAX_SQUARE ? VP_MATTESOLVE_MAX_SQUARE : side / 29);
  if (erode < 1 || erode > VP_MATTESOLVE_MAX_SQUARE) { set_err("%s: erode %d outside 1 .. %d (or 0: the default)", who, erode, VP_MATTESOLVE_MAX_SQUARE); return VP_ERR_ARG; }
  if (dilate < 1 || dilate > VP_MATTESOLVE_MAX_SQUARE) { set_err("%s: dilate %d outside 1 .. %d (or 0: the default)", who, dilate, VP_MATTESOLVE_MAX_SQUARE); return VP_ERR_ARG; }
  if (overlaps(out, matte, (size_t)n * height * width)) {
    set_err("%s: out overlaps the matte (a tile reads its neighbours' pixels)", who);
    return VP_ERR_ARG;
  }
  const dim3 grid = ms_grid(n, height, width);
  h->tile_height = height;
  h->tile_width = width;
  MsTriArgs g;
  memset(&g, 0, sizeof(g));
  g.matte = matte; g.out = out; g.active = h->active; g.H = height; g.W = width; g.support = support; g.core = core; g.erode = erode;
  g.dilate = dilate; g.tiles = grid.x * grid.y;
  hipLaunchKernelGGL(ms_trimap_kernel, grid, dim3(kMsLanes), 0, (hipStream_t)stream, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_mattesolve_solve(vp_mattesolve_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                        const unsigned char* trimap, int radius, double eps, int iters, double tol, unsigned char* matte, void* stream) {
  const char* who = "vp_mattesolve_solve";
  if (const int rc = ms_frames(h, who, frames, row_pitch, frame_stride, n, height, width, radius, eps)) return rc;
  if (!trimap) { set_err("%s: bad argument (device trimap)", who); return VP_ERR_ARG; }
  if (!matte) { set_err("%s: bad argument (device matte)", who); return VP_ERR_ARG; }
  if (iters < 1 || iters > VP_MATTESOLVE_MAX_ITERS) { set_err("%s: iters %d outside 1 .. %d", who, iters, VP_MATTESOLVE_MAX_ITERS); return VP_ERR_ARG; }
  if (!(std::isfinite(tol) && tol >= 0.0)) { set_err("%s: tol must be finite and not negative", who); return VP_ERR_ARG; }
  // in place works because the finish launch reads and writes a pixel's own byte only; at a shifted address it would not
  if (matte != trimap && overlaps(matte, trimap, (size_t)n * height * width)) {
    set_err("%s: matte overlaps the trimap at another address (identical or disjoint buffers only)", who);
    return VP_ERR_ARG;
  }
  const dim3 grid = ms_grid(n, height, width), lanes(kMsLanes);
  h->height = h->tile_height = height;
  h->width = h->tile_width = width;
  hipStream_t st = (hipStream_t)stream;
  VP_HIP_CHECK(hipMemsetAsync(h->flag, 0, (size_t)n * sizeof(int), st));
  VP_HIP_CHECK(hipMemsetAsync(h->report, 0, (size_t)n * kMsReport * sizeof(int), st));
  MsArgs g;
  memset(&g, 0, sizeof(g));
  g.frames = frames; g.pitch = row_pitch; g.stride = frame_stride; g.tri = trimap;
  g.x = h->x; g.r = h->r; g.dinv = h->dinv; g.p0 = h->p0; g.p1 = h->p1; g.ap = h->ap;
  g.part = h->part; g.pcap = (size_t)h->d.max_frames * h->max_tiles; g.active = h->active; g.flag = h->flag; g.report = h->report;
  g.mom = h->mom; g.mcap = (size_t)h->d.max_frames * h->d.max_height * h->d.max_width;
  g.matte = matte; g.eps = eps; g.tol2 = tol * tol; g.H = height; g.W = width; g.radius = radius; g.iters = iters; g.tiles = grid.x * grid.y;
#if VP_MS_STORED
  hipLaunchKernelGGL(ms_moments_kernel, grid, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
#endif
  hipLaunchKernelGGL(ms_init_kernel, grid, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  for (int it = 0; it < iters; ++it) {
    g.it = it;
    hipLaunchKernelGGL(ms_product_kernel, grid, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ms_update_kernel, grid, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
  }
  g.it = iters;
  hipLaunchKernelGGL(ms_finish_kernel, grid, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_mattesolve_laplacian(vp_mattesolve_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                            int radius, double eps, const double* p, double* out, void* stream) {
  const char* who = "vp_mattesolve_laplacian";
  if (const int rc = ms_frames(h, who, frames, row_pitch, frame_stride, n, height, width, radius, eps)) return rc;
  if (!p || !out || ((uintptr_t)p & 7) || ((uintptr_t)out & 7)) { set_err("%s: bad argument (device p, device out, on 8-byte boundaries)", who); return VP_ERR_ARG; }
  if (overlaps(out, p, (size_t)n * height * width * sizeof(double))) {
    set_err("%s: out overlaps p (a tile reads its neighbours' pixels)", who);
    return VP_ERR_ARG;
  }
  MsArgs g;
  memset(&g, 0, sizeof(g));
  g.frames = frames; g.pitch = row_pitch; g.stride = frame_stride; g.pin = p; g.pout = out; g.eps = eps; g.H = height; g.W = width; g.radius = radius;
  hipLaunchKernelGGL(ms_laplacian_kernel, ms_grid(n, height, width), dim3(kMsLanes), 0, (hipStream_t)stream, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_mattesolve_tensor(vp_mattesolve_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_mattesolve_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  int64_t e1 = 1, e2 = 1;
  if (s == "alpha") { *ptr = h->x; e1 = h->height; e2 = h->width; }
  else if (s == "report") { *ptr = h->report; e1 = kMsReport; }
  else if (s == "tiles") { *ptr = h->active; e1 = (h->tile_height + kMsTile - 1) / kMsTile; e2 = (h->tile_width + kMsTile - 1) / kMsTile; }
  else { set_err("vp_mattesolve_tensor: no tensor '%s' (alpha, report, tiles)", name); return VP_ERR_ARG; }
  if (shape) { shape[0] = h->d.max_frames; shape[1] = e1; shape[2] = e2; shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

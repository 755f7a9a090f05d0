// Alpha mattes for clips in front of a plain backdrop (include/vp_hip.h, vp_keymatte_*): a colour model of the backdrop fitted to the
// frames' border, a soft key on the distance from it and one guided-filter pass with the frame's luma as the guide.  The header defines
// every number and the order of every float64 operation; this translation unit is compiled with -ffp-contract=off.
//
// Fit: one fill of the moments and four launches.
//   moments   one workgroup per 16 sample rows and frame.  A lane keeps the 21 integer sums of its samples; wavefront shuffles, one LDS
//             exchange, then 21 lanes add the workgroup's sums with 64-bit integer atomics: exact in any order.
//   solve     one lane: km_solve, the __host__ __device__ function vp_keymatte_solve_host also runs.
//   the same two again, the moments restricted to the samples within `trim` of pass 1's model.
// Apply: radius 0 is one pointwise launch.  Otherwise two launches of one workgroup of 256 lanes per 32 x 32 tile and frame:
//   coeff     reads the tile's frame bytes with a halo of `radius` once, forms the guide I and the raw key p as bytes in LDS (outside the
//             image: 0, which leaves every window sum that of the clipped window), the four integer row sums for (32 + 2 radius) rows x
//             32 columns, then per pixel the column sums, a_k and b_k: two float64 planes in the workspace.
//   mean      per plane: the tile with its halo into LDS (outside the image +0.0: adding it changes no bit of a sum that started from
//             +0.0), row sums in increasing x, column sums in increasing y; then q and the matte byte.
// Foreground (vp_key_foreground): one pointwise launch, the subject's colours from the frame, the matte and the model's planes.
// LDS: coeff 2 x 64 x 64 bytes + 4 x 64 x 32 ints = 40 KiB, mean 64 x 64 + 64 x 32 doubles = 48 KiB: three workgroups per CU of 160 KiB.
// A single launch would hold the bytes of a 96 x 96 footprint, both float64 planes of 64 x 64 and the integer row sums (over 110 KiB at
// radius 16) and would evaluate the key 9 times per pixel there; the planes cost 16 bytes per pixel written and read back instead
// (DESIGN.md 6).  Every read and write is bounded by the call's height and width, which the host has checked against the descriptor,
// the pitch and the stride before anything is enqueued.
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

namespace vp {

constexpr int kKmLanes = 256;
constexpr int kKmTile = 32;                                       // output pixels per tile edge
constexpr int kKmEdge = kKmTile + 2 * VP_KEYMATTE_MAX_RADIUS;     // 64: a tile with its halo
constexpr int kKmModel = VP_KEYMATTE_MODEL_DOUBLES;
constexpr int kKmMoments = 21;

// (double)(n * sab - sa * sb) / nn of SOLVE: the integer exact in 128 bits, converted by its magnitude's two 64-bit halves
__host__ __device__ inline double km_centred(long long n, long long sab, long long sa, long long sb, double nn) {
  const __int128 v = (__int128)n * sab - (__int128)sa * sb;
  const unsigned __int128 u = v < 0 ? (unsigned __int128)(-v) : (unsigned __int128)v;
  const double d = (double)(unsigned long long)(u >> 64) * 18446744073709551616.0 + (double)(unsigned long long)u;
  return (v < 0 ? -d : d) / nn;
}

// SOLVE of the header: S the 21 moments, m the model record
__host__ __device__ inline void km_solve(const long long* S, double sigma_min, double* m) {
  for (int i = 0; i < kKmModel; ++i) m[i] = 0.0;
  const double s2 = sigma_min * sigma_min;
  const long long N = S[20];
  m[16] = 1.0;
  if (N < 1) {
    m[9] = m[12] = m[14] = 1.0 / s2;
    m[18] = 1.0;
    return;
  }
  const double Nd = (double)N;
  const double mx = (double)S[5] / Nd, my = (double)S[10] / Nd;
  const double mc[3] = {(double)S[14] / Nd, (double)S[17] / Nd, (double)S[19] / Nd};
  const double nn = Nd * Nd;
  const double Cxx = km_centred(N, S[0], S[5], S[5], nn), Cxy = km_centred(N, S[1], S[5], S[10], nn), Cyy = km_centred(N, S[6], S[10], S[10], nn);
  const double Cxc[3] = {km_centred(N, S[2], S[5], S[14], nn), km_centred(N, S[3], S[5], S[17], nn), km_centred(N, S[4], S[5], S[19], nn)};
  const double Cyc[3] = {km_centred(N, S[7], S[10], S[14], nn), km_centred(N, S[8], S[10], S[17], nn), km_centred(N, S[9], S[10], S[19], nn)};
  const double C00 = km_centred(N, S[11], S[14], S[14], nn), C01 = km_centred(N, S[12], S[14], S[17], nn), C02 = km_centred(N, S[13], S[14], S[19], nn);
  const double C11 = km_centred(N, S[15], S[17], S[17], nn), C12 = km_centred(N, S[16], S[17], S[19], nn), C22 = km_centred(N, S[18], S[19], S[19], nn);
  const double det = Cxx * Cyy - Cxy * Cxy;
  bool degenerate = N < 16 || !(det > 1e-9 * (Cxx * Cyy));
  double px[3], py[3];
  for (int c = 0; c < 3; ++c) {
    px[c] = degenerate ? 0.0 : (Cxc[c] * Cyy - Cyc[c] * Cxy) / det;
    py[c] = degenerate ? 0.0 : (Cyc[c] * Cxx - Cxc[c] * Cxy) / det;
    m[3 * c + 0] = (mc[c] - px[c] * mx) - py[c] * my;
    m[3 * c + 1] = px[c];
    m[3 * c + 2] = py[c];
  }
  double R00 = (C00 - px[0] * Cxc[0]) - py[0] * Cyc[0], R01 = (C01 - px[0] * Cxc[1]) - py[0] * Cyc[1];
  double R02 = (C02 - px[0] * Cxc[2]) - py[0] * Cyc[2], R11 = (C11 - px[1] * Cxc[1]) - py[1] * Cyc[1];
  double R12 = (C12 - px[1] * Cxc[2]) - py[1] * Cyc[2], R22 = (C22 - px[2] * Cxc[2]) - py[2] * Cyc[2];
  if (R00 < 0.0) R00 = 0.0;
  if (R11 < 0.0) R11 = 0.0;
  if (R22 < 0.0) R22 = 0.0;
  m[17] = sqrt(((R00 + R11) + R22) / 3.0);
  const double a = R00 + s2, b = R01, c = R02, d = R11 + s2, e = R12, f = R22 + s2;
  const double A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d, A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
  const double D = (a * A00 + b * A01) + c * A02;
  if (D > 0.0) {
    m[9] = A00 / D; m[10] = A01 / D; m[11] = A02 / D; m[12] = A11 / D; m[13] = A12 / D; m[14] = A22 / D;
  } else {
    m[9] = m[12] = m[14] = 1.0 / s2;
    m[10] = m[11] = m[13] = 0.0;
    degenerate = true;
  }
  m[15] = Nd;
  m[18] = degenerate ? 1.0 : 0.0;
}

// d2 of APPLY
__device__ __forceinline__ double km_d2(const double* m, int x, int y, int R, int G, int B) {
  const double xd = (double)x, yd = (double)y;
  const double r0 = (double)R - ((m[0] + m[1] * xd) + m[2] * yd);
  const double r1 = (double)G - ((m[3] + m[4] * xd) + m[5] * yd);
  const double r2 = (double)B - ((m[6] + m[7] * xd) + m[8] * yd);
  const double q0 = (m[9] * r0 + m[10] * r1) + m[11] * r2;
  const double q1 = (m[10] * r0 + m[12] * r1) + m[13] * r2;
  const double q2 = (m[11] * r0 + m[13] * r1) + m[14] * r2;
  return (r0 * q0 + r1 * q1) + r2 * q2;
}

// the raw key p; lo2 = lo * lo, den = hi * hi - lo * lo
__device__ __forceinline__ int km_key(double d2, double lo2, double den) {
  const double t = fmin(fmax((d2 - lo2) / den, 0.0), 1.0);      // fmax(NaN, 0) = 0
  const double a = (t * t) * (3.0 - 2.0 * t);
  return (int)floor(255.0 * a + 0.5);
}

__device__ __forceinline__ int km_guide(int R, int G, int B) { return (77 * R + 150 * G + 29 * B + 128) >> 8; }

constexpr int kKmFitRows = 16;               // sample rows per workgroup of the moments kernels

struct KmFitArgs {
  const unsigned char* frames;
  size_t pitch, stride;                      // bytes
  long long* moments;                        // [21], zeroed before the launch
  const double* model;                       // pass 2: pass 1's model
  double trim;
  int H, W, band, side_rows;
};

// grid (ceil(side_rows / 16), n): a workgroup takes 16 sample rows of one frame
template <bool kTrim>
__global__ __launch_bounds__(kKmLanes) void km_moments_kernel(const KmFitArgs g) {
  __shared__ long long part[kKmLanes / 64][kKmMoments];
  const int y0 = blockIdx.x * kKmFitRows, f = blockIdx.y;
  const int rows = min(kKmFitRows, g.side_rows - y0);
  const unsigned char* frame = g.frames + (size_t)f * g.stride;
  long long s[kKmMoments];
#pragma unroll
  for (int i = 0; i < kKmMoments; ++i) s[i] = 0;
  for (int i = threadIdx.x; i < rows * g.W; i += kKmLanes) {
    const int ly = i / g.W, x = i - ly * g.W, y = y0 + ly;
    if (!(y < g.band || x < g.band || x >= g.W - g.band)) continue;
    const unsigned char* px = frame + (size_t)y * g.pitch + 3 * x;
    const int R = px[0], G = px[1], B = px[2];
    if (kTrim && !(km_d2(g.model, x, y, R, G, B) <= g.trim)) continue;
    const int v[6] = {x, y, R, G, B, 1};
    int at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) s[at++] += v[a] * v[b];         // at most 1023 * 1023: an int
  }
  // integers: any order gives the same sums.  Lanes of a wavefront by shuffle, the four wavefronts through LDS, one atomic per moment
#pragma unroll
  for (int i = 0; i < kKmMoments; ++i) {
    long long v = s[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kKmMoments) {
    const long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (v != 0) atomicAdd((unsigned long long*)&g.moments[threadIdx.x], (unsigned long long)v);
  }
}

// first: null, or pass 1's moments (kept = N2 / N1)
__global__ void km_solve_kernel(const long long* moments, const long long* first, double sigma_min, double* model) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double m[kKmModel];
  km_solve(moments, sigma_min, m);
  if (first) m[16] = first[20] > 0 ? (double)moments[20] / (double)first[20] : 0.0;
  for (int i = 0; i < kKmModel; ++i) model[i] = m[i];
}

struct KmApplyArgs {
  const unsigned char* frames;
  size_t pitch, stride;                      // bytes
  const double* model;
  double *ak, *bk;                           // [n][H][W]
  unsigned char *raw, *matte;                // [n][H][W]; raw may be null
  double lo2, den, eps;
  int H, W, radius;
};

// radius 0: grid (ceil(H W / 256), n)
__global__ __launch_bounds__(kKmLanes) void km_key_kernel(const KmApplyArgs g) {
  const int i = blockIdx.x * kKmLanes + threadIdx.x, f = blockIdx.y;
  if (i >= g.H * g.W) return;
  const int y = i / g.W, x = i - y * g.W;
  const unsigned char* px = g.frames + (size_t)f * g.stride + (size_t)y * g.pitch + 3 * x;
  const unsigned char p = (unsigned char)km_key(km_d2(g.model, x, y, px[0], px[1], px[2]), g.lo2, g.den);
  const size_t o = (size_t)f * g.H * g.W + i;
  g.matte[o] = p;
  if (g.raw) g.raw[o] = p;
}

// grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kKmLanes) void km_coeff_kernel(const KmApplyArgs g) {
  __shared__ unsigned char sI[kKmEdge][kKmEdge];
  __shared__ unsigned char sP[kKmEdge][kKmEdge];
  __shared__ int hs[4][kKmEdge][kKmTile];    // row sums of I, p, I^2, I p
  const int tid = threadIdx.x, r = g.radius, E = kKmTile + 2 * r, taps = 2 * r + 1;
  const int x0 = blockIdx.x * kKmTile, y0 = blockIdx.y * kKmTile, f = blockIdx.z;
  const unsigned char* frame = g.frames + (size_t)f * g.stride;
  const size_t plane = (size_t)f * g.H * g.W;
  for (int i = tid; i < E * E; i += kKmLanes) {
    const int ly = i / E, lx = i - ly * E, gx = x0 - r + lx, gy = y0 - r + ly;
    int I = 0, p = 0;
    if (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) {
      const unsigned char* px = frame + (size_t)gy * g.pitch + 3 * gx;
      const int R = px[0], G = px[1], B = px[2];
      I = km_guide(R, G, B);
      p = km_key(km_d2(g.model, gx, gy, R, G, B), g.lo2, g.den);
      if (g.raw && lx >= r && lx < r + kKmTile && ly >= r && ly < r + kKmTile) g.raw[plane + (size_t)gy * g.W + gx] = (unsigned char)p;
    }
    sI[ly][lx] = (unsigned char)I;
    sP[ly][lx] = (unsigned char)p;
  }
  __syncthreads();
  for (int i = tid; i < E * kKmTile; i += kKmLanes) {
    const int ly = i / kKmTile, cx = i - ly * kKmTile;
    int tI = 0, tp = 0, tII = 0, tIp = 0;
    for (int k = 0; k < taps; ++k) {
      const int I = sI[ly][cx + k], p = sP[ly][cx + k];
      tI += I; tp += p; tII += I * I; tIp += I * p;
    }
    hs[0][ly][cx] = tI; hs[1][ly][cx] = tp; hs[2][ly][cx] = tII; hs[3][ly][cx] = tIp;
  }
  __syncthreads();
  for (int i = tid; i < kKmTile * kKmTile; i += kKmLanes) {
    const int ty = i / kKmTile, tx = i - ty * kKmTile, gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    long long sI_ = 0, sp = 0, sII = 0, sIp = 0;                  // at most 33 * 33 * 255 * 255: the products below need 64 bits
    for (int k = 0; k < taps; ++k) { sI_ += hs[0][ty + k][tx]; sp += hs[1][ty + k][tx]; sII += hs[2][ty + k][tx]; sIp += hs[3][ty + k][tx]; }
    const long long nw = (long long)window_extent(gx, r, g.W) * window_extent(gy, r, g.H);
    const double a = (double)(sIp * nw - sI_ * sp) / ((double)(sII * nw - sI_ * sI_) + g.eps * (double)(nw * nw));
    const double b = ((double)sp - a * (double)sI_) / (double)nw;
    g.ak[plane + (size_t)gy * g.W + gx] = a;
    g.bk[plane + (size_t)gy * g.W + gx] = b;
  }
}

// grid (tiles_x, tiles_y, n)
__global__ __launch_bounds__(kKmLanes) void km_mean_kernel(const KmApplyArgs g) {
  __shared__ double pl[kKmEdge][kKmEdge];
  __shared__ double hd[kKmEdge][kKmTile];
  constexpr int kPer = kKmTile * kKmTile / kKmLanes;              // 4 pixels per lane
  const int tid = threadIdx.x, r = g.radius, E = kKmTile + 2 * r, taps = 2 * r + 1;
  const int x0 = blockIdx.x * kKmTile, y0 = blockIdx.y * kKmTile, f = blockIdx.z;
  const size_t plane = (size_t)f * g.H * g.W;
  double acc[2][kPer];
  for (int q = 0; q < 2; ++q) {
    const double* src = (q ? g.bk : g.ak) + plane;
    for (int i = tid; i < E * E; i += kKmLanes) {
      const int ly = i / E, lx = i - ly * E, gx = x0 - r + lx, gy = y0 - r + ly;
      pl[ly][lx] = (gx >= 0 && gx < g.W && gy >= 0 && gy < g.H) ? src[(size_t)gy * g.W + gx] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < E * kKmTile; i += kKmLanes) {
      const int ly = i / kKmTile, cx = i - ly * kKmTile;
      double s = 0.0;
      for (int k = 0; k < taps; ++k) s += pl[ly][cx + k];
      hd[ly][cx] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + j * kKmLanes, ty = i / kKmTile, tx = i - ty * kKmTile;
      double s = 0.0;
      for (int k = 0; k < taps; ++k) s += hd[ty + k][tx];
      acc[q][j] = s;
    }
    __syncthreads();                         // pl and hd are rewritten by the next plane
  }
  const unsigned char* frame = g.frames + (size_t)f * g.stride;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + j * kKmLanes, ty = i / kKmTile, tx = i - ty * kKmTile, gx = x0 + tx, gy = y0 + ty;
    if (gx >= g.W || gy >= g.H) continue;
    const unsigned char* px = frame + (size_t)gy * g.pitch + 3 * gx;
    const double I = (double)km_guide(px[0], px[1], px[2]);
    const double nw = (double)(window_extent(gx, r, g.W) * window_extent(gy, r, g.H));
    const double v = (acc[0][j] / nw) * I + acc[1][j] / nw;
    g.matte[plane + (size_t)gy * g.W + gx] = (unsigned char)(int)floor(fmin(fmax(v, 0.0), 255.0) + 0.5);
  }
}

struct KmForeArgs {
  const unsigned char* frames;
  size_t pitch, stride;                      // bytes
  const double* model;
  const unsigned char* matte;                // [n][H][W]
  unsigned char* out;                        // [n][H][W][3]
  double despill;
  int H, W;
};

__device__ __forceinline__ double km_plane(const double* m, int c, int x, int y) { return (m[3 * c] + m[3 * c + 1] * (double)x) + m[3 * c + 2] * (double)y; }

// FOREGROUND of the header: grid (ceil(H W / 256), n)
__global__ __launch_bounds__(kKmLanes) void km_foreground_kernel(const KmForeArgs g) {
  const int i = blockIdx.x * kKmLanes + threadIdx.x, f = blockIdx.y;
  if (i >= g.H * g.W) return;
  const int y = i / g.W, x = i - y * g.W;
  const size_t o = (size_t)f * g.H * g.W + i;
  const int m = g.matte[o];
  unsigned char* dst = g.out + 3 * o;
  if (m == 0) { dst[0] = dst[1] = dst[2] = 0; return; }
  const unsigned char* px = g.frames + (size_t)f * g.stride + (size_t)y * g.pitch + 3 * x;
  double e[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e[c] = (double)px[c];
    if (m != 255) {
      const double b = km_plane(g.model, c, x, y);
      e[c] = fmin(fmax(b + (e[c] - b) * (255.0 / (double)m), 0.0), 255.0);
    }
  }
  if (g.despill > 0.0) {
    const double v0 = km_plane(g.model, 0, g.W / 2, g.H / 2), v1 = km_plane(g.model, 1, g.W / 2, g.H / 2), v2 = km_plane(g.model, 2, g.W / 2, g.H / 2);
    const int k = v0 >= v1 && v0 >= v2 ? 0 : (v1 >= v2 ? 1 : 2);
    const double vk = k == 0 ? v0 : (k == 1 ? v1 : v2);
    const double lead = vk - (k == 0 ? fmax(v1, v2) : (k == 1 ? fmax(v0, v2) : fmax(v0, v1)));
    if (lead >= 16.0) {
      const double ek = k == 0 ? e[0] : (k == 1 ? e[1] : e[2]);
      const double others = k == 0 ? e[1] + e[2] : (k == 1 ? e[0] + e[2] : e[0] + e[1]);
      const double cut = ek - g.despill * fmax(0.0, ek - others / 2.0);
      if (k == 0) e[0] = cut; else if (k == 1) e[1] = cut; else e[2] = cut;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = (unsigned char)(int)floor(e[c] + 0.5);
}

}  // namespace vp

struct vp_keymatte {
  vp_keymatte_desc d;
  long long* moments;                        // [2][21]
  double* model;                             // [19]
  double *ak, *bk;                           // [max_frames][max_height][max_width] each; null with max_radius 0
};

using namespace vp;

static int km_check(const vp_keymatte_desc* d, vp_keymatte* h) {
  if (const int rc = check_desc(d, "vp_keymatte")) return rc;
  if (const int rc = check_extents_desc("vp_keymatte", d->max_frames, VP_KEYMATTE_MAX_FRAMES, d->max_height, d->max_width, 16, VP_KEYMATTE_MAX_SIZE)) return rc;
  if (const int rc = check_radius_desc("vp_keymatte", d->max_radius, 0, VP_KEYMATTE_MAX_RADIUS)) return rc;
  h->d = *d;
  return VP_OK;
}

static size_t km_carve(vp_keymatte* h, void* base) {
  Arena ar(base);
  const size_t pixels = h->d.max_radius > 0 ? (size_t)h->d.max_frames * h->d.max_height * h->d.max_width : 0;
  h->moments = ar.take<long long>(2 * kKmMoments);
  h->model = ar.take<double>(kKmModel);
  h->ak = pixels ? ar.take<double>(pixels) : nullptr;
  h->bk = pixels ? ar.take<double>(pixels) : nullptr;
  return align256(ar.total());
}

// what fit and apply share: the handle, the frames and their layout
static int km_frames(const vp_keymatte* h, const char* who, const void* frames, size_t pitch, size_t stride, int n, int H, int W) {
  if (!h || !frames) { set_err("%s: bad argument (handle, device frames)", who); return VP_ERR_ARG; }
  if (const int rc = check_batch(who, n, H, W, 16, h->d.max_frames, h->d.max_height, h->d.max_width)) return rc;
  return check_pitch(who, "", pitch, stride, H, (size_t)W * 3);
}

extern "C" {

size_t vp_keymatte_desc_size(void) { return sizeof(vp_keymatte_desc); }

size_t vp_keymatte_workspace_bytes(const vp_keymatte_desc* d) {
  vp_keymatte h;
  return km_check(d, &h) ? 0 : km_carve(&h, nullptr);
}

int vp_keymatte_create(const vp_keymatte_desc* d, void* workspace, size_t bytes, vp_keymatte_t** out) {
  return open_handle("vp_keymatte_create", d, km_check, km_carve, workspace, bytes, out);
}

void vp_keymatte_destroy(vp_keymatte_t* h) { delete h; }

int vp_keymatte_fit(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                    int band, int side_rows, double trim, double sigma_min, void* stream) {
  const char* who = "vp_keymatte_fit";
  if (const int rc = km_frames(h, who, frames, row_pitch, frame_stride, n, height, width)) return rc;
  if (band == 0) band = height / 16 > 2 ? height / 16 : 2;
  if (side_rows == 0) side_rows = height / 2;
  if (band < 1 || 2 * (long long)band > width) { set_err("%s: band %d outside 1 .. width / 2 = %d", who, band, width / 2); return VP_ERR_ARG; }
  if (side_rows < band || side_rows > height) { set_err("%s: side_rows %d outside band %d .. height %d", who, side_rows, band, height); return VP_ERR_ARG; }
  if (!(std::isfinite(trim) && trim >= 0.0)) { set_err("%s: trim must be finite and not negative", who); return VP_ERR_ARG; }
  if (!(std::isfinite(sigma_min) && sigma_min > 0.0)) { set_err("%s: sigma_min must be finite and positive", who); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  VP_HIP_CHECK(hipMemsetAsync(h->moments, 0, 2 * kKmMoments * sizeof(long long), st));
  KmFitArgs g;
  memset(&g, 0, sizeof(g));
  g.frames = frames; g.pitch = row_pitch; g.stride = frame_stride;
  g.moments = h->moments; g.model = h->model; g.trim = trim;
  g.H = height; g.W = width; g.band = band; g.side_rows = side_rows;
  const dim3 grid((side_rows + kKmFitRows - 1) / kKmFitRows, n);  // at most 64 x 4096
  hipLaunchKernelGGL(km_moments_kernel<false>, grid, dim3(kKmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(km_solve_kernel, dim3(1), dim3(64), 0, st, (const long long*)h->moments, (const long long*)nullptr, sigma_min, h->model);
  VP_HIP_CHECK(hipGetLastError());
  g.moments = h->moments + kKmMoments;
  hipLaunchKernelGGL(km_moments_kernel<true>, grid, dim3(kKmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(km_solve_kernel, dim3(1), dim3(64), 0, st, (const long long*)(h->moments + kKmMoments), (const long long*)h->moments, sigma_min,
                     h->model);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_keymatte_apply(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                      double lo, double hi, int radius, double eps, unsigned char* raw, unsigned char* matte, void* stream) {
  const char* who = "vp_keymatte_apply";
  if (const int rc = km_frames(h, who, frames, row_pitch, frame_stride, n, height, width)) return rc;
  if (!matte) { set_err("%s: bad argument (device matte)", who); return VP_ERR_ARG; }
  if (!(std::isfinite(lo) && std::isfinite(hi) && lo >= 0.0 && lo < hi)) { set_err("%s: lo %g and hi %g must be finite with 0 <= lo < hi", who, lo, hi); return VP_ERR_ARG; }
  if (radius < 0 || radius > h->d.max_radius) { set_err("%s: radius %d outside 0 .. max_radius %d", who, radius, h->d.max_radius); return VP_ERR_ARG; }
  if (!(std::isfinite(eps) && eps > 0.0)) { set_err("%s: eps must be finite and positive", who); return VP_ERR_ARG; }
  KmApplyArgs g;
  memset(&g, 0, sizeof(g));
  g.frames = frames; g.pitch = row_pitch; g.stride = frame_stride;
  g.model = h->model; g.ak = h->ak; g.bk = h->bk; g.raw = raw; g.matte = matte;
  g.lo2 = lo * lo; g.den = hi * hi - lo * lo; g.eps = eps;
  g.H = height; g.W = width; g.radius = radius;
  hipStream_t st = (hipStream_t)stream;
  if (radius == 0) {
    hipLaunchKernelGGL(km_key_kernel, dim3((height * width + kKmLanes - 1) / kKmLanes, n), dim3(kKmLanes), 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    return VP_OK;
  }
  const dim3 grid((width + kKmTile - 1) / kKmTile, (height + kKmTile - 1) / kKmTile, n);   // at most 32 x 32 x 4096
  hipLaunchKernelGGL(km_coeff_kernel, grid, dim3(kKmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(km_mean_kernel, grid, dim3(kKmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_key_foreground(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                      const unsigned char* matte, double despill, unsigned char* out, void* stream) {
  const char* who = "vp_key_foreground";
  if (const int rc = km_frames(h, who, frames, row_pitch, frame_stride, n, height, width)) return rc;
  if (!matte) { set_err("%s: bad argument (device matte)", who); return VP_ERR_ARG; }
  if (!out) { set_err("%s: bad argument (device out)", who); return VP_ERR_ARG; }
  if (!(despill >= 0.0 && despill <= 1.0)) { set_err("%s: despill %g outside 0 .. 1", who, despill); return VP_ERR_ARG; }
  KmForeArgs g;
  memset(&g, 0, sizeof(g));
  g.frames = frames; g.pitch = row_pitch; g.stride = frame_stride;
  g.model = h->model; g.matte = matte; g.out = out; g.despill = despill; g.H = height; g.W = width;
  hipLaunchKernelGGL(km_foreground_kernel, dim3((height * width + kKmLanes - 1) / kKmLanes, n), dim3(kKmLanes), 0, (hipStream_t)stream, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_keymatte_get_model(vp_keymatte_t* h, double* model, void* stream) {
  if (!h || !model || ((uintptr_t)model & 7)) { set_err("vp_keymatte_get_model: bad argument (handle, device model on an 8-byte boundary)"); return VP_ERR_ARG; }
  VP_HIP_CHECK(hipMemcpyAsync(model, h->model, kKmModel * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VP_OK;
}

int vp_keymatte_set_model(vp_keymatte_t* h, const double* model, void* stream) {
  if (!h || !model || ((uintptr_t)model & 7)) { set_err("vp_keymatte_set_model: bad argument (handle, device model on an 8-byte boundary)"); return VP_ERR_ARG; }
  VP_HIP_CHECK(hipMemcpyAsync(h->model, model, kKmModel * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VP_OK;
}

int vp_keymatte_tensor(vp_keymatte_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_keymatte_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  int64_t e0 = 1, e1 = 1;
  if (s == "moments") { *ptr = h->moments; e0 = 2; e1 = kKmMoments; }
  else if (s == "model") { *ptr = h->model; e0 = kKmModel; }
  else { set_err("vp_keymatte_tensor: no tensor '%s' (moments, model)", name); return VP_ERR_ARG; }
  if (shape) { shape[0] = e0; shape[1] = e1; shape[2] = shape[3] = 1; }
  return VP_OK;
}

int vp_keymatte_solve_host(const int64_t moments[21], double sigma_min, double* model) {
  if (!moments || !model) { set_err("vp_keymatte_solve_host: bad argument (moments, model)"); return VP_ERR_ARG; }
  if (!(std::isfinite(sigma_min) && sigma_min > 0.0)) { set_err("vp_keymatte_solve_host: sigma_min must be finite and positive"); return VP_ERR_ARG; }
  long long S[kKmMoments];
  for (int i = 0; i < kKmMoments; ++i) S[i] = moments[i];
  km_solve(S, sigma_min, model);
  return VP_OK;
}

}  // extern "C"

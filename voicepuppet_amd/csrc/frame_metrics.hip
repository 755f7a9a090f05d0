// Frame quality metrics on the device (include/vp_hip.h, vp_frame_metrics_*): per frame pair mean |a - b|, mean (a - b)^2, PSNR and SSIM
// (Wang et al. 2004; 11 x 11 Gaussian window of sigma 1.5, the interior windows only, all moments in float64).
//
// Two launches per call.
//   tile      one workgroup of 256 lanes per tile of 16 x 16 windows and frame.  It loads the tile's (up to) 26 x 26 x 3 values of both
//             operands into LDS once, as doubles (rows of 78 consecutive elements: coalesced), and adds |a - b| and (a - b)^2 over the
//             values the tile OWNS: its first 16 columns and rows, and the 10 behind them for the last tile of a row or column (every value
//             of the frame is owned by exactly one tile).  Per channel: a horizontal 11-tap pass gives the five moments (a, b, a^2, b^2,
//             a b) for 26 rows x 16 columns, a vertical pass gives them per window, one lane per window; windows past the ragged right and
//             bottom edge are masked.  A wavefront-shuffle and LDS reduction in a fixed order gives the tile's partial sums: one record of
//             the workspace.
//   finalise  one workgroup per frame: lane l adds the records l, l + 256, ... in index order, a fixed tree adds the lanes, lane 0 writes
//             the four outputs and, for uint8, the two integer sums.
// No atomics, no floating-point order that depends on scheduling.  LDS: 2 x 3 x 26 x 26 + 5 x 26 x 16 doubles = 49 088 bytes: three
// workgroups per CU of 160 KiB.  Reads are bounded by the call's height and width, which the host has checked against the descriptor, the
// pitches and the strides before anything is enqueued.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <string>

#include "frame_args.h"
#include "workspace.h"

namespace vp {

constexpr int kFmTile = 16;                  // windows per tile edge
constexpr int kFmTaps = 11;
constexpr int kFmPix = kFmTile + kFmTaps - 1;   // 26: values per tile edge
constexpr int kFmLanes = kFmTile * kFmTile;  // 256

struct FmPartial {                           // one tile's sums; dabs / dsq for float32 input, iabs / isq for uint8
  double ssim, dabs, dsq;
  long long iabs, isq;
};

struct FmArgs {
  const void* a;
  const void* b;
  size_t a_pitch, a_stride, b_pitch, b_stride;     // bytes
  FmPartial* part;                           // [n][tiles]
  long long* abs_sum;                        // [max_frames]
  long long* sq_sum;
  double* out;                               // [n][4]
  double w[kFmTaps];
  double scale, offset;
  int n, H, W, tiles_x, tiles_y, is_u8;
};

template <typename V>
__device__ __forceinline__ V fm_block_sum(V v, V* scratch) {
  // lanes of a wavefront by shuffle (offsets 32 .. 1), then the four wavefronts in order: the same tree on every run; valid in lane 0
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();                           // scratch may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

__device__ __forceinline__ double fm_value(unsigned char x, double, double) { return (double)x; }
__device__ __forceinline__ double fm_value(float x, double scale, double offset) {
  return fmin(fmax((double)x * scale + offset, 0.0), 255.0);       // fmax(NaN, 0) = 0
}

template <typename T>
__global__ __launch_bounds__(kFmLanes) void frame_metrics_tile_kernel(const FmArgs g) {
  __shared__ double pa[3][kFmPix][kFmPix];
  __shared__ double pb[3][kFmPix][kFmPix];
  __shared__ double hm[5][kFmPix][kFmTile];
  __shared__ double red_d[4];
  __shared__ long long red_i[4];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kFmTile, y0 = blockIdx.y * kFmTile, f = blockIdx.z;
  const int wins_x = min(kFmTile, g.W - (kFmTaps - 1) - x0), wins_y = min(kFmTile, g.H - (kFmTaps - 1) - y0);   // >= 1 by the grid
  const int pix_w = wins_x + kFmTaps - 1, pix_h = wins_y + kFmTaps - 1;                                         // x0 + pix_w <= W
  const int own_w = (int)blockIdx.x == g.tiles_x - 1 ? pix_w : kFmTile, own_h = (int)blockIdx.y == g.tiles_y - 1 ? pix_h : kFmTile;
  const char* fa = (const char*)g.a + (size_t)f * g.a_stride;
  const char* fb = (const char*)g.b + (size_t)f * g.b_stride;

  double dabs = 0.0, dsq = 0.0;
  unsigned iabs = 0, isq = 0;                // at most 26 * 78 / 256 = 8 values per lane: 8 * 65025 fits
  for (int i = tid; i < kFmPix * kFmPix * 3; i += kFmLanes) {
    const int ly = i / (kFmPix * 3), e = i - ly * (kFmPix * 3), lx = e / 3, c = e - lx * 3;
    double va = 0.0, vb = 0.0;
    if (ly < pix_h && lx < pix_w) {
      const size_t col = (size_t)(x0 + lx) * 3 + c;
      const T xa = *(const T*)(fa + (size_t)(y0 + ly) * g.a_pitch + col * sizeof(T));
      const T xb = *(const T*)(fb + (size_t)(y0 + ly) * g.b_pitch + col * sizeof(T));
      va = fm_value(xa, g.scale, g.offset);
      vb = fm_value(xb, g.scale, g.offset);
      if (ly < own_h && lx < own_w) {
        if (sizeof(T) == 1) {
          const int d = (int)xa - (int)xb;
          iabs += (unsigned)abs(d);
          isq += (unsigned)(d * d);
        } else {
          const double d = va - vb;
          dabs += fabs(d);
          dsq += d * d;
        }
      }
    }
    pa[c][ly][lx] = va;
    pb[c][ly][lx] = vb;
  }
  __syncthreads();

  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const int wy = tid / kFmTile, wx = tid - wy * kFmTile;
  double ssim = 0.0;
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < kFmPix * kFmTile; i += kFmLanes) {
      const int r = i / kFmTile, cx = i - r * kFmTile;
      double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
      for (int k = 0; k < kFmTaps; ++k) {
        const double a = pa[c][r][cx + k], b = pb[c][r][cx + k], w = g.w[k];
        const double wa = w * a, wb = w * b;
        sa += wa; sb += wb; saa += wa * a; sbb += wb * b; sab += wa * b;
      }
      hm[0][r][cx] = sa; hm[1][r][cx] = sb; hm[2][r][cx] = saa; hm[3][r][cx] = sbb; hm[4][r][cx] = sab;
    }
    __syncthreads();
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < kFmTaps; ++k) s += g.w[k] * hm[q][wy + k][wx];
      m[q] = s;
    }
    if (wy < wins_y && wx < wins_x) {
      const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
      const double va = m[2] - maa, vb = m[3] - mbb, cov = m[4] - mab;
      ssim += ((2.0 * mab + C1) * (2.0 * cov + C2)) / ((maa + mbb + C1) * (va + vb + C2));
    }
    __syncthreads();                         // hm is rewritten by the next channel
  }

  const double t_ssim = fm_block_sum(ssim, red_d);
  double t_dabs = 0.0, t_dsq = 0.0;
  long long t_iabs = 0, t_isq = 0;
  if (sizeof(T) == 1) {
    t_iabs = fm_block_sum((long long)iabs, red_i);
    t_isq = fm_block_sum((long long)isq, red_i);
  } else {
    t_dabs = fm_block_sum(dabs, red_d);
    t_dsq = fm_block_sum(dsq, red_d);
  }
  if (tid == 0) {
    FmPartial p;
    p.ssim = t_ssim; p.dabs = t_dabs; p.dsq = t_dsq; p.iabs = t_iabs; p.isq = t_isq;
    g.part[(size_t)f * g.tiles_x * g.tiles_y + (size_t)blockIdx.y * g.tiles_x + blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(kFmLanes) void frame_metrics_final_kernel(const FmArgs g) {
  __shared__ double red_d[4];
  __shared__ long long red_i[4];
  const int f = blockIdx.x, tiles = g.tiles_x * g.tiles_y;
  const FmPartial* p = g.part + (size_t)f * tiles;
  double ssim = 0.0, dabs = 0.0, dsq = 0.0;
  long long iabs = 0, isq = 0;
  for (int t = threadIdx.x; t < tiles; t += kFmLanes) {
    ssim += p[t].ssim; dabs += p[t].dabs; dsq += p[t].dsq; iabs += p[t].iabs; isq += p[t].isq;
  }
  ssim = fm_block_sum(ssim, red_d);
  dabs = fm_block_sum(dabs, red_d);
  dsq = fm_block_sum(dsq, red_d);
  iabs = fm_block_sum(iabs, red_i);
  isq = fm_block_sum(isq, red_i);
  if (threadIdx.x == 0) {
    const double count = 3.0 * (double)g.H * (double)g.W;
    const double windows = 3.0 * (double)(g.H - (kFmTaps - 1)) * (double)(g.W - (kFmTaps - 1));
    if (g.is_u8) {
      dabs = (double)iabs; dsq = (double)isq;            // exact: below 2^53
      g.abs_sum[f] = iabs;
      g.sq_sum[f] = isq;
    }
    const double l1 = dabs / count, mse = dsq / count;
    double* o = g.out + (size_t)f * 4;
    o[0] = l1;
    o[1] = mse;
    o[2] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse);
    o[3] = ssim / windows;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
static int fm_tiles(int size) { return (size - (kFmTaps - 1) + kFmTile - 1) / kFmTile; }

}  // namespace vp

struct vp_frame_metrics {
  vp_frame_metrics_desc d;
  vp::FmPartial* part;                       // [max_frames][tiles of the largest frame]
  long long *abs_sum, *sq_sum;
  double w[vp::kFmTaps];
};

using namespace vp;

static int fm_check(const vp_frame_metrics_desc* d, vp_frame_metrics* h) {
  if (const int rc = check_desc(d, "vp_frame_metrics")) return rc;
  if (const int rc = check_extents_desc("vp_frame_metrics", d->max_frames, VP_FRAME_METRICS_MAX_FRAMES, d->max_height, d->max_width, kFmTaps, 8192)) return rc;
  h->d = *d;
  return VP_OK;
}

static size_t fm_carve(vp_frame_metrics* h, void* base) {
  Arena ar(base);
  const size_t frames = h->d.max_frames, tiles_cap = (size_t)fm_tiles(h->d.max_height) * fm_tiles(h->d.max_width);
  h->part = ar.take<FmPartial>(frames * tiles_cap);
  h->abs_sum = ar.take<long long>(frames);
  h->sq_sum = ar.take<long long>(frames);
  return align256(ar.total());
}

static int fm_run(vp_frame_metrics* h, const char* who, int elem, const void* a, size_t a_pitch, size_t a_stride, const void* b, size_t b_pitch,
                  size_t b_stride, int n, int H, int W, double scale, double offset, double* out, void* stream) {
  if (!h || !a || !b || !out) { set_err("%s: bad argument (handle, device operands a and b, device out)", who); return VP_ERR_ARG; }
  if ((uintptr_t)out & 7) { set_err("%s: out must be on an 8-byte boundary", who); return VP_ERR_ARG; }
  if (const int rc = check_batch(who, n, H, W, kFmTaps, h->d.max_frames, h->d.max_height, h->d.max_width)) return rc;
  const size_t row = (size_t)W * 3 * elem;
  const struct { const char *name, *prefix; const void* p; size_t pitch, stride; } ops[2] = {{"a", "a_", a, a_pitch, a_stride}, {"b", "b_", b, b_pitch, b_stride}};
  for (const auto& o : ops) {
    if (const int rc = check_pitch(who, o.prefix, o.pitch, o.stride, H, row)) return rc;
    if (elem == 4 && (((uintptr_t)o.p | o.pitch | o.stride) & 3)) {
      set_err("%s: %s, its row_pitch and its frame_stride must be multiples of 4 bytes", who, o.name);
      return VP_ERR_ARG;
    }
  }
  if ((unsigned long long)fm_tiles(W) * fm_tiles(H) * n > (1ull << 23)) {       // 2^31 lanes in one grid
    set_err("%s: %d frames of %d x %d are more than 2^23 tiles of 16 x 16 windows in one call: split the batch", who, n, H, W);
    return VP_ERR_ARG;
  }
  if (elem == 4 && !(std::isfinite(scale) && std::isfinite(offset))) { set_err("%s: scale and offset must be finite", who); return VP_ERR_ARG; }
  FmArgs g;
  memset(&g, 0, sizeof(g));
  g.a = a; g.b = b; g.a_pitch = a_pitch; g.a_stride = a_stride; g.b_pitch = b_pitch; g.b_stride = b_stride;
  g.part = h->part;
  g.abs_sum = h->abs_sum;
  g.sq_sum = h->sq_sum;
  g.out = out;
  for (int k = 0; k < kFmTaps; ++k) g.w[k] = h->w[k];
  g.scale = scale; g.offset = offset;
  g.n = n; g.H = H; g.W = W; g.tiles_x = fm_tiles(W); g.tiles_y = fm_tiles(H); g.is_u8 = elem == 1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.tiles_x, g.tiles_y, n);   // at most 512 x 512 x 4096
  if (elem == 1) hipLaunchKernelGGL(frame_metrics_tile_kernel<unsigned char>, grid, dim3(kFmLanes), 0, st, g);
  else hipLaunchKernelGGL(frame_metrics_tile_kernel<float>, grid, dim3(kFmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(frame_metrics_final_kernel, dim3(n), dim3(kFmLanes), 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

extern "C" {

size_t vp_frame_metrics_desc_size(void) { return sizeof(vp_frame_metrics_desc); }

size_t vp_frame_metrics_workspace_bytes(const vp_frame_metrics_desc* d) {
  vp_frame_metrics h;
  return fm_check(d, &h) ? 0 : fm_carve(&h, nullptr);
}

int vp_frame_metrics_create(const vp_frame_metrics_desc* d, void* workspace, size_t bytes, vp_frame_metrics_t** out) {
  if (const int rc = open_handle("vp_frame_metrics_create", d, fm_check, fm_carve, workspace, bytes, out)) return rc;
  vp_frame_metrics* h = *out;
  double sum = 0.0;
  for (int i = 0; i < kFmTaps; ++i) { h->w[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += h->w[i]; }
  for (int i = 0; i < kFmTaps; ++i) h->w[i] /= sum;
  return VP_OK;
}

void vp_frame_metrics_destroy(vp_frame_metrics_t* h) { delete h; }

int vp_frame_metrics_u8(vp_frame_metrics_t* h, const unsigned char* a, size_t a_row_pitch, size_t a_frame_stride, const unsigned char* b,
                        size_t b_row_pitch, size_t b_frame_stride, int n, int height, int width, double* out, void* stream) {
  return fm_run(h, "vp_frame_metrics_u8", 1, a, a_row_pitch, a_frame_stride, b, b_row_pitch, b_frame_stride, n, height, width, 1.0, 0.0, out, stream);
}

int vp_frame_metrics_f32(vp_frame_metrics_t* h, const float* a, size_t a_row_pitch, size_t a_frame_stride, const float* b, size_t b_row_pitch,
                         size_t b_frame_stride, int n, int height, int width, double scale, double offset, double* out, void* stream) {
  return fm_run(h, "vp_frame_metrics_f32", 4, a, a_row_pitch, a_frame_stride, b, b_row_pitch, b_frame_stride, n, height, width, scale, offset, out,
                stream);
}

int vp_frame_metrics_tensor(vp_frame_metrics_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_frame_metrics_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  if (s == "abs_sum") *ptr = h->abs_sum;
  else if (s == "sq_sum") *ptr = h->sq_sum;
  else { set_err("vp_frame_metrics_tensor: no tensor '%s' (abs_sum, sq_sum)", name); return VP_ERR_ARG; }
  if (shape) { shape[0] = h->d.max_frames; shape[1] = shape[2] = shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

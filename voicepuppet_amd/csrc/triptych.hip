// PixReferNet training triptychs on the device: [frame | 3-D face on the frame | mask], what step 5 of the reference's data preparation
// writes per frame (datasets/make_data_from_GRID.py:408-471, deep_video_portraits) and, with an alpha matte, step 6's layout (:690-695).
// The inputs are what the rest of this library already produces on the device: the decoded frame, ClipRenderer.render_view's 224 x 224
// render (rasteriser channel order) and its face_mask, and the paste geometry (side, y0, x0) per frame.
//
// Stages, per frame (include/vp_hip.h has the definitions; tests/triptych_ref.py restates them in numpy and is compared byte for byte):
//   a  scipy.ndimage.binary_fill_holes(face_mask > 0)                  (:431-433)  one workgroup per frame, bitmaps in LDS
//   b  cv2.resize of the 0/1 float32 mask to side x side, INTER_LINEAR (:435-436)  float32, no contraction
//   c  cv2.erode with a 5 x 5 kernel                                   (:438-439)
//   d  (uint8)(m * 255), GaussianBlur (21, 21), sigma 4, REFLECT_101   (:441-442)  integer taps, exact
//   e  paste of the mask and of the resized, channel-swapped render    (:444-458)  resize_core.h: the bytes of vp_resize_paste_u8
//   f  the three panels                                                (:460-469)  float32, no contraction, truncated
// Truncation to uint8 is monotone, so the kernels quantise right after the resize and erode the bytes: min and (uint8)(. * 255) commute,
// and the float32 plane between b and c is never stored.
// Geometry: the caller passes (side, y0, x0); the Python layer computes it with infer_bfmvid.paste_geometry, which is step 6's and
// inference's arithmetic (int(), :83-86 of infer_bfmvid.py), NOT step 5's int(round()) of :397-398: training then sees the paste that
// inference produces.
// This file is compiled with -ffp-contract=off (the resize tables are OpenCV's host float / double arithmetic).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "resize_core.h"
#include "vp_common.h"
#include "workspace.h"

namespace vp {

constexpr int kTrTaps = 21, kTrRadius = 10;          // GaussianBlur (21, 21)
constexpr int kFillMax = 256;                        // fill holes: h, w <= 256 (two bitmaps of 256 rows x 8 words in LDS)
constexpr int kFillStride = 9;                       // words per bitmap row in LDS: 8 + 1, so that the row pass (one lane per row) hits 64 banks

struct FTab { int ofs; float c0, c1; };              // float32 bilinear: source index, the two coefficients

// stage b's table: f = (d + 0.5) * (src / dst) - 0.5 in double, s = floor(f), fraction f - s, clamped, cast to float32
static void build_ftab(int ssize, int dsize, FTab* tab) {
  const double scale = (double)ssize / (double)dsize;
  for (int d = 0; d < dsize; ++d) {
    const double f = (d + 0.5) * scale - 0.5;
    int s = (int)floor(f);
    double fr = f - s;
    if (s < 0) { s = 0; fr = 0.0; }
    if (s >= ssize - 1) { s = ssize - 1; fr = 0.0; }
    tab[d].ofs = s;
    tab[d].c0 = (float)(1.0 - fr);
    tab[d].c1 = (float)fr;
  }
}

// stage d's taps: q[k] = round(65536 g[k]), g the normalised exp(-(k - 10)^2 / 32), the centre tap adjusted so that they sum to 65536
static void blur_taps(int* q) {
  double g[kTrTaps], sum = 0.0;
  for (int k = 0; k < kTrTaps; ++k) { g[k] = exp(-(double)((k - kTrRadius) * (k - kTrRadius)) / 32.0); sum += g[k]; }
  int total = 0;
  for (int k = 0; k < kTrTaps; ++k) { q[k] = (int)floor(65536.0 * (g[k] / sum) + 0.5); total += q[k]; }
  q[kTrRadius] += 65536 - total;
}

// 0 built; 1 side < 11 (REFLECT_101 of a 21-tap blur); 2 side > max_side; 3 the paste rectangle is not wholly inside the canvas
__host__ __device__ __forceinline__ int geom_status(int side, int y0, int x0, int S, int max_side) {
  if (side < kTrRadius + 1) return 1;
  if (side > max_side) return 2;
  if (y0 < 0 || x0 < 0 || y0 > S - side || x0 > S - side) return 3;
  return 0;
}

__host__ __device__ __forceinline__ size_t tab_base(int side) { return (size_t)side * (side - 1) / 2; }   // tables of sides 1 .. max_side, back to back

struct TrArgs {
  const unsigned char* frames;     // [T][S][S][3]
  const unsigned char* render;     // [T][face][face][3]
  const unsigned char* mask_in;    // [T][face][face]: stage b's source (the filled mask, or the caller's as it is)
  const unsigned char* alpha;      // [T][S][S] or null
  const int* geom;                 // [T][3] side, y0, x0
  unsigned char* trip;             // [T][S][3S][3]
  int* status;                     // [T]
  const ResizeTab* xt; const ResizeTab* yt; const int* yrow1; const FTab* ft;
  unsigned char* qa;               // [T][ms][ms] quantised resized mask, then the blurred mask
  unsigned char* er;               // [T][ms][ms]
  int* hb;                         // [T][ms][ms] horizontal blur sums
  int q[kTrTaps];
  int T, S, face, ms;
};

struct FillArgs {
  const unsigned char* in;         // [n][h][w]
  unsigned char* out;              // [n][h][w] 0 / 1
  const int* geom;                 // null, or frames with a nonzero status are skipped
  int h, w, S, ms;
};

// Stage a.  free = zero pixels, outside = free pixels joined to the border by a 4-connected path of free pixels.  A round is a row pass
// (one lane per row: every run of free pixels that holds an outside pixel becomes outside, by the carry of an addition, word to word in
// both directions) and a column pass (one lane per 32 columns: a sweep down and a sweep up); rounds repeat until one changes nothing.
__global__ __launch_bounds__(256) void triptych_fill_holes_kernel(const FillArgs a) {
  __shared__ uint32_t s_free[kFillMax * kFillStride], s_out[kFillMax * kFillStride];
  __shared__ int s_changed;
  const int t = blockIdx.x, tid = threadIdx.x, h = a.h, w = a.w;
  if (a.geom && geom_status(a.geom[3 * t], a.geom[3 * t + 1], a.geom[3 * t + 2], a.S, a.ms)) return;    // (the whole workgroup)
  const int nw = (w + 31) >> 5;
  const unsigned char* in = a.in + (size_t)t * h * w;
  // four rows per wave and step: sixteen coalesced 64-pixel loads in flight, then the 64 "is zero" bits of each by ballot (the loop is
  // uniform within a wave)
  const int lane = tid & 63;
  for (int r0 = (tid >> 6) * 4; r0 < h; r0 += 16) {
    unsigned char v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int r = r0 + i, x = c * 64 + lane;
        v[i][c] = (r < h && x < w) ? in[(size_t)r * w + x] : (unsigned char)1;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long bits = __ballot(v[i][c] == 0);
        const int r = r0 + i;
        if (lane == 0 && r < h && 2 * c < nw) {
          s_free[r * kFillStride + 2 * c] = (uint32_t)bits;
          if (2 * c + 1 < nw) s_free[r * kFillStride + 2 * c + 1] = (uint32_t)(bits >> 32);
        }
      }
  }
  __syncthreads();
  for (int i = tid; i < h * nw; i += 256) {
    const int r = i / nw, k = i - r * nw;
    uint32_t border = (r == 0 || r == h - 1) ? 0xffffffffu : 0u;
    if (k == 0) border |= 1u;
    if (k == ((w - 1) >> 5)) border |= 1u << ((w - 1) & 31);
    s_out[r * kFillStride + k] = s_free[r * kFillStride + k] & border;
  }
  for (;;) {
    __syncthreads();
    if (tid == 0) s_changed = 0;
    __syncthreads();
    bool ch = false;
    // (both passes read their words into registers first and store afterwards, so that the LDS reads of a chain do not wait for its stores)
    if (tid < h) {
      uint32_t* o = s_out + tid * kFillStride;
      const uint32_t* f = s_free + tid * kFillStride;
      uint32_t fw[8], ow[8], nv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { fw[k] = k < nw ? f[k] : 0u; ow[k] = k < nw ? o[k] : 0u; }      // (words past the row: not free, no carry)
      uint32_t carry = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {                             // towards larger x
        const uint32_t s = ow[k] | (carry & fw[k]);
        nv[k] = s | (((fw[k] + s) ^ fw[k]) & fw[k]);
        carry = nv[k] >> 31;
      }
      carry = 0;
#pragma unroll
      for (int k = 7; k >= 0; --k) {                            // towards smaller x: the same on the reversed words
        const uint32_t fk = __brev(fw[k]), s = __brev(nv[k]) | (carry & fk);
        const uint32_t nr = s | (((fk + s) ^ fk) & fk);
        carry = nr >> 31;
        nv[k] = __brev(nr);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < nw && nv[k] != ow[k]) { o[k] = nv[k]; ch = true; }
    }
    __syncthreads();
    if (tid < nw) {
      uint32_t cur = 0;
      for (int r0 = 0; r0 < h; r0 += 16) {                      // down
        uint32_t fw[16], ow[16], nv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int r = r0 + j;
          fw[j] = r < h ? s_free[r * kFillStride + tid] : 0u;
          ow[j] = r < h ? s_out[r * kFillStride + tid] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) { nv[j] = ow[j] | (cur & fw[j]); cur = nv[j]; }
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (r0 + j < h && nv[j] != ow[j]) { s_out[(r0 + j) * kFillStride + tid] = nv[j]; ch = true; }
      }
      cur = 0;
      for (int r0 = h - 1; r0 >= 0; r0 -= 16) {                 // up
        uint32_t fw[16], ow[16], nv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int r = r0 - j;
          fw[j] = r >= 0 ? s_free[r * kFillStride + tid] : 0u;
          ow[j] = r >= 0 ? s_out[r * kFillStride + tid] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) { nv[j] = ow[j] | (cur & fw[j]); cur = nv[j]; }
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (r0 - j >= 0 && nv[j] != ow[j]) { s_out[(r0 - j) * kFillStride + tid] = nv[j]; ch = true; }
      }
    }
    if (ch) s_changed = 1;
    __syncthreads();
    if (!s_changed) break;
  }
  unsigned char* out = a.out + (size_t)t * h * w;
  for (int i = tid; i < h * w; i += 256) {
    const int r = i / w, x = i - r * w;
    out[i] = ((s_out[r * kFillStride + (x >> 5)] >> (x & 31)) & 1u) ? 0 : 1;
  }
}

// the frame of blockIdx.y: false when its status is nonzero (nothing of it is read or written)
__device__ __forceinline__ bool frame_geom(const TrArgs& a, int t, int* side, int* y0, int* x0) {
  *side = a.geom[3 * t]; *y0 = a.geom[3 * t + 1]; *x0 = a.geom[3 * t + 2];
  return geom_status(*side, *y0, *x0, a.S, a.ms) == 0;
}

// Stage b and the quantisation of stage d: horizontal pass, then vertical pass, each v0 * c0 + v1 * c1 in float32
__global__ __launch_bounds__(256) void triptych_resize_mask_kernel(const TrArgs a) {
  const int t = blockIdx.y;
  int side, y0, x0;
  if (!frame_geom(a, t, &side, &y0, &x0)) return;
  const FTab* ft = a.ft + tab_base(side);
  const unsigned char* m = a.mask_in + (size_t)t * a.face * a.face;
  unsigned char* q = a.qa + (size_t)t * a.ms * a.ms;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < side * side; i += gridDim.x * 256) {
    const int dy = i / side, dx = i - dy * side;
    const FTab tx = ft[dx], ty = ft[dy];
    const int sx1 = min(tx.ofs + 1, a.face - 1), sy1 = min(ty.ofs + 1, a.face - 1);
    const unsigned char* r0 = m + (size_t)ty.ofs * a.face;
    const unsigned char* r1 = m + (size_t)sy1 * a.face;
    const float h0 = __fadd_rn(__fmul_rn(r0[tx.ofs] ? 1.f : 0.f, tx.c0), __fmul_rn(r0[sx1] ? 1.f : 0.f, tx.c1));
    const float h1 = __fadd_rn(__fmul_rn(r1[tx.ofs] ? 1.f : 0.f, tx.c0), __fmul_rn(r1[sx1] ? 1.f : 0.f, tx.c1));
    const float v = __fadd_rn(__fmul_rn(h0, ty.c0), __fmul_rn(h1, ty.c1));
    q[(size_t)dy * a.ms + dx] = (unsigned char)(int)__fmul_rn(v, 255.f);
  }
}

// Stage c on the bytes: 5 x 5 minimum, anchor at the centre, pixels outside the image take no part
__global__ __launch_bounds__(256) void triptych_erode_kernel(const TrArgs a) {
  const int t = blockIdx.y;
  int side, y0, x0;
  if (!frame_geom(a, t, &side, &y0, &x0)) return;
  const unsigned char* q = a.qa + (size_t)t * a.ms * a.ms;
  unsigned char* e = a.er + (size_t)t * a.ms * a.ms;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < side * side; i += gridDim.x * 256) {
    const int dy = i / side, dx = i - dy * side;
    int v = 255;
    for (int y = max(dy - 2, 0); y <= min(dy + 2, side - 1); ++y)
      for (int x = max(dx - 2, 0); x <= min(dx + 2, side - 1); ++x) v = min(v, (int)q[(size_t)y * a.ms + x]);
    e[(size_t)dy * a.ms + dx] = (unsigned char)v;
  }
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }     // n >= 11, |overhang| <= 10

__global__ __launch_bounds__(256) void triptych_hblur_kernel(const TrArgs a) {
  const int t = blockIdx.y;
  int side, y0, x0;
  if (!frame_geom(a, t, &side, &y0, &x0)) return;
  const unsigned char* e = a.er + (size_t)t * a.ms * a.ms;
  int* hb = a.hb + (size_t)t * a.ms * a.ms;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < side * side; i += gridDim.x * 256) {
    const int dy = i / side, dx = i - dy * side;
    int s = 0;                                                   // <= 255 * 65536
#pragma unroll
    for (int k = 0; k < kTrTaps; ++k) s += a.q[k] * (int)e[(size_t)dy * a.ms + reflect101(dx + k - kTrRadius, side)];
    hb[(size_t)dy * a.ms + dx] = s;
  }
}

__global__ __launch_bounds__(256) void triptych_vblur_kernel(const TrArgs a) {
  const int t = blockIdx.y;
  int side, y0, x0;
  if (!frame_geom(a, t, &side, &y0, &x0)) return;
  const int* hb = a.hb + (size_t)t * a.ms * a.ms;
  unsigned char* u = a.qa + (size_t)t * a.ms * a.ms;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < side * side; i += gridDim.x * 256) {
    const int dy = i / side, dx = i - dy * side;
    long long s = 0;                                             // <= 255 * 2^32
#pragma unroll
    for (int k = 0; k < kTrTaps; ++k) s += (long long)a.q[k] * hb[(size_t)reflect101(dy + k - kTrRadius, side) * a.ms + dx];
    u[(size_t)dy * a.ms + dx] = (unsigned char)((s + (1ll << 31)) >> 32);
  }
}

// Stages e-g: one lane per canvas pixel writes its three panel pixels; the status of every frame of the call is written here
__global__ __launch_bounds__(256) void triptych_compose_kernel(const TrArgs a) {
  const int t = blockIdx.y;
  int side, y0, x0;
  const bool ok = frame_geom(a, t, &side, &y0, &x0);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.status[t] = geom_status(side, y0, x0, a.S, a.ms);
  if (!ok) return;
  const int S = a.S, mode = resize_mode(a.face, a.face, side, side);
  const size_t tb = tab_base(side);
  const unsigned char* frame = a.frames + (size_t)t * S * S * 3;
  const unsigned char* ren = a.render + (size_t)t * a.face * a.face * 3;
  const unsigned char* u = a.qa + (size_t)t * a.ms * a.ms;
  unsigned char* trip = a.trip + (size_t)t * S * S * 9;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < S * S; i += gridDim.x * 256) {
    const int y = i / S, x = i - y * S;
    const int dy = y - y0, dx = x - x0;
    const bool inside = dy >= 0 && dy < side && dx >= 0 && dx < side;
    unsigned char* o = trip + ((size_t)y * 3 * S + x) * 3;
    const unsigned char* f = frame + (size_t)i * 3;
    int face[3] = {0, 0, 0};
    if (inside) {
#pragma unroll
      for (int c = 0; c < 3; ++c) face[c] = resize_px(ren, a.face, mode, a.xt + tb, a.yt + tb, a.yrow1 + tb, dy, dx, 2 - c);
    }
    if (a.alpha) {                                               // step 6: the pasted render on black, the matte
      const unsigned char al = a.alpha[(size_t)t * S * S + i];
#pragma unroll
      for (int c = 0; c < 3; ++c) { o[c] = f[c]; o[3 * S + c] = (unsigned char)face[c]; o[6 * S + c] = al; }
      continue;
    }
    const float m = inside ? __fdiv_rn((float)u[(size_t)dy * a.ms + dx], 255.f) : 0.f;
    const float keep = __fsub_rn(1.f, m), on = m > 0.f ? 1.f : 0.f;
    const unsigned char p3 = (unsigned char)(int)__fmul_rn(m, 255.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = __fmul_rn(__fadd_rn(__fmul_rn((float)f[c], keep), __fmul_rn((float)face[c], m)), on);
      o[c] = f[c]; o[3 * S + c] = (unsigned char)(int)r; o[6 * S + c] = p3;
    }
  }
}

}  // namespace vp

struct vp_triptych {
  vp_triptych_desc d;
  size_t entries;                            // of the tables: side s at entry s (s - 1) / 2, sides 1 .. max_side
  vp::ResizeTab *xt, *yt;
  int* yrow1;
  vp::FTab* ft;
  unsigned char *filled, *qa, *er;
  int* hb;
  int q[vp::kTrTaps];
};

using namespace vp;

static int tr_check(const vp_triptych_desc* d, vp_triptych* h) {
  if (const int rc = check_desc(d, "vp_triptych")) return rc;
  if (d->max_frames < 1 || d->max_frames > VP_TRIPTYCH_MAX_FRAMES) {
    set_err("vp_triptych: bad descriptor (max_frames %d, 1 .. %d)", d->max_frames, VP_TRIPTYCH_MAX_FRAMES);
    return VP_ERR_ARG;
  }
  if (d->size < kTrRadius + 1 || d->size > VP_TRIPTYCH_MAX_SIZE) {
    set_err("vp_triptych: bad descriptor (size %d, %d .. %d)", d->size, kTrRadius + 1, VP_TRIPTYCH_MAX_SIZE);
    return VP_ERR_ARG;
  }
  if (d->face_size < 2 || d->face_size > kFillMax) { set_err("vp_triptych: bad descriptor (face_size %d, 2 .. %d)", d->face_size, kFillMax); return VP_ERR_ARG; }
  if (d->max_side < kTrRadius + 1 || d->max_side > d->size) {
    set_err("vp_triptych: bad descriptor (max_side %d, %d .. size %d)", d->max_side, kTrRadius + 1, d->size);
    return VP_ERR_ARG;
  }
  h->d = *d;
  h->entries = (size_t)d->max_side * (d->max_side + 1) / 2;
  return VP_OK;
}

static size_t tr_carve(vp_triptych* h, void* base) {
  Arena ar(base);
  const vp_triptych_desc& d = h->d;
  const size_t n = h->entries, plane = (size_t)d.max_frames * d.max_side * d.max_side;
  h->xt = ar.take<ResizeTab>(n);
  h->yt = ar.take<ResizeTab>(n);
  h->yrow1 = ar.take<int>(n);
  h->ft = ar.take<FTab>(n);
  h->filled = ar.take<unsigned char>((size_t)d.max_frames * d.face_size * d.face_size);
  h->qa = ar.take<unsigned char>(plane);
  h->er = ar.take<unsigned char>(plane);
  h->hb = ar.take<int>(plane);
  return align256(ar.total());
}

static int launch_fill(const unsigned char* in, unsigned char* out, int n, int h, int w, const int* geom, int S, int ms, hipStream_t st) {
  FillArgs f;
  f.in = in; f.out = out; f.geom = geom; f.h = h; f.w = w; f.S = S; f.ms = ms;
  hipLaunchKernelGGL(triptych_fill_holes_kernel, dim3(n), dim3(256), 0, st, f);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

static void tr_args(const vp_triptych* h, TrArgs* a) {
  memset(a, 0, sizeof(*a));
  a->xt = h->xt; a->yt = h->yt; a->yrow1 = h->yrow1; a->ft = h->ft;
  a->qa = h->qa; a->er = h->er; a->hb = h->hb;
  for (int k = 0; k < kTrTaps; ++k) a->q[k] = h->q[k];
  a->S = h->d.size; a->face = h->d.face_size; a->ms = h->d.max_side;
}

// stages a (optional) to d of n frames into the "mask" planes
static int run_mask(vp_triptych* h, TrArgs& a, const unsigned char* face_mask, int fill, hipStream_t st) {
  const vp_triptych_desc& d = h->d;
  a.mask_in = face_mask;
  if (fill) {
    const int rc = launch_fill(face_mask, h->filled, a.T, d.face_size, d.face_size, a.geom, d.size, d.max_side, st);
    if (rc) return rc;
    a.mask_in = h->filled;
  }
  const int bx = std::min(((int)d.max_side * d.max_side + 255) / 256, 256);
  const dim3 grid(bx, a.T);
  hipLaunchKernelGGL(triptych_resize_mask_kernel, grid, dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(triptych_erode_kernel, grid, dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(triptych_hblur_kernel, grid, dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(triptych_vblur_kernel, grid, dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

extern "C" {

size_t vp_triptych_desc_size(void) { return sizeof(vp_triptych_desc); }

size_t vp_triptych_workspace_bytes(const vp_triptych_desc* d) {
  vp_triptych h;
  return tr_check(d, &h) ? 0 : tr_carve(&h, nullptr);
}

int vp_triptych_blur_taps(int q[21]) {
  if (!q) { set_err("vp_triptych_blur_taps: bad argument"); return VP_ERR_ARG; }
  blur_taps(q);
  return VP_OK;
}

int vp_triptych_create(const vp_triptych_desc* d, void* workspace, size_t bytes, void* stream, vp_triptych_t** out) {
  if (const int rc = open_handle("vp_triptych_create", d, tr_check, tr_carve, workspace, bytes, out)) return rc;
  vp_triptych* h = *out;
  blur_taps(h->q);
  // every frame has its own side: the tables of all sides 1 .. max_side are built here, once, side s at entry s (s - 1) / 2
  std::vector<ResizeTab> xt(h->entries), yt(h->entries);
  std::vector<int> r1(h->entries);
  std::vector<FTab> ft(h->entries);
  for (int s = 1; s <= d->max_side; ++s) {
    const size_t b = tab_base(s);
    build_table(d->face_size, s, xt.data() + b);
    build_row_table(d->face_size, s, yt.data() + b, r1.data() + b);
    build_ftab(d->face_size, s, ft.data() + b);
  }
  hipStream_t st = (hipStream_t)stream;
  // create is not a build: it may wait (pageable sources), once per builder
  hipError_t e = hipMemcpyAsync(h->xt, xt.data(), xt.size() * sizeof(ResizeTab), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->yt, yt.data(), yt.size() * sizeof(ResizeTab), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->yrow1, r1.data(), r1.size() * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->ft, ft.data(), ft.size() * sizeof(FTab), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_err("vp_triptych_create: table upload -> %s", hipGetErrorString(e)); delete h; *out = nullptr; return VP_ERR_HIP; }
  return VP_OK;
}

void vp_triptych_destroy(vp_triptych_t* h) { delete h; }

int vp_triptych_fill_holes(const unsigned char* masks, int n, int height, int width, unsigned char* out, void* stream) {
  if (!masks || !out) { set_err("vp_triptych_fill_holes: bad argument (device masks and out)"); return VP_ERR_ARG; }
  if (n < 1 || n > VP_TRIPTYCH_MAX_FRAMES) { set_err("vp_triptych_fill_holes: n %d outside 1 .. %d", n, VP_TRIPTYCH_MAX_FRAMES); return VP_ERR_ARG; }
  if (height < 1 || height > kFillMax) { set_err("vp_triptych_fill_holes: height %d outside 1 .. %d", height, kFillMax); return VP_ERR_ARG; }
  if (width < 1 || width > kFillMax) { set_err("vp_triptych_fill_holes: width %d outside 1 .. %d", width, kFillMax); return VP_ERR_ARG; }
  return launch_fill(masks, out, n, height, width, nullptr, 0, 0, (hipStream_t)stream);
}

int vp_triptych_mask(vp_triptych_t* h, const unsigned char* face_mask, const int* geometry, int n, int fill, void* stream) {
  if (!h || !face_mask || !geometry) { set_err("vp_triptych_mask: bad argument (handle, device face_mask and geometry)"); return VP_ERR_ARG; }
  if (n < 1 || n > h->d.max_frames) { set_err("vp_triptych_mask: n %d outside 1 .. max_frames %d", n, h->d.max_frames); return VP_ERR_ARG; }
  if ((uintptr_t)geometry & 3) { set_err("vp_triptych_mask: geometry must be on a 4-byte boundary"); return VP_ERR_ARG; }
  TrArgs a;
  tr_args(h, &a);
  a.geom = geometry; a.T = n;
  return run_mask(h, a, face_mask, fill, (hipStream_t)stream);
}

int vp_triptych_build(vp_triptych_t* h, const unsigned char* frames, const unsigned char* render, const unsigned char* face_mask, const int* geometry,
                      const unsigned char* alpha, int n, unsigned char* triptych, int* status, void* stream) {
  if (!h || !frames || !render || !geometry || !triptych || !status) {
    set_err("vp_triptych_build: bad argument (handle, device frames, render, geometry, triptych and status)");
    return VP_ERR_ARG;
  }
  if (!alpha && !face_mask) { set_err("vp_triptych_build: one of face_mask and alpha is needed"); return VP_ERR_ARG; }
  if (n < 1 || n > h->d.max_frames) { set_err("vp_triptych_build: n %d outside 1 .. max_frames %d", n, h->d.max_frames); return VP_ERR_ARG; }
  if (((uintptr_t)geometry | (uintptr_t)status) & 3) { set_err("vp_triptych_build: geometry and status must be on 4-byte boundaries"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  TrArgs a;
  tr_args(h, &a);
  a.frames = frames; a.render = render; a.alpha = alpha; a.geom = geometry; a.trip = triptych; a.status = status; a.T = n;
  if (!alpha) {
    const int rc = run_mask(h, a, face_mask, 1, st);
    if (rc) return rc;
  }
  const int bx = std::min((h->d.size * h->d.size + 255) / 256, 256);
  hipLaunchKernelGGL(triptych_compose_kernel, dim3(bx, n), dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_triptych_tensor(vp_triptych_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_triptych_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  int64_t side;
  if (s == "mask") { *ptr = h->qa; side = h->d.max_side; }
  else if (s == "filled") { *ptr = h->filled; side = h->d.face_size; }
  else { set_err("vp_triptych_tensor: no tensor '%s' (mask, filled)", name); return VP_ERR_ARG; }
  if (shape) { shape[0] = h->d.max_frames; shape[1] = shape[2] = side; shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

// Clean-up of alpha mattes (include/vp_hip.h, vp_matteclean_*): connected components of the matte's support, of which the ones that are
// large enough and leave through the bottom edge or hold an anchor are kept with their soft fringe, and enclosed holes of the core,
// which are filled.  Integers only; the header defines every number.
//
// Labelling is union-find with the smaller index as the root (matte_clean_core.h), the same three templated kernels for both passes
// (8-connected m >= support; 4-connected m1 < core):
//   local    one workgroup of 256 lanes per 32 x 32 tile: parents in LDS, joins with those neighbours before a pixel in raster order
//            that mc_pick names (the tile's view), the tile's roots as frame indices into the global parent array, and per tile root
//            its pixel count and edge flags (LDS atomics).
//   merge    the pixels on a tile's border join with the neighbours mc_pick names in the frame's view that lie in other tiles: integer
//            atomicMin on the global parents.
//   gather   every pixel's parent becomes its root; every tile root adds its count and flags to its component's root (integer
//            atomicAdd / atomicOr); anchors mark their component.
// Then per pass one decide launch over the roots and the apply: for the components the dilation by `grow` as a row pass and a column
// pass, for the holes one fill.  Twelve launches and one fill of the report with the hole pass, seven without; no launch waits on
// another workgroup: every loop is a lock-free retry with a step cap (status bit 2 when a cap is reached, which a correct run cannot).
//
// Per-root records: two pixels side by side that are both in the set belong to one component, so a pair (2 j, 2 j + 1) of a row holds at
// most one root of either connectivity and the record of a root is the word of its pair: 2 bytes per pixel.  Workspace per pixel: labels
// 4, the hole pass's parents 4 (its first byte plane doubles as the dilation's bit plane, which is dead by then), records 2, and the
// report's 32 bytes per frame.  The intermediate matte m1 lives in the caller's `out`.  Every index is bounded by the call's height and
// width, checked against the descriptor before anything is enqueued; pixel indices are per frame (< 2^20), frame offsets size_t.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "frame_args.h"
#include "matte_clean_core.h"
#include "workspace.h"

namespace vp {

constexpr int kMcLanes = 256;
constexpr int kMcTile = 32;
constexpr int kMcTilePixels = kMcTile * kMcTile;
constexpr int kMcArea = (1 << 21) - 1;       // a record's pixel count: at most 2^20
constexpr int kMcBottom = 1 << 24, kMcEdge = 1 << 25, kMcAnchored = 1 << 26, kMcChosen = 1 << 27;   // chosen: kept (components), filled (holes)
constexpr int kMcFlags = kMcBottom | kMcEdge | kMcAnchored;
constexpr int kMcReport = VP_MATTECLEAN_REPORT_INTS;

struct McArgs {
  const unsigned char* src;                  // [n][H][W]: the matte (components), m1 (holes)
  unsigned char* out;                        // [n][H][W]
  int* parent;                               // [n][H][W]
  int* info;                                 // [n][H][(W + 1) / 2]
  unsigned char* plane;                      // [n][H][W]: bit 0 kept, bit 1 kept within `grow` along the row
  int* report;                               // [n][8]
  const int* anchors;                        // [n][k][2]
  int H, W, thresh, support, limit, keep_all, grow, k;   // limit: min_area (components), max_hole (holes)
};

template <bool kHole>
__device__ __forceinline__ bool mc_in_set(int v, int thresh) { return kHole ? v < thresh : v >= thresh; }

__device__ __forceinline__ int mc_slot(int i, int W) {
  const int y = i / W, x = i - y * W;
  return y * ((W + 1) >> 1) + (x >> 1);
}

// the pixel of pair `slot` that can be a root: the left one when it is in the set, else the right one; -1 when neither is
__device__ __forceinline__ int mc_pair_pixel(const int* parent, int slot, int W) {
  const int wh = (W + 1) >> 1, y = slot / wh, x = 2 * (slot - y * wh), i = y * W + x;
  if (mc_load(parent + i) >= 0) return i;
  return x + 1 < W && mc_load(parent + i + 1) >= 0 ? i + 1 : -1;
}

// the components pass keeps everything when its rule kept nothing (report: 0 components, 1 kept, written by decide)
__device__ __forceinline__ bool mc_fallback(const McArgs& g, int f) {
  return !g.keep_all && g.report[f * kMcReport + 1] == 0 && g.report[f * kMcReport + 0] > 0;
}

// grid (tiles_x, tiles_y, n)
template <bool kHole>
__global__ __launch_bounds__(kMcLanes) void mc_local_kernel(const McArgs g) {
  __shared__ int lp[kMcTilePixels];
  __shared__ int la[kMcTilePixels];
  constexpr int kPer = kMcTilePixels / kMcLanes;
  const int tid = threadIdx.x, x0 = blockIdx.x * kMcTile, y0 = blockIdx.y * kMcTile, f = blockIdx.z;
  const int cap = g.H * g.W;
  const size_t base = (size_t)f * g.H * g.W;
  int hit = 0;
  bool in[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int li = tid + j * kMcLanes, gx = x0 + (li & 31), gy = y0 + (li >> 5);
    in[j] = gx < g.W && gy < g.H && mc_in_set<kHole>(g.src[base + (size_t)gy * g.W + gx], g.thresh);
    lp[li] = in[j] ? li : -1;
    la[li] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!in[j]) continue;
    const int li = tid + j * kMcLanes, lx = li & 31, ly = li >> 5;
    bool nin[4], pick[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nx = lx + mc_back_neighbour(q).dx, ny = ly + mc_back_neighbour(q).dy;
      nin[q] = nx >= 0 && nx < kMcTile && ny >= 0 && mc_load(lp + ny * kMcTile + nx) >= 0;       // the tile's view
    }
    mc_pick(!kHole, nin, pick);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (pick[q]) mc_union(lp, li, (ly + mc_back_neighbour(q).dy) * kMcTile + lx + mc_back_neighbour(q).dx, cap, &hit);
  }
  __syncthreads();
  int root[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) root[j] = in[j] ? mc_find(lp, tid + j * kMcLanes, cap, &hit) : -1;
  __syncthreads();                           // nothing joins any more: the roots are final, every lane has read its own
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int li = tid + j * kMcLanes;
    lp[li] = root[j];
    if (!in[j]) continue;
    const int gx = x0 + (li & 31), gy = y0 + (li >> 5);
    atomicAdd(&la[root[j]], 1);
    const int flags = (gy == g.H - 1 ? kMcBottom : 0) | (gx == 0 || gy == 0 || gx == g.W - 1 || gy == g.H - 1 ? kMcEdge : 0);
    if (flags) atomicOr(&la[root[j]], flags);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int li = tid + j * kMcLanes, gx = x0 + (li & 31), gy = y0 + (li >> 5);
    if (gx >= g.W || gy >= g.H) continue;
    const int r = root[j];
    g.parent[base + (size_t)gy * g.W + gx] = r < 0 ? -1 : (y0 + (r >> 5)) * g.W + x0 + (r & 31);
  }
  const int wh = (g.W + 1) >> 1;
  const size_t ibase = (size_t)f * g.H * wh;
  for (int p = tid; p < kMcTilePixels / 2; p += kMcLanes) {
    const int li = 2 * p, gx = x0 + (li & 31), gy = y0 + (li >> 5);
    if (gx >= g.W || gy >= g.H) continue;
    const int v = lp[li] == li ? la[li] : (lp[li + 1] == li + 1 ? la[li + 1] : 0);   // (a pixel past the frame's width holds -1)
    g.info[ibase + (size_t)gy * wh + (gx >> 1)] = v;
  }
  if (hit) atomicOr(&g.report[f * kMcReport + 6], 2);
}

// grid (ceil(H W / 256), n)
template <bool kHole>
__global__ __launch_bounds__(kMcLanes) void mc_merge_kernel(const McArgs g) {
  const int i = blockIdx.x * kMcLanes + threadIdx.x, f = blockIdx.y;
  if (i >= g.H * g.W) return;
  const int y = i / g.W, x = i - y * g.W;
  if ((x & 31) != 0 && (y & 31) != 0 && (x & 31) != 31) return;
  int* parent = g.parent + (size_t)f * g.H * g.W;
  if (mc_load(parent + i) < 0) return;
  int hit = 0;
  bool nin[4], pick[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int nx = x + mc_back_neighbour(q).dx, ny = y + mc_back_neighbour(q).dy;
    nin[q] = nx >= 0 && nx < g.W && ny >= 0 && mc_load(parent + ny * g.W + nx) >= 0;              // the frame's view
  }
  mc_pick(!kHole, nin, pick);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int nx = x + mc_back_neighbour(q).dx, ny = y + mc_back_neighbour(q).dy;
    if (!pick[q] || ((nx >> 5) == (x >> 5) && (ny >> 5) == (y >> 5))) continue;                   // the same tile: joined in LDS
    mc_union(parent, i, ny * g.W + nx, g.H * g.W, &hit);
  }
  if (hit) atomicOr(&g.report[f * kMcReport + 6], 2);
}

// grid (ceil(H W / 256) + 1, n): the last workgroup of a frame takes its anchors
template <bool kHole>
__global__ __launch_bounds__(kMcLanes) void mc_gather_kernel(const McArgs g) {
  const int f = blockIdx.y, cap = g.H * g.W;
  int* parent = g.parent + (size_t)f * g.H * g.W;
  int* info = g.info + (size_t)f * g.H * ((g.W + 1) >> 1);
  int hit = 0;
  if (blockIdx.x == gridDim.x - 1) {
    if (!kHole && (int)threadIdx.x < g.k) {
      const int* a = g.anchors + ((size_t)f * g.k + threadIdx.x) * 2;
      const int ax = a[0], ay = a[1];
      if (ax >= 0 && ax < g.W && ay >= 0 && ay < g.H && mc_load(parent + ay * g.W + ax) >= 0)
        atomicOr(&info[mc_slot(mc_find(parent, ay * g.W + ax, cap, &hit), g.W)], kMcAnchored);
    }
  } else {
    const int i = blockIdx.x * kMcLanes + threadIdx.x;
    if (i < cap) {
      const int y = i / g.W, x = i - y * g.W;
      if (mc_load(parent + i) >= 0) mc_store(parent + i, mc_find(parent, i, cap, &hit));   // a shorter path to the same root
      if ((x & 1) == 0) {
        const int slot = mc_slot(i, g.W), q = mc_pair_pixel(parent, slot, g.W);
        if (q >= 0) {
          const int r = mc_find(parent, q, cap, &hit);
          // r == q: the component's own record, which the others add to.  Otherwise nothing else touches this one.
          const int v = r != q ? info[slot] : 0;
          if (v & kMcArea) {
            int* dst = &info[mc_slot(r, g.W)];
            atomicAdd(dst, v & kMcArea);
            if (v & kMcFlags) atomicOr(dst, v & kMcFlags);
          }
        }
      }
    }
  }
  if (hit) atomicOr(&g.report[f * kMcReport + 6], 2);
}

// grid (ceil(H ceil(W / 2) / 256), n): one lane per pair; the roots among them decide
template <bool kHole>
__global__ __launch_bounds__(kMcLanes) void mc_decide_kernel(const McArgs g) {
  const int s = blockIdx.x * kMcLanes + threadIdx.x, f = blockIdx.y, wh = (g.W + 1) >> 1;
  if (s >= g.H * wh) return;
  const int* parent = g.parent + (size_t)f * g.H * g.W;
  int* info = g.info + (size_t)f * g.H * wh;
  int* rep = g.report + f * kMcReport;
  const int q = mc_pair_pixel(parent, s, g.W);
  if (q < 0 || parent[q] != q) return;
  const int v = info[s], area = v & kMcArea;
  if (kHole) {
    if (!(v & kMcEdge) && area <= g.limit) {
      info[s] = v | kMcChosen;
      atomicAdd(&rep[4], 1);
      atomicAdd(&rep[5], area);
    }
  } else {
    atomicAdd(&rep[0], 1);
    if (area >= g.limit && (g.keep_all || (v & (kMcBottom | kMcAnchored)))) {
      info[s] = v | kMcChosen;
      atomicAdd(&rep[1], 1);
    }
  }
}

// grid (ceil(W / 256), H, n): bit 0: the pixel is of a kept component; bit 1: one within `grow` of it along the row is
__global__ __launch_bounds__(kMcLanes) void mc_row_kernel(const McArgs g) {
  __shared__ unsigned char kept[kMcLanes + 2 * VP_MATTECLEAN_MAX_GROW];
  const int y = blockIdx.y, f = blockIdx.z, xb = blockIdx.x * kMcLanes - g.grow;
  const int* parent = g.parent + (size_t)f * g.H * g.W;
  const int* info = g.info + (size_t)f * g.H * ((g.W + 1) >> 1);
  const bool all = mc_fallback(g, f);
  for (int t = threadIdx.x; t < kMcLanes + 2 * g.grow; t += kMcLanes) {
    const int x = xb + t;
    bool k = false;
    if (x >= 0 && x < g.W) {
      const int r = parent[y * g.W + x];
      k = r >= 0 && (all || (info[mc_slot(r, g.W)] & kMcChosen));
    }
    kept[t] = k;
  }
  __syncthreads();
  const int x = blockIdx.x * kMcLanes + threadIdx.x;
  if (x >= g.W) return;
  int near = 0;
  for (int d = 0; d <= 2 * g.grow; ++d) near |= kept[threadIdx.x + d];
  g.plane[(size_t)f * g.H * g.W + y * g.W + x] = (unsigned char)(kept[threadIdx.x + g.grow] | (near << 1));
}

// grid (ceil(H W / 256), n): the column pass of the dilation and m1 into `out`
__global__ __launch_bounds__(kMcLanes) void mc_apply_kernel(const McArgs g) {
  const int i = blockIdx.x * kMcLanes + threadIdx.x, f = blockIdx.y;
  const size_t base = (size_t)f * g.H * g.W;
  int removed = 0, zeroed = 0;
  if (i < g.H * g.W) {
    const int m = g.src[base + i];
    int o = 0;
    if (m >= g.support) {
      if (g.plane[base + i] & 1) o = m; else removed = 1;
    } else if (m > 0) {
      const int y = i / g.W, lo = max(y - g.grow, 0), hi = min(y + g.grow, g.H - 1);
      int near = 0;
      for (int yy = lo; yy <= hi; ++yy) near |= g.plane[base + (size_t)(i + (yy - y) * g.W)];
      if (near & 2) o = m; else zeroed = 1;
    }
    g.out[base + i] = (unsigned char)o;
  }
  // integers: any order gives the same counts
  int packed = removed | (zeroed << 16);                          // at most 64 of each per wavefront
  for (int off = 32; off > 0; off >>= 1) packed += __shfl_down(packed, off, 64);
  if ((threadIdx.x & 63) == 0 && packed) {
    if (packed & 0xffff) atomicAdd(&g.report[f * kMcReport + 2], packed & 0xffff);
    if (packed >> 16) atomicAdd(&g.report[f * kMcReport + 3], packed >> 16);
  }
}

// grid (ceil(H W / 256), n)
__global__ __launch_bounds__(kMcLanes) void mc_fill_kernel(const McArgs g) {
  const int i = blockIdx.x * kMcLanes + threadIdx.x, f = blockIdx.y;
  if (i >= g.H * g.W) return;
  const int r = g.parent[(size_t)f * g.H * g.W + i];
  if (r >= 0 && (g.info[(size_t)f * g.H * ((g.W + 1) >> 1) + mc_slot(r, g.W)] & kMcChosen)) g.out[(size_t)f * g.H * g.W + i] = 255;
}

// one lane per frame
__global__ void mc_finish_kernel(const McArgs g, int n) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  if (mc_fallback(g, f)) {
    g.report[f * kMcReport + 1] = g.report[f * kMcReport + 0];
    g.report[f * kMcReport + 6] |= 1;
  }
}

}  // namespace vp

struct vp_matteclean {
  vp_matteclean_desc d;
  int* labels;                               // [max_frames][max_height][max_width]
  int* holes;                                // the same: the hole pass's parents; its first bytes are the dilation's plane
  int* info;                                 // [max_frames][max_height][(max_width + 1) / 2]
  int* report;                               // [max_frames][8]
  int height, width;                         // of the last call
};

using namespace vp;

static int mc_check(const vp_matteclean_desc* d, vp_matteclean* h) {
  if (const int rc = check_desc(d, "vp_matteclean")) return rc;
  if (const int rc = check_extents_desc("vp_matteclean", d->max_frames, VP_MATTECLEAN_MAX_FRAMES, d->max_height, d->max_width, 16, VP_MATTECLEAN_MAX_SIZE)) return rc;
  h->d = *d;
  h->height = d->max_height;
  h->width = d->max_width;
  return VP_OK;
}

static size_t mc_carve(vp_matteclean* h, void* base) {
  Arena ar(base);
  const size_t rows = (size_t)h->d.max_frames * h->d.max_height;
  h->labels = ar.take<int>(rows * h->d.max_width);
  h->holes = ar.take<int>(rows * h->d.max_width);
  h->info = ar.take<int>(rows * ((h->d.max_width + 1) / 2));
  h->report = ar.take<int>((size_t)h->d.max_frames * kMcReport);
  return align256(ar.total());
}

extern "C" {

size_t vp_matteclean_desc_size(void) { return sizeof(vp_matteclean_desc); }

size_t vp_matteclean_workspace_bytes(const vp_matteclean_desc* d) {
  vp_matteclean h;
  return mc_check(d, &h) ? 0 : mc_carve(&h, nullptr);
}

int vp_matteclean_create(const vp_matteclean_desc* d, void* workspace, size_t bytes, vp_matteclean_t** out) {
  return open_handle("vp_matteclean_create", d, mc_check, mc_carve, workspace, bytes, out);
}

void vp_matteclean_destroy(vp_matteclean_t* h) { delete h; }

int vp_matteclean_clean(vp_matteclean_t* h, const unsigned char* matte, int n, int height, int width, int support, int core, int min_area,
                        int max_hole, int grow, int keep, const int* anchors, int k, unsigned char* out, void* stream) {
  const char* who = "vp_matteclean_clean";
  if (!h || !matte || !out) { set_err("%s: bad argument (handle, device matte, device out)", who); return VP_ERR_ARG; }
  if (const int rc = check_batch(who, n, height, width, 16, h->d.max_frames, h->d.max_height, h->d.max_width)) return rc;
  if (support < 1 || support > 255) { set_err("%s: support %d outside 1 .. 255", who, support); return VP_ERR_ARG; }
  if (core < 1 || core > 255) { set_err("%s: core %d outside 1 .. 255", who, core); return VP_ERR_ARG; }
  const int pixels = height * width;                              // at most 2^20
  if (min_area < -1 || min_area > pixels) { set_err("%s: min_area %d outside 0 .. height * width (or -1: the default)", who, min_area); return VP_ERR_ARG; }
  if (max_hole < -1 || max_hole > pixels) { set_err("%s: max_hole %d outside 0 .. height * width (or -1: the default)", who, max_hole); return VP_ERR_ARG; }
  if (grow < 0 || grow > VP_MATTECLEAN_MAX_GROW) { set_err("%s: grow %d outside 0 .. %d", who, grow, VP_MATTECLEAN_MAX_GROW); return VP_ERR_ARG; }
  if (keep != VP_MATTECLEAN_KEEP_ALL && keep != VP_MATTECLEAN_KEEP_ANCHORED) { set_err("%s: keep %d is neither 0 (all) nor 1 (anchored)", who, keep); return VP_ERR_ARG; }
  if (k < 0 || k > VP_MATTECLEAN_MAX_ANCHORS) { set_err("%s: k %d anchors outside 0 .. %d", who, k, VP_MATTECLEAN_MAX_ANCHORS); return VP_ERR_ARG; }
  if (k > 0 && !anchors) { set_err("%s: bad argument (device anchors with k %d)", who, k); return VP_ERR_ARG; }
  // in place works because every launch reads and writes a pixel's own byte only; at a shifted address it would not
  if (out != matte && overlaps(out, matte, (size_t)n * pixels)) {
    set_err("%s: out overlaps the matte at another address (identical or disjoint buffers only)", who);
    return VP_ERR_ARG;
  }
  if (min_area < 0) min_area = pixels / 1024;
  if (max_hole < 0) max_hole = pixels / 256;
  h->height = height;
  h->width = width;
  hipStream_t st = (hipStream_t)stream;
  VP_HIP_CHECK(hipMemsetAsync(h->report, 0, (size_t)n * kMcReport * sizeof(int), st));
  McArgs g;
  memset(&g, 0, sizeof(g));
  g.src = matte; g.out = out; g.parent = h->labels; g.info = h->info; g.plane = (unsigned char*)h->holes; g.report = h->report;
  g.anchors = anchors; g.H = height; g.W = width; g.thresh = support; g.support = support; g.limit = min_area;
  g.keep_all = keep == VP_MATTECLEAN_KEEP_ALL; g.grow = grow; g.k = k;
  const dim3 lanes(kMcLanes);
  const dim3 tiles((width + kMcTile - 1) / kMcTile, (height + kMcTile - 1) / kMcTile, n);     // at most 32 x 32 x 4096
  const int blocks = (pixels + kMcLanes - 1) / kMcLanes;                                       // at most 4096
  const dim3 per_pixel(blocks, n), per_pair((height * ((width + 1) / 2) + kMcLanes - 1) / kMcLanes, n);
  hipLaunchKernelGGL(mc_local_kernel<false>, tiles, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mc_merge_kernel<false>, per_pixel, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mc_gather_kernel<false>, dim3(blocks + 1, n), lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mc_decide_kernel<false>, per_pair, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mc_row_kernel, dim3((width + kMcLanes - 1) / kMcLanes, height, n), lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mc_apply_kernel, per_pixel, lanes, 0, st, g);
  VP_HIP_CHECK(hipGetLastError());
  if (max_hole > 0) {
    g.src = out; g.parent = h->holes; g.thresh = core; g.limit = max_hole; g.k = 0;
    hipLaunchKernelGGL(mc_local_kernel<true>, tiles, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mc_merge_kernel<true>, per_pixel, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mc_gather_kernel<true>, dim3(blocks + 1, n), lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mc_decide_kernel<true>, per_pair, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mc_fill_kernel, per_pixel, lanes, 0, st, g);
    VP_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(mc_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, g, n);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_matteclean_tensor(vp_matteclean_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_matteclean_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  int64_t e1 = 1, e2 = 1;
  if (s == "labels") { *ptr = h->labels; e1 = h->height; e2 = h->width; }
  else if (s == "report") { *ptr = h->report; e1 = kMcReport; }
  else { set_err("vp_matteclean_tensor: no tensor '%s' (labels, report)", name); return VP_ERR_ARG; }
  if (shape) { shape[0] = h->d.max_frames; shape[1] = e1; shape[2] = e2; shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

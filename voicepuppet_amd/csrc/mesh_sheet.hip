// Visual evaluation of BFMNet on the device (include/vp_hip.h): the montage of rendered mesh tiles that utils/bfm_visual.py
// plot_bfm_coeff_seq assembles in numpy (:127-128, with the cvtColor of :125), and the 68-landmark distance between two projected
// sequences (no reference counterpart: the reference has only the picture).
//
//   sheet tile   tile i of [n,h,w,3] uint8 goes to cell first_cell + i of a [rows*h, cols*w, 3] sheet.  A tile row is 3*w bytes.
//                wide path (w a multiple of 4, both bases on 4-byte boundaries: then every row of every tile and its place in the
//                sheet are): a lane moves 4 pixels = 3 dwords, consecutive lanes consecutive 12 bytes of a row, so a wavefront
//                reads and writes 768 contiguous bytes; the R/B swap is a byte shuffle of the three words.
//                byte path otherwise: a lane moves one pixel.
//   landmarks    one wavefront per frame: lane l takes landmark l (and l + 64 for l < 4), the 64 partial sums go down a shuffle
//                tree of fixed shape, so a frame's two numbers do not depend on the batch it is in.
// The host checks every cell against the sheet before anything is enqueued; the kernels index only inside the tile they were given.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "errors.h"

#pragma clang fp contract(off)

namespace vp {

struct SheetArgs {
  const unsigned char* tiles;
  unsigned char* sheet;
  int h, w, cols, first_cell, swap_rb;
  size_t pitch;              // bytes of a sheet row: cols * w * 3
};

__device__ __forceinline__ unsigned char* sheet_cell(const SheetArgs& a, int tile) {
  const int cell = a.first_cell + tile, cr = cell / a.cols, cc = cell - cr * a.cols;
  return a.sheet + (size_t)cr * a.h * a.pitch + (size_t)cc * a.w * 3;
}

__global__ __launch_bounds__(256) void sheet_tile_wide_kernel(const SheetArgs a) {
  const int upr = a.w >> 2;                                  // 12-byte units per tile row
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= a.h * upr) return;
  const int y = u / upr, x = u - y * upr;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tiles + ((size_t)blockIdx.y * a.h + y) * a.w * 3) + 3 * x;
  uint32_t* dst = reinterpret_cast<uint32_t*>(sheet_cell(a, blockIdx.y) + (size_t)y * a.pitch) + 3 * x;
  const uint32_t p = src[0], q = src[1], r = src[2];         // bytes 0..11: four pixels
  if (a.swap_rb) {
    dst[0] = ((p >> 16) & 0xffu) | (p & 0xff00u) | ((p & 0xffu) << 16) | ((q & 0xff00u) << 16);
    dst[1] = (q & 0xffu) | ((p >> 24) << 8) | ((r & 0xffu) << 16) | (q & 0xff000000u);
    dst[2] = ((q >> 16) & 0xffu) | ((r >> 24) << 8) | (r & 0xff0000u) | ((r & 0xff00u) << 16);
  } else {
    dst[0] = p; dst[1] = q; dst[2] = r;
  }
}

__global__ __launch_bounds__(256) void sheet_tile_byte_kernel(const SheetArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;              // one pixel
  if (u >= a.h * a.w) return;
  const int y = u / a.w, x = u - y * a.w;
  const unsigned char* src = a.tiles + (((size_t)blockIdx.y * a.h + y) * a.w + x) * 3;
  unsigned char* dst = sheet_cell(a, blockIdx.y) + (size_t)y * a.pitch + (size_t)x * 3;
  const unsigned char c0 = src[0], c1 = src[1], c2 = src[2];
  dst[0] = a.swap_rb ? c2 : c0; dst[1] = c1; dst[2] = a.swap_rb ? c0 : c2;
}

constexpr int kLandmarks = 68, kMouthFirst = 48;

__global__ __launch_bounds__(64) void landmark_distance_kernel(const double* __restrict__ pa, const double* __restrict__ pb,
                                                               const int* __restrict__ keypoints, int nver, double* __restrict__ out) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const double* A = pa + (size_t)f * nver * 2;
  const double* B = pb + (size_t)f * nver * 2;
  double all = 0.0, mouth = 0.0;
  for (int l = lane; l < kLandmarks; l += 64) {              // lane l: landmark l, then l + 64
    const int k = keypoints[l];
    double d = NAN;                                          // an index outside the mesh poisons the frame's numbers, it is not read
    if (k >= 0 && k < nver) {
      const double dx = A[2 * k] - B[2 * k], dy = A[2 * k + 1] - B[2 * k + 1];
      d = sqrt(dx * dx + dy * dy);
    }
    all += d;
    if (l >= kMouthFirst) mouth += d;
  }
  for (int off = 32; off > 0; off >>= 1) {
    all += __shfl_down(all, off, 64);
    mouth += __shfl_down(mouth, off, 64);
  }
  if (lane == 0) {
    out[2 * f] = all / (double)kLandmarks;
    out[2 * f + 1] = mouth / (double)(kLandmarks - kMouthFirst);
  }
}

}  // namespace vp

extern "C" {

int vp_sheet_tile_u8(const unsigned char* tiles, int n, int h, int w, unsigned char* sheet, int sheet_rows, int sheet_cols, int first_cell,
                     int swap_rb, void* stream) {
  if (!tiles || !sheet) { vp::set_err("vp_sheet_tile_u8: bad argument (device tiles and sheet)"); return VP_ERR_ARG; }
  if (n < 1 || n > 65535 || h < 1 || h > 16384 || w < 1 || w > 16384) {
    vp::set_err("vp_sheet_tile_u8: bad argument (%d tiles of %d x %d: 1 .. 65535 tiles, sides 1 .. 16384)", n, h, w);
    return VP_ERR_ARG;
  }
  if (sheet_rows < 1 || sheet_cols < 1 || sheet_rows > 65536 || sheet_cols > 65536) {
    vp::set_err("vp_sheet_tile_u8: bad argument (sheet of %d x %d cells)", sheet_rows, sheet_cols);
    return VP_ERR_ARG;
  }
  const long long cells = (long long)sheet_rows * sheet_cols;
  if (first_cell < 0 || (long long)first_cell + n > cells) {
    vp::set_err("vp_sheet_tile_u8: cells %d .. %lld are outside the sheet's %lld", first_cell, (long long)first_cell + n - 1, cells);
    return VP_ERR_ARG;
  }
  vp::SheetArgs a;
  a.tiles = tiles; a.sheet = sheet; a.h = h; a.w = w; a.cols = sheet_cols; a.first_cell = first_cell; a.swap_rb = swap_rb ? 1 : 0;
  a.pitch = (size_t)sheet_cols * w * 3;
  hipStream_t st = (hipStream_t)stream;
  // w % 4 == 0: a tile row, a tile, a sheet row and a cell's column offset are all multiples of 12 bytes, so two aligned bases suffice
  const bool wide = (w & 3) == 0 && (((uintptr_t)tiles | (uintptr_t)sheet) & 3) == 0;
  if (wide) hipLaunchKernelGGL(vp::sheet_tile_wide_kernel, dim3((h * (w >> 2) + 255) / 256, n), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(vp::sheet_tile_byte_kernel, dim3((h * w + 255) / 256, n), dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_landmark_distance(const double* proj_a, const double* proj_b, const int* keypoints, int frames, int nver, double* out, void* stream) {
  if (!proj_a || !proj_b || !keypoints || !out || frames < 1 || nver < 1) {
    vp::set_err("vp_landmark_distance: bad argument (device projections [frames,nver,2], keypoints [68], out [frames,2])");
    return VP_ERR_ARG;
  }
  hipLaunchKernelGGL(vp::landmark_distance_kernel, dim3(frames), dim3(64), 0, (hipStream_t)stream, proj_a, proj_b, keypoints, nver, out);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

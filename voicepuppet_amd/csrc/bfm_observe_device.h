// Device code of the photo observation that more than one translation unit evaluates (bfm_appear.hip: vp_bfmfit_observe; bfm_observe.hip:
// vp_bfmfit_observe_ex): per (frame, vertex) the rotated one-ring normal -> Y [9], the projection -> the photo position, the inside test,
// the bilinear sample and the facing weight, each the expression sequence bfm_appear_observe_kernel always had.  No FMA contraction
// (bfm_device.h switches it off): the float64 results are compared bit for bit.
#pragma once
#include "bfm_device.h"

namespace vp {

struct ObserveArgs {
  const double* shape;       // [frames,N,3] unrotated, centred
  const double* fn;          // [frames,F+1,3]
  const int* point_buf;
  const double* rot;         // [frames,9]
  const float* coeff;        // [frames,257]
  const unsigned char* photo;          // [photo_frames,H,W,3]
  const double* affine;      // [frames,3] (a, bx, by)
  const double* vertex_weights;        // optional [N]
  double* sh; double* weight; double* observed;
  int nver, ntri, photo_frames, height, width;
  double focal, center;
  double shc[5];
};

// what one (frame, vertex) knows before the photo is read
struct ObservedVertex {
  double prx, pry, zb;       // face_projection and the z buffer value (bfm_project)
  double px, py;             // the photo position a prx + bx, a pry + by
  double mz;                 // (n . R)_z
  bool inside;               // 0 <= px <= W-1 and 0 <= py <= H-1 (false for a NaN)
};

// geometry of vertex v of frame f; writes sh [fv*9 ..]
__device__ __forceinline__ void observe_vertex(const ObserveArgs& a, int f, int v, size_t fv, ObservedVertex& o) {
  const double* R = a.rot + f * 9;
  double nx, ny, nz, mx, my, mz;
  bfm_vertex_normal(a.fn + (size_t)f * (a.ntri + 1) * 3, a.point_buf, v, nx, ny, nz);
  bfm_rotate(R, nx, ny, nz, mx, my, mz);
  const float* C = a.coeff + (size_t)f * 257;
  bfm_project(R, a.shape[fv * 3], a.shape[fv * 3 + 1], a.shape[fv * 3 + 2], (double)C[254], (double)C[255], (double)C[256], a.focal, a.center, o.prx,
              o.pry, o.zb);
  double Y[9];
  bfm_sh_terms(a.shc, mx, my, mz, Y);
#pragma unroll
  for (int k = 0; k < 9; ++k) a.sh[fv * 9 + k] = Y[k];
  const double s = a.affine[f * 3];
  o.px = s * o.prx + a.affine[f * 3 + 1];
  o.py = s * o.pry + a.affine[f * 3 + 2];
  o.mz = mz;
  o.inside = o.px >= 0.0 && o.px <= (double)(a.width - 1) && o.py >= 0.0 && o.py <= (double)(a.height - 1);      // false for a NaN
}

__device__ __forceinline__ const unsigned char* observe_image(const ObserveArgs& a, int f) {
  return a.photo + (a.photo_frames == 1 ? 0 : (size_t)f * a.height * a.width * 3);
}

// the bilinear sample of img [H,W,3] at a position inside it
__device__ __forceinline__ void observe_tap(const unsigned char* __restrict__ img, int height, int width, double px, double py, double* o) {
  int x0 = (int)floor(px), y0 = (int)floor(py);
  if (x0 > width - 2) x0 = width - 2;                    // px = W-1 is inside: the last cell with fx = 1
  if (y0 > height - 2) y0 = height - 2;
  const double fx = px - (double)x0, fy = py - (double)y0;
  const unsigned char* q0 = img + ((size_t)y0 * width + x0) * 3;
  const unsigned char* q1 = q0 + (size_t)width * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double top = (1.0 - fx) * (double)q0[c] + fx * (double)q0[3 + c];
    const double bot = (1.0 - fx) * (double)q1[c] + fx * (double)q1[3 + c];
    o[c] = (1.0 - fy) * top + fy * bot;
  }
}

__device__ __forceinline__ double observe_weight(const ObserveArgs& a, int v, const ObservedVertex& o) {
  const double vw = a.vertex_weights ? a.vertex_weights[v] : 1.0;
  return o.inside ? vw * fmax(0.0, o.mz) : 0.0;
}

}  // namespace vp

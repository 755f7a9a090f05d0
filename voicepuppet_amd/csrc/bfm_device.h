// Device code of the BFM reconstruction that more than one translation unit evaluates (bfm_recon.hip: vp_bfm_reconstruct*; bfm_appear.hip:
// vp_bfmfit_observe): the per-vertex steps of `Reconstruction` (utils/reconstruct_mesh.py:172-194) as inline functions, each the
// expression sequence bfm_vertex_kernel always had, and the launchers of the two kernels that come before it (defined in bfm_recon.hip).
// No FMA contraction from here to the end of the including file: the float64 results are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "vp_hip.h"

#pragma clang fp contract(off)

namespace vp {

// one-ring vertex normal (:50-52); FN [ntri+1,3] of the frame, the last row the appended zero normal
__device__ __forceinline__ void bfm_vertex_normal(const double* __restrict__ FN, const int* __restrict__ point_buf, int v, double& nx, double& ny,
                                                  double& nz) {
  nx = 0; ny = 0; nz = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = point_buf[v * 8 + j];
    nx += FN[3 * t]; ny += FN[3 * t + 1]; nz += FN[3 * t + 2];
  }
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  nx /= len; ny /= len; nz /= len;
}

// (x, y, z) . R for a row-major R [9] (:182, :111)
__device__ __forceinline__ void bfm_rotate(const double* __restrict__ R, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = x * R[0] + y * R[3] + z * R[6]; oy = x * R[1] + y * R[4] + z * R[7]; oz = x * R[2] + y * R[5] + z * R[8];
}

// Projection_layer (:100-120) of a point that is rotated here, + the y flip of :186: prx, pry pixels of the 224 image, zb the z buffer value
__device__ __forceinline__ void bfm_project(const double* __restrict__ R, double px, double py, double pz, double tx, double ty, double tz, double focal,
                                            double center, double& prx, double& pry, double& zb) {
  const double qx = (px * R[0] + py * R[3] + pz * R[6]) + tx;
  const double qy = (px * R[1] + py * R[4] + pz * R[7]) + ty;
  const double qz = -((px * R[2] + py * R[5] + pz * R[8]) + tz) + 10.0;
  const double ux = focal * qx + center * qz, uy = focal * qy + center * qz;
  prx = ux / qz; pry = 224.0 - uy / qz; zb = -qz;
}

// the nine SH terms of Illumination_layer (:137-155) of the rotated normal m; sh = the model's five a_i c_i products
__device__ __forceinline__ void bfm_sh_terms(const double* sh, double mx, double my, double mz, double* Y) {
  Y[0] = sh[0];
  Y[1] = -sh[1] * my; Y[2] = sh[1] * mz; Y[3] = -sh[1] * mx;
  Y[4] = sh[2] * mx * my; Y[5] = -sh[2] * my * mz;
  Y[6] = sh[3] * (3.0 * (mz * mz) - 1.0);
  Y[7] = -sh[2] * mx * mz;
  Y[8] = sh[4] * (mx * mx - my * my);
}

// shape [frames,nver,3] = idBase alpha + exBase beta + meanshape - centre (Shape_formation, :20-29): one bfm_linear_kernel launch
void bfm_launch_shape(const vp_bfm_model* m, const float* coeff, int frames, double* shape, hipStream_t st);
// fn [frames,ntri+1,3]: the face normals (:41-49): one bfm_fnormal_kernel launch
void bfm_launch_fnormal(const vp_bfm_model* m, const double* shape, int frames, double* fn, hipStream_t st);

}  // namespace vp

// What the rasterisers share (raster.hip: flat-shaded colours; raster_dense.hip: triangle ids, barycentric weights, texture):
// the depth key and the barycentric arithmetic of the reference's isPointInTri / get_point_weight (utils/cython/mesh_core.cpp:23-82),
// in its operation order.  Both translation units are compiled with contraction off (x86-64 g++ -O2 emits no FMA).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace vp {

__device__ __forceinline__ unsigned int depth_bits(float d) {
  const unsigned int u = __float_as_uint(d + 0.f);           // -0 -> +0: the reference compares floats, where they are equal
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // monotone float -> uint
}

// u, v of mesh_core.cpp:45-46 / :75-76 (the two functions compute them identically)
__device__ __forceinline__ void point_uv(float px, float py, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y, float& u, float& v) {
  const float v0x = p2x - p0x, v0y = p2y - p0y;
  const float v1x = p1x - p0x, v1y = p1y - p0y;
  const float v2x = px - p0x, v2y = py - p0y;
  const float dot00 = ((v0x * v0x) + (v0y * v0y));
  const float dot01 = ((v0x * v1x) + (v0y * v1y));
  const float dot02 = ((v0x * v2x) + (v0y * v2y));
  const float dot11 = ((v1x * v1x) + (v1y * v1y));
  const float dot12 = ((v1x * v2x) + (v1y * v2y));
  const float den = ((dot00 * dot11) - (dot01 * dot01));
  const float inv = (den == 0.f) ? 0.f : (1.f / den);
  u = ((dot11 * dot02) - (dot01 * dot12)) * inv;
  v = ((dot00 * dot12) - (dot01 * dot02)) * inv;
}

__device__ __forceinline__ bool point_in_tri(float px, float py, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y) {
  float u, v;
  point_uv(px, py, p0x, p0y, p1x, p1y, p2x, p2y, u, v);
  return (u >= 0.f) && (v >= 0.f) && ((u + v) < 1.f);
}

}  // namespace vp

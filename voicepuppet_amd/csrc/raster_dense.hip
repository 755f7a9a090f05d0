// The dense half of the reference's mesh_core (utils/cython/mesh_core.cpp): _rasterize_triangles_core (:108-166: per pixel the visible
// triangle, its barycentric weights and the interpolated depth), _render_texture_core (:234-333), _get_normal_core (:85-105) and the
// interpolation of per-vertex attributes through the buffers - bit-exact with the serial C++, batched over frames that share a
// triangle list.  raster.hip is the flat-shaded quarter (_render_colors_core); the depth key and the barycentric arithmetic are shared
// (raster_common.h).  vp_raster_vertex_visibility, which has no counterpart there, asks the depth buffer which vertices it shows.
//
// Visibility.  The reference visits triangles in index order and overwrites a pixel when the candidate's depth is strictly greater
// than the buffer, so a pixel's survivor is the maximum over its candidates of (p_depth, lowest index).  Parallel form, as in
// raster.hip: a 64-bit atomicMax per candidate pixel on key = depth_bits(p_depth) << 32 | (0xFFFFFFFE - index), seeded from the given
// depth buffer with low word 0xFFFFFFFF (which beats every triangle of equal depth); a second kernel recomputes the winner's weights
// and depth from its index.  Unlike raster.hip the depth is PER PIXEL (w0*d0 + w1*d1 + w2*d2 with get_point_weight's weights,
// :53-82), so the key is computed per pixel, and a pixel in the two-pixel border ring is a candidate of every triangle whose clamped
// bounding box holds it (:148, :292: no inside test there).  A NaN depth never wins in the reference ('>' is false); its bit pattern
// would beat everything here, so it is skipped.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#include "workspace.h"
#include "raster_common.h"

#pragma clang fp contract(off)

namespace vp {

// get_point_weight (:53-82) and the depth of :151 / :295
__device__ __forceinline__ float point_weights(float px, float py, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y, float d0,
                                               float d1, float d2, float& w0, float& w1, float& w2) {
  float u, v;
  point_uv(px, py, p0x, p0y, p1x, p1y, p2x, p2y, u, v);
  w0 = (1.f - u) - v;
  w1 = v;
  w2 = u;
  return ((w0 * d0) + (w1 * d1)) + (w2 * d2);
}

__global__ __launch_bounds__(256) void dense_init_kernel(const float* __restrict__ depth, unsigned long long* __restrict__ keys, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = depth[i];
  const unsigned int hi = (d != d) ? 0xFFFFFFFFu : depth_bits(d);       // nothing is greater than a NaN already in the buffer
  keys[i] = ((unsigned long long)hi << 32) | 0xFFFFFFFFull;
}

// one candidate pixel: the border quirk, the inside test, the per-pixel key
__device__ __forceinline__ void dense_candidate(unsigned long long* __restrict__ K, int x, int y, int h, int w, unsigned int klo, float p0x, float p0y,
                                                float p1x, float p1y, float p2x, float p2y, float d0, float d1, float d2) {
  const float px = (float)x, py = (float)y;
  float u, v;
  point_uv(px, py, p0x, p0y, p1x, p1y, p2x, p2y, u, v);
  const bool border = x < 2 || x > w - 3 || y < 2 || y > h - 3;
  if (!(border || ((u >= 0.f) && (v >= 0.f) && ((u + v) < 1.f)))) return;
  const float w0 = (1.f - u) - v;
  const float pd = ((w0 * d0) + (v * d1)) + (u * d2);
  if (pd != pd) return;
  atomicMax(K + (size_t)y * w + x, ((unsigned long long)depth_bits(pd) << 32) | klo);
}

// bounding boxes up to this many pixels are scanned by the triangle's own lane; larger ones by the whole wave
constexpr int DENSE_LANE_AREA = 32;

// tex_triangles != nullptr: triangles with a texture index outside 0 .. tex_nver-1 are no candidates either (vp_render_texture)
__global__ __launch_bounds__(256) void dense_tri_kernel(const float* __restrict__ vertices, const int* __restrict__ triangles,
                                                        const int* __restrict__ tex_triangles, unsigned long long* __restrict__ keys, int ntri,
                                                        int nver, int tex_nver, int h, int w) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const float* V = vertices + (size_t)b * nver * 3;
  unsigned long long* K = keys + (size_t)b * h * w;
  float p0x = 0, p0y = 0, p1x = 0, p1y = 0, p2x = 0, p2y = 0, d0 = 0, d1 = 0, d2 = 0;
  int x_min = 0, x_max = -1, y_min = 0, y_max = -1;
  unsigned int klo = 0;
  if (t < ntri) {
    const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    bool ok = (unsigned)i0 < (unsigned)nver && (unsigned)i1 < (unsigned)nver && (unsigned)i2 < (unsigned)nver;
    if (ok && tex_triangles)
      ok = (unsigned)tex_triangles[3 * t] < (unsigned)tex_nver && (unsigned)tex_triangles[3 * t + 1] < (unsigned)tex_nver &&
           (unsigned)tex_triangles[3 * t + 2] < (unsigned)tex_nver;
    if (ok) {
      p0x = V[3 * i0]; p0y = V[3 * i0 + 1]; d0 = V[3 * i0 + 2];
      p1x = V[3 * i1]; p1y = V[3 * i1 + 1]; d1 = V[3 * i1 + 2];
      p2x = V[3 * i2]; p2y = V[3 * i2 + 1]; d2 = V[3 * i2 + 2];
      x_min = max((int)ceilf(fminf(p0x, fminf(p1x, p2x))), 0);
      x_max = min((int)floorf(fmaxf(p0x, fmaxf(p1x, p2x))), w - 1);
      y_min = max((int)ceilf(fminf(p0y, fminf(p1y, p2y))), 0);
      y_max = min((int)floorf(fmaxf(p0y, fmaxf(p1y, p2y))), h - 1);
      klo = 0xFFFFFFFEu - (unsigned)t;
    }
  }
  const bool covers = x_max >= x_min && y_max >= y_min;
  const int bw = x_max - x_min + 1;
  const int area = covers ? bw * (y_max - y_min + 1) : 0;                 // <= h * w < 2^31
  if (area > 0 && area <= DENSE_LANE_AREA) {
    for (int y = y_min; y <= y_max; ++y)
      for (int x = x_min; x <= x_max; ++x) dense_candidate(K, x, y, h, w, klo, p0x, p0y, p1x, p1y, p2x, p2y, d0, d1, d2);
  }
  // triangles with a large box: one at a time, pixels across the 64 lanes (raster.hip)
  unsigned long long big = __ballot(area > DENSE_LANE_AREA);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const float q0x = __shfl(p0x, src), q0y = __shfl(p0y, src), q1x = __shfl(p1x, src), q1y = __shfl(p1y, src);
    const float q2x = __shfl(p2x, src), q2y = __shfl(p2y, src);
    const float e0 = __shfl(d0, src), e1 = __shfl(d1, src), e2 = __shfl(d2, src);
    const int xm = __shfl(x_min, src), ym = __shfl(y_min, src), qw = __shfl(bw, src), qa = __shfl(area, src);
    const unsigned int qlo = __shfl(klo, src);
    for (int i = lane; i < qa; i += 64) dense_candidate(K, xm + i % qw, ym + i / qw, h, w, qlo, q0x, q0y, q1x, q1y, q2x, q2y, e0, e1, e2);
  }
}

__global__ __launch_bounds__(256) void dense_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ vertices,
                                                            const int* __restrict__ triangles, float* __restrict__ depth, int* __restrict__ tri_buf,
                                                            float* __restrict__ bary, int nver, int h, int w, int batch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t hw = (size_t)h * w;
  if (i >= (size_t)batch * hw) return;
  const unsigned int low = (unsigned int)keys[i];
  if (low == 0xFFFFFFFFu) return;                          // no candidate beat the given depth: all three buffers stay as given
  const int b = (int)(i / hw);
  const int p = (int)(i - (size_t)b * hw);
  const int t = (int)(0xFFFFFFFEu - low);
  const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
  const float* V = vertices + (size_t)b * nver * 3;
  float w0, w1, w2;
  const float pd = point_weights((float)(p % w), (float)(p / w), V[3 * i0], V[3 * i0 + 1], V[3 * i1], V[3 * i1 + 1], V[3 * i2], V[3 * i2 + 1],
                                 V[3 * i0 + 2], V[3 * i1 + 2], V[3 * i2 + 2], w0, w1, w2);
  depth[i] = pd;
  tri_buf[i] = t;
  bary[3 * i] = w0;
  bary[3 * i + 1] = w1;
  bary[3 * i + 2] = w2;
}

// std::min / std::max as mesh_core.cpp:304-305 calls them: min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a
__device__ __forceinline__ float clamp_tex(float x, float top) {
  const float m = (top < x) ? top : x;
  return (m < 0.f) ? 0.f : m;
}

__device__ __forceinline__ int texel(float f, int n) { return min(max((int)f, 0), n - 1); }   // no effect on a finite, clamped coordinate

__global__ __launch_bounds__(256) void texture_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ vertices,
                                                              const int* __restrict__ triangles, const float* __restrict__ texture,
                                                              const float* __restrict__ tex_coords, const int* __restrict__ tex_triangles,
                                                              float* __restrict__ image, float* __restrict__ depth, int nver, int h, int w, int c,
                                                              int tex_h, int tex_w, int tex_c, int mapping_type, int batch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t hw = (size_t)h * w;
  if (i >= (size_t)batch * hw) return;
  const unsigned int low = (unsigned int)keys[i];
  if (low == 0xFFFFFFFFu) return;
  const int b = (int)(i / hw);
  const int p = (int)(i - (size_t)b * hw);
  const int t = (int)(0xFFFFFFFEu - low);
  const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
  const int t0 = tex_triangles[3 * t], t1 = tex_triangles[3 * t + 1], t2 = tex_triangles[3 * t + 2];
  const float* V = vertices + (size_t)b * nver * 3;
  float w0, w1, w2;
  const float pd = point_weights((float)(p % w), (float)(p / w), V[3 * i0], V[3 * i0 + 1], V[3 * i1], V[3 * i1 + 1], V[3 * i2], V[3 * i2 + 1],
                                 V[3 * i0 + 2], V[3 * i1 + 2], V[3 * i2 + 2], w0, w1, w2);
  // x through the texture triangle, y through the MESH triangle, stride 3 (:270-272, as written)
  float tx = ((w0 * tex_coords[3 * t0]) + (w1 * tex_coords[3 * t1])) + (w2 * tex_coords[3 * t2]);
  float ty = ((w0 * tex_coords[3 * i0 + 1]) + (w1 * tex_coords[3 * i1 + 1])) + (w2 * tex_coords[3 * i2 + 1]);
  tx = clamp_tex(tx, (float)(tex_w - 1));
  ty = clamp_tex(ty, (float)(tex_h - 1));
  float* out = image + i * c;
  const size_t row = (size_t)tex_w * tex_c;
  if (mapping_type == 0) {
    const float* src = texture + texel(roundf(ty), tex_h) * row + (size_t)texel(roundf(tx), tex_w) * tex_c;
    for (int k = 0; k < c; ++k) out[k] = src[k];
  } else {
    const float yd = ty - floorf(ty), xd = tx - floorf(tx);
    const size_t yf = texel(floorf(ty), tex_h) * row, yc = texel(ceilf(ty), tex_h) * row;
    const size_t xf = (size_t)texel(floorf(tx), tex_w) * tex_c, xc = (size_t)texel(ceilf(tx), tex_w) * tex_c;
    for (int k = 0; k < c; ++k) {
      const float ul = texture[yf + xf + k], ur = texture[yf + xc + k], dl = texture[yc + xf + k], dr = texture[yc + xc + k];
      out[k] = (((ul * (1.f - xd)) * (1.f - yd) + (ur * xd) * (1.f - yd)) + (dl * (1.f - xd)) * yd) + (dr * xd) * yd;
    }
  }
  depth[i] = pd;
}

__global__ __launch_bounds__(256) void interpolate_kernel(float* __restrict__ out, const int* __restrict__ tri_buf, const float* __restrict__ bary,
                                                          const int* __restrict__ triangles, const float* __restrict__ attributes, int nver,
                                                          int ntri, int k, size_t hw, int batch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)batch * hw) return;
  const int t = tri_buf[i];
  if (t < 0 || t >= ntri) return;
  const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
  if ((unsigned)i0 >= (unsigned)nver || (unsigned)i1 >= (unsigned)nver || (unsigned)i2 >= (unsigned)nver) return;
  const float* A = attributes + (size_t)(i / hw) * nver * k;
  const float w0 = bary[3 * i], w1 = bary[3 * i + 1], w2 = bary[3 * i + 2];
  const float *a0 = A + (size_t)i0 * k, *a1 = A + (size_t)i1 * k, *a2 = A + (size_t)i2 * k;
  for (int ch = 0; ch < k; ++ch) out[i * k + ch] = ((w0 * a0[ch]) + (w1 * a1[ch])) + (w2 * a2[ch]);
}

// ---- vertex -> (triangle, corner) adjacency: offsets int32 [nver + 1], entries int32 [3 * ntri] (3 * triangle + corner, ascending per
// vertex), cursor int32 [nver] (scratch of the build).  Counting and the scan are integer work, the fill's arrival order is undone by a
// per-vertex sort: the result is a function of `triangles` alone.
__global__ __launch_bounds__(256) void adjacency_count_kernel(const int* __restrict__ triangles, int* __restrict__ cursor, int n3, int nver) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int v = triangles[e];
  if ((unsigned)v < (unsigned)nver) atomicAdd(cursor + v, 1);
}

__global__ __launch_bounds__(1024) void adjacency_scan_kernel(int* __restrict__ offsets, int* __restrict__ cursor, int nver) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int chunk = (nver + 1023) / 1024;
  const int lo = (int)min((long long)tid * chunk, (long long)nver), hi = min(lo + chunk, nver);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += cursor[i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int i = lo; i < hi; ++i) {
    const int n = cursor[i];
    offsets[i] = run;
    cursor[i] = run;
    run += n;
  }
  if (tid == 1023) offsets[nver] = part[1023];
}

__global__ __launch_bounds__(256) void adjacency_fill_kernel(const int* __restrict__ triangles, int* __restrict__ cursor, int* __restrict__ entries,
                                                             int n3, int nver) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int v = triangles[e];
  if ((unsigned)v < (unsigned)nver) entries[atomicAdd(cursor + v, 1)] = e;
}

__device__ __forceinline__ void sift_down(int* a, int root, int n) {
  for (;;) {
    int child = 2 * root + 1;
    if (child >= n) return;
    if (child + 1 < n && a[child] < a[child + 1]) ++child;
    if (a[root] >= a[child]) return;
    const int tmp = a[root]; a[root] = a[child]; a[child] = tmp;
    root = child;
  }
}

__global__ __launch_bounds__(256) void adjacency_sort_kernel(const int* __restrict__ offsets, int* __restrict__ entries, int nver) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nver) return;
  int* a = entries + offsets[v];
  const int n = offsets[v + 1] - offsets[v];
  if (n <= 32) {                                            // a mesh vertex has a handful of triangles
    for (int i = 1; i < n; ++i) {
      const int x = a[i];
      int j = i - 1;
      for (; j >= 0 && a[j] > x; --j) a[j + 1] = a[j];
      a[j + 1] = x;
    }
  } else {                                                  // a fan's hub: heap sort, n log n whatever the arrival order
    for (int r = n / 2 - 1; r >= 0; --r) sift_down(a, r, n);
    for (int m = n - 1; m > 0; --m) {
      const int tmp = a[0]; a[0] = a[m]; a[m] = tmp;
      sift_down(a, 0, m);
    }
  }
}

// one lane per (frame, vertex): the additions of mesh_core.cpp:100-102 that touch this vertex, in the serial loop's order
__global__ __launch_bounds__(256) void vertex_normals_kernel(float* __restrict__ normal, const float* __restrict__ tri_normal,
                                                             const int* __restrict__ offsets, const int* __restrict__ entries, int nver, int ntri) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nver) return;
  float* N = normal + ((size_t)blockIdx.y * nver + v) * 3;
  const float* T = tri_normal + (size_t)blockIdx.y * ntri * 3;
  float n0 = N[0], n1 = N[1], n2 = N[2];
  const int end = offsets[v + 1];
  for (int e = offsets[v]; e < end; ++e) {
    const int t = entries[e] / 3;
    n0 = n0 + T[3 * t];
    n1 = n1 + T[3 * t + 1];
    n2 = n2 + T[3 * t + 2];
  }
  N[0] = n0; N[1] = n1; N[2] = n2;
}

// one lane per (frame, vertex): is the vertex in front of (or on) the surface the depth buffer holds around it?  The four pixel centres
// that surround (x, y) are compared, the nearest-to-the-back of them decides (fminf: a NaN depth is ignored).
__global__ __launch_bounds__(256) void vertex_visibility_kernel(const float* __restrict__ vertices, const float* __restrict__ depth,
                                                                unsigned char* __restrict__ visible, int nver, int h, int w, float tol) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nver) return;
  const size_t bv = (size_t)blockIdx.y * nver + v;
  const float x = vertices[bv * 3], y = vertices[bv * 3 + 1], z = vertices[bv * 3 + 2];
  unsigned char vis = 1;                                    // off the buffer or a NaN: the buffer says nothing about the vertex
  if (x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1) && z == z) {
    const int x0 = min((int)floorf(x), w - 2), y0 = min((int)floorf(y), h - 2);
    const float* D = depth + (size_t)blockIdx.y * h * w + (size_t)y0 * w + x0;
    const float m = fminf(fminf(D[0], D[1]), fminf(D[w], D[w + 1]));
    vis = (z + tol >= m) ? 1 : 0;
  }
  visible[bv] = vis;
}

static bool dense_sizes_ok(int nver, int ntri, int h, int w, int batch) {
  return ntri >= 0 && ntri <= INT_MAX / 3 && nver >= 1 && nver <= INT_MAX / 3 && h >= 1 && w >= 1 && (long long)h * w <= INT_MAX && batch >= 1 &&
         batch <= 65535;
}

// the keys of both rasterisers: seeded from the given depths, then every candidate pixel of every triangle
static void dense_visibility(const float* vertices, const int* triangles, const int* tex_triangles, const float* depth_buffer,
                            unsigned long long* keys, int nver, int tex_nver, int ntri, int h, int w, int batch, hipStream_t st) {
  const size_t n = (size_t)batch * h * w;
  hipLaunchKernelGGL(dense_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, depth_buffer, keys, n);
  if (ntri > 0)
    hipLaunchKernelGGL(dense_tri_kernel, dim3((ntri + 255) / 256, batch), dim3(256), 0, st, vertices, triangles, tex_triangles, keys, ntri, nver,
                       tex_nver, h, w);
}

}  // namespace vp

extern "C" {

size_t vp_rasterize_triangles_workspace_bytes(int batch, int h, int w) {
  return (batch < 1 || h < 1 || w < 1 || (long long)h * w > INT_MAX) ? 0 : (size_t)batch * h * w * sizeof(unsigned long long) + 256;
}

size_t vp_render_texture_workspace_bytes(int batch, int h, int w) { return vp_rasterize_triangles_workspace_bytes(batch, h, w); }

int vp_rasterize_triangles(const float* vertices, const int* triangles, float* depth_buffer, int* triangle_buffer, float* barycentric_weight,
                           int nver, int ntri, int h, int w, int batch, void* workspace, void* stream) {
  if (!vertices || (!triangles && ntri > 0) || !depth_buffer || !triangle_buffer || !barycentric_weight || !workspace ||
      !vp::dense_sizes_ok(nver, ntri, h, w, batch)) {
    vp::set_err("vp_rasterize_triangles: bad argument (null pointer, or nver %d, ntri %d, h %d, w %d, batch %d out of range)", nver, ntri, h, w,
                batch);
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const size_t n = (size_t)batch * h * w;
  vp::dense_visibility(vertices, triangles, nullptr, depth_buffer, keys, nver, 0, ntri, h, w, batch, st);
  if (ntri > 0)
    hipLaunchKernelGGL(vp::dense_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, vertices, triangles, depth_buffer,
                       triangle_buffer, barycentric_weight, nver, h, w, batch);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_render_texture(float* image, const float* vertices, const int* triangles, const float* texture, const float* tex_coords,
                      const int* tex_triangles, float* depth_buffer, int nver, int tex_nver, int tex_rows, int ntri, int h, int w, int c, int tex_h,
                      int tex_w, int tex_c, int mapping_type, int batch, void* workspace, void* stream) {
  if (!image || !vertices || (!triangles && ntri > 0) || !texture || !tex_coords || (!tex_triangles && ntri > 0) || !depth_buffer || !workspace ||
      !vp::dense_sizes_ok(nver, ntri, h, w, batch) || tex_nver < 1 || c < 1 || tex_h < 1 || tex_w < 1 || tex_c < 1) {
    vp::set_err("vp_render_texture: bad argument (null pointer, or nver %d, tex_nver %d, ntri %d, h %d, w %d, c %d, tex_h %d, tex_w %d, tex_c %d, "
                "batch %d out of range)", nver, tex_nver, ntri, h, w, c, tex_h, tex_w, tex_c, batch);
    return VP_ERR_ARG;
  }
  if (c > tex_c) {
    vp::set_err("vp_render_texture: c %d > tex_c %d (the reference would read the next texel's channels)", c, tex_c);
    return VP_ERR_ARG;
  }
  if (tex_rows < nver || tex_rows < tex_nver) {
    vp::set_err("vp_render_texture: tex_rows %d < max(nver %d, tex_nver %d) (y is read through the mesh triangle, mesh_core.cpp:270-272)", tex_rows,
                nver, tex_nver);
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const size_t n = (size_t)batch * h * w;
  vp::dense_visibility(vertices, triangles, tex_triangles, depth_buffer, keys, nver, tex_nver, ntri, h, w, batch, st);
  if (ntri > 0)
    hipLaunchKernelGGL(vp::texture_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, vertices, triangles, texture,
                       tex_coords, tex_triangles, image, depth_buffer, nver, h, w, c, tex_h, tex_w, tex_c, mapping_type, batch);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_raster_interpolate(float* out, const int* triangle_buffer, const float* barycentric_weight, const int* triangles, const float* attributes,
                          int nver, int ntri, int k, int h, int w, int batch, void* stream) {
  if (!out || !triangle_buffer || !barycentric_weight || (!triangles && ntri > 0) || !attributes || !vp::dense_sizes_ok(nver, ntri, h, w, batch) ||
      k < 1) {
    vp::set_err("vp_raster_interpolate: bad argument (null pointer, or nver %d, ntri %d, k %d, h %d, w %d, batch %d out of range)", nver, ntri, k, h,
                w, batch);
    return VP_ERR_ARG;
  }
  if (ntri == 0) return VP_OK;                              // no pixel can name a triangle
  const size_t n = (size_t)batch * h * w;
  hipLaunchKernelGGL(vp::interpolate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, triangle_buffer,
                     barycentric_weight, triangles, attributes, nver, ntri, k, (size_t)h * w, batch);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_raster_vertex_visibility(const float* vertices, const float* depth_buffer, unsigned char* visible, int nver, int h, int w, int batch, float tol,
                                void* stream) {
  if (!vertices || !depth_buffer || !visible || !vp::dense_sizes_ok(nver, 0, h, w, batch) || h < 2 || w < 2 || !(tol >= 0.f) || !(tol <= FLT_MAX)) {
    vp::set_err("vp_raster_vertex_visibility: bad argument (null pointer, or nver %d, h %d, w %d, batch %d out of range (h, w >= 2), or tol %g "
                "negative or not finite)", nver, h, w, batch, (double)tol);
    return VP_ERR_ARG;
  }
  hipLaunchKernelGGL(vp::vertex_visibility_kernel, dim3((nver + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, vertices, depth_buffer,
                     visible, nver, h, w, tol);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

size_t vp_vertex_adjacency_bytes(int nver, int ntri) {
  if (nver < 1 || ntri < 0 || nver > INT_MAX / 3 || ntri > INT_MAX / 3) return 0;
  return vp::align256(((size_t)2 * nver + 1 + (size_t)3 * ntri) * sizeof(int));
}

int vp_vertex_adjacency_build(const int* triangles, int nver, int ntri, void* adjacency, size_t adjacency_bytes, void* stream) {
  const size_t need = vp_vertex_adjacency_bytes(nver, ntri);
  if ((!triangles && ntri > 0) || !adjacency || need == 0) {
    vp::set_err("vp_vertex_adjacency_build: bad argument (null pointer, or nver %d, ntri %d out of range)", nver, ntri);
    return VP_ERR_ARG;
  }
  if (adjacency_bytes < need) {
    vp::set_err("vp_vertex_adjacency_build: adjacency of %zu bytes, %zu needed", adjacency_bytes, need);
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* offsets = (int*)adjacency;
  int* entries = offsets + nver + 1;
  int* cursor = entries + (size_t)3 * ntri;
  const int n3 = 3 * ntri;
  VP_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)nver * sizeof(int), st));
  if (ntri > 0) hipLaunchKernelGGL(vp::adjacency_count_kernel, dim3((n3 + 255) / 256), dim3(256), 0, st, triangles, cursor, n3, nver);
  hipLaunchKernelGGL(vp::adjacency_scan_kernel, dim3(1), dim3(1024), 0, st, offsets, cursor, nver);
  if (ntri > 0) {
    hipLaunchKernelGGL(vp::adjacency_fill_kernel, dim3((n3 + 255) / 256), dim3(256), 0, st, triangles, cursor, entries, n3, nver);
    hipLaunchKernelGGL(vp::adjacency_sort_kernel, dim3((nver + 255) / 256), dim3(256), 0, st, offsets, entries, nver);
  }
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_vertex_normals(float* normal, const float* tri_normal, const void* adjacency, int nver, int ntri, int batch, void* stream) {
  if (!normal || (!tri_normal && ntri > 0) || !adjacency || vp_vertex_adjacency_bytes(nver, ntri) == 0 || batch < 1 || batch > 65535) {
    vp::set_err("vp_vertex_normals: bad argument (null pointer, or nver %d, ntri %d, batch %d out of range)", nver, ntri, batch);
    return VP_ERR_ARG;
  }
  if (ntri == 0) return VP_OK;
  const int* offsets = (const int*)adjacency;
  hipLaunchKernelGGL(vp::vertex_normals_kernel, dim3((nver + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, normal, tri_normal, offsets,
                     offsets + nver + 1, nver, ntri);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

// vp_bfmfit_observe_ex: vp_bfmfit_observe (bfm_appear.hip) with two opt-in corrections of what the photo is taken to show at a vertex.
// The geometry, sh, the inside test and the facing weight are bfm_observe_device.h's, the code vp_bfmfit_observe runs; with both options
// off the three outputs are its bits.
//
//   visibility  self-occlusion.  Per frame the mesh is rasterised into a depth buffer of (224 ss)^2 pixels by the dense rasteriser
//               (vp_rasterize_triangles, raster_dense.hip) from float32 vertices (ss x, ss y, z_buffer), (x, y) = face_projection, the
//               products in float64 and then rounded; vp_raster_vertex_visibility compares every vertex with the buffer around it, and
//               weight is multiplied by the 0 / 1 result.  Frames go through the raster buffers in chunks of at most OBS_CHUNK, so the
//               buffers (28 B per pixel, the rasteriser's keys included) do not grow with the clip.
//   prefilter   area mean.  A frame with scale a > 1 reads k x k bilinear taps per vertex, k = min(ceil(a), 16), at
//               (px + ((i + 0.5) / k - 0.5) a, py + ((j + 0.5) / k - 0.5) a), each coordinate clamped to the photo, and returns their mean.
//               `inside` is the centre's.  A wave serves its 64 vertices one after the other with the taps spread over its lanes: tap
//               t = i + k j (i along x) belongs to lane t % 64.  ORDER OF THE SUM: a lane adds its taps in ascending t onto 0; the 64 lane
//               sums are combined by the xor butterfly with strides 32, 16, 8, 4, 2, 1 (lane l adds lane l ^ stride's value to its own);
//               the total is divided by k k.  The order depends on k alone, so a frame's numbers are the same bits in any batch.
//               A frame with a <= 1 (k = 1) takes vp_bfmfit_observe's single tap.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "workspace.h"
#include "bfm_observe_device.h"      // (switches FMA contraction off from here on, through bfm_device.h)

namespace vp {

constexpr int OBS_CHUNK = 8;         // frames rasterised at a time
constexpr int OBS_MAX_K = 16;
constexpr float OBS_DEPTH_CLEAR = -99999.f;       // the clear value of the reference's callers

struct ObserveExArgs {
  ObserveArgs o;
  float* raster_vertices;    // optional [frames,N,3]: (ss x, ss y, z_buffer)
  double raster_scale;
  int prefilter;
};

__device__ __forceinline__ double clamp_coord(double x, double top) { return fmin(fmax(x, 0.0), top); }

// one thread per (frame, vertex) for everything but the k x k taps, which the wave's lanes share (file head)
__global__ __launch_bounds__(256) void bfm_observe_ex_kernel(ObserveExArgs e) {
  const ObserveArgs& a = e.o;
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const bool valid = v < a.nver;
  const size_t fv = (size_t)f * a.nver + (valid ? v : 0);
  const unsigned char* img = observe_image(a, f);
  ObservedVertex ov{};
  double o[3] = {0.0, 0.0, 0.0};
  if (valid) {
    observe_vertex(a, f, v, fv, ov);
    if (e.raster_vertices) {
      float* rv = e.raster_vertices + fv * 3;
      rv[0] = (float)(e.raster_scale * ov.prx); rv[1] = (float)(e.raster_scale * ov.pry); rv[2] = (float)ov.zb;
    }
  }
  const double s = a.affine[f * 3];
  const int k = (e.prefilter && s > 1.0) ? (int)ceil(fmin(s, (double)OBS_MAX_K)) : 1;       // (a NaN scale: 1, and no vertex is inside)
  if (k == 1) {
    if (valid && ov.inside) observe_tap(img, a.height, a.width, ov.px, ov.py, o);
  } else {
    const int taps = k * k;
    const double xtop = (double)(a.width - 1), ytop = (double)(a.height - 1), dk = (double)k;
    unsigned long long todo = __ballot(valid && ov.inside);
    while (todo) {                                         // the same for every lane of the wave
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const double cx = __shfl(ov.px, src), cy = __shfl(ov.py, src);
      double sum[3] = {0.0, 0.0, 0.0};
      for (int t = lane; t < taps; t += 64) {
        const int i = t % k, j = t / k;
        const double tx = clamp_coord(cx + (((double)i + 0.5) / dk - 0.5) * s, xtop);
        const double ty = clamp_coord(cy + (((double)j + 0.5) / dk - 0.5) * s, ytop);
        double q[3];
        observe_tap(img, a.height, a.width, tx, ty, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += q[c];
      }
#pragma unroll
      for (int stride = 32; stride >= 1; stride >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += __shfl_xor(sum[c], stride);
      }
      if (lane == src) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = sum[c] / (double)taps;
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.observed[fv * 3 + c] = o[c];
  a.weight[fv] = observe_weight(a, v, ov);
}

__global__ __launch_bounds__(256) void bfm_observe_mask_kernel(double* __restrict__ weight, const unsigned char* __restrict__ visible, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) weight[i] = weight[i] * (double)visible[i];
}

static bool observe_opts_ok(const vp_bfmfit_observe_opts* o, const char* who) {
  if (!o) { set_err("%s: bad options (null)", who); return false; }
  if ((size_t)o->struct_bytes != sizeof(vp_bfmfit_observe_opts)) {
    set_err("%s: bad options (struct_bytes %u, this library's vp_bfmfit_observe_opts is %d bytes)", who, (unsigned)o->struct_bytes,
            (int)sizeof(vp_bfmfit_observe_opts));
    return false;
  }
  if ((o->visibility != 0 && o->visibility != 1) || (o->prefilter != 0 && o->prefilter != 1)) {
    set_err("%s: bad options (visibility %d, prefilter %d: 0 or 1)", who, o->visibility, o->prefilter);
    return false;
  }
  if (o->raster_scale != 1 && o->raster_scale != 2 && o->raster_scale != 4) {
    set_err("%s: bad options (raster_scale %d: 1, 2 or 4)", who, o->raster_scale);
    return false;
  }
  if (!(o->depth_tol >= 0.f && o->depth_tol <= FLT_MAX)) {
    set_err("%s: bad options (depth_tol %g: finite and >= 0)", who, (double)o->depth_tol);
    return false;
  }
  return true;
}

// the workspace: one block that is linear in frames (whole 256-byte lines per frame), then the raster buffers of a chunk
struct ObserveExSpace {
  double* shape; double* fn; float* raster_vertices; unsigned char* visible;
  float* depth; int* tri_buf; float* bary; void* keys;
};

static size_t observe_ex_carve(ObserveExSpace* s, void* base, int nver, int ntri, int frames, const vp_bfmfit_observe_opts* o) {
  Arena ar(base);
  const size_t shape_b = (size_t)nver * 3 * sizeof(double), fn_b = (size_t)(ntri + 1) * 3 * sizeof(double);
  const size_t rv_b = o->visibility ? (size_t)nver * 3 * sizeof(float) : 0, vis_b = o->visibility ? (size_t)nver : 0;
  char* lin = (char*)ar.alloc((size_t)frames * align256(shape_b + fn_b + rv_b + vis_b));
  s->shape = (double*)lin;                                   // (descending alignment: doubles, floats, bytes)
  s->fn = (double*)(lin + (size_t)frames * shape_b);
  s->raster_vertices = (float*)(lin + (size_t)frames * (shape_b + fn_b));
  s->visible = (unsigned char*)(lin + (size_t)frames * (shape_b + fn_b + rv_b));
  if (o->visibility) {
    const int side = 224 * o->raster_scale;
    const size_t px = (size_t)OBS_CHUNK * side * side;
    s->depth = ar.take<float>(px);
    s->tri_buf = ar.take<int>(px);
    s->bary = ar.take<float>(px * 3);
    s->keys = ar.alloc(vp_rasterize_triangles_workspace_bytes(OBS_CHUNK, side, side));
  }
  return ar.total();
}

}  // namespace vp

extern "C" {

size_t vp_bfmfit_observe_opts_size(void) { return sizeof(vp_bfmfit_observe_opts); }

size_t vp_bfmfit_observe_ex_workspace_bytes(int nver, int ntri, int frames, const vp_bfmfit_observe_opts* o) {
  if (nver < 1 || ntri < 1 || frames < 1 || !vp::observe_opts_ok(o, "vp_bfmfit_observe_ex_workspace_bytes")) return 0;
  vp::ObserveExSpace s{};
  return vp::observe_ex_carve(&s, nullptr, nver, ntri, frames, o);
}

int vp_bfmfit_observe_ex(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, const unsigned char* photo, int photo_frames,
                         int height, int width, const double* affine, const double* vertex_weights, double* sh, double* weight, double* observed,
                         void* workspace, size_t workspace_bytes, void* stream, const vp_bfmfit_observe_opts* o, unsigned char* visible) {
  if (!vp::observe_opts_ok(o, "vp_bfmfit_observe_ex")) return VP_ERR_ARG;
  if (!m || !coeff || !rotation || !photo || !affine || !sh || !weight || !observed || !workspace || frames < 1 || frames > 65535 || m->nver < 1 ||
      m->ntri < 1 ||
      !m->idBase || !m->exBase || !m->meanshape || !m->tri || !m->point_buf) {
    vp::set_err("vp_bfmfit_observe_ex: bad argument (null pointer, or frames outside 1 .. 65535)");
    return VP_ERR_ARG;
  }
  if (height < 2 || width < 2 || (photo_frames != 1 && photo_frames != frames)) {
    vp::set_err("vp_bfmfit_observe_ex: bad argument (photo %d x %d x %d: at least 2 x 2, one photo or one per frame)", photo_frames, height, width);
    return VP_ERR_ARG;
  }
  if (workspace_bytes < vp_bfmfit_observe_ex_workspace_bytes(m->nver, m->ntri, frames, o)) {
    vp::set_err("vp_bfmfit_observe_ex: workspace too small");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  vp::ObserveExSpace s{};
  vp::observe_ex_carve(&s, workspace, m->nver, m->ntri, frames, o);
  vp::bfm_launch_shape(m, coeff, frames, s.shape, st);
  vp::bfm_launch_fnormal(m, s.shape, frames, s.fn, st);
  vp::ObserveExArgs e{};
  vp::ObserveArgs& a = e.o;
  a.shape = s.shape; a.fn = s.fn; a.point_buf = m->point_buf; a.rot = rotation; a.coeff = coeff; a.photo = photo; a.affine = affine;
  a.vertex_weights = vertex_weights; a.sh = sh; a.weight = weight; a.observed = observed;
  a.nver = m->nver; a.ntri = m->ntri; a.photo_frames = photo_frames; a.height = height; a.width = width;
  a.focal = m->focal; a.center = m->image_center;
  for (int i = 0; i < 5; ++i) a.shc[i] = m->sh[i];
  e.raster_vertices = o->visibility ? s.raster_vertices : nullptr;
  e.raster_scale = (double)o->raster_scale;
  e.prefilter = o->prefilter;
  hipLaunchKernelGGL(vp::bfm_observe_ex_kernel, dim3((m->nver + 255) / 256, frames), dim3(256), 0, st, e);
  VP_HIP_CHECK(hipGetLastError());
  if (!o->visibility) return VP_OK;
  const int side = 224 * o->raster_scale;
  unsigned char* vis = visible ? visible : s.visible;
  union { float f; int i; } clear;
  clear.f = vp::OBS_DEPTH_CLEAR;
  for (int f0 = 0; f0 < frames; f0 += vp::OBS_CHUNK) {
    const int n = frames - f0 < vp::OBS_CHUNK ? frames - f0 : vp::OBS_CHUNK;
    const size_t px = (size_t)n * side * side;
    VP_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.depth, clear.i, px, st));
    VP_HIP_CHECK(hipMemsetAsync(s.tri_buf, 0xFF, px * sizeof(int), st));                  // -1
    const float* rv = s.raster_vertices + (size_t)f0 * m->nver * 3;
    if (const int rc = vp_rasterize_triangles(rv, m->tri, s.depth, s.tri_buf, s.bary, m->nver, m->ntri, side, side, n, s.keys, stream)) return rc;
    if (const int rc = vp_raster_vertex_visibility(rv, s.depth, vis + (size_t)f0 * m->nver, m->nver, side, side, n, o->depth_tol, stream)) return rc;
  }
  const size_t nv = (size_t)frames * m->nver;
  hipLaunchKernelGGL(vp::bfm_observe_mask_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, weight, vis, nv);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

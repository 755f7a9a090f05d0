// Fit BFM texture (coefficients 144:224) and lighting (227:254) to a photo's pixels, the geometry fixed at what the landmark fit returned:
// the inverse of face_color = Illumination_layer(Texture_formation(tex), normals . R, gamma) (utils/reconstruct_mesh.py:58-62, :129-168,
// as `Reconstruction` :172-194 calls them) for the colours a photo shows at the projected vertices.  float64 throughout.
//
//   unknowns   p[107] = [delta(80) | gamma(27)];  T_vc = meantex + texBase delta;  L_vc = sum_k Y_vk (gamma_ck + init_k), init = (0.8, 0, ...)
//   cost       E = (1/W) sum_v w_v sum_c (T_vc L_vc - I_vc)^2 + lam_tex |delta|^2 + lam_gamma |gamma|^2,   W = 3 sum_v w_v
//   solver     the Levenberg-Marquardt rule of bfm_fit.hip with a RELATIVE stopping test: |g|_inf <= gtol E (or E = 0) -> status 0
//
//   observe    : shape and face normals by bfm_recon.hip's kernels, then per (frame, vertex): rotated one-ring normal -> Y [9], projection ->
//                photo position (a x + bx, a y + by) -> bilinear sample I [3], weight = vertex_weight max(0, (n . R)_z) inside
//   accumulate : grid (frame, slab, half).  A block owns a slab of vertices (a function of nver alone) and half of the 8 x 8 tiles of the
//                packed 108-row triangle [A | g ; E]: it stages 16-row slices of sqrt(w) [L B | T Y (own channel) | r] in LDS (the next
//                slice's texBase values are in flight meanwhile) and accumulates its tiles in registers, four row quarters per tile,
//                combined in quarter order.  The frame is the fastest grid index: a slab of texBase is read from HBM by the first frame
//                and from L2 / the Infinity Cache by the others.  `half` is the SLOWEST index: texBase is traversed twice per trial,
//                once per half, and each half repeats the staging (T, L, the scaled slice).  That the second pass does not go back to
//                HBM relies on the 68.6 MB basis staying in the 256 MB Infinity Cache between the passes; nothing in the structure
//                guarantees it, and it is measured only on the synthetic BFM-sized model (scripts/bfm_appearance_latency.py).
//                One partial system per (frame, slab): no atomics.
//   reduce     : grid (frame, 23): a frame's partials added in slab order, element by element (the second, fixed-order level)
//   step       : one workgroup per frame applies accept / reject, keeps the accepted system in the
//                workspace, factorises (A + mu diag A) in LDS (fit_device.h's Cholesky) and writes the next trial point.
// A frame with a status set is left alone by both.  Every sum has a fixed order: a frame's results do not depend on the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "workspace.h"
#include "fit_device.h"
#include "bfm_observe_device.h"      // ObserveArgs and the per-vertex steps, shared with bfm_observe.hip (switches FMA contraction off from
                                     // here on, through bfm_device.h: the observation repeats bfm_recon.hip's bits)

namespace vp {

constexpr int AP_NP = 107;          // unknowns
constexpr int AP_ND = 80;           // delta
constexpr int AP_TRI = 108 * 109 / 2;            // 5886: packed lower triangle, row 107 = [g | E]
constexpr int AP_PART = AP_TRI + 2;              // + sum_v w_v, + the non-finite flag
constexpr int AP_COLS = 112;        // 108 padded to 14 tiles of 8
constexpr int AP_SLICE = 16;        // rows per LDS slice
constexpr int AP_TILES = 14 * 15 / 2;            // 105 tiles in the lower triangle
constexpr int AP_HALVES = 2;        // blocks per slab, each with every second tile
constexpr int AP_TPB = (AP_TILES + AP_HALVES - 1) / AP_HALVES;       // 53 tiles per block
constexpr int AP_KQ = 4;            // row quarters per tile: 53 x 4 = 212 of the 256 threads
constexpr int AP_MAX_SLABS = 128;
// per-frame solver state in the workspace (doubles)
constexpr int ST_P = 0, ST_PTRY = 112, ST_E = 224, ST_MU = 225, ST_STATUS = 226, ST_ITERS = 227, ST_GMAX = 228, ST_TRIALS = 229, ST_SYS = 232;
constexpr int AP_STATE = 6120;      // ST_SYS + AP_TRI, rounded up

// vertices per slab: a function of nver alone (at most AP_MAX_SLABS slabs, a multiple of 16 vertices so that a slab is whole slices)
static int ap_slab_verts(int nver) {
  const int per = (nver + AP_MAX_SLABS - 1) / AP_MAX_SLABS;
  const int v = (per + 15) / 16 * 16;
  return v < 64 ? 64 : v;
}
static int ap_slabs(int nver) { const int sv = ap_slab_verts(nver); return (nver + sv - 1) / sv; }

__global__ __launch_bounds__(256) void bfm_appear_observe_kernel(ObserveArgs a) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (v >= a.nver) return;
  const size_t fv = (size_t)f * a.nver + v;
  ObservedVertex ov;
  observe_vertex(a, f, v, fv, ov);
  double o[3] = {0.0, 0.0, 0.0};
  if (ov.inside) observe_tap(observe_image(a, f), a.height, a.width, ov.px, ov.py, o);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.observed[fv * 3 + c] = o[c];
  a.weight[fv] = observe_weight(a, v, ov);
}

struct InitArgs {
  double* state; const float* coeff_in; const double* params; int params_in; int frames;
};

__global__ __launch_bounds__(128) void bfm_appear_init_kernel(InitArgs a) {
  const int f = blockIdx.x, t = threadIdx.x;
  double* S = a.state + (size_t)f * AP_STATE;
  if (t < AP_NP) {
    const float* C = a.coeff_in + (size_t)f * 257;
    const double v = a.params_in ? a.params[(size_t)f * AP_NP + t] : (double)(t < AP_ND ? C[144 + t] : C[227 + (t - AP_ND)]);
    S[ST_P + t] = v;
    S[ST_PTRY + t] = v;
  }
  if (t == 0) {
    S[ST_E] = 0.0; S[ST_MU] = 1e-3; S[ST_STATUS] = -1.0; S[ST_ITERS] = 0.0; S[ST_GMAX] = 0.0; S[ST_TRIALS] = 0.0;
  }
}

struct AccumArgs {
  const double* texBase;     // [80][3N] k-major
  const double* meantex;     // [3N]
  const double* sh;          // [frames,N,9]
  const double* weight;      // [frames,N]
  const double* observed;    // [frames,N,3]
  const double* state;       // [frames,AP_STATE]
  double* part;              // [frames,slabs,AP_PART]
  int nver, slabs, slab_verts;
};

__global__ __launch_bounds__(FIT_THREADS) void bfm_appear_accum_kernel(AccumArgs a) {
  __shared__ double U[AP_SLICE * AP_COLS];         // the slice: sqrt(w) [L B (80) | T Y of the row's channel (27) | r | 0 0 0 0]
  __shared__ double raw[AP_ND * AP_SLICE];         // texBase of the slice, [col][row]
  __shared__ double tpart[16 * AP_SLICE];          // partial sums of B delta, [part][row]
  __shared__ double swl[AP_SLICE];                 // sqrt(w) L per row
  __shared__ double pv[AP_COLS];                   // the trial point
  __shared__ double comb[64 * AP_TPB];             // one row quarter's tiles, [element][tile]
  __shared__ double red[32];
  const int t = threadIdx.x, f = blockIdx.x, slab = blockIdx.y, half = blockIdx.z;
  const double* S = a.state + (size_t)f * AP_STATE;
  if (S[ST_STATUS] >= 0.0) return;                 // a finished frame (the same value for every thread)
  if (t < AP_COLS) pv[t] = t < AP_NP ? S[ST_PTRY + t] : 0.0;
  const int tl = t % AP_TPB, kq = t / AP_TPB, tile = half + AP_HALVES * tl;
  const bool active = kq < AP_KQ && tile < AP_TILES;
  int bi = 0, bj = 0;
  if (active) {
    while ((bi + 1) * (bi + 2) / 2 <= tile && bi < 13) ++bi;
    bj = tile - bi * (bi + 1) / 2;
  }
  double acc[8][8];
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int y = 0; y < 8; ++y) acc[x][y] = 0.0;

  const int rows3 = 3 * a.nver;
  const int row_begin = 3 * slab * a.slab_verts;
  const int row_end = min(row_begin + 3 * a.slab_verts, rows3);
  const int nslices = (row_end - row_begin + AP_SLICE - 1) / AP_SLICE;
  // element e = t + 256 i of a slice: row e % 16 (fastest: 128-byte runs of one basis vector), column e / 16
  auto load_slice = [&](int r0, double* nb) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int e = t + FIT_THREADS * i, row = r0 + (e & 15), col = e >> 4;
      nb[i] = row < row_end ? a.texBase[(size_t)col * rows3 + row] : 0.0;
    }
  };
  double nb[5];
  load_slice(row_begin, nb);
#pragma unroll
  for (int i = 0; i < 5; ++i) raw[t + FIT_THREADS * i] = nb[i];
  double wsum = 0.0, bad = 0.0;
  __syncthreads();
  for (int s = 0; s < nslices; ++s) {
    const int r0 = row_begin + s * AP_SLICE;
    {                                               // B delta: 16 partial sums of 5 terms per row
      const int row = t & 15, prt = t >> 4;
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < 5; ++j) sum = fma(raw[(prt * 5 + j) * AP_SLICE + row], pv[prt * 5 + j], sum);
      tpart[prt * AP_SLICE + row] = sum;
    }
    __syncthreads();
    if (t < AP_SLICE) {                             // per row: T, L, r and the 28 columns behind the texture block
      const int row = r0 + t;
      double* u = U + t * AP_COLS;
      double sl = 0.0, st = 0.0, sr = 0.0;
      int c = 0;
      double Y[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (row < row_end) {
        const int v = row / 3;
        c = row - 3 * v;
        const size_t fv = (size_t)f * a.nver + v;
        double bsum = 0.0;
        for (int q = 0; q < 16; ++q) bsum += tpart[q * AP_SLICE + t];
        const double T = a.meantex[row] + bsum;
        const double wraw = a.weight[fv], obs = a.observed[fv * 3 + c];
        if (!isfinite(wraw) || !isfinite(obs)) bad = 1.0;
        double L = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          Y[k] = a.sh[fv * 9 + k];
          if (!isfinite(Y[k])) bad = 1.0;
          L += Y[k] * (pv[AP_ND + 9 * c + k] + (k == 0 ? 0.8 : 0.0));
        }
        const double w = wraw > 0.0 ? wraw : 0.0;     // (a negative weight drops the vertex)
        if (c == 0) wsum += w;
        if (w > 0.0) {
          const double sw = sqrt(w);
          sl = sw * L; st = sw * T; sr = sw * (T * L - obs);
        }
      }
      swl[t] = sl;
#pragma unroll
      for (int j = 0; j < 27; ++j) u[AP_ND + j] = (j / 9 == c) ? st * Y[j % 9] : 0.0;
      u[107] = sr;
      u[108] = u[109] = u[110] = u[111] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int e = t + FIT_THREADS * i, row = e & 15, col = e >> 4;
      U[row * AP_COLS + col] = swl[row] * raw[e];
    }
    __syncthreads();
    if (s + 1 < nslices) load_slice(r0 + AP_SLICE, nb);      // in flight during the products below
    if (active) {
#pragma unroll
      for (int rr = 0; rr < AP_SLICE / AP_KQ; ++rr) {
        const double* u = U + (kq * (AP_SLICE / AP_KQ) + rr) * AP_COLS;
        double av[8], bv[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) { av[x] = u[8 * bi + x]; bv[x] = u[8 * bj + x]; }
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < 8; ++y) acc[x][y] = fma(av[x], bv[y], acc[x][y]);
      }
    }
    __syncthreads();
    if (s + 1 < nslices) {
#pragma unroll
      for (int i = 0; i < 5; ++i) raw[t + FIT_THREADS * i] = nb[i];
    }
    __syncthreads();
  }
  double* part = a.part + ((size_t)f * a.slabs + slab) * AP_PART;
  // the four row quarters of a tile, added in quarter order
  for (int q = 1; q < AP_KQ; ++q) {
    __syncthreads();
    if (active && kq == q) {
#pragma unroll
      for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) comb[(x * 8 + y) * AP_TPB + tl] = acc[x][y];
    }
    __syncthreads();
    if (active && kq == 0) {
#pragma unroll
      for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) acc[x][y] += comb[(x * 8 + y) * AP_TPB + tl];
    }
  }
  if (active && kq == 0) {
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        const int i = 8 * bi + x, j = 8 * bj + y;
        if (i < 108 && j <= i) part[tri_idx(i, j)] = acc[x][y];
      }
  }
  if (t < AP_SLICE) { red[t] = wsum; red[16 + t] = bad; }
  __syncthreads();
  if (t == 0 && half == 0) {
    double ws = 0.0, bd = 0.0;
    for (int i = 0; i < AP_SLICE; ++i) { ws += red[i]; bd += red[16 + i]; }
    part[AP_TRI] = ws;
    part[AP_TRI + 1] = bd;
  }
}

// second level of the fixed-order sum: element e of a frame's system = its slabs' partials added in slab order (many blocks per frame: one
// workgroup alone would take 0.4 ms to pull the 5.9 MB of a BFM-sized frame's partials through its CU)
__global__ __launch_bounds__(FIT_THREADS) void bfm_appear_reduce_kernel(const double* __restrict__ state, const double* __restrict__ part,
                                                                        double* __restrict__ sum, int slabs) {
  const int f = blockIdx.x, e = blockIdx.y * FIT_THREADS + threadIdx.x;
  if (state[(size_t)f * AP_STATE + ST_STATUS] >= 0.0 || e >= AP_PART) return;
  const double* P = part + (size_t)f * slabs * AP_PART + e;
  double s = 0.0;
  for (int sl = 0; sl < slabs; ++sl) s += P[(size_t)sl * AP_PART];
  sum[(size_t)f * AP_PART + e] = s;
}

struct StepArgs {
  double* state; const double* sum;      // sum [frames,AP_PART]: the reduced systems
  int max_trials;
  double lam_tex, lam_gamma, gtol;
  const float* coeff_in; float* coeff; double* report; double* params;
};

__global__ __launch_bounds__(FIT_THREADS) void bfm_appear_step_kernel(StepArgs a) {
  extern __shared__ double lds[];
  double* sys = lds;                    // [AP_PART] the system of the accepted point: A + Lambda, row 107 = [g | E of the data]
  double* wrk = sys + AP_PART;          // [AP_PART] the damped copy the factorisation works in
  double* p = wrk + AP_PART;            // [112] accepted point
  double* pt = p + AP_COLS;             // [112] trial point
  double* d = pt + AP_COLS;             // [112]
  double* piv = d + AP_COLS;            // [112]
  double* red = piv + AP_COLS;          // [256]
  const int t = threadIdx.x, f = blockIdx.x;
  double* S = a.state + (size_t)f * AP_STATE;
  if (S[ST_STATUS] >= 0.0) return;
  const int trials = (int)S[ST_TRIALS];
  const bool first = trials == 0;
  const double* P = a.sum + (size_t)f * AP_PART;
  for (int e = t; e < AP_PART; e += FIT_THREADS) sys[e] = P[e];
  if (t < AP_COLS) { p[t] = t < AP_NP ? S[ST_P + t] : 0.0; pt[t] = t < AP_NP ? S[ST_PTRY + t] : 0.0; }
  __syncthreads();
  const double wsum = sys[AP_TRI], badin = sys[AP_TRI + 1];
  const double lam = t < AP_ND ? a.lam_tex : a.lam_gamma;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double mu = S[ST_MU], E = S[ST_E], gmax = S[ST_GMAX];
  int iters = (int)S[ST_ITERS], status = -1;
  const double W = 3.0 * wsum;
  __syncthreads();
  for (int e = t; e < AP_TRI; e += FIT_THREADS) sys[e] = sys[e] / W;
  const double pbad = block_sum((t < AP_NP && !isfinite(pt[t])) ? 1.0 : 0.0, red);
  const double reg = block_sum(t < AP_NP ? lam * pt[t] * pt[t] : 0.0, red);
  const double Et = sys[tri_idx(AP_NP, AP_NP)] + reg;
  if (first && (badin != 0.0 || !(wsum > 0.0) || pbad != 0.0 || !isfinite(Et))) {      // status 3: the start values go back
    float* out = a.coeff + (size_t)f * 257;
    const float* in = a.coeff_in + (size_t)f * 257;
    for (int i = t; i < 257; i += FIT_THREADS) out[i] = in[i];
    if (a.params && t < AP_NP) a.params[(size_t)f * AP_NP + t] = pt[t];
    if (t == 0) {
      double* r = a.report + (size_t)f * 4;
      r[0] = 3.0; r[1] = 0.0; r[2] = nan; r[3] = nan;
      S[ST_STATUS] = 3.0;
    }
    return;
  }
  const bool accept = first || Et < E;              // false for a non-finite cost
  if (accept) {
    __syncthreads();
    if (t < AP_NP) {
      p[t] = pt[t];
      sys[tri_idx(t, t)] += lam;
      sys[tri_idx(AP_NP, t)] += lam * pt[t];
    }
    __syncthreads();
    E = Et;
    if (!first) { mu = fmax(mu / 3.0, 1e-9); ++iters; }
    gmax = block_max(t < AP_NP ? fabs(sys[tri_idx(AP_NP, t)]) : 0.0, red);
    for (int e = t; e < AP_TRI; e += FIT_THREADS) S[ST_SYS + e] = sys[e];
    if (gmax <= a.gtol * E || E == 0.0) status = 0;
  } else {
    __syncthreads();
    for (int e = t; e < AP_TRI; e += FIT_THREADS) sys[e] = S[ST_SYS + e];
    mu *= 4.0;
    if (mu > 1e8) status = 2;
  }
  if (status < 0 && trials + 1 >= a.max_trials) status = 1;
  if (status < 0) {
    for (;;) {                                        // at most 29 rounds: mu grows from >= 1e-9 by 4 to 1e8
      __syncthreads();
      for (int e = t; e < AP_TRI; e += FIT_THREADS) wrk[e] = sys[e];
      __syncthreads();
      if (t < AP_NP) {
        const double a_tt = sys[tri_idx(t, t)];
        wrk[tri_idx(t, t)] = a_tt + mu * a_tt;
        wrk[tri_idx(AP_NP, t)] = -sys[tri_idx(AP_NP, t)];
      }
      bool ok = chol_solve(wrk, piv, d, AP_NP);
      if (ok) ok = block_sum((t < AP_NP && !isfinite(p[t] + d[t])) ? 1.0 : 0.0, red) == 0.0;
      if (ok) {
        if (t < AP_NP) pt[t] = p[t] + d[t];
        break;
      }
      mu *= 4.0;                                      // no factorisation: as a rejected trial, without an evaluation
      if (mu > 1e8) { status = 2; break; }
    }
  }
  __syncthreads();
  if (t < AP_NP) { S[ST_P + t] = p[t]; S[ST_PTRY + t] = pt[t]; }
  if (t == 0) {
    S[ST_E] = E; S[ST_MU] = mu; S[ST_STATUS] = (double)status; S[ST_ITERS] = (double)iters; S[ST_GMAX] = gmax; S[ST_TRIALS] = (double)(trials + 1);
    double* r = a.report + (size_t)f * 4;
    r[0] = (double)status; r[1] = (double)iters; r[2] = E; r[3] = gmax;
  }
  float* out = a.coeff + (size_t)f * 257;
  const float* in = a.coeff_in + (size_t)f * 257;
  for (int i = t; i < 257; i += FIT_THREADS) {
    out[i] = (i >= 144 && i < 224) ? (float)p[i - 144] : (i >= 227 && i < 254) ? (float)p[AP_ND + i - 227] : in[i];
  }
  if (a.params && t < AP_NP) a.params[(size_t)f * AP_NP + t] = p[t];
}

constexpr size_t AP_STEP_LDS_BYTES = (size_t)(2 * AP_PART + 4 * AP_COLS + FIT_THREADS) * sizeof(double);

}  // namespace vp

extern "C" {

size_t vp_bfmfit_observe_workspace_bytes(int nver, int ntri, int frames) {
  if (nver < 1 || ntri < 1 || frames < 1) return 0;
  return ((size_t)frames * nver * 3 + (size_t)frames * (ntri + 1) * 3) * sizeof(double) + 512;
}

int vp_bfmfit_observe(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, const unsigned char* photo, int photo_frames,
                      int height, int width, const double* affine, const double* vertex_weights, double* sh, double* weight, double* observed,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !coeff || !rotation || !photo || !affine || !sh || !weight || !observed || !workspace || frames < 1 || frames > 65535 || m->nver < 1 ||
      m->ntri < 1 ||
      !m->idBase || !m->exBase || !m->meanshape || !m->tri || !m->point_buf) {
    vp::set_err("vp_bfmfit_observe: bad argument (null pointer, or frames outside 1 .. 65535)");
    return VP_ERR_ARG;
  }
  if (height < 2 || width < 2 || (photo_frames != 1 && photo_frames != frames)) {
    vp::set_err("vp_bfmfit_observe: bad argument (photo %d x %d x %d: at least 2 x 2, one photo or one per frame)", photo_frames, height, width);
    return VP_ERR_ARG;
  }
  if (workspace_bytes < vp_bfmfit_observe_workspace_bytes(m->nver, m->ntri, frames)) {
    vp::set_err("vp_bfmfit_observe: workspace too small");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double* shape = vp::align256((double*)workspace);
  double* fn = shape + (size_t)frames * m->nver * 3;
  vp::bfm_launch_shape(m, coeff, frames, shape, st);
  vp::bfm_launch_fnormal(m, shape, frames, fn, st);
  vp::ObserveArgs a{};
  a.shape = shape; a.fn = fn; a.point_buf = m->point_buf; a.rot = rotation; a.coeff = coeff; a.photo = photo; a.affine = affine;
  a.vertex_weights = vertex_weights; a.sh = sh; a.weight = weight; a.observed = observed;
  a.nver = m->nver; a.ntri = m->ntri; a.photo_frames = photo_frames; a.height = height; a.width = width;
  a.focal = m->focal; a.center = m->image_center;
  for (int i = 0; i < 5; ++i) a.shc[i] = m->sh[i];
  hipLaunchKernelGGL(vp::bfm_appear_observe_kernel, dim3((m->nver + 255) / 256, frames), dim3(256), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

size_t vp_bfmfit_appearance_workspace_bytes(int nver, int frames) {
  if (nver < 1 || frames < 1) return 0;
  return ((size_t)frames * vp::AP_STATE + (size_t)frames * (vp::ap_slabs(nver) + 1) * vp::AP_PART) * sizeof(double) + 512;
}

int vp_bfmfit_appearance(const vp_bfm_model* m, const double* sh, const double* weight, const double* observed, const float* coeff_in, double* params,
                         int params_in, int frames, double lam_tex, double lam_gamma, double gtol, int max_trials, int stages, float* coeff,
                         double* report, void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !sh || !weight || !observed || !coeff_in || !coeff || !report || !workspace || frames < 1 || frames > 65535 || m->nver < 1 ||
      !m->texBase || !m->meantex || (params_in && !params)) {
    vp::set_err("vp_bfmfit_appearance: bad argument");
    return VP_ERR_ARG;
  }
  if (!(lam_tex >= 0.0 && lam_tex <= 1e12) || !(lam_gamma >= 0.0 && lam_gamma <= 1e12) || !(gtol >= 0.0) || max_trials < 1 || max_trials > 100000 ||
      stages < 1 || stages > 3) {
    vp::set_err("vp_bfmfit_appearance: bad argument (0 <= lam <= 1e12; gtol >= 0; 1 <= max_trials <= 100000; stages 1 .. 3)");
    return VP_ERR_ARG;
  }
  if (workspace_bytes < vp_bfmfit_appearance_workspace_bytes(m->nver, frames)) {
    vp::set_err("vp_bfmfit_appearance: workspace too small");
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)vp::bfm_appear_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vp::AP_STEP_LDS_BYTES);
    attr_done = true;
  }
  const int slabs = vp::ap_slabs(m->nver);
  double* state = vp::align256((double*)workspace);
  double* sum = state + (size_t)frames * vp::AP_STATE;
  double* part = sum + (size_t)frames * vp::AP_PART;
  vp::InitArgs ia{state, coeff_in, params, params_in ? 1 : 0, frames};
  hipLaunchKernelGGL(vp::bfm_appear_init_kernel, dim3(frames), dim3(128), 0, st, ia);
  vp::AccumArgs aa{};
  aa.texBase = m->texBase; aa.meantex = m->meantex; aa.sh = sh; aa.weight = weight; aa.observed = observed; aa.state = state; aa.part = part;
  aa.nver = m->nver; aa.slabs = slabs; aa.slab_verts = vp::ap_slab_verts(m->nver);
  vp::StepArgs sa{};
  sa.state = state; sa.sum = sum; sa.max_trials = max_trials; sa.lam_tex = lam_tex; sa.lam_gamma = lam_gamma; sa.gtol = gtol;
  sa.coeff_in = coeff_in; sa.coeff = coeff; sa.report = report; sa.params = params;
  for (int k = 0; k < max_trials; ++k) {
    if (stages & 1) {
      hipLaunchKernelGGL(vp::bfm_appear_accum_kernel, dim3(frames, slabs, vp::AP_HALVES), dim3(vp::FIT_THREADS), 0, st, aa);
      hipLaunchKernelGGL(vp::bfm_appear_reduce_kernel, dim3(frames, (vp::AP_PART + vp::FIT_THREADS - 1) / vp::FIT_THREADS), dim3(vp::FIT_THREADS), 0,
                         st, state, part, sum, slabs);
    }
    if (stages & 2) hipLaunchKernelGGL(vp::bfm_appear_step_kernel, dim3(frames), dim3(vp::FIT_THREADS), vp::AP_STEP_LDS_BYTES, st, sa);
  }
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

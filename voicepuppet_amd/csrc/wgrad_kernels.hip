// Weight-gradient kernels for gfx950 (MI355X), the register-transposing form (wgrad_tr.hip / wgrad_mm.hip: the LDS-DMA forms).
//   wgrad_kernel       bwd-weight: K = pixels (the strided NHWC dim): register loader + 8x8 transposes into LDS planes (plane_device.h),
//                      division-free padded-grid K walk, split-K slabs + deterministic reduces
//   wgrad_reduce_kernel, wgrad_reduce_wave_kernel
#include "conv_prof.h"
#include "igemm_device.h"
#include "launch.h"
#include "plane_device.h"
#include "vp_common.h"

namespace vp {

// ------------------------------------------------------------------------------------------------
// wgrad_kernel: grid = (M tiles over (tap, g), N tiles over d, splitk over pixels)
//   A operand rows = (tap, g channel) of the gathered tensor, B operand cols = d channel of the
//   dense tensor, K = pixels.  A loader task = E consecutive pixels x E consecutive channels,
//   transposed in registers into E 16-byte pieces "one channel, E consecutive pixels".
// ------------------------------------------------------------------------------------------------
template <typename T> struct Transposer;
template <> struct Transposer<float> {
  __device__ static __forceinline__ void run(const uint4 (&in)[4], uint4 (&out)[4]) {
    out[0] = make_uint4(in[0].x, in[1].x, in[2].x, in[3].x);
    out[1] = make_uint4(in[0].y, in[1].y, in[2].y, in[3].y);
    out[2] = make_uint4(in[0].z, in[1].z, in[2].z, in[3].z);
    out[3] = make_uint4(in[0].w, in[1].w, in[2].w, in[3].w);
  }
};
template <> struct Transposer<bf16> {
  // in[p] = 8 channels of pixel p (dword d = channels 2d, 2d+1); out[c] = 8 pixels of channel c
  __device__ static __forceinline__ uint32_t lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
  __device__ static __forceinline__ uint32_t hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
  __device__ static __forceinline__ void run(const uint4 (&in)[8], uint4 (&out)[8]) {
#define VP_TR(dw, c0)                                                                                 \
    out[c0]     = make_uint4(lo(in[0].dw, in[1].dw), lo(in[2].dw, in[3].dw), lo(in[4].dw, in[5].dw), lo(in[6].dw, in[7].dw)); \
    out[c0 + 1] = make_uint4(hi(in[0].dw, in[1].dw), hi(in[2].dw, in[3].dw), hi(in[4].dw, in[5].dw), hi(in[6].dw, in[7].dw));
    VP_TR(x, 0) VP_TR(y, 2) VP_TR(z, 4) VP_TR(w, 6)
#undef VP_TR
  }
};

// One loader task: E consecutive pixels x E consecutive channels of ONE source tensor, fixed for the whole
// K loop (which tensor, which channels, which tap); only the pixel window moves.
template <typename T> struct WgTask {
  const T* base;      // source pointer + channel offset (plain path)
  int C;              // channels of that source (pixel stride)
  int s, dh, dw;      // source pixel = (q*s + dh, r*s + dw)
  int Hs, Ws;
  int ch;             // channel index inside the PixSrc (prologue path)
  bool ok;
};

template <typename T, int E, int KCH, bool PLAIN>
__device__ __forceinline__ void wg_stage_load(const WgradArgs& a, const WgTask<T>& t, const PixSrc& src, int it, int kq, int P,
                                              uint4 (&rin)[E]) {
  constexpr int KC = 4 * E;
  int pidx = it * (KC * KCH) + kq * E;
  const int hw = a.Hb * a.Wb;
  int n = pidx / hw;
  const int rem = pidx - n * hw;
  int q = rem / a.Wb;
  int r = rem - q * a.Wb;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int ih = q * t.s + t.dh, iw = r * t.s + t.dw;
    const bool ok = t.ok && (pidx + e < P);
    if (PLAIN) {
      const bool inb = ok && (unsigned)ih < (unsigned)t.Hs && (unsigned)iw < (unsigned)t.Ws;
      const T* p = t.base + ((size_t)(n * t.Hs + ih) * t.Ws + iw) * t.C;
      typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
      const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)(inb ? (const void*)p : a.zeros);
      rin[e] = make_uint4(v.x, v.y, v.z, v.w);    // unconditional global load: all E loads stay in flight
    } else {
      rin[e] = load_pix_piece<T>(src, n, ih, iw, t.Hs, t.Ws, t.ch, ok);
    }
    const bool wrap = (r + 1 == a.Wb);
    r = wrap ? 0 : r + 1;
    const bool wrap2 = wrap && (q + 1 == a.Hb);
    q = wrap ? (wrap2 ? 0 : q + 1) : q;
    n += wrap2 ? 1 : 0;
  }
}

// Padded-grid K walk (a.fastw): K runs over slots of the grid [N][2^lh][2^lw] (Hb, Wb rounded up to powers of two), SL slots per
// iteration, so a slot's (n, q, r) are bit fields of its index - no divisions - and, because 2^lw divides SL, the column r of each of a
// thread's E pixels never changes: column validity and the column part of the address are computed ONCE (WgFix); an iteration only
// adds its row offset.  Slots outside the real grid, and padding taps, load the zero page.
template <int E> struct WgFix {
  int coff[E];        // (r*s + dw) * C for the thread's E pixels (element offset inside a row), valid columns only
  unsigned okmask;    // bit e: column r < Wb and r*s + dw inside [0, Ws)
  int fq, fn;         // fixed (low) part of the row / image index of the thread's pixel group
};

template <typename T, int E, int SL>
__device__ __forceinline__ void wg_fix_init(const WgradArgs& a, const WgTask<T>& t, int kq, WgFix<E>& f) {
  const int mw = (1 << a.lw) - 1, mh = (1 << a.lh) - 1;
  const int l0 = kq * E;                         // slot inside the iteration; 2^lw >= E: the E pixels share one row
  f.fq = (l0 >> a.lw) & mh;
  f.fn = l0 >> (a.lw + a.lh);
  f.okmask = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int r = (l0 + e) & mw;
    const int iw = r * t.s + t.dw;
    const bool ok = r < a.Wb && (unsigned)iw < (unsigned)t.Ws;
    f.coff[e] = ok ? iw * t.C : 0;
    f.okmask |= ok ? (1u << e) : 0u;
  }
}

template <typename T, int E, int SL>
__device__ __forceinline__ void wg_stage_load_fast(const WgradArgs& a, const WgTask<T>& t, const WgFix<E>& f, int it, uint4 (&rin)[E]) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  // uniform part of the slot index: it * SL supplies the high bits of (q, n); the thread's fixed low bits add without carries
  const int hi = it * SL;
  const int q = ((hi >> a.lw) & ((1 << a.lh) - 1)) + f.fq;
  const int n = (hi >> (a.lw + a.lh)) + f.fn;
  const int ih = q * t.s + t.dh;
  const bool rowok = t.ok && n < a.N && q < a.Hb && (unsigned)ih < (unsigned)t.Hs;
  const int rowoff = (n * t.Hs + ih) * t.Ws * t.C;          // elements; every tensor here is far below 2^31 elements
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const bool ok = rowok && ((f.okmask >> e) & 1u);
    const T* p = t.base + (rowoff + f.coff[e]);
    const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)(ok ? (const void*)p : a.zeros);
    rin[e] = make_uint4(v.x, v.y, v.z, v.w);
  }
}

template <typename T, int WC, int WP, int TC, int TP, int KCH, bool PLAIN>
__global__ __launch_bounds__(WC * WP * 64) void wgrad_kernel(const WgradArgs a) {
  constexpr int NT = WC * WP * 64;                    // 4 waves, or 8 for the 256-row tiles
  constexpr int E = Elem<T>::E, KC = 4 * E;           // KC pixels per 64-byte chunk; KCH chunks per iteration
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16;
  constexpr int CH = 4 * (BC + BP);                   // slots of one chunk (A planes then B planes)
  constexpr int BUF = KCH * CH;
  constexpr int TA = KCH * 4 * BC / E, TB = KCH * 4 * BP / E;   // loader tasks per iteration
  static_assert(TA + TB <= NT, "one task per thread");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m_base = blockIdx.x * BC, d_base = blockIdx.y * BP, split = blockIdx.z;
  const int P = a.N * a.Hb * a.Wb;
  const bool fastw = PLAIN && a.fastw;
  const int Pk = fastw ? (a.N << (a.lw + a.lh)) : P;    // K extent: padded slots or real pixels
  const int niter = (Pk + KC * KCH - 1) / (KC * KCH);
  const int per = (niter + a.splitk - 1) / a.splitk;
  const int it0 = split * per, it1 = min(niter, it0 + per);

  // this thread's loader task (A: gathered operand rows (tap, channel); B: dense operand channels)
  const bool isA = tid < TA;
  const bool active = tid < TA + TB;
  const int tt = isA ? tid : tid - TA;
  const int ncg = (isA ? BC : BP) / E;
  const int cg = tt % ncg, kq = tt / ncg;    // channel group, pixel group (kq / 4 = chunk, kq % 4 = plane)
  WgTask<T> task;
  {
    int ch, tap = 0;
    if (isA) { const int m = m_base + cg * E; tap = m >> a.log2Gc; ch = m & a.gc_mask; task.ok = m < a.ntaps * a.Gc; }   // (1 tap: log2Gc = 30, any channel count)
    else { ch = d_base + cg * E; task.ok = ch < a.Dc; }
    task.ok = task.ok && active;
    int tdh = 0, tdw = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) if (t == tap) { tdh = a.taps.dh[t]; tdw = a.taps.dw[t]; }
    task.s = isA ? a.s : 1; task.dh = isA ? tdh : 0; task.dw = isA ? tdw : 0;
    task.Hs = isA ? a.Hgin : a.Hb; task.Ws = isA ? a.Wgin : a.Wb;
    task.ch = ch;
    const int c0 = isA ? a.g.C[0] : a.d.C[0];
    const int c1 = isA ? a.g.C[1] : a.d.C[1];
    const void* p0 = isA ? a.g.ptr[0] : a.d.ptr[0];
    const void* p1 = isA ? a.g.ptr[1] : a.d.ptr[1];
    const bool second = ch >= c0;
    task.C = second ? c1 : c0;
    task.base = reinterpret_cast<const T*>(second ? p1 : p0) + (second ? ch - c0 : ch);
    if (!task.ok) { task.base = reinterpret_cast<const T*>(a.zeros); task.C = 0; }
  }
  const PixSrc& psrc = isA ? a.g : a.d;
  WgFix<E> fix;
  if (fastw) wg_fix_init<T, E, KC * KCH>(a, task, kq, fix);
  auto stage_load = [&](int it, uint4 (&rin)[E]) {
    if (PLAIN && fastw) wg_stage_load_fast<T, E, KC * KCH>(a, task, fix, it, rin);
    else wg_stage_load<T, E, KCH, PLAIN>(a, task, psrc, it, kq, P, rin);
  };

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 rin[E], rout[E];
  const int wc = wave / WP, wpi = wave - wc * WP;
  const int rowA0 = wc * TC * 16, rowB0 = wpi * TP * 16;
  const int store_off = (kq >> 2) * CH + (isA ? 0 : 4 * BC) + (kq & 3) * (isA ? BC : BP);

  if (it0 < it1) {
    stage_load(it0, rin);
    Transposer<T>::run(rin, rout);
    if (active) {
#pragma unroll
      for (int e = 0; e < E; ++e) lds[store_off + lds_slot<1, E>(cg * E + e)] = rout[e];
    }
    __syncthreads();
    for (int it = it0; it < it1; ++it) {
      const int buf = (it - it0) & 1;
      const bool more = it + 1 < it1;
      if (more) stage_load(it + 1, rin);
#pragma unroll
      for (int c = 0; c < KCH; ++c) {
        const uint4* la = lds + buf * BUF + c * CH;
        mma_chunk<T, TC, TP, BC, BP, 1>(la, la + 4 * BC, rowA0, rowB0, lane, acc);
      }
      if (more) {
        Transposer<T>::run(rin, rout);
        if (active) {
          uint4* dst = lds + (buf ^ 1) * BUF + store_off;
#pragma unroll
          for (int e = 0; e < E; ++e) dst[lds_slot<1, E>(cg * E + e)] = rout[e];
        }
      }
      __syncthreads();
    }
  }

  // lane holds d column (lane&15), rows 4*(lane>>4) .. +3
  if (a.splitk == 1) {   // no K split: write the gradient itself (real taps / channels only), no slab, no reduce pass
#pragma unroll
    for (int tc = 0; tc < TC; ++tc)
#pragma unroll
      for (int tp = 0; tp < TP; ++tp) {
        const int m0 = m_base + rowA0 + tc * 16 + 4 * (lane >> 4);
        const int d = d_base + rowB0 + tp * 16 + (lane & 15);
        if (d >= a.Dreal) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + e, tap = m >> a.log2Gc, gc = m & a.gc_mask;
          if (tap < a.ntaps && gc < a.Greal) {
            float* o = a.dW + ((size_t)tap * a.Greal + gc) * a.Dreal + d;
            *o = acc[tc][tp][e] + (a.accumulate ? *o : 0.f);
          }
        }
      }
    return;
  }
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp) {
      const int m0 = m_base + rowA0 + tc * 16 + 4 * (lane >> 4);
      const int d = d_base + rowB0 + tp * 16 + (lane & 15);
      float* pp = a.partial + ((size_t)split * a.Mpad + m0) * a.Dpad + d;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(size_t)e * a.Dpad] = acc[tc][tp][e];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradArgs a) {
  if ((a.Dreal & 3) == 0) {   // 16-byte path
    const int dq = a.Dreal >> 2;
    const size_t total = (size_t)a.ntaps * a.Greal * dq;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
      const int d = (int)(i % dq) * 4;
      const size_t t = i / dq;
      const int gc = (int)(t % a.Greal);
      const int tap = (int)(t / a.Greal);
      const size_t m = (size_t)tap * a.Gc + gc;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      // slabs added in slab order, eight loads in flight (the slabs of one element lie Mpad * Dpad floats apart: load latency)
      const float* src = a.partial + m * a.Dpad + d;
      const size_t sstride = (size_t)a.Mpad * a.Dpad;
      for (int k0 = 0; k0 < a.splitk; k0 += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = k0 + u < a.splitk ? *reinterpret_cast<const float4*>(src + (size_t)(k0 + u) * sstride) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (k0 + u >= a.splitk) break;
          s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
        }
      }
      float4* o = reinterpret_cast<float4*>(a.dW + (t * a.Dreal + d));
      if (a.accumulate) { const float4 e = *o; s.x += e.x; s.y += e.y; s.z += e.z; s.w += e.w; }
      *o = s;
    }
    return;
  }
  const size_t total = (size_t)a.ntaps * a.Greal * a.Dreal;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int d = (int)(i % a.Dreal);
    const size_t t = i / a.Dreal;
    const int gc = (int)(t % a.Greal);
    const int tap = (int)(t / a.Greal);
    const size_t m = (size_t)tap * a.Gc + gc;
    float s = 0.f;
    for (int k = 0; k < a.splitk; ++k) s += a.partial[((size_t)k * a.Mpad + m) * a.Dpad + d];
    if (a.accumulate) s += a.dW[i];
    a.dW[i] = s;
  }
}

// many splits, few outputs (the 3/6/4/1-channel layers): one block per gradient row (tap, g).  Thread (k group, d quad) sums
// float4s of slabs k = kg, kg + KG, ... - a wave reads whole 16-byte-aligned row segments of consecutive slabs (coalesced; one
// wave per output element read 4 bytes per slab at a 32 KB stride) - and the KG partial sums fold through LDS in a fixed order.
__global__ __launch_bounds__(256) void wgrad_reduce_wave_kernel(const WgradArgs a) {
  __shared__ float4 sm[256];
  const int row = blockIdx.x;                       // (tap, gc) with gc < Greal
  const int tap = row / a.Greal, gc = row - tap * a.Greal;
  const size_t m = (size_t)tap * a.Gc + gc;
  const int dq = (a.Dreal + 3) >> 2;                // float4 columns (Dpad is a multiple of 16: reads stay inside the slab row)
  int dqp = 1;
  while (dqp < dq) dqp <<= 1;                       // threads per k group (power of two <= 256)
  const int KG = 256 / dqp;
  const int d4 = threadIdx.x % dqp, kg = threadIdx.x / dqp;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (d4 < dq) {
    // this thread's slabs kg, kg + KG, ... in that order, four loads in flight
    const float* src = a.partial + m * a.Dpad + d4 * 4;
    const size_t sstride = (size_t)a.Mpad * a.Dpad;
    for (int k0 = kg; k0 < a.splitk; k0 += 4 * KG) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = k0 + u * KG < a.splitk ? *reinterpret_cast<const float4*>(src + (size_t)(k0 + u * KG) * sstride) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + u * KG >= a.splitk) break;
        s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
      }
    }
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (kg == 0 && d4 < dq) {
    for (int j = 1; j < KG; ++j) { const float4 v = sm[j * dqp + d4]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    float* o = a.dW + ((size_t)tap * a.Greal + gc) * a.Dreal + d4 * 4;
    const float r[4] = {s.x, s.y, s.z, s.w};
    for (int e = 0; e < 4; ++e)
      if (d4 * 4 + e < a.Dreal) o[e] = r[e] + (a.accumulate ? o[e] : 0.f);
  }
}

template <typename T, int WC, int WP, int TC, int TP>
static hipError_t launch_wgrad_cfg(const WgradArgs& a, hipStream_t st) {
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16;
  dim3 grid(a.Mpad / BC, a.Dpad / BP, a.splitk);
  // bf16 tasks are 8x8 blocks: two chunks per iteration keep all 256 threads loading
  constexpr int KCH = (sizeof(T) == 2) ? 2 : 1;
  const size_t smem = 2 * KCH * 4 * (BC + BP) * 16;
  const bool plain = a.zeros && !a.g.aff_a[0] && !a.g.aff_a[1] && a.g.act == ACT_NONE && !a.d.aff_a[0] && !a.d.aff_a[1] && a.d.act == ACT_NONE;
  if (smem > 64 * 1024) {
    static bool done[2] = {false, false};
    if (!done[plain ? 1 : 0]) {
      if (plain) (void)hipFuncSetAttribute((const void*)wgrad_kernel<T, WC, WP, TC, TP, KCH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      else (void)hipFuncSetAttribute((const void*)wgrad_kernel<T, WC, WP, TC, TP, KCH, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      done[plain ? 1 : 0] = true;
    }
  }
  if (plain) hipLaunchKernelGGL((wgrad_kernel<T, WC, WP, TC, TP, KCH, true>), grid, dim3(WC * WP * 64), smem, st, a);
  else hipLaunchKernelGGL((wgrad_kernel<T, WC, WP, TC, TP, KCH, false>), grid, dim3(WC * WP * 64), smem, st, a);
  return hipGetLastError();
}

template <typename T> static hipError_t launch_wgrad_t(const WgradArgs& a, int cfg, hipStream_t st) {
  hipError_t e;
  int pbm, pbn;
  wgrad_tile(cfg, &pbm, &pbn);
  const double Pn = (double)a.N * a.Hb * a.Wb;
  ProfScope prof("wgrad", sizeof(T) == 2, pbm, pbn, 2.0 * Pn * a.ntaps * a.Greal * a.Dreal,
                 sizeof(T) * ((double)a.N * a.Hgin * a.Wgin * a.Greal + Pn * a.Dreal) + 4.0 * a.ntaps * a.Greal * a.Dreal, st);
  if (sizeof(T) == 4 && wgrad_mm_eligible(a, cfg)) {               // one-tap float32 products: transpose-free LDS-DMA kernel (wgrad_mm.hip)
    g_prof_family = "mm";
    e = launch_wgrad_mm(a, cfg, st);
  } else
  switch (cfg) {
    case WG_128x128: e = launch_wgrad_cfg<T, 2, 2, 4, 4>(a, st); break;
    case WG_128x64: e = launch_wgrad_cfg<T, 2, 2, 4, 2>(a, st); break;
    case WG_128x16: e = launch_wgrad_cfg<T, 4, 1, 2, 1>(a, st); break;
    case WG_TR_256x128: case WG_TR_128x128: {                                            // 256 / 128 rows x 128 cols, LDS-DMA + transpose reads (wgrad_tr.hip; bf16, plain operands)
      const bool plain = a.zeros && !a.g.aff_a[0] && !a.g.aff_a[1] && a.g.act == ACT_NONE && !a.d.aff_a[0] && !a.d.aff_a[1] && a.d.act == ACT_NONE;
      if (sizeof(T) != 2 || !plain) return hipErrorInvalidValue;
      int cols = pbn;
      e = launch_wgrad_tr(a, st, &g_prof_family, &cols);
      prof.bp = cols;                                                // (the 256-column tile where the launcher took it: the class names the template instance)
      break;
    }
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess || a.splitk == 1) return e;
  if (a.splitk >= 32 && a.Dreal <= 1024) {
    hipLaunchKernelGGL(wgrad_reduce_wave_kernel, dim3(a.ntaps * a.Greal), dim3(256), 0, st, a);
    return hipGetLastError();
  }
  const size_t total = (size_t)a.ntaps * a.Greal * a.Dreal / ((a.Dreal & 3) ? 1 : 4);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_wgrad(const WgradArgs& a, int is_bf16, int cfg, hipStream_t st) {
  return is_bf16 ? launch_wgrad_t<bf16>(a, cfg, st) : launch_wgrad_t<float>(a, cfg, st);
}

void wgrad_tile(int cfg, int* bm, int* bn) {
  static const int t[7][2] = {{128, 128}, {128, 64}, {128, 16}, {0, 0}, {0, 0}, {256, 128}, {128, 128}};   // (3, 4: unused)
  *bm = t[cfg][0]; *bn = t[cfg][1];
}

}  // namespace vp

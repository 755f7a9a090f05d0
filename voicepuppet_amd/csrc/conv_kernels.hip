// The generic implicit-GEMM convolution for gfx950 (MI355X), hand-written MFMA kernels (16x16x32 bf16 / 16x16x4 f32 tiles): the CK_IGEMM
// row of the kernel table (conv_dispatch.hip).
//
// Kernels (DESIGN.md section 3 has the measurements and what bounds each):
//   igemm_dma_kernel   conv fwd / bwd-data, deconv fwd / bwd-data: both operands HBM/L2 -> LDS by LDS-DMA (rb_swz image: coalesced 64-byte
//                      segments, conflict-free ds_read_b128), 3-deep ring with counted vmcnt, one barrier per 64-byte K chunk,
//                      scalar-stepped buffer-descriptor loader (fastk), staged LDS epilogue with 16-byte row stores (+ BN statistics)
//   igemm_ws_kernel    the same GEMM with 4 producer waves issuing every DMA and consumer waves doing only ds_read + MFMA
//   igemm_kernel       register loader with the deferred-BN prologue (plane_device.h): serves the single-op API
//   igemm_splitk_reduce_kernel
// The kernel variants that were measured slower (register-operand loader, resident-weight persistent tiles, 128-byte K chunks,
// register-double-buffered 256x256 tile, direct epilogue: EXPERIMENTS.md) were deleted in round 4; `git log -- voicepuppet_amd/csrc/conv_db.hip`
// and `.../experiments/igemm_experiments.inc` have them.  The weight-gradient kernels are in wgrad_kernels.hip.
#include "conv_prof.h"
#include "igemm_device.h"
#include "launch.h"
#include "plane_device.h"
#include "vp_common.h"

#ifndef VP_RING
#define VP_RING 3      // LDS ring depth of the DMA GEMM loop (stages); 3 = one chunk in flight across the barrier
#endif
#ifndef VP_ABLATE
#define VP_ABLATE 0   // build-time ablation of the LDS-DMA GEMM loop: 1 = no MFMA, 2 = no DMA in the loop
#endif

namespace vp {

// ------------------------------------------------------------------------------------------------
// epilogue shared by igemm_kernel and splitk_reduce_kernel: 4 consecutive output channels of one pixel
// ------------------------------------------------------------------------------------------------
template <typename T, bool DUAL = false>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& a, int cls, int pidx, int c0, float v[4]) {
  if (c0 >= a.Cout) return;
  const int hw = a.Hg * a.Wg;
  const int n = pidx / hw;
  const int rem = pidx - n * hw;
  const int q = rem / a.Wg;
  const int r = rem - q * a.Wg;
  const size_t pix = ((size_t)n * a.Hof + (q * a.os + a.o0h[cls])) * a.Wof + (r * a.os + a.o0w[cls]);
  const int nv = min(4, a.Cout - c0);
  void* Yp = a.Y;
  const void* refp = a.ref;
  int accu = a.accumulate, yf32 = a.y_f32;
  if constexpr (DUAL) {
    if (c0 >= a.split_c) { Yp = a.Y2; refp = a.ref2; accu = a.accumulate2; yf32 = a.y2_f32; c0 -= a.split_c; }     // two-output form (conv_args.h)
  }
  const size_t off = pix * a.ldY + c0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < nv) {
      if (a.bias) v[e] += a.bias[c0 + e];
      v[e] = act_apply(a.out_act, v[e]);
    }
  }
  if (refp) {
    const T* rp = reinterpret_cast<const T*>(refp) + off;
    const int goff = (n / a.ref_group_n) * a.Cout + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nv) {
        float z = Elem<T>::ld(rp + e);
        if (a.ref_a) z = fmaf(a.ref_a[goff + e], z, a.ref_b[goff + e]);
        v[e] *= act_grad(a.ref_act, z);
      }
    }
  }
  if (yf32) {
    float* yp = reinterpret_cast<float*>(Yp) + off;
    if (accu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nv) v[e] += yp[e];
    }
    if (nv == 4 && (a.ldY & 3) == 0) *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nv) yp[e] = v[e];
    }
  } else {
    T* yp = reinterpret_cast<T*>(Yp) + off;
    if (accu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nv) v[e] += Elem<T>::ld(yp + e);
    }
    if (nv == 4 && (a.ldY & 3) == 0) {
      if (sizeof(T) == 4) *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<uint2*>(yp) = make_uint2(f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16),
                                                     f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nv) Elem<T>::st(yp + e, v[e]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// igemm_kernel: grid = (pixel tiles, channel tiles, nclass * splitk), 256 threads = 4 waves (WC x WP)
//   MFMA A operand = weights (rows -> output channels), B operand = pixels (cols), so one lane ends
//   up with 4 consecutive channels of one pixel: a single 16-byte (f32) / 8-byte (bf16) NHWC store.
// ------------------------------------------------------------------------------------------------
template <typename T, int WC, int WP, int TC, int TP>
__global__ __launch_bounds__(256) void igemm_kernel(const IgemmArgs a) {
  constexpr int E = Elem<T>::E, KC = 4 * E;
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16;
  constexpr int PA = (BC + 63) / 64, PB = (BP + 63) / 64;   // staging passes (64 rows per pass)
  constexpr int BUF = 4 * (BC + BP);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);
  int* ltap = reinterpret_cast<int*>(lds + 2 * BUF);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cls = blockIdx.z / a.splitk, split = blockIdx.z - cls * a.splitk;
  const int P = a.N * a.Hg * a.Wg;
  const int p_base = blockIdx.x * BP, c_base = blockIdx.y * BC;

  if (tid < 16) ltap[tid] = (tid < a.ntaps) ? (((int)a.taps[cls].dh[tid] << 16) | ((int)a.taps[cls].dw[tid] & 0xffff)) : 0;

  // staging thread -> (row within 16, k-piece g): 8 consecutive lanes = 8 consecutive rows of one plane
  const int r16 = (lane & 7) + 8 * (lane >> 5);
  const int g = (lane >> 3) & 3;

  // per-thread pixel rows (fixed over the K loop)
  int pn[PB], pbh[PB], pbw[PB];
  bool pok[PB];
#pragma unroll
  for (int ps = 0; ps < PB; ++ps) {
    const int row = ps * 64 + wave * 16 + r16;
    const int pidx = p_base + row;
    pok[ps] = (row < BP) && (pidx < P);
    const int hw = a.Hg * a.Wg;
    const int pc = pok[ps] ? pidx : 0;
    const int n = pc / hw, rem = pc - n * hw, q = rem / a.Wg;
    pn[ps] = n; pbh[ps] = q * a.sh; pbw[ps] = (rem - q * a.Wg) * a.sw;
  }
  const T* wp = reinterpret_cast<const T*>(a.Wp) + (size_t)cls * a.wp_rows * a.Kpad;   // [K chunk][row][KC]

  const int nchunk = a.Kpad / KC;
  const int per = (nchunk + a.splitk - 1) / a.splitk;
  const int kc0 = split * per, kc1 = min(nchunk, kc0 + per);

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // staging registers as named scalars (arrays captured by the lambdas below end up in scratch)
  uint4 ra0, ra1, rb0, rb1;
  ra0 = ra1 = rb0 = rb1 = make_uint4(0, 0, 0, 0);
  __syncthreads();   // tap table visible

  auto load_a = [&](int kc, int ps) -> uint4 {
    const int row = ps * 64 + wave * 16 + r16;
    if (BC % 64 == 0 || row < BC) return *reinterpret_cast<const uint4*>(wp + ((size_t)kc * a.wp_rows + c_base + row) * KC + g * E);
    return make_uint4(0, 0, 0, 0);
  };
  auto load_b = [&](int kc, int ps, int n, int bh, int bw, bool ok) -> uint4 {
    const int k0 = kc * KC + g * E;
    const int tap = k0 >> a.log2Cin;
    const int ci = k0 & a.cin_mask;
    const bool tok = tap < a.ntaps;
    const int tv = ltap[tok ? tap : 0];
    const int dh = tv >> 16, dw = (int)(short)(tv & 0xffff);
    const int row = ps * 64 + wave * 16 + r16;
    if (BP % 64 == 0 || row < BP) return load_pix_piece<T>(a.x, n, bh + dh, bw + dw, a.Hin, a.Win, ci, ok && tok);
    return make_uint4(0, 0, 0, 0);
  };
  auto stage_load = [&](int kc) {
    ra0 = load_a(kc, 0);
    if (PA > 1) ra1 = load_a(kc, 1);
    rb0 = load_b(kc, 0, pn[0], pbh[0], pbw[0], pok[0]);
    if (PB > 1) rb1 = load_b(kc, 1, pn[PB - 1], pbh[PB - 1], pbw[PB - 1], pok[PB - 1]);
  };
  auto stage_store = [&](int buf) {
    uint4* la = lds + buf * BUF;
    uint4* lb = la + 4 * BC;
    const int row = wave * 16 + r16;
    if (BC % 64 == 0 || row < BC) la[g * BC + row] = ra0;
    if (PA > 1) la[g * BC + 64 + row] = ra1;
    if (BP % 64 == 0 || row < BP) lb[g * BP + row] = rb0;
    if (PB > 1) lb[g * BP + 64 + row] = rb1;
  };

  const int wc = wave / WP, wpi = wave - wc * WP;
  const int rowA0 = wc * TC * 16, rowB0 = wpi * TP * 16;

  if (kc0 < kc1) {
    stage_load(kc0);
    stage_store(0);
    __syncthreads();
    for (int kc = kc0; kc < kc1; ++kc) {
      const int buf = (kc - kc0) & 1;
      const bool more = kc + 1 < kc1;
      if (more) stage_load(kc + 1);
      const uint4* la = lds + buf * BUF;
      mma_chunk<T, TC, TP, BC, BP, 0>(la, la + 4 * BC, rowA0, rowB0, lane, acc);
      if (more) stage_store(buf ^ 1);
      __syncthreads();
    }
  }

  // epilogue: lane holds pixel (lane&15), channels 4*(lane>>4) .. +3 of each 16x16 tile
#pragma unroll
  for (int tp = 0; tp < TP; ++tp) {
    const int pidx = p_base + rowB0 + tp * 16 + (lane & 15);
    if (pidx >= P) continue;
#pragma unroll
    for (int tc = 0; tc < TC; ++tc) {
      const int c0 = c_base + tile_chan0(a.rowperm, rowA0 / 16 + tc, lane >> 4);
      float v[4] = {acc[tc][tp][0], acc[tc][tp][1], acc[tc][tp][2], acc[tc][tp][3]};
      if (a.splitk > 1) {
        float* pp = a.partial + (((size_t)(cls * a.splitk + split) * P + pidx) * a.CoutPad + c0);
        *reinterpret_cast<float4*>(pp) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        igemm_epilogue<T>(a, cls, pidx, c0, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// igemm_dma_kernel: same GEMM, operands that need no prologue (materialised activations, gradients,
// packed weights) go HBM/L2 -> LDS directly with global_load_lds_dwordx4 (no VGPR round trip, no
// ds_write pass).  One wave instruction moves a 16-row block x 4 k-pieces = 64 consecutive 16-byte
// slots; the LDS image is [row block][16 rows][4 k-pieces] with the pieces of each row XOR-permuted
// (rb_swz) so that global reads are coalesced AND ds_read_b128 stays conflict-free.  Padding / ragged
// pixels read a 16-byte zero page instead (LDS-DMA cannot zero-fill).  One barrier per K chunk.
// ------------------------------------------------------------------------------------------------
template <typename T, int WC, int WP, int TC, int TP, bool STAGED, int STATS = 0, bool DUAL = false>
__global__ __launch_bounds__(WC * WP * 64) void igemm_dma_kernel(const IgemmArgs a) {
  constexpr int E = Elem<T>::E, KC = 4 * E;
  constexpr int NW = WC * WP, NT = NW * 64;             // 4 waves (256 threads) or 8 waves (512 threads: 128x256 / 256x256 tiles)
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16;
  constexpr int NBA = BC / 16, NBB = BP / 16;          // 16-row blocks per operand tile
  constexpr int JA = (NBA + NW - 1) / NW, JB = (NBB + NW - 1) / NW; // DMA instructions per wave per chunk
  constexpr int BUF = 4 * (BC + BP);
  // every wave issues the same number of DMAs per chunk -> a counted vmcnt can keep one chunk in flight
  // across the barrier (3-deep LDS ring); otherwise 2 buffers and a full drain per chunk
  constexpr bool RING = (NBA % NW == 0) && (NBB % NW == 0);
  constexpr int NST = RING ? VP_RING : 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);
  int* ltap = reinterpret_cast<int*>(lds + NST * BUF);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cls = blockIdx.z / a.splitk, split = blockIdx.z - cls * a.splitk;
  const int P = a.N * a.Hg * a.Wg;
  // XCD-aware tile order (speed only): workgroup b is observed to run on XCD b % 8, each XCD has a private 4 MiB L2.
  // Give every XCD a contiguous range of logical tiles, ordered pixel-tile major / channel-tile minor, so the channel
  // tiles that re-read one activation tile run back to back on the same L2 and the weight slabs stay resident.
  int pt, ct;
  {
    const int nb = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
    const int q8 = nb >> 3, r8 = nb & 7, xcd = id & 7, slot = id >> 3;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    ct = logical % (int)gridDim.y; pt = logical / (int)gridDim.y;
  }
  const int p_base = pt * BP, c_base = ct * BC;
#if VP_ABLATE & 4
  // bandwidth experiment (results are garbage): a DMA instruction fetches 8 rows x 128 contiguous bytes instead of 16 x 64
  const int r = lane >> 3, g = lane & 7;
#else
  const int r = lane >> 2, g = (lane & 3) ^ rb_swz(lane >> 2);   // row in the 16-row block, k-piece fetched
#endif

  if (tid < 16) ltap[tid] = (tid < a.ntaps) ? (((int)a.taps[cls].dh[tid] << 16) | ((int)a.taps[cls].dw[tid] & 0xffff)) : 0;

  // fixed per-thread rows
  const T* wrow[JA];
#pragma unroll
  for (int j = 0; j < JA; ++j)
    wrow[j] = reinterpret_cast<const T*>(a.Wp) + (size_t)cls * a.wp_rows * a.Kpad + ((size_t)c_base + (wave + NW * j) * 16 + r) * KC + g * E;
  int pn[JB], pbh[JB], pbw[JB];
  bool pok[JB];
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int pidx = p_base + (wave + NW * j) * 16 + r;
    pok[j] = (wave + NW * j < NBB) && (pidx < P);
    const int hw = a.Hg * a.Wg;
    const int pc = pok[j] ? pidx : 0;
    const int n = pc / hw, rem = pc - n * hw, q = rem / a.Wg;
    pn[j] = n * a.Hin; pbh[j] = q * a.sh; pbw[j] = (rem - q * a.Wg) * a.sw;
  }
  const T* x0 = reinterpret_cast<const T*>(a.x.ptr[0]);
  const T* x1 = reinterpret_cast<const T*>(a.x.ptr[1]);
  const int C0 = a.x.C[0], C1 = a.x.C[1];

  const int nchunk = a.Kpad / KC;
  const int per = (nchunk + a.splitk - 1) / a.splitk;
  const int kc0 = split * per, kc1 = min(nchunk, kc0 + per);

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int kc, int buf) {
    uint4* la = lds + buf * BUF;
    uint4* lb = la + 4 * BC;
#pragma unroll
    for (int j = 0; j < JA; ++j)
      if (NBA % NW == 0 || wave + NW * j < NBA) dma16(wrow[j] + (size_t)kc * a.wp_rows * KC, la + (wave + NW * j) * 64);
    const int k0 = kc * KC + g * E;
    const int tap = k0 >> a.log2Cin;
    const int ci = k0 & a.cin_mask;
    const bool tok = tap < a.ntaps;
    const int tv = ltap[tok ? tap : 0];
    const int dh = tv >> 16, dw = (int)(short)(tv & 0xffff);
    const bool s1 = ci >= C0;
    const T* xb = s1 ? x1 : x0;
    const int Cs = s1 ? C1 : C0;
    const int cl = s1 ? ci - C0 : ci;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      if (NBB % NW == 0 || wave + NW * j < NBB) {
        const int ih = pbh[j] + dh, iw = pbw[j] + dw;
        const bool ok = pok[j] && tok && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
        const void* src = ok ? (const void*)(xb + ((size_t)(pn[j] + ih) * a.Win + iw) * Cs + cl) : a.zeros;
        dma16(src, lb + (wave + NW * j) * 64);
      }
    }
  };

  // ---- fast loader (a.fastk: every 64-byte K chunk lies inside one tap and one source tensor) -------------------
  // K is walked as segments (tap, source); per segment each lane computes ONE byte offset per pixel row (or DMA_OOB for
  // padding), inside a segment a chunk only bumps a scalar offset.  The weight stream is chunk-major: scalar bump too.
  const unsigned es = sizeof(T);
  __amdgpu_buffer_rsrc_t rsW = make_rsrc(reinterpret_cast<const T*>(a.Wp) + (size_t)cls * a.wp_rows * a.Kpad, 0xFFFFFFFFu);
  __amdgpu_buffer_rsrc_t rsX0 = make_rsrc(x0, (unsigned)((size_t)a.N * a.Hin * a.Win * C0 * es));
  __amdgpu_buffer_rsrc_t rsX1 = make_rsrc(x1 ? (const void*)x1 : (const void*)x0, (unsigned)((size_t)a.N * a.Hin * a.Win * C1 * es));
  unsigned wvo[JA];
#pragma unroll
  for (int j = 0; j < JA; ++j) wvo[j] = (unsigned)(((c_base + (wave + NW * j) * 16 + r) * KC + g * E) * es);
  const unsigned wstep = (unsigned)(a.wp_rows * KC * es);
  unsigned f_wso = (unsigned)kc0 * wstep;          // scalar: weight chunk offset
  unsigned f_xso = 0;                              // scalar: channel offset inside the segment (bytes)
  int f_left = 0;                                  // chunks left in the current segment
  int f_tap = 0, f_src = 0;                        // next segment to open
  unsigned f_xvo[JB];
  bool f_use1 = false;
  if (a.fastk) {
    const int k0 = kc0 * KC;
    f_tap = k0 >> a.log2Cin;
    const int ci = k0 & a.cin_mask;
    f_src = ci >= C0 ? 1 : 0;
    // a split that starts inside a segment: open it now and skip the consumed chunks
    const int cl = f_src ? ci - C0 : ci;
    f_xso = (unsigned)cl * es;
    f_left = -(cl / KC);                            // negative: corrected when the segment opens below
  }
  auto open_segment = [&]() {
    const bool tok = f_tap < a.ntaps;
    const int tv = ltap[tok ? f_tap : 0];
    const int dh = tv >> 16, dw = (int)(short)(tv & 0xffff);
    f_use1 = f_src != 0;
    const int Cs = f_use1 ? C1 : C0;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const int ih = pbh[j] + dh, iw = pbw[j] + dw;
      const bool ok = pok[j] && tok && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      f_xvo[j] = ok ? (unsigned)((((pn[j] + ih) * a.Win + iw) * Cs + g * E) * es) : DMA_OOB;
    }
    f_left += Cs / KC;
    // next segment: the other source of the same tap, or the next tap
    if (!f_use1 && C1 > 0) f_src = 1; else { f_src = 0; ++f_tap; }
  };
  auto issue_fast = [&](int buf) {
    uint4* la = lds + buf * BUF;
    uint4* lb = la + 4 * BC;
    if (f_left <= 0) { const int skipped = -f_left; f_left = 0; open_segment(); f_left -= skipped; if (skipped == 0) f_xso = 0; }
#pragma unroll
    for (int j = 0; j < JA; ++j)
      if (NBA % NW == 0 || wave + NW * j < NBA) dma16_buf(rsW, wvo[j], f_wso, la + (wave + NW * j) * 64);
    const __amdgpu_buffer_rsrc_t rx = f_use1 ? rsX1 : rsX0;
#pragma unroll
    for (int j = 0; j < JB; ++j)
      if (NBB % NW == 0 || wave + NW * j < NBB) dma16_buf(rx, f_xvo[j], f_xso, lb + (wave + NW * j) * 64);
    f_wso += wstep;
    f_xso += KC * es;
    --f_left;
  };
  auto issue_any = [&](int kc, int buf) { if (a.fastk) issue_fast(buf); else issue(kc, buf); };

  const int wc = wave / WP, wpi = wave - wc * WP;
  const int blkA0 = wc * TC, blkB0 = wpi * TP;

  __syncthreads();   // tap table visible
  if (kc0 < kc1) {
    if (RING) {
      // NST-deep ring: chunks kc+1 .. kc+NST-2 stay in flight across the barrier while chunk kc is consumed
#pragma unroll
      for (int d = 0; d < NST - 1; ++d) if (kc0 + d < kc1) issue_any(kc0 + d, d);
      int st = 0;
      for (int kc = kc0; kc < kc1; ++kc) {
        if (kc + NST - 2 < kc1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * (JA + JB)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tail: fewer batches outstanding than the constant assumes
        __builtin_amdgcn_s_barrier();   // every wave's DMA of chunk kc landed; every wave is done reading chunk kc-1
        asm volatile("" ::: "memory");
        const int stn = st == 0 ? NST - 1 : st - 1;   // the buffer chunk kc-1 used
#if !(VP_ABLATE & 2)
        if (kc + NST - 1 < kc1) issue_any(kc + NST - 1, stn);
#endif
        const uint4* la = lds + st * BUF;
#if !(VP_ABLATE & 1)
        mma_chunk_rb<T, TC, TP, BC, BP>(la, la + 4 * BC, blkA0, blkB0, lane, acc);
#endif
        st = st == NST - 1 ? 0 : st + 1;
      }
    } else {
      issue_any(kc0, 0);
      for (int kc = kc0; kc < kc1; ++kc) {
        const int buf = (kc - kc0) & 1;
        __syncthreads();   // waits for this wave's DMA (vmcnt) and for every wave's reads of the other buffer
        if (kc + 1 < kc1) issue_any(kc + 1, buf ^ 1);
        const uint4* la = lds + buf * BUF;
        mma_chunk_rb<T, TC, TP, BC, BP>(la, la + 4 * BC, blkA0, blkB0, lane, acc);
      }
    }
  }

#if VP_ABLATE & 8
  {   // epilogue ablation: every accumulator stays live (no dead-code elimination of the MFMAs), nothing is stored
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
      for (int j = 0; j < TP; ++j) sum += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (sum == 123.456f) reinterpret_cast<float*>(a.Y)[0] = 1.f;
    return;
  }
#endif
  if (STAGED) {
    constexpr int RINGB = NST * BUF * 16;
    constexpr int NPASS = epi_passes(BC, BP, WP, RINGB);
    staged_epilogue<T, TC, TP, BC, BP, NPASS, NT, STATS, 0, DUAL>(a, LinearPix{a, cls, p_base, P}, c_base, blkA0, blkB0, acc, smem, pt, cls);
    return;
  }
#pragma unroll
  for (int tp = 0; tp < TP; ++tp) {
    const int pidx = p_base + (blkB0 + tp) * 16 + (lane & 15);
    if (pidx >= P) continue;
#pragma unroll
    for (int tc = 0; tc < TC; ++tc) {
      const int c0 = c_base + tile_chan0(a.rowperm, blkA0 + tc, lane >> 4);
      float v[4] = {acc[tc][tp][0], acc[tc][tp][1], acc[tc][tp][2], acc[tc][tp][3]};
      if (a.splitk > 1) {
        float* pp = a.partial + (((size_t)(cls * a.splitk + split) * P + pidx) * a.CoutPad + c0);
        *reinterpret_cast<float4*>(pp) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        igemm_epilogue<T, DUAL>(a, cls, pidx, c0, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// igemm_ws_kernel: wave-specialised form of igemm_dma_kernel.  An LDS-DMA costs its issuing wave 60-185 cycles of issue
// time (MI355X_MICROARCH.md), comparable to the 16 MFMAs of a K chunk, so in the kernels above the DMA issue and the
// matrix pipe take turns inside every wave.  Here NPW = 4 producer waves (one per SIMD) issue ALL the DMAs of a stage and
// the WC x WP consumer waves only do barrier -> ds_read -> MFMA; the producers' issue stalls overlap the consumers' MFMAs
// on the same SIMD.  One barrier per K chunk, NST-deep ring:
//   producer kc: wait vmcnt (its share of chunk kc landed) -> barrier kc -> issue chunk kc+NST-1 into the stage chunk kc-1 used
//   consumer kc: barrier kc -> fragments + MFMAs of chunk kc
// fastk operands only (scalar K stepping, hardware zero fill); epilogue = the staged 16-byte row stores, all waves storing.
// ------------------------------------------------------------------------------------------------
template <typename T, int WC, int WP, int TC, int TP, int NST, int STATS = 0, bool DUAL = false>
__global__ __launch_bounds__((WC * WP + 4) * 64) void igemm_ws_kernel(const IgemmArgs a) {
  constexpr int E = Elem<T>::E, KC = 4 * E;
  constexpr int NPW = 4;
  constexpr int NW = WC * WP, NT = (NW + NPW) * 64;
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16;
  constexpr int NBA = BC / 16, NBB = BP / 16, NB = NBA + NBB;
  static_assert(NB % NPW == 0, "every producer issues the same number of DMAs per chunk");
  constexpr int J = NB / NPW;
  constexpr int BUF = 4 * (BC + BP);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);
  int* ltap = reinterpret_cast<int*>(lds + NST * BUF);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave >= NW;
  const int cls = blockIdx.z;
  const int P = a.N * a.Hg * a.Wg;
  int pt, ct;
  {
    const int nb = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
    const int q8 = nb >> 3, r8 = nb & 7, xcd = id & 7, slot = id >> 3;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    ct = logical % (int)gridDim.y; pt = logical / (int)gridDim.y;
  }
  const int p_base = pt * BP, c_base = ct * BC;
  if (tid < 16) ltap[tid] = (tid < a.ntaps) ? (((int)a.taps[cls].dh[tid] << 16) | ((int)a.taps[cls].dw[tid] & 0xffff)) : 0;
  const int nchunk = a.Kpad / KC;
  const int wc = producer ? 0 : wave / WP, wpi = producer ? 0 : wave - wc * WP;
  const int blkA0 = wc * TC, blkB0 = producer ? (1 << 20) : wpi * TP;     // producers stage nothing in the epilogue

  f32x4 acc[TC][TP];   // consumers only: left undefined on the producer path so it holds no registers there

  __syncthreads();   // tap table visible

  if (producer) {
    const int pw = wave - NW;
    const unsigned es = sizeof(T);
    const T* x0 = reinterpret_cast<const T*>(a.x.ptr[0]);
    const T* x1 = reinterpret_cast<const T*>(a.x.ptr[1]);
    const int C0 = a.x.C[0], C1 = a.x.C[1];
    __amdgpu_buffer_rsrc_t rsW = make_rsrc(reinterpret_cast<const T*>(a.Wp) + (size_t)cls * a.wp_rows * a.Kpad, 0xFFFFFFFFu);
    __amdgpu_buffer_rsrc_t rsX0 = make_rsrc(x0, (unsigned)((size_t)a.N * a.Hin * a.Win * C0 * es));
    __amdgpu_buffer_rsrc_t rsX1 = make_rsrc(x1 ? (const void*)x1 : (const void*)x0, (unsigned)((size_t)a.N * a.Hin * a.Win * C1 * es));
    const int r = lane >> 2, g = (lane & 3) ^ rb_swz(lane >> 2);
    // row block b = pw + NPW*j: weight block b (b < NBA) or pixel block b - NBA
    unsigned wvo[J];
    int pn[J], pbh[J], pbw[J];
    bool pok[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int b = pw + NPW * j;
      wvo[j] = (unsigned)(((c_base + b * 16 + r) * KC + g * E) * es);
      const int pidx = p_base + (b - NBA) * 16 + r;
      pok[j] = b >= NBA && pidx < P;
      const int hw = a.Hg * a.Wg;
      const int pc = pok[j] ? pidx : 0;
      const int n = pc / hw, rem = pc - n * hw, q = rem / a.Wg;
      pn[j] = n * a.Hin; pbh[j] = q * a.sh; pbw[j] = (rem - q * a.Wg) * a.sw;
    }
    const unsigned wstep = (unsigned)(a.wp_rows * KC * es);
    unsigned wso = 0, xso = 0;
    int left = 0, tap = 0, src = 0;
    bool use1 = false;
    unsigned xvo[J];
    auto open_segment = [&]() {
      const bool tok = tap < a.ntaps;
      const int tv = ltap[tok ? tap : 0];
      const int dh = tv >> 16, dw = (int)(short)(tv & 0xffff);
      use1 = src != 0;
      const int Cs = use1 ? C1 : C0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int ih = pbh[j] + dh, iw = pbw[j] + dw;
        const bool ok = pok[j] && tok && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
        xvo[j] = ok ? (unsigned)((((pn[j] + ih) * a.Win + iw) * Cs + g * E) * es) : DMA_OOB;
      }
      left = Cs / KC;
      xso = 0;
      if (!use1 && C1 > 0) src = 1; else { src = 0; ++tap; }
    };
    auto issue = [&](int buf) {
      uint4* la = lds + buf * BUF;
      uint4* lb = la + 4 * BC;
      if (left == 0) open_segment();
      const __amdgpu_buffer_rsrc_t rx = use1 ? rsX1 : rsX0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int b = pw + NPW * j;
        if (b < NBA) dma16_buf(rsW, wvo[j], wso, la + b * 64);
        else dma16_buf(rx, xvo[j], xso, lb + (b - NBA) * 64);
      }
      wso += wstep;
      xso += KC * es;
      --left;
    };
#pragma unroll
    for (int d = 0; d < NST - 1; ++d) if (d < nchunk) issue(d);
    int st = 0;
    for (int kc = 0; kc < nchunk; ++kc) {
      if (kc + NST - 2 < nchunk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * J) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const int stn = st == 0 ? NST - 1 : st - 1;
      if (kc + NST - 1 < nchunk) issue(stn);
      st = st == NST - 1 ? 0 : st + 1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
      for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int st = 0;
    for (int kc = 0; kc < nchunk; ++kc) {
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const uint4* la = lds + st * BUF;
      if constexpr (TC <= 4) {
        mma_chunk_rb<T, TC, TP, BC, BP>(la, la + 4 * BC, blkA0, blkB0, lane, acc);
      } else {
        // 128-row wave tiles: channel fragments in groups of four (the 128 accumulator registers leave room for no more)
        const uint4* lb = la + 4 * BC;
        const int i = lane & 15, g = lane >> 4;
        const int so = i * 4 + (g ^ rb_swz(i));
        uint4 fb[TP];
#pragma unroll
        for (int t = 0; t < TP; ++t) fb[t] = lb[(blkB0 + t) * 64 + so];
#pragma unroll
        for (int h = 0; h < TC; h += 4) {
          uint4 fa[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) fa[t] = la[(blkA0 + h + t) * 64 + so];
#pragma unroll
          for (int tc = 0; tc < 4; ++tc)
#pragma unroll
            for (int tp = 0; tp < TP; ++tp) acc[h + tc][tp] = mma16<T>(fa[tc], fb[tp], acc[h + tc][tp]);
        }
      }
      st = st == NST - 1 ? 0 : st + 1;
    }
  }

#if VP_ABLATE & 8
  if (!producer) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
      for (int j = 0; j < TP; ++j) sum += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (sum == 123.456f) reinterpret_cast<float*>(a.Y)[0] = 1.f;
  }
  return;
#endif
  constexpr int RINGB = NST * BUF * 16;
  constexpr int NPASS = epi_passes(BC, BP, WP, RINGB);
  staged_epilogue<T, TC, TP, BC, BP, NPASS, NT, STATS, 0, DUAL>(a, LinearPix{a, cls, p_base, P}, c_base, blkA0, blkB0, acc, smem, pt, cls);
}


// sums the split-K slabs in a fixed order (deterministic) and applies the igemm epilogue
template <typename T, bool DUAL = false>
__global__ __launch_bounds__(256) void igemm_splitk_reduce_kernel(const IgemmArgs a) {
  const int P = a.N * a.Hg * a.Wg;
  const int cq = a.CoutPad >> 2;
  const size_t total = (size_t)a.nclass * P * cq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c0 = (int)(i % cq) * 4;
    const size_t t = i / cq;
    const int pidx = (int)(t % P);
    const int cls = (int)(t / P);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    // the slabs are added in slab order (deterministic, same sums as a one-load-per-trip loop); eight loads are in flight at a
    // time - a thread's slabs lie P * CoutPad floats apart, the pass is pure load latency otherwise
    const float* src = a.partial + (((size_t)cls * a.splitk * P + pidx) * a.CoutPad + c0);
    const size_t sstride = (size_t)P * a.CoutPad;
    for (int s0 = 0; s0 < a.splitk; s0 += 8) {
      float4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = s0 + u < a.splitk ? *reinterpret_cast<const float4*>(src + (size_t)(s0 + u) * sstride) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (s0 + u >= a.splitk) break;
        v[0] += x[u].x; v[1] += x[u].y; v[2] += x[u].z; v[3] += x[u].w;
      }
    }
    igemm_epilogue<T, DUAL>(a, cls, pidx, c0, v);
  }
}



// ------------------------------------------------------------------------------------------------
// host-side dispatch
// ------------------------------------------------------------------------------------------------
template <typename T, int WC, int WP, int TC, int TP>
static hipError_t launch_igemm_cfg(const IgemmArgs& a, hipStream_t st) {
  constexpr int BC = WC * TC * 16, BP = WP * TP * 16, NW = WC * WP;
  const int P = a.N * a.Hg * a.Wg;
  dim3 grid((P + BP - 1) / BP, a.CoutPad / BC, a.nclass * a.splitk);
  constexpr bool RING = ((BC / 16) % NW == 0) && ((BP / 16) % NW == 0);
  constexpr int RINGB = (RING ? VP_RING : 2) * 4 * (BC + BP) * 16;
  constexpr int NPASS = epi_passes(BC, BP, WP, RINGB);
  size_t smem = RINGB + 64 + BP * 8;      // ring, tap table, output-offset table of the direct epilogue
  const size_t smem_epi = (size_t)(BP / NPASS) * (BC * 4 + 16) + (BP / NPASS) * 8;
  if (smem_epi > smem) smem = smem_epi;
  const bool plain = a.zeros && !a.x.aff_a[0] && !a.x.aff_a[1] && a.x.act == ACT_NONE;
  if (plain) {
    IgemmArgs b = a;
    b.vec_epi = (a.splitk == 1 && a.Cout % 8 == 0 && a.ldY % 8 == 0) ? 1 : 0;
    const bool bst = a.bst_y || a.bst_y2;              // backward sums of a batch-normalised tensor in the epilogue (staged_epilogue, STATS == 2)
    // register-direct epilogue: measured SLOWER than the LDS-staged one (64-byte store segments vs 256-byte rows): opt-in
    // scalar-stepped loader: every 64-byte K chunk inside one tap and one source tensor, sources below the 2 GiB lane-offset range
    constexpr int KCE = 16 * 4 / (int)sizeof(T);
    const size_t xb0 = (size_t)a.N * a.Hin * a.Win * a.x.C[0] * sizeof(T), xb1 = (size_t)a.N * a.Hin * a.Win * a.x.C[1] * sizeof(T);
    b.fastk = (a.Cin % KCE == 0 && a.x.C[0] % KCE == 0 && a.x.C[1] % KCE == 0 && a.x.C[0] + a.x.C[1] == a.Cin &&
               xb0 < 0x70000000ull && xb1 < 0x70000000ull) ? 1 : 0;
    // wave-specialised kernel, per tile shape (bit = IgemmCfg): measured gains for 128x128, 64x128, 256x256; 128x256 is faster without
    constexpr int ws_cfgs = (1 << IG_128x128) | (1 << IG_64x128) | (1 << IG_256x256);
    constexpr int my_cfg = (BC == 128 && BP == 128) ? IG_128x128 : (BC == 64 && BP == 128) ? IG_64x128 : (BC == 128 && BP == 256) ? IG_128x256 :
                           (BC == 256 && BP == 256) ? IG_256x256 : 31;
    if constexpr (((BC + BP) / 16) % 4 == 0 && NW <= 8) {
      if (((ws_cfgs >> my_cfg) & 1) && b.vec_epi && b.fastk && a.splitk == 1) {
        constexpr int NSTW = (NW == 8) ? 4 : 4;
        constexpr int RB = NSTW * 4 * (BC + BP) * 16;
        constexpr int NPE = epi_passes(BC, BP, WP, RB);
        size_t sm = RB + 64 + BP * 8;
        const size_t se = (size_t)(BP / NPE) * (BC * 4 + 16) + (BP / NPE) * 8;
        if (se > sm) sm = se;
        g_prof_family = "ws";
        if (bst && b.split_c) hipLaunchKernelGGL((igemm_ws_kernel<T, WC, WP, TC, TP, NSTW, 2, true>), grid, dim3((NW + 4) * 64), sm, st, b);
        else if (bst) hipLaunchKernelGGL((igemm_ws_kernel<T, WC, WP, TC, TP, NSTW, 2>), grid, dim3((NW + 4) * 64), sm, st, b);
        else if (b.bn_part) hipLaunchKernelGGL((igemm_ws_kernel<T, WC, WP, TC, TP, NSTW, 1>), grid, dim3((NW + 4) * 64), sm, st, b);
        else if (b.split_c) hipLaunchKernelGGL((igemm_ws_kernel<T, WC, WP, TC, TP, NSTW, 0, true>), grid, dim3((NW + 4) * 64), sm, st, b);
        else hipLaunchKernelGGL((igemm_ws_kernel<T, WC, WP, TC, TP, NSTW, 0>), grid, dim3((NW + 4) * 64), sm, st, b);
        return hipGetLastError();
      }
    }
    g_prof_family = "dma";
    if (bst && !b.vec_epi) return hipErrorInvalidValue;          // (the backward sums exist in the staged epilogue only: the host asks for them under its conditions)
    if (bst && b.split_c) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, true, 2, true>), grid, dim3(NW * 64), smem, st, b);
    else if (bst) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, true, 2>), grid, dim3(NW * 64), smem, st, b);
    else if (b.vec_epi && b.bn_part) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, true, 1>), grid, dim3(NW * 64), smem, st, b);
    else if (b.vec_epi && b.split_c) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, true, 0, true>), grid, dim3(NW * 64), smem, st, b);
    else if (b.vec_epi) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, true>), grid, dim3(NW * 64), smem, st, b);
    else if (b.split_c) hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, false, 0, true>), grid, dim3(NW * 64), smem, st, b);
    else hipLaunchKernelGGL((igemm_dma_kernel<T, WC, WP, TC, TP, false>), grid, dim3(NW * 64), smem, st, b);
    return hipGetLastError();
  }
  g_prof_family = "reg";
  if (a.bst_y || a.bst_y2) return hipErrorInvalidValue;     // (the staged epilogue of the LDS-DMA kernels only)
  if (a.split_c) return hipErrorInvalidValue;        // the two-output form exists on the LDS-DMA kernels only
  if constexpr (NW == 4) hipLaunchKernelGGL((igemm_kernel<T, WC, WP, TC, TP>), grid, dim3(256), 2 * 4 * (BC + BP) * 16 + 64, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}


// The CK_IGEMM row's launcher (conv_dispatch.hip): the plan's tile (IgemmPlan::cfg, launch.h IgemmCfg), then the reduce pass of a K split
template <typename T> static hipError_t launch_igemm_generic_t(const IgemmArgs& a, int cfg, hipStream_t st) {
  hipError_t e;
  switch (cfg) {
    case IG_128x128: e = launch_igemm_cfg<T, 2, 2, 4, 4>(a, st); break;   // 128 ch x 128 px (the same tile on 8 + 4 waves for small grids: +-0, EXPERIMENTS.md 0.2)
    case IG_64x128: e = launch_igemm_cfg<T, 1, 4, 4, 2>(a, st); break;   //  64 ch x 128 px
    case IG_16x128: e = launch_igemm_cfg<T, 1, 4, 1, 2>(a, st); break;   //  16 ch x 128 px
    case IG_128x32: e = launch_igemm_cfg<T, 4, 1, 2, 2>(a, st); break;   // 128 ch x  32 px
    case IG_128x16: e = launch_igemm_cfg<T, 4, 1, 2, 1>(a, st); break;   // 128 ch x  16 px
    case IG_64x32: e = launch_igemm_cfg<T, 2, 2, 2, 1>(a, st); break;   //  64 ch x  32 px
    case IG_128x256: e = launch_igemm_cfg<T, 2, 4, 4, 4>(a, st); break;   // 128 ch x 256 px, 8 waves
    case IG_256x256: e = launch_igemm_cfg<T, 2, 4, 8, 4>(a, st); break;   // 256 ch x 256 px, 8 waves
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  if (a.splitk > 1) {
    const size_t total = (size_t)a.nclass * a.N * a.Hg * a.Wg * (a.CoutPad / 4);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (a.split_c) hipLaunchKernelGGL((igemm_splitk_reduce_kernel<T, true>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_splitk_reduce_kernel<T>), dim3(blocks), dim3(256), 0, st, a);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_igemm_generic(const IgemmArgs& a, int is_bf16, int cfg, hipStream_t st) {
  return is_bf16 ? launch_igemm_generic_t<bf16>(a, cfg, st) : launch_igemm_generic_t<float>(a, cfg, st);
}

void igemm_tile(int cfg, int* bc, int* bp) {
  static const int t[19][2] = {{128, 128}, {64, 128}, {16, 128}, {128, 32}, {128, 16}, {64, 32}, {128, 256}, {256, 256}, {0, 0}, {0, 0},      // (8, 9: unused)
                               {256, 256}, {128, 512}, {64, 512}, {128, 256}, {64, 256}, {256, 128},     // PATCH_*: patch kernel tiles (conv_ops.h patch_tile_hw)
                               {32, 16}, {32, 32}, {32, 64}};                                               // SMALLP_*: few-pixel kernel (conv_smallp.hip)
  *bc = t[cfg][0]; *bp = t[cfg][1];
}

}  // namespace vp

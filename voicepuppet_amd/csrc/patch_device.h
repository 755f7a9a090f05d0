// What the LDS-patch convolution kernels share (conv_patch.hip: generic stride-1 schedule; conv_patch3.hip: unrolled 3x3 / 4x4;
// conv_patch2.hip: the 2x2-tap parity classes of the 4x4 stride-2 transposed convolutions): the tile and LDS geometry (PatchGeom, read
// by kernels and launchers alike), the tile -> output pixel map, the block -> tile decode, the lane offsets and the issue of the
// weight DMAs and the host launch.  Each kernel keeps what is its own: the step order, the vmcnt arithmetic and which
// weight chunk belongs to which patch position.  For the two unrolled kernels also the inline-asm LDS fragment reads with immediate
// offsets and the MFMAs of one step.  The asm reads, wait_vm and static_steps serve the register-resident
// kernels (conv_c64.hip, conv_dc64.hip, conv_s2c64.hip, bfm_dwproj.hip) as well.
#pragma once
#include <utility>

#include "igemm_device.h"

namespace vp {

// Geometry of a patch tile: WC x WP waves of TC x TP 16 x 16 MFMA blocks compute BC channel rows x TH x TW pixels; per 64-byte channel
// chunk a (TH + HALO) x (TW + HALO) input patch sits in one of two LDS buffers, the weights of a step in one of NSTW ring stages.
// HALO: taps per side - 1 (KW - 1 for the unrolled kernels, 1 for the 2x2-tap classes; the generic kernel, whose kw is a run-time value,
// sizes for 3 - GenericPatchGeom in conv_patch.hip)
template <typename T, int WC_, int WP_, int TC_, int TP_, int TH_, int TW_, int HALO, int NSTW_>
struct PatchGeom {
  static constexpr int WC = WC_, WP = WP_, TC = TC_, TP = TP_, TH = TH_, TW = TW_, NSTW = NSTW_;
  static constexpr int E = Elem<T>::E, KC = 4 * E;                  // elements of a 16-byte piece, of a 64-byte channel chunk
  static constexpr unsigned ES = sizeof(T);
  static constexpr int NW = 8, NT = NW * 64;
  static_assert(WC * WP == NW, "eight waves");
  static constexpr int BC = WC * TC * 16, BP = TH * TW;
  static_assert(BP == WP * TP * 16, "pixel blocks of the tile = pixel blocks of the waves");
  static constexpr int NBA = BC / 16;                                // 16-row weight blocks of a stage
  static_assert(NBA % NW == 0 || NBA == 4, "weight DMAs: whole instructions per wave (64-row tiles: half an instruction per wave)");
  static constexpr int JA = (NBA + NW - 1) / NW;                     // weight DMA instructions per wave and step
  static constexpr bool HALFW = NBA < NW;
  static constexpr int PW = TW + HALO, PH = TH + HALO, NPATCH = PW * PH;
  static constexpr int PPAD = (NPATCH + 127) / 128 * 128;            // patch pixels, padded to whole DMA rounds of the 8 waves
  static constexpr int JP = PPAD / 128;                              // patch DMA instructions per wave and chunk
  static constexpr int PBUFB = PPAD * 64;                            // bytes of one patch buffer
  static constexpr int WSTB = 4 * BC * 16;                           // bytes of one weight stage
  // unrolled kernels: patches first in LDS, the weight ring behind them, every read offset an immediate (the generic kernel puts the
  // ring first and computes its addresses; its tiles pass the assertion all the same)
  static constexpr int WBASE = 2 * PBUFB;
  static_assert(PBUFB + HALO * PW * 64 + 64 < 65536 && (NSTW - 1) * WSTB + 7 * 1024 + 16 < 65536, "read offsets are DS immediates");
  static constexpr int RINGB = NSTW * WSTB + 2 * PBUFB;
  static constexpr int NPASS = epi_passes(BC, BP, WP, RINGB);        // the epilogue stages its f32 tile in the same LDS
  static constexpr int EPIB = (BP / NPASS) * (BC * 4 + 16) + (BP / NPASS) * 8;
  static constexpr int LDS_BYTES = EPIB > RINGB ? EPIB : RINGB;      // dynamic LDS of a launch
};

// output pixel of tile row `row` (pixel block row / 16, lane row % 16) -> offset into Y, -1 outside the image.  STRIDED: grid pixel
// (y, x) of a parity class with origin (oh, ow) lands on output pixel (y * os + oh, x * os + ow)
template <int TW, bool STRIDED = false>
struct PatchTilePix {
  const IgemmArgs& a; int n, y0, x0, oh, ow;
  __device__ __forceinline__ long long operator()(int row) const {
    constexpr int BPR = TW / 16;                         // 16-pixel blocks per tile row
    const int pb = row >> 4, i = row & 15;
    const int y = y0 + pb / BPR, x = x0 + (pb % BPR) * 16 + i;
    if (y >= a.Hg || x >= a.Wg) return -1;
    long long off;
    if constexpr (STRIDED) off = (((long long)n * a.Hof + (y * a.os + oh)) * a.Wof + (x * a.os + ow)) * a.ldY;
    else off = (((long long)n * a.Hof + y) * a.Wof + x) * a.ldY;
    return (off << 8) | (long long)(n / a.ref_group_n);
  }
  // 2x2 max pool of the tile: pooled pixel (row pr, column pc) of this tile -> element offset in the pooled image, -1 outside.
  // Meaningful for 16-pixel-wide tiles (the staged epilogue walks 8 pooled pixels per pooled row) and even image sizes.
  static constexpr bool HAS_POOL = !STRIDED && TW == 16;
  __device__ __forceinline__ long long pool(int pr, int pc) const {
    const int y = (y0 >> 1) + pr, x = (x0 >> 1) + pc;
    if (y >= (a.Hg >> 1) || x >= (a.Wg >> 1)) return -1;
    return (((long long)n * (a.Hg >> 1) + y) * (a.Wg >> 1) + x) * a.ldY;
  }
};

// block index -> pixel tile bt of the launch, its image n and origin (y0, x0)
// xcd_remap: XCD-aware tile order - each XCD a contiguous run of tiles, so that halo pixels meet in one L2.  No change for the
// kernel alone (the shared infinity cache already serves the halos); it takes L2-miss traffic off the fabric the co-running
// streams share
struct PatchTile { int bt, n, y0, x0; };
template <int TH, int TW>
__device__ __forceinline__ PatchTile patch_tile_origin(const IgemmArgs& a, bool xcd_remap = false) {
  const int tiles_x = (a.Wg + TW - 1) / TW, tiles_y = (a.Hg + TH - 1) / TH;
  int bt = blockIdx.x;
  if (xcd_remap && (gridDim.x & 7) == 0) bt = (bt & 7) * (gridDim.x >> 3) + (bt >> 3);
  const int n = bt / (tiles_y * tiles_x);
  const int trem = bt - n * (tiles_y * tiles_x);
  return {bt, n, (trem / tiles_x) * TH, (trem % tiles_x) * TW};
}

// Weight DMAs of a wave: lane offsets of the rb_swz image of a stage (as in igemm_dma_kernel) and the issue of one stage.  64-row tiles
// have four 16-row blocks for eight waves: every wave moves HALF a block (lanes 0-31: 8 rows).  All waves must issue the same number
// of DMAs per step: the loops wait with a counted vmcnt, which counts the wave's own instructions only
template <typename G>
struct PatchWeightDma {
  unsigned wvo[G::JA];
  int wave, lane;
  __device__ __forceinline__ PatchWeightDma(int c_base, int wave_, int lane_) : wave(wave_), lane(lane_) {
    const int r = G::HALFW ? (wave & 1) * 8 + (lane >> 2) : lane >> 2;       // row inside the 16-row block
    const int g = (lane & 3) ^ rb_swz(r & 15);
#pragma unroll
    for (int j = 0; j < G::JA; ++j) {
      const int blk = G::HALFW ? (wave >> 1) : wave + G::NW * j;
      wvo[j] = (unsigned)(((c_base + blk * 16 + r) * G::KC + g * G::E) * G::ES);
    }
  }
  // the chunk at byte offset wso of the packed weights -> ring stage la
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsW, unsigned wso, uint4* la) const {
    if constexpr (G::HALFW) {
      if (lane < 32) dma16_buf(rsW, wvo[0], wso, la + (wave >> 1) * 64 + (wave & 1) * 32);
    } else {
#pragma unroll
      for (int j = 0; j < G::JA; ++j) dma16_buf(rsW, wvo[j], wso, la + (wave + G::NW * j) * 64);
    }
  }
};

// Fragment reads as inline asm.  hipcc drains vmcnt in front of every LDS load it can see while an LDS-DMA is pending (the
// __restrict__ route of conv_patch.hip loses its alias scopes in this fully unrolled form), which would serialise the DMA stream;
// the ring discipline of the loop - counted vmcnt + barrier - is what orders these reads.  The destination registers are only
// valid behind lds_fence() (s_waitcnt lgkmcnt(0) + a dependency on every register, so that no consumer is scheduled above it).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <int IMM> __device__ __forceinline__ u32x2 lds_rd64(int addr) {
  u32x2 r;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(IMM));
  return r;
}
template <int IMM> __device__ __forceinline__ u32x4 lds_rd128(int addr) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(IMM));
  return r;
}
// second half of a B piece: address ^ 8, formed inside the asm so that it never occupies a register across steps
template <int IMM> __device__ __forceinline__ u32x2 lds_rd64_x8(int addr) {
  u32x2 r;
  int t;
  asm volatile("v_xor_b32 %1, 8, %2\n\tds_read_b64 %0, %1 offset:%3" : "=v"(r), "=&v"(t) : "v"(addr), "n"(IMM));
  return r;
}
// B fragments of the step + the A fragments [A0, A0 + NA) of the wave, valid on return
template <int NA, int TP, int AIMM, int BIMM, bool WITH_B>
__device__ __forceinline__ void patch_frag_read_imm(int aaddr, const int (&b0)[TP], uint4 (&fa)[NA], uint4 (&fb)[TP]) {
  u32x4 ra[NA];
  u32x2 rl[TP], rh[TP];
  if constexpr (WITH_B) {
#pragma unroll
    for (int t = 0; t < TP; ++t) { rl[t] = lds_rd64<BIMM>(b0[t]); rh[t] = lds_rd64_x8<BIMM>(b0[t]); }
  }
  static_assert(NA == 2 || NA == 4, "weight blocks per read batch");
  ra[0] = lds_rd128<AIMM>(aaddr); ra[1] = lds_rd128<AIMM + 1024>(aaddr);
  if constexpr (NA >= 4) { ra[2] = lds_rd128<AIMM + 2048>(aaddr); ra[3] = lds_rd128<AIMM + 3072>(aaddr); }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (WITH_B) {
#pragma unroll
    for (int t = 0; t < TP; ++t) { asm volatile("" : "+v"(rl[t])); asm volatile("" : "+v"(rh[t])); fb[t] = make_uint4(rl[t].x, rl[t].y, rh[t].x, rh[t].y); }
  }
#pragma unroll
  for (int t = 0; t < NA; ++t) { asm volatile("" : "+v"(ra[t])); fa[t] = make_uint4(ra[t].x, ra[t].y, ra[t].z, ra[t].w); }
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <typename F, int... Is> __device__ __forceinline__ void static_steps(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}

// The MFMAs of one step (TC weight blocks x TP pixel blocks per wave; stage / buffer / tap offsets are the immediates AIMM, BIMM).
// Weight blocks are read in batches of NA (register budget).  Two batches: rolling form - a block's registers are refilled with
// block + NA as soon as its MFMAs are issued, so the second batch lands under the first batch's MFMAs (VP_P3_NO_ROLL: batch by batch).  ROLL: the 3x3 kernel (128x256 tile
// 940 -> 970 TF); the 2x2-tap kernel measured 1.5 % slower with it
template <typename T, int TC, int TP, int NA, int AIMM, int BIMM, bool ROLL>
__device__ __forceinline__ void patch_step_mma(int aaddr, const int (&b0)[TP], f32x4 (&acc)[TC][TP]) {
  uint4 fb[TP];
#ifndef VP_P3_NO_ROLL
  if constexpr (ROLL && TC / NA == 2) {
    uint4 fa[NA];
    u32x4 rn[NA];
    patch_frag_read_imm<NA, TP, AIMM, BIMM, true>(aaddr, b0, fa, fb);
    static_steps([&](auto tci) {
      constexpr int tc = decltype(tci)::value;
#pragma unroll
      for (int tp = 0; tp < TP; ++tp) acc[tc][tp] = mma16<T>(fa[tc], fb[tp], acc[tc][tp]);
      __builtin_amdgcn_sched_barrier(0);
      rn[tc] = lds_rd128<AIMM + (NA + tc) * 1024>(aaddr);
      __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, NA>{});
    static_steps([&](auto tci) {
      constexpr int tc = decltype(tci)::value;
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NA - 1 - tc) : "memory");
      asm volatile("" : "+v"(rn[tc]));
      const uint4 f = make_uint4(rn[tc].x, rn[tc].y, rn[tc].z, rn[tc].w);
#pragma unroll
      for (int tp = 0; tp < TP; ++tp) acc[NA + tc][tp] = mma16<T>(f, fb[tp], acc[NA + tc][tp]);
      __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, NA>{});
    return;
  }
#endif
  static_steps([&](auto hi) {
    constexpr int h = decltype(hi)::value;
    uint4 fa[NA];
    patch_frag_read_imm<NA, TP, AIMM + h * NA * 1024, BIMM, h == 0>(aaddr, b0, fa, fb);
#pragma unroll
    for (int tc = 0; tc < NA; ++tc)
#pragma unroll
      for (int tp = 0; tp < TP; ++tp) acc[h * NA + tc][tp] = mma16<T>(fa[tc], fb[tp], acc[h * NA + tc][tp]);
  }, std::make_integer_sequence<int, TC / NA>{});
}


// launch of a patch kernel of geometry G: one block per (pixel tile, BC channel rows, class)
template <typename G, typename K>
hipError_t launch_patch_grid(K kern, const IgemmArgs& b, int nclass, hipStream_t st) {
  const int tiles = b.N * ((b.Hg + G::TH - 1) / G::TH) * ((b.Wg + G::TW - 1) / G::TW);
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
  hipLaunchKernelGGL(kern, dim3(tiles, b.CoutPad / G::BC, nclass), dim3(G::NT), G::LDS_BYTES, st, b);
  return hipGetLastError();
}

}  // namespace vp

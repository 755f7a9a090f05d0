// igemm_patch3_kernel: the 3x3 / stride-1 form of the patch kernel (conv_patch.hip) with the whole (chunk pair x tap) schedule
// unrolled.  PMC counters of the generic kernel on VGG conv1_2 (profiles/r02_pmc_sq_patch.txt): 7.6 vector-ALU and 9 scalar
// instructions per MFMA - fragment addresses (a swizzle of pixel index + tap offset), tap / ring / chunk cursors, a branch tree for
// the per-step patch DMA - and a vmcnt that waited for the patch DMA issued one step earlier.  Here
//   * the patch swizzle depends on the COLUMN of a patch pixel only (slot = piece ^ ((px >> 2) & 3)): a tap's row shift is a
//     plain byte offset.  With the taps unrolled the row shift, the buffer of the chunk and the ring stage are instruction
//     immediates; the lane part of a B address is one of 3 (column shifts) x TP precomputed registers, of an A address one
//     register.  A step issues NO vector ALU and a handful of scalar instructions;
//   * the counted vmcnt of every step is exact (a compile-time function of the tap): only the weights of the step, never a patch
//     DMA issued in the last two steps, are waited for;
//   * patches first in LDS (their read offsets fit the 16-bit DS immediate), the weight ring behind them.
// Bank behaviour of the fragment reads is that of conv_patch.hip: of the 16 consecutive pixels of a B fragment, the four that share
// an address class (pp & 3) have four different (px >> 2) & 3, so a 32-lane service group of a ds_read_b64 hits 32 distinct 8-byte
// slots for every column shift.  Two chunks (K = 2 x 64 bytes per tap) per trip: channel counts are multiples of 64 (bf16) / 32 (f32).
#include <stdlib.h>
// outputs of this kernel are the perceptual trunk's full-resolution tensors (34-270 MB per launch): streamed stores (`nt`) in the
// epilogue - batch 32: 8.25 -> 8.19 ms, every class of this file +1 %; for the other kernel families the hint is neutral (section 11)
#ifndef VP_P3_NO_NT
#define VP_NT_STORE 1
#endif
// VP_P3_ABL: build-time ablations of the loop for timing only (results are wrong): 1 no barrier, 2 no vmcnt wait, 4 no DMA in the
// loop, 8 no epilogue, 16 no loop (make ablate3 ABL=n -> ../libvp_p3abl<n>.so, select with VP_LIB)
#ifndef VP_P3_ABL
#define VP_P3_ABL 0
#endif

#include <utility>

#include "conv_ops.h"
#include "igemm_device.h"
#include "launch.h"
#include "patch_device.h"

namespace vp {

template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int NSTW, int KW>
using Patch3Geom = PatchGeom<T, WC, WP, TC, TP, TH, TW, KW - 1, NSTW>;

// NSTW: stages of the weight ring = NSTW - 1 steps of weights in flight.  A step of a 64-row tile is 8 MFMAs per wave, far shorter than
// the 1-1.5 us an LDS-DMA takes to land under load: with 3 stages the loop ran at the DMA latency (0.7 us per step whatever the tile),
// with 6 the weights of five steps are in flight.  18 steps per trip: NSTW divides 18, stage indices stay compile-time.
// KW: 3 (3x3 taps) or 4 (4x4 taps: the discriminator's layer_4 backward-data passes, round 5 - 32 steps per trip, four ring stages)
template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int STATS, int OCC, int NSTW = 3, int KW = 3>
__global__ __launch_bounds__(512, OCC) void igemm_patch3_kernel(const IgemmArgs a) {
  using G = Patch3Geom<T, WC, WP, TC, TP, TH, TW, NSTW, KW>;
  constexpr int E = G::E, KC = G::KC, NW = G::NW, LA = NSTW - 1;
  constexpr int KS2 = KW * KW, TRIP = 2 * KS2;                       // patch positions of a chunk, steps of a trip (two chunks)
  static_assert(TRIP % NSTW == 0 && NSTW >= 3, "ring stages");
  constexpr int JA = G::JA, PW = G::PW, JP = G::JP, PBUFB = G::PBUFB, WSTB = G::WSTB, WBASE = G::WBASE;
  static_assert(JP + LA <= KS2, "one patch DMA per tap step, none in the last LA steps of a chunk");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c_base = blockIdx.y * G::BC;
  const PatchTile tile = patch_tile_origin<TH, TW>(a, a.xcd_remap);
  const int n = tile.n, y0 = tile.y0, x0 = tile.x0;
  // tap t = 3r + c reads input pixel (y + p_dhf + r * p_dhs, x + p_dwf + c * p_dws); both steps are +1 (forward) or both -1
  // (backward-data: the flipped kernel).  The loop walks PATCH positions (pr, pc) in a fixed order; the weight chunk that belongs
  // to patch position u is tap u (forward) or tap 8 - u (flipped)
  const bool flip = a.p_dhs < 0;
  const int dh0 = flip ? a.p_dhf - (KW - 1) : a.p_dhf, dw0 = flip ? a.p_dwf - (KW - 1) : a.p_dwf;
  const unsigned es = sizeof(T);
  const int C0 = a.x.C[0];
  const int nchunkc = C0 / KC;                  // channel chunks (even)

  __amdgpu_buffer_rsrc_t rsW = make_rsrc(reinterpret_cast<const T*>(a.Wp), 0xFFFFFFFFu);
  __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * C0 * es));

  // patch DMA lanes: instruction j of this wave covers patch pixels (wave + 8j) * 16 .. + 15, lane -> (pixel, slot)
  unsigned pvo[JP];
#pragma unroll
  for (int j = 0; j < JP; ++j) {
    const int pp = (wave + NW * j) * 16 + (lane >> 2);
    const int py = pp / PW, px = pp - py * PW;
    const int ih = y0 + dh0 + py, iw = x0 + dw0 + px;
    const bool ok = pp < G::NPATCH && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
    const int piece = (lane & 3) ^ ((px >> 2) & 3);
    pvo[j] = ok ? (unsigned)((((n * a.Hin + ih) * a.Win + iw) * C0 + piece * E) * es) : DMA_OOB;
  }
  const PatchWeightDma<G> wdma(c_base, wave, lane);
  const unsigned wstep = (unsigned)(a.wp_rows * KC * es);
  // weights of patch position u (tap u or 8 - u) and channel chunk c -> ring stage `stage`
  auto issue_w = [&](int u, int chunk, int stage) {
    const int tap = flip ? KS2 - 1 - u : u;
    wdma.issue(rsW, (unsigned)(tap * nchunkc + chunk) * wstep, reinterpret_cast<uint4*>(smem + WBASE + stage * WSTB));
  };
  auto issue_p = [&](int chunk, int buf, int j) {
    uint4* lb = reinterpret_cast<uint4*>(smem + buf * PBUFB);
    dma16_buf(rsX, pvo[j], (unsigned)(chunk * KC) * es, lb + (wave + NW * j) * 64);
  };

  const int wc = wave / WP, wpi = wave - wc * WP;
  const int blkA0 = wc * TC, blkB0 = wpi * TP;
  const int fi = lane & 15, fg = lane >> 4;
  const int aaddr = WBASE + (blkA0 * 64 + fi * 4 + (fg ^ rb_swz(fi))) * 16;     // (ring base folded in: stage and block offsets fit the immediate)
  // B fragment lane offsets per column shift c: patch pixel (row of the pixel block, its first column + lane + c)
  int tb0[KW][TP];
#pragma unroll
  for (int c = 0; c < KW; ++c)
#pragma unroll
    for (int q = 0; q < TP; ++q) {
      constexpr int BPR = TW / 16;
      const int pb = blkB0 + q;
      const int px = (pb % BPR) * 16 + fi + c;
      const int pp = (pb / BPR) * PW + px;
      tb0[c][q] = (pp << 6) + (((fg ^ (px >> 2)) & 3) << 4) + ((fg & 1) << 3);
    }

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // prologue: the whole first patch, then the weights of the first LA steps
#pragma unroll
  for (int j = 0; j < JP; ++j) issue_p(0, 0, j);
#pragma unroll
  for (int d = 0; d < LA; ++d) issue_w(d % KS2, d / KS2, d % NSTW);

  // One trip = 2 chunks x 9 patch positions.  Step U = 9 * cc + u (cc: chunk of the pair = patch buffer, u: patch position);
  // ring stage U % NSTW.  In DMA order behind the weights of step U (issued at step U - LA): the patch piece of step U - LA, then per
  // later step its weights and its patch piece - a piece is issued at the steps with u < JP, always (behind the last chunk it
  // fetches bytes nobody reads, into the idle buffer)
  for (int c = 0; c < ((VP_P3_ABL & 16) ? 0 : nchunkc); c += 2) {
    const bool last_pair = c + 2 >= nchunkc;
    auto step = [&](auto uc) {
      constexpr int U = decltype(uc)::value;
      constexpr int cc = U / KS2, u = U % KS2, pr = u / KW, pc = u % KW, stage = U % NSTW;
      // DMAs issued behind the weights of this step: the patch pieces of the LA previous steps, the weights of the LA - 1 next ones
      constexpr int NPIECE = [] { int n = 0; for (int k = 1; k <= LA; ++k) n += ((U + TRIP - k) % TRIP % KS2) < JP ? 1 : 0; return n; }();
      constexpr int NV = (LA - 1) * JA + NPIECE;
      constexpr int WLAST = (TRIP - 1 - U < LA - 1 ? TRIP - 1 - U : LA - 1);                 // behind the last pair no weights of a next trip follow
#if !(VP_P3_ABL & 2)
      if (U + LA - 1 > TRIP - 1 && last_pair) wait_vm<WLAST * JA + NPIECE>();
      else wait_vm<NV>();
#endif
#if !(VP_P3_ABL & 1)
      __builtin_amdgcn_s_barrier();
#endif
      asm volatile("" ::: "memory");
      // weights LA steps ahead (ring stage (U + LA) % NSTW, last read in step U - 1)
#if !(VP_P3_ABL & 4)
      {
        constexpr int UL = (U + LA) % TRIP;
        if (U + LA < TRIP) issue_w(UL % KS2, c + UL / KS2, (U + LA) % NSTW);
        else if (!last_pair) issue_w(UL % KS2, c + 2 + UL / KS2, (U + LA) % NSTW);
      }
      if constexpr (u < JP) issue_p(c + cc + 1, 1 - cc, u);
#endif
      // eight weight blocks per wave: two read batches of four (16 fragment registers instead of 32); the 64-accumulator tile at
      // two blocks per CU (128 registers per lane): batches of two
      constexpr int NA = TC == 8 ? 4 : ((TC == 4 && OCC == 4) ? 2 : TC);
      patch_step_mma<T, TC, TP, NA, stage * WSTB, cc * PBUFB + pr * PW * 64, true>(aaddr, tb0[pc], acc);
    };
    static_steps(step, std::make_integer_sequence<int, TRIP>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the trailing patch pieces: the epilogue reuses the LDS

#ifndef VP_P3_NO_FASTEPI
  constexpr int NPASS16 = G::BC == 64 ? epi_passes16(G::BC, G::BP, WP, G::RINGB) : 0;    // 64-row tiles: +4 %; 128 rows: -8 %, 256 rows: +-0
#else
  constexpr int NPASS16 = 0;
#endif
  if (!(VP_P3_ABL & 8) || acc[0][0][0] == 1.2345f) staged_epilogue<T, TC, TP, G::BC, G::BP, G::NPASS, G::NT, STATS, NPASS16>(a, PatchTilePix<TW>{a, n, y0, x0}, c_base, blkA0, blkB0, acc, smem, tile.bt, 0);
}

template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int OCC, int NSTW = 3, int KW = 3>
static hipError_t launch_patch3_t(const IgemmArgs& b, hipStream_t st) {
  auto kern = b.bn_part ? igemm_patch3_kernel<T, WC, WP, TC, TP, TH, TW, 1, OCC, NSTW, KW> : igemm_patch3_kernel<T, WC, WP, TC, TP, TH, TW, 0, OCC, NSTW, KW>;
  if (b.bst_y) {       // backward sums of a batch-normalised tensor (the discriminator's layer_3 under layer_4's backward-data): the 4x4 form only
    if constexpr (KW == 4) kern = igemm_patch3_kernel<T, WC, WP, TC, TP, TH, TW, 2, OCC, NSTW, KW>;
    else return hipErrorInvalidValue;
  }
  return launch_patch_grid<Patch3Geom<T, WC, WP, TC, TP, TH, TW, NSTW, KW>>(kern, b, 1, st);
}

// 3x3 taps on a +1 / +1 or -1 / -1 grid, an even number of 64-byte channel chunks: what the unrolled kernel handles
bool patch3_eligible(const IgemmArgs& a, int is_bf16) {
  const int kc = is_bf16 ? 32 : 16;
  return conv_staging(a.kern) == CK_PATCH && a.ntaps == 9 && a.p_kw == 3 && a.p_dhs == a.p_dws && (a.p_dhs == 1 || a.p_dhs == -1) && a.x.C[0] % (2 * kc) == 0 &&
         a.x.C[1] == 0;
}

// 4x4 taps (stride 1) on the same kernel (the discriminator's layer_4: forward with its batch statistics, backward-data): bf16, channel
// rows a multiple of 128: the 128-row x 16 x 16-pixel tile (80 KB of LDS with four ring stages: two blocks per CU; the 256-row tile would
// need 96 KB) - plan_make_patch names that tile for 4x4 layers
bool patch4_eligible(const IgemmArgs& a, int is_bf16) {
  return is_bf16 && conv_staging(a.kern) == CK_PATCH && a.ntaps == 16 && a.p_kw == 4 && a.p_dhs == a.p_dws && (a.p_dhs == 1 || a.p_dhs == -1) &&
         a.x.C[0] % 64 == 0 && a.x.C[1] == 0 && a.CoutPad % 128 == 0 && !a.pool_out;
}
hipError_t launch_igemm_patch4(const IgemmArgs& a, hipStream_t st) {
  IgemmArgs b = a;
  b.vec_epi = 1;
  b.xcd_remap = patch_xcd_knob();
  return launch_patch3_t<bf16, 2, 4, 4, 4, 16, 16, 4, 4, 4>(b, st);
}

// same tile menu as launch_igemm_patch (conv_patch.hip)
hipError_t launch_igemm_patch3(const IgemmArgs& a, int is_bf16, int bc, int bp, hipStream_t st) {
  IgemmArgs b = a;
  b.vec_epi = 1;
  b.xcd_remap = patch_xcd_knob();
#define VP_PATCH3_GO(WC, WP, TC, TP, TH, TW, OCC) \
  (is_bf16 ? launch_patch3_t<bf16, WC, WP, TC, TP, TH, TW, OCC>(b, st) : launch_patch3_t<float, WC, WP, TC, TP, TH, TW, OCC>(b, st))
#define VP_PATCH3_GO6(WC, WP, TC, TP, TH, TW, OCC) \
  (is_bf16 ? launch_patch3_t<bf16, WC, WP, TC, TP, TH, TW, OCC, 6>(b, st) : launch_patch3_t<float, WC, WP, TC, TP, TH, TW, OCC, 6>(b, st))
  // 64-row tiles of 16 x 16 pixels: six weight stages (73 KB of LDS, still two blocks per CU; the three-stage form: EXPERIMENTS.md 6 (5))
  if (bc == 256) return bp == 128 ? VP_PATCH3_GO(2, 4, 8, 2, 8, 16, 4) : VP_PATCH3_GO(2, 4, 8, 4, 16, 16, 2);
  if (bc == 128) return bp == 512 ? VP_PATCH3_GO(1, 8, 8, 4, 16, 32, 2) : VP_PATCH3_GO(2, 4, 4, 4, 16, 16, 4);
  if (bp == 512) return VP_PATCH3_GO(1, 8, 4, 4, 16, 32, 2);
  return VP_PATCH3_GO6(2, 4, 2, 4, 16, 16, 4);
#undef VP_PATCH3_GO6
#undef VP_PATCH3_GO
}

}  // namespace vp

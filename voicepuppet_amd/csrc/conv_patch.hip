// igemm_patch_kernel: stride-1 convolutions (VGG 3x3, discriminator layer_4 4x4 and their backward-data passes) with the INPUT
// PATCH STAGED ONCE PER CHANNEL CHUNK.  The gather-per-tap kernels (conv_kernels.hip) DMA every input pixel into LDS once per tap
// (9 or 16 times) and are bound by that L2 -> LDS traffic, not by the matrix pipe.  Here a block owns a 2-D
// tile of TH x TW output pixels of one image; per 64-byte channel chunk the (TH + kh - 1) x (TW + kw - 1) input patch is DMA'd into
// LDS ONCE and all taps read their B fragments from shifted positions of it; only the weights (BC x 64 bytes per tap) stream per tap.
// DMA bytes per MAC drop 1.75x (256 ch x 16x16 px), 3.2x (128 ch x 16x32 px) and 5x (64 ch x 16x32 px).
//
// LDS image of the patch: pixel pp = py * PW + px owns 64 consecutive bytes = four 16-byte k-pieces, piece p stored at slot
// p ^ ((pp >> 2) & 3).  A B fragment = 16 consecutive pixels of one patch row starting ANYWHERE (the tap shift), lane (i, g) needs
// piece g of pixel pp0 + i.  It is read as two ds_read_b64 (each serviced in two 32-lane groups over a 256-byte bank window): lanes
// with even g take the low 8 bytes first, lanes with odd g the high 8 bytes first.  Inside a window the four pixels of a class
// (pp & 3) carry (pp >> 2) & 3 = all four values, so the 8 lanes of a class (4 pixels x 2 values of g) hit 8 distinct 8-byte slots:
// conflict-free for every shift.  The price - odd k-groups arrive with their two halves swapped - is paid once by the weight
// packer (PackDesc::kswap stores the same permutation of k in the A operand; a permutation of k common to A and B leaves the
// product unchanged).
//
// Pipeline: step s = (chunk c, tap t); weights of step s in ring stage s % NSTW (issued NSTW-1 steps ahead); patch of chunk c in
// buffer c & 1, the next chunk's patch is issued one DMA instruction per step over the first steps of chunk c (after the barrier
// that retires the last reads of the buffer it overwrites).  One barrier per step, counted vmcnt, every wave issues its share of
// the DMAs; 8 waves (two per SIMD), 128 (or 64) accumulator registers per lane, one block per CU.
#include <stdlib.h>

#include "igemm_device.h"
#include "launch.h"
#include "conv_ops.h"
#include "patch_device.h"

namespace vp {

// kw is a run-time value in this kernel: its patch buffers are sized for HALO = 3, the widest layer it serves (4x4); PW / PH of a
// launch are TW / TH + kw - 1 <= the geometry's
template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int NSTW>
using GenericPatchGeom = PatchGeom<T, WC, WP, TC, TP, TH, TW, 3, NSTW>;

// fragment reads behind __restrict__ parameters: keeps hipcc from draining vmcnt in front of LDS reads that may alias a pending
// LDS-DMA (EXPERIMENTS.md, "double-buffered register fragments", has the story); the counted vmcnt + barrier of the loop is what orders them
template <int TC, int TP>
__device__ __forceinline__ void patch_frag_read_restrict(const uint4* __restrict__ pa, const char* __restrict__ pbuf, const int (&boff)[TP],
                                                uint4 (&fa)[TC], uint4 (&fb)[TP]) {
#pragma unroll
  for (int t = 0; t < TP; ++t) {
    const uint2 r1 = *reinterpret_cast<const uint2*>(pbuf + boff[t]);
    const uint2 r2 = *reinterpret_cast<const uint2*>(pbuf + (boff[t] ^ 8));
    fb[t] = make_uint4(r1.x, r1.y, r2.x, r2.y);
  }
#pragma unroll
  for (int t = 0; t < TC; ++t) fa[t] = pa[t * 64];
}

template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int NSTW, int STATS, int OCC>
__global__ __launch_bounds__(WC * WP * 64, OCC) void igemm_patch_kernel(const IgemmArgs a) {
  using G = GenericPatchGeom<T, WC, WP, TC, TP, TH, TW, NSTW>;
  constexpr int E = G::E, KC = G::KC, NW = G::NW, JA = G::JA, JP = G::JP;
  constexpr int WST = G::WSTB / 16;                                  // uint4 slots of one weight stage
  constexpr int PBUF = G::PBUFB / 16;                                // uint4 slots of one patch buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* lds = reinterpret_cast<uint4*>(smem);
  uint4* lpatch = lds + NSTW * WST;                                  // the ring first, the patches behind it

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c_base = blockIdx.y * G::BC;
  const PatchTile tile = patch_tile_origin<TH, TW>(a);
  const int n = tile.n, y0 = tile.y0, x0 = tile.x0;
  // tap t = r * kw + c  ->  (dh, dw) = (p_dhf + r * p_dhs, p_dwf + c * p_dws)
  const int kw = a.p_kw, kh = a.ntaps / kw;
  const int dh0 = a.p_dhs > 0 ? a.p_dhf : a.p_dhf - (kh - 1), dw0 = a.p_dws > 0 ? a.p_dwf : a.p_dwf - (kw - 1);
  const int PW = TW + kw - 1, PH = TH + kh - 1;
  const int npatch = PW * PH;
  const unsigned es = sizeof(T);
  const int C0 = a.x.C[0];
  const int nchunkc = C0 / KC;                  // channel chunks
  const int S = nchunkc * a.ntaps;              // steps

  __amdgpu_buffer_rsrc_t rsW = make_rsrc(reinterpret_cast<const T*>(a.Wp), 0xFFFFFFFFu);
  __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * C0 * es));

  // patch DMA lanes: instruction j of this wave covers patch pixels (wave + 8j) * 16 .. + 15, lane -> (pixel, slot)
  unsigned pvo[JP];
#pragma unroll
  for (int j = 0; j < JP; ++j) {
    const int pp = (wave + NW * j) * 16 + (lane >> 2);
    const int py = pp / PW, px = pp - py * PW;
    const int ih = y0 + dh0 + py, iw = x0 + dw0 + px;
    const bool ok = pp < npatch && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
    const int piece = (lane & 3) ^ ((pp >> 2) & 3);
    pvo[j] = ok ? (unsigned)((((n * a.Hin + ih) * a.Win + iw) * C0 + piece * E) * es) : DMA_OOB;
  }
  const PatchWeightDma<G> wdma(c_base, wave, lane);
  const unsigned wstep = (unsigned)(a.wp_rows * KC * es);
  // weight issue cursor: step (wc_c, wc_t) -> packed chunk index wc_t * nchunkc + wc_c (tap-major K)
  int wc_c = 0, wc_t = 0, wc_stage = 0;
  auto issue_w = [&]() {
    wdma.issue(rsW, (unsigned)(wc_t * nchunkc + wc_c) * wstep, lds + wc_stage * WST);
    if (++wc_t == a.ntaps) { wc_t = 0; ++wc_c; }
    wc_stage = wc_stage == NSTW - 1 ? 0 : wc_stage + 1;
  };
  auto issue_p = [&](int chunk, int j) {        // j: compile-time after unrolling at the call sites
    uint4* lb = lpatch + (chunk & 1) * PBUF;
    dma16_buf(rsX, pvo[j], (unsigned)(chunk * KC) * es, lb + (wave + NW * j) * 64);
  };

  const int wc = wave / WP, wpi = wave - wc * WP;
  const int blkA0 = wc * TC, blkB0 = wpi * TP;
  const int fi = lane & 15, fg = lane >> 4;
  const int so = fi * 4 + (fg ^ rb_swz(fi));
  // B fragments: patch pixel of (pixel block t, lane) at tap offset 0
  int bpp[TP];
#pragma unroll
  for (int t = 0; t < TP; ++t) {
    constexpr int BPR = TW / 16;
    const int pb = blkB0 + t;
    bpp[t] = (pb / BPR) * PW + (pb % BPR) * 16 + fi;
  }

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // prologue: the whole first patch, then the first NSTW-1 weight stages
#pragma unroll
  for (int j = 0; j < JP; ++j) issue_p(0, j);
#pragma unroll
  for (int d = 0; d < NSTW - 1; ++d) if (d < S) issue_w();

  int c = 0, t = 0, st = 0;
  int tr = 0, tcol = 0;                          // tap row / column of step s
  for (int s = 0; s < S; ++s) {
    if (s + NSTW - 2 < S) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTW - 2) * JA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + NSTW - 1 < S) issue_w();
    if (t < JP && c + 1 < nchunkc) {
#pragma unroll
      for (int j = 0; j < JP; ++j) if (j == t) issue_p(c + 1, j);
    }
    // fragments of step s
    const int tapoff = (a.p_dhf + tr * a.p_dhs - dh0) * PW + (a.p_dwf + tcol * a.p_dws - dw0);
    int boff[TP];
#pragma unroll
    for (int q = 0; q < TP; ++q) {
      const int pp = bpp[q] + tapoff;
      boff[q] = (pp << 6) + (((fg ^ (pp >> 2)) & 3) << 4) + ((fg & 1) << 3);
    }
    uint4 fa[TC], fb[TP];
    patch_frag_read_restrict<TC, TP>(lds + st * WST + blkA0 * 64 + so, reinterpret_cast<const char*>(lpatch + (c & 1) * PBUF), boff, fa, fb);
#pragma unroll
    for (int tc = 0; tc < TC; ++tc)
#pragma unroll
      for (int tp = 0; tp < TP; ++tp) acc[tc][tp] = mma16<T>(fa[tc], fb[tp], acc[tc][tp]);
    st = st == NSTW - 1 ? 0 : st + 1;
    if (++tcol == kw) { tcol = 0; ++tr; }
    if (++t == a.ntaps) { t = 0; tr = 0; ++c; }
  }

  staged_epilogue<T, TC, TP, G::BC, G::BP, G::NPASS, G::NT, STATS>(a, PatchTilePix<TW>{a, n, y0, x0}, c_base, blkA0, blkB0, acc, smem, tile.bt, 0);
}

// OCC: waves per SIMD the register allocation must allow (2: one 8-wave block per CU, 4: two)
template <typename T, int WC, int WP, int TC, int TP, int TH, int TW, int NSTW, int OCC>
static hipError_t launch_patch_t(const IgemmArgs& b, hipStream_t st) {
  if (b.bst_y || b.bst_y2) return hipErrorInvalidValue;      // (backward sums in the epilogue: the unrolled 4x4 kernel and the 2x2-tap kernel only; the host asks accordingly)
  auto kern = b.bn_part ? igemm_patch_kernel<T, WC, WP, TC, TP, TH, TW, NSTW, 1, OCC> : igemm_patch_kernel<T, WC, WP, TC, TP, TH, TW, NSTW, 0, OCC>;
  return launch_patch_grid<GenericPatchGeom<T, WC, WP, TC, TP, TH, TW, NSTW>>(kern, b, 1, st);
}

// bc: channel rows of the tile, bp: pixels of the tile (128: 8 x 16, 256: 16 x 16, 512: 16 x 32).  The 256-pixel tiles of the 128- and 64-row
// variants run TWO blocks per CU (64 / 32 accumulator registers, 72 / 60 KB of LDS): the blocks are not in lockstep with each
// other, so one block's barrier / DMA-issue / ds_read phase overlaps the other's MFMAs.
hipError_t launch_igemm_patch(const IgemmArgs& a, int is_bf16, int bc, int bp, hipStream_t st) {
  IgemmArgs b = a;
  b.vec_epi = 1;
#define VP_PATCH_GO(WC, WP, TC, TP, TH, TW, NS, OCC) \
  (is_bf16 ? launch_patch_t<bf16, WC, WP, TC, TP, TH, TW, NS, OCC>(b, st) : launch_patch_t<float, WC, WP, TC, TP, TH, TW, NS, OCC>(b, st))
  if (bc == 256) return bp == 128 ? VP_PATCH_GO(2, 4, 8, 2, 8, 16, 3, 4) : VP_PATCH_GO(2, 4, 8, 4, 16, 16, 4, 2);
  if (bc == 128) return bp == 512 ? VP_PATCH_GO(1, 8, 8, 4, 16, 32, 4, 2) : VP_PATCH_GO(2, 4, 4, 4, 16, 16, 3, 4);
  return bp == 512 ? VP_PATCH_GO(1, 8, 4, 4, 16, 32, 4, 2) : VP_PATCH_GO(2, 4, 2, 4, 16, 16, 3, 4);
#undef VP_PATCH_GO
}

}  // namespace vp

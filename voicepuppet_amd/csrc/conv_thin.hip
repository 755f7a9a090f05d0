// Thin-channel convolution kernels (bf16): layers with 8 or fewer channels on one side, where a tiled GEMM is all prologue and epilogue.
//   conv_cin8_kernel           8-channel (padded image) inputs, 64 outputs: pieces straight from global memory, weights as LDS fragments
//   deconv_cout4_tile_kernel   4x4 stride-2 transposed conv to 4 channels, f32 output (decoder_1): 4 parity classes x 4 channels = one MFMA tile
//   conv3x3_cout8_tile_kernel  3x3 stride-1 conv from 64 to <= 8 channels (VGG conv1_1 backward-data)
//   deconv_cout8_tile_kernel   4x4 stride-2 transposed conv from 64 to <= 8 channels (discriminator layer_1 backward-data)
// The three tile kernels and their launchers take the halo tile's geometry and the LDS sizes from thin_device.h; the tile schedule, the
// halo staging and the weight image are written out in each kernel (shared helpers changed the register allocation and put branches
// into the tile loops: profiles/thin_tile_isa_ab.txt).  Each kernel's preconditions (conv_*_eligible) and launcher (launch_conv_*) are at
// the end of the file.
#include "conv_ops.h"
#include "igemm_device.h"
#include "launch.h"
#include "thin_device.h"
#include "vp_common.h"

namespace vp {

// ------------------------------------------------------------------------------------------------
// conv_cin8_kernel: the first layers of the three nets (3- and 6-channel images padded to 8: VGG conv1_1, discriminator layer_1,
// encoder_1, encoder_fg_1; all 64 output channels, bf16).  K = taps x 8 is only 3-4 MFMA steps, so a tiled GEMM is all
// prologue and epilogue; these layers are bound by writing the output (8 channels in, 64 out).  Direct form, no LDS:
//   * a tap of a padded pixel is exactly one 16-byte piece = the 8 k values one lane feeds to mfma 16x16x32; lane (pixel i,
//     k group g) loads tap 4s+g of its pixel for MFMA step s straight from global memory (buffer load: padding reads zeros);
//   * the whole weight matrix (64 x K) sits in registers as A fragments for the life of the wave (S x 4 x 4 VGPRs);
//   * MFMA row (tile t, 4q+e) is channel 32*(t>>1) + 8q + 4*(t&1) + e, so after the 4 tiles a lane holds channels 8q..8q+7 and
//     32+8q..32+8q+7 of its pixel: two 16-byte stores per lane, and the four lanes of a pixel write 64 contiguous bytes per store;
//   * each wave walks 16-pixel tiles with the next tile's pieces in flight (double-buffered fragments).
// ------------------------------------------------------------------------------------------------
// Round 6: the tile loop is BRANCH-FREE.  The round-1 form guarded every load / finish / store by `tile < ntile`, a run-time switch on
// out_act and null checks of the three output pointers: 8175 lines of ISA, and - what cost the time - hipcc's s_waitcnt pass, which merges
// the pending-operation state at every join, put `vmcnt(2)` behind the loads of tile t + 2: a wave drained its previous tile's stores
// and the loads of tile t + 1 in every iteration (ablation, profiles/r06_cin8_ablation.txt: conv1_1 0.178 ms = 0.053 instruction stream +
// 0.12 stores, not overlapped: 3.1 TB/s with 16 waves x 2 KB of stores in flight per CU).  Now: tile indices are clamped to the wave's last
// tile (a wave past its end recomputes and re-stores that tile: same bytes), the pixel count is a multiple of 16 (eligibility), out_act is
// NONE or RELU as a floor value, which outputs exist is a template parameter (OUTS: 1 raw, 2 lrelu copy, 4 relu copy), and the four
// fragment sets rotate through a loop unrolled by four: the compiler's own counts come out exact (the loads of tile t wait with the
// stores of the previous tiles and the loads of three tiles still in flight).
// (Forcing five / six waves per SIMD with amdgpu_waves_per_eu - the kernel allocates 104-124 registers, four / three waves - spills: conv1_1 0.155
// -> 0.155 / 0.253 ms, the stride-2 layers 0.093 -> 0.117 / 0.183: profiles/r06_cin8_ablation.txt.)
template <int S, int OUTS>
__global__ __launch_bounds__(256) void conv_cin8_kernel(const IgemmArgs a, int lgW, int lgH) {
  const int lane = threadIdx.x & 63;
  const int i = lane & 15, g = lane >> 4;
  const int P = a.N << (lgW + lgH);
  const int ntile = P >> 4;
  const int wave_global = blockIdx.x * 4 + (threadIdx.x >> 6), nwave = gridDim.x * 4;

  // A fragments: packed weights are [K chunk s][row][32 k]; this lane's row of tile t is channel 32*(t>>1) + 8*(i>>2) + 4*(t&1) + (i&3).
  // They live in LDS in fragment order [s][t][lane] (each lane re-reads its own 16 bytes: conflict-free, 12-16 KB per block),
  // which leaves the registers to occupancy and to the pixel pieces in flight.
  __shared__ uint4 wfrag[S * 4 * 64];
  __shared__ uint4 otile[4 * 16 * 144 / 16];
  // output rows are dense ([pixel][64]) and the pixel grid is the output grid: a tile's 16 pixels are one 2 KB run in every output
  // (measured: conv1_1, stride 1, 64 images: 0.209 -> 0.178 ms in round 5, where the stride-2 first layers lost 8 us each with it; on the
  // branch-free loop of round 6 they gain: layer_1 0.093 -> 0.089 ms, encoder_1 0.046 -> 0.044 - one store path for every output)
  constexpr bool ACTS = (OUTS & 6) != 0;
  {
    const bf16* wp = reinterpret_cast<const bf16*>(a.Wp);
    for (int idx = threadIdx.x; idx < S * 4 * 64; idx += 256) {
      const int l = idx & 63, t = (idx >> 6) & 3, s = idx >> 8;
      // with the global row permutation this is simply packed row 16t + i
      const int row = a.rowperm ? t * 16 + (l & 15) : (t >> 1) * 32 + 8 * ((l & 15) >> 2) + (t & 1) * 4 + (l & 3);
      wfrag[idx] = *reinterpret_cast<const uint4*>(wp + ((size_t)s * a.wp_rows + row) * 32 + (l >> 4) * 8);
    }
    __syncthreads();
  }
  float bias[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) bias[e] = a.bias ? a.bias[(e >> 3) * 32 + 8 * g + (e & 7)] : 0.f;
  const float act_floor = a.out_act == ACT_RELU ? 0.f : -__builtin_inff();     // relu as a floor: no branch per element
  // this lane's tap of step s
  int tdh[S], tdw[S];
  bool tok[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int tap = 4 * s + g;
    tok[s] = tap < a.ntaps;
    int dh = 0, dw = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) if (t == tap) { dh = a.taps[0].dh[t]; dw = a.taps[0].dw[t]; }
    tdh[s] = dh; tdw[s] = dw;
  }
  __amdgpu_buffer_rsrc_t rsX = make_rsrc(a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * 16));
  // a wave's tiles: wave_global, + nwave, ...; indices past its last one are clamped to it
  const int my_n = wave_global < ntile ? (ntile - 1 - wave_global) / nwave + 1 : 0;
  if (my_n == 0) return;
  const int tile_last = wave_global + (my_n - 1) * nwave;

  auto load_tile = [&](int tile_, uint4 (&fb)[S]) {
    const int tile = tile_ < tile_last ? tile_ : tile_last;
    const int p = tile * 16 + i;
    const int ow = p & ((1 << lgW) - 1), oh = (p >> lgW) & ((1 << lgH) - 1), n = p >> (lgW + lgH);
    const int bh = oh * a.sh, bw = ow * a.sw;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int ih = bh + tdh[s], iw = bw + tdw[s];
      const bool ok = tok[s] && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      const unsigned off = ok ? (unsigned)(((n * a.Hin + ih) * a.Win + iw) * 16) : DMA_OOB;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsX, (int)off, 0, 0);
      fb[s] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  auto finish_tile = [&](int tile_, const uint4 (&fb)[S]) {
    const int tile = tile_ < tile_last ? tile_ : tile_last;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int wl = lane;
    asm volatile("" : "+v"(wl));      // opaque: keeps the weight fragments in LDS (hoisted into registers they cost 48-64 VGPRs)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mma16<bf16>(wfrag[(s * 4 + t) * 64 + wl], fb[s], acc[t]);
    const int p = tile * 16 + i;
    float lo[8], hi[8];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = fmaxf(acc[t][e] + bias[4 * t + e], act_floor);
        if (t < 2) lo[4 * t + e] = x; else hi[4 * (t - 2) + e] = x;
      }
    const uint4 plo = Elem<bf16>::pack(lo), phi = Elem<bf16>::pack(hi);
    // the 16 pixels of a tile are 2 KB of consecutive output (dense [pixel][64] rows, pixel grid == output grid: eligibility); a lane's own
    // two pieces are 64-byte segments 128 bytes apart (half cache lines per store instruction).  Transpose through a wave-private LDS
    // tile (pixel pitch 144 bytes: conflict-free both ways) so that each of the two store instructions writes one contiguous 1 KB run
    char* tb = reinterpret_cast<char*>(otile) + (threadIdx.x >> 6) * (16 * 144);
    auto store_run = [&](void* dst, const uint4& v0, const uint4& v1) {
      *reinterpret_cast<uint4*>(tb + i * 144 + g * 16) = v0;
      *reinterpret_cast<uint4*>(tb + i * 144 + 64 + g * 16) = v1;
      __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): the wave's own LDS writes have landed (same-wave, no barrier)
      __builtin_amdgcn_wave_barrier();
      const uint4 q0 = *reinterpret_cast<const uint4*>(tb + (lane >> 3) * 144 + (lane & 7) * 16);
      const uint4 q1 = *reinterpret_cast<const uint4*>(tb + (8 + (lane >> 3)) * 144 + (lane & 7) * 16);
      bf16* yt = reinterpret_cast<bf16*>(dst) + (size_t)tile * 16 * 64;
      reinterpret_cast<uint4*>(yt)[lane] = q0;
      reinterpret_cast<uint4*>(yt)[64 + lane] = q1;
      __builtin_amdgcn_wave_barrier();
    };
    if constexpr (OUTS & 1) store_run(a.Y, plo, phi);
    // the consumers' activations of the ROUNDED output (what act_apply computes from the stored tensor: same bits)
    if constexpr (ACTS) {
      float rl[8], rh[8];
      Elem<bf16>::unpack(plo, rl);
      Elem<bf16>::unpack(phi, rh);
      if constexpr (OUTS & 2) {
        float t0[8], t1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { t0[e] = act_apply(ACT_LRELU, rl[e]); t1[e] = act_apply(ACT_LRELU, rh[e]); }
        store_run(a.xa_lrelu, Elem<bf16>::pack(t0), Elem<bf16>::pack(t1));
      }
      if constexpr (OUTS & 4) {
        float t0[8], t1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { t0[e] = act_apply(ACT_RELU, rl[e]); t1[e] = act_apply(ACT_RELU, rh[e]); }
        store_run(a.xa_relu, Elem<bf16>::pack(t0), Elem<bf16>::pack(t1));
      }
    }
  };

  // four fragment sets: three tiles of loads stay in flight behind the tile being finished; trips of four tiles, no branch inside
  // (four sets, three tiles of loads in flight: the stride-2 first layers 0.053 / 0.043 -> 0.045 / 0.038 ms against three sets; conv1_1 +-0)
  uint4 fb0[S], fb1[S], fb2[S], fb3[S];
  int tile = wave_global;
  load_tile(tile, fb0);
  load_tile(tile + nwave, fb1);
  load_tile(tile + 2 * nwave, fb2);
  for (int trip = (my_n + 3) / 4; trip > 0; --trip) {
    load_tile(tile + 3 * nwave, fb3);
    finish_tile(tile, fb0);
    load_tile(tile + 4 * nwave, fb0);
    finish_tile(tile + nwave, fb1);
    load_tile(tile + 5 * nwave, fb1);
    finish_tile(tile + 2 * nwave, fb2);
    load_tile(tile + 6 * nwave, fb2);
    finish_tile(tile + 3 * nwave, fb3);
    tile += 4 * nwave;
  }
}

// ------------------------------------------------------------------------------------------------
// deconv_cout4_tile_kernel: the generator's last layer (decoder_1: 4x4 stride-2 transposed conv, Cin -> 4 channels, f32 output).
// A tiled GEMM wastes 15/16 of its rows on 4 channels and re-launches per parity class.  Here the 4 classes x 4 channels ARE the
// 16 rows of one MFMA tile: K runs over the 3x3 input neighbourhood of a base pixel (the union of the four classes' 2x2 taps;
// a class's unused taps are zero rows of the weight image), columns are 16 consecutive base pixels.  After the K loop lane
// (pixel i, group g) holds the 4 channels of output pixel (2q + g/2, 2r + g%2): one 16-byte f32 store, the four groups of a
// base-pixel run fill two contiguous 512-byte output rows.  Weights: fragment-ordered LDS image built once per block.
// The input is staged ONCE per block (fetched per tap from whichever lane needs it, every input pixel moves nine times: 1.2 GB of
// L1 / L2 traffic for a 134 MB tensor, 0.145 ms against 0.02 ms of HBM time, r02 layer table).  A block owns 4 rows x 16 columns of
// base pixels: its 256 threads load the 6 x 18 pixel halo tile (1.7x the interior) with 16-byte loads - one tile ahead, in registers,
// while the current tile computes - and store it to LDS at a padded pixel pitch (Cin * 2 + 16 bytes: the 16 lanes of a fragment read
// hit 64 distinct banks); wave w then builds the B fragments of row w for all nine taps from LDS.
// The tile loop is branch-free (see conv3x3_cout8_tile_kernel).
// ------------------------------------------------------------------------------------------------
template <int SPT, int HALVED>
__global__ __launch_bounds__(256) void deconv_cout4_tile_kernel(const IgemmArgs a, int lgW, int lgH) {
  typedef ThinHalo<SPT * 32> H;
  constexpr int S = 9 * SPT, CIN = H::CIN, PPP = H::PPP, PIXB = H::PIXB, TPX = H::TPX, NPIECE = H::NPIECE, NJ = H::NJ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* wfrag = reinterpret_cast<uint4*>(smem);                  // [S][64]
  char* stage = smem + thin_weight_image_bytes<SPT, 1>;                     // [6][18][PIXB], then 256 dummy 16-byte slots
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  {
    const bf16* wp = reinterpret_cast<const bf16*>(a.Wp);
    const int nchunk_c = a.Kpad / 32;
    for (int idx = threadIdx.x; idx < S * 64; idx += 256) {
      const int l = idx & 63, s = idx >> 6;
      const int u = s / SPT, c0 = (s % SPT) * 32 + (l >> 4) * 8;
      const int dy = u / 3 - 1, dx = u % 3 - 1;
      const int cls = (l & 15) >> 2, co = l & 3;
      uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        int tdh = 0, tdw = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c == cls) { tdh = a.taps[c].dh[t]; tdw = a.taps[c].dw[t]; }
        if (tdh == dy && tdw == dx) {
          const int k = t * CIN + c0;
          v = *reinterpret_cast<const uint4*>(wp + (((size_t)cls * nchunk_c + (k >> 5)) * a.wp_rows + co) * 32 + (k & 31));
        }
      }
      wfrag[idx] = v;
    }
  }
  const int tw = 1 << (lgW - 4), th = 1 << (lgH - 2);             // tiles per row / per column of one image
  const int ntile = a.N * tw * th;
  const int my_n = (int)blockIdx.x < ntile ? (ntile - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  if (my_n == 0) return;
  const int tile_last = blockIdx.x + (my_n - 1) * gridDim.x;
  // One source per wave: with two equally wide concatenated sources (HALVED: the decoder's skip connection, the only form the plans
  // reach and the only one instantiated) waves 0-1 fetch the first one's channels and waves 2-3 the second's, so that the buffer
  // descriptor is a scalar select and every piece is ONE load; otherwise (HALVED == 0) there is a single source.
  const int src = HALVED ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)) : 0;
  const int CS = HALVED ? CIN / 2 : CIN;                          // channels of one source
  constexpr int PPS = HALVED ? PPP / 2 : PPP, NTH = HALVED ? 128 : 256;
  __amdgpu_buffer_rsrc_t rs0 = make_rsrc(src ? a.x.ptr[1] : a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * CS * 2));
  __amdgpu_buffer_rsrc_t rsY = make_rsrc(a.Y, (unsigned)((size_t)a.N * a.Hof * a.Wof * 4 * 4));
  float bias[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bias[e] = a.bias ? a.bias[e] : 0.f;

  // this thread's pieces of a halo tile: (pixel slot, 8-channel group) -> LDS byte offset, channel offset inside the source
  int soff[NJ], spix_r[NJ], spix_c[NJ], sch[NJ];
  bool sok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int idx = (int)(threadIdx.x & (NTH - 1)) + NTH * j;
    const int px = idx / PPS, c = (idx - px * PPS) * 8;
    spix_r[j] = px / 18; spix_c[j] = px - spix_r[j] * 18;
    sch[j] = c;
    sok[j] = idx < TPX * PPS;
    soff[j] = sok[j] ? px * PIXB + (src * CS + c) * 2 : TPX * PIXB + (int)threadIdx.x * 16;   // (beyond the halo: the thread's dummy slot)
  }
  uint4 pre[NJ];
  // The tile loop is branch-free (see conv3x3_cout8_tile_kernel): tiles beyond the block's last one are clamped to it, threads beyond the
  // halo write a dummy LDS slot.
  auto load_tile = [&](int tile_) {
    const int tile = tile_ < tile_last ? tile_ : tile_last;
    const bool live = tile_ <= tile_last;                         // (beyond the block's last tile: every offset out of range, no data moves)
    const int tc = tile & (tw - 1), tr = (tile >> (lgW - 4)) & (th - 1), n = tile >> (lgW - 4 + lgH - 2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ih = tr * 4 - 1 + spix_r[j], iw = tc * 16 - 1 + spix_c[j];
      const bool ok = live && sok[j] && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      const unsigned off = ok ? (unsigned)((((n * a.Hin + ih) * a.Win + iw) * CS + sch[j]) * 2) : DMA_OOB;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs0, (int)off, 0, 0);
      pre[j] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  int tile = blockIdx.x;
  load_tile(tile);
  __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsY, (int)DMA_OOB, 0, 0);   // (see conv3x3_cout8_tile_kernel)
  for (int it = my_n; it > 0; --it) {
    __syncthreads();                                              // previous tile's fragment reads are done (first pass: wfrag is complete)
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<uint4*>(stage + soff[j]) = pre[j];
    __syncthreads();
    load_tile(tile + gridDim.x);
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    int wl = lane;
    asm volatile("" : "+v"(wl));                                  // keep the weight image in LDS (no hoisting into registers)
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const char* px = stage + ((wv + u / 3) * 18 + i + u % 3) * PIXB + g * 16;
#pragma unroll
      for (int k = 0; k < SPT; ++k)
        acc = mma16<bf16>(wfrag[(u * SPT + k) * 64 + wl], *reinterpret_cast<const uint4*>(px + k * 64), acc);
    }
    const int tc = tile & (tw - 1), tr = (tile >> (lgW - 4)) & (th - 1), n = tile >> (lgW - 4 + lgH - 2);
    const int q = tr * 4 + wv, r = tc * 16 + i;
    const unsigned yo = (unsigned)(((n * a.Hof + 2 * q + (g >> 1)) * a.Wof + 2 * r + (g & 1)) * 16);
    const float4 o = make_float4(acc[0] + bias[0], acc[1] + bias[1], acc[2] + bias[2], acc[3] + bias[3]);
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)}, rsY, (int)yo, 0, 0);
    tile += gridDim.x;
  }
}

// conv3x3_cout8_tile_kernel: 3x3 stride-1 convolution from 64 channels to <= 8 (VGG conv1_1 backward-data: the perceptual gradient
// arriving at the composited image).  As a 16-row GEMM tile on the gather-per-tap kernel every dY pixel is fetched nine times
// (0.193 ms for 0.04 ms of HBM traffic, r02 layer table).  Same plan as deconv_cout4_tile_kernel: a block owns 4 rows x 16 columns,
// stages the 6 x 18 pixel halo once in LDS (one tile ahead in registers), wave w multiplies row w against the weight fragments -
// which are only 18 x 16 bytes per lane and stay in registers.  Rows 0..7 of the MFMA tile are the channels: lanes g = 0 / 1 hold
// channels 0..3 / 4..7 of pixel i, one cross-lane move joins them into the 16-byte output row (the store below).
// Round 6: branch-free tile loop (as conv_cin8_kernel, EXPERIMENTS.md 0.7): the block's tile index is clamped to its last tile, the LDS
// staging writes of the threads beyond the halo's 864 pieces go to a dummy slot, the output store is a buffer store whose offset is out of
// range for the lanes that hold no output piece (dropped by the hardware), and the epilogue is the plain one (no bias / activation /
// reference / accumulation: eligibility) - so hipcc's s_waitcnt pass counts exactly and the tile's store stays in flight across the next
// tile's barrier instead of being drained by a vmcnt(0) in front of it.
__global__ __launch_bounds__(256) void conv3x3_cout8_tile_kernel(const IgemmArgs a, int lgW, int lgH) {
  typedef ThinHalo<64> H;
  constexpr int PIXB = H::PIXB, TPX = H::TPX, NPIECE = H::NPIECE, NJ = H::NJ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* stage = smem;                                             // [6][18][PIXB], then 256 dummy 16-byte slots
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  uint4 af[18];
  int toff[9];
  {
    const bf16* wp = reinterpret_cast<const bf16*>(a.Wp);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      toff[t] = ((1 + a.taps[0].dh[t]) * 18 + 1 + a.taps[0].dw[t]) * PIXB;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int kk = t * 64 + k * 32 + g * 8;
        af[t * 2 + k] = *reinterpret_cast<const uint4*>(wp + ((size_t)(kk >> 5) * a.wp_rows + i) * 32 + (kk & 31));
      }
    }
  }
  const int tw = 1 << (lgW - 4), th = 1 << (lgH - 2);
  const int ntile = a.N * tw * th;
  const int my_n = (int)blockIdx.x < ntile ? (ntile - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  if (my_n == 0) return;
  const int tile_last = blockIdx.x + (my_n - 1) * gridDim.x;
  __amdgpu_buffer_rsrc_t rs0 = make_rsrc(a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * 64 * 2));
  __amdgpu_buffer_rsrc_t rsY = make_rsrc(a.Y, (unsigned)((size_t)a.N * a.Hof * a.Wof * a.ldY * 2));
  int soff[NJ], spix_r[NJ], spix_c[NJ], sch[NJ];
  bool sok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int idx = threadIdx.x + 256 * j;
    const int px = idx >> 3, c = (idx & 7) * 8;
    spix_r[j] = px / 18; spix_c[j] = px - spix_r[j] * 18;
    sch[j] = c;
    sok[j] = idx < NPIECE;
    soff[j] = sok[j] ? px * PIXB + c * 2 : TPX * PIXB + (int)threadIdx.x * 16;      // (beyond the halo: the thread's dummy slot)
  }
  uint4 pre[NJ];
  auto load_tile = [&](int tile_) {
    const int tile = tile_ < tile_last ? tile_ : tile_last;
    const bool live = tile_ <= tile_last;                         // (beyond the block's last tile: every offset out of range, no data moves)
    const int tc = tile & (tw - 1), tr = (tile >> (lgW - 4)) & (th - 1), n = tile >> (lgW - 4 + lgH - 2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ih = tr * 4 - 1 + spix_r[j], iw = tc * 16 - 1 + spix_c[j];
      const bool ok = live && sok[j] && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      const unsigned off = ok ? (unsigned)((((n * a.Hin + ih) * a.Win + iw) * 64 + sch[j]) * 2) : DMA_OOB;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs0, (int)off, 0, 0);
      pre[j] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  int tile = blockIdx.x;
  load_tile(tile);
  // (a store that goes nowhere - offset out of range - behind the first tile's loads: the loop's first trip then looks like every other one
  // to the s_waitcnt pass, which otherwise merges "no store pending" with "one store pending" into vmcnt(0) at the loop header)
  __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsY, (int)DMA_OOB, 0, 0);
  for (int it = my_n; it > 0; --it) {
    __syncthreads();                                              // previous tile's fragment reads are done
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<uint4*>(stage + soff[j]) = pre[j];
    __syncthreads();
    load_tile(tile + gridDim.x);
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const char* px = stage + (wv * 18 + i) * PIXB + g * 16;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int k = 0; k < 2; ++k) acc = mma16<bf16>(af[t * 2 + k], *reinterpret_cast<const uint4*>(px + toff[t] + k * 64), acc);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = acc[e]; v[4 + e] = __shfl(acc[e], (lane + 16) & 63); }
    const int tl = tile < tile_last ? tile : tile_last;
    const int tc = tl & (tw - 1), tr = (tl >> (lgW - 4)) & (th - 1), n = tl >> (lgW - 4 + lgH - 2);
    const unsigned yo = g == 0 ? (unsigned)((((n * a.Hof + tr * 4 + wv) * a.Wof + tc * 16 + i) * a.ldY) * 2) : DMA_OOB;
    const uint4 pk = Elem<bf16>::pack(v);
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk.x, pk.y, pk.z, pk.w}, rsY, (int)yo, 0, 0);
    tile += gridDim.x;
  }
}

// deconv_cout8_tile_kernel: 4x4 stride-2 transposed conv to <= 8 channels (discriminator layer_1 backward-data towards the generator:
// 64 -> 6 (+2 pad) channels at 256x256).  deconv_cout4_tile_kernel with two MFMA tiles: rows 16T .. 16T+15 = parity classes 2T, 2T+1
// x 8 channels; lane (i, g) of tile T holds channels 4 (g & 1) .. +3 of class 2T + (g >> 1) at base pixel i, its neighbour group
// g ^ 1 the other half: one cross-lane move, then the even groups write the 16-byte bf16 rows (the store below).
template <int SPT>
__global__ __launch_bounds__(256) void deconv_cout8_tile_kernel(const IgemmArgs a, int lgW, int lgH) {
  typedef ThinHalo<SPT * 32> H;
  constexpr int S = 9 * SPT, CIN = H::CIN, PPP = H::PPP, PIXB = H::PIXB, TPX = H::TPX, NPIECE = H::NPIECE, NJ = H::NJ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* wfrag = reinterpret_cast<uint4*>(smem);                  // [2][S][64]
  char* stage = smem + thin_weight_image_bytes<SPT, 2>;                 // [6][18][PIXB], then 256 dummy 16-byte slots
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  {
    const bf16* wp = reinterpret_cast<const bf16*>(a.Wp);
    const int nchunk_c = a.Kpad / 32;
    for (int idx = threadIdx.x; idx < 2 * S * 64; idx += 256) {
      const int l = idx & 63, s = (idx >> 6) % S, T = idx / (S * 64);
      const int u = s / SPT, c0 = (s % SPT) * 32 + (l >> 4) * 8;
      const int dy = u / 3 - 1, dx = u % 3 - 1;
      const int cls = 2 * T + ((l & 15) >> 3), co = l & 7;
      uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        int tdh = 0, tdw = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c == cls) { tdh = a.taps[c].dh[t]; tdw = a.taps[c].dw[t]; }
        if (tdh == dy && tdw == dx) {
          const int k = t * CIN + c0;
          v = *reinterpret_cast<const uint4*>(wp + (((size_t)cls * nchunk_c + (k >> 5)) * a.wp_rows + co) * 32 + (k & 31));
        }
      }
      wfrag[idx] = v;
    }
  }
  const int tw = 1 << (lgW - 4), th = 1 << (lgH - 2);
  const int ntile = a.N * tw * th;
  const int my_n = (int)blockIdx.x < ntile ? (ntile - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  if (my_n == 0) return;
  const int tile_last = blockIdx.x + (my_n - 1) * gridDim.x;
  __amdgpu_buffer_rsrc_t rs0 = make_rsrc(a.x.ptr[0], (unsigned)((size_t)a.N * a.Hin * a.Win * CIN * 2));
  __amdgpu_buffer_rsrc_t rsY = make_rsrc(a.Y, (unsigned)((size_t)a.N * a.Hof * a.Wof * a.ldY * 2));
  int soff[NJ], spix_r[NJ], spix_c[NJ], sch[NJ];
  bool sok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int idx = threadIdx.x + 256 * j;
    const int px = idx / PPP, c = (idx - px * PPP) * 8;
    spix_r[j] = px / 18; spix_c[j] = px - spix_r[j] * 18;
    sch[j] = c;
    sok[j] = idx < NPIECE;
    soff[j] = sok[j] ? px * PIXB + c * 2 : TPX * PIXB + (int)threadIdx.x * 16;      // (beyond the halo: the thread's dummy slot)
  }
  uint4 pre[NJ];
  // The tile loop is branch-free (see conv3x3_cout8_tile_kernel): tiles beyond the block's last one are clamped to it, threads beyond the
  // halo write a dummy LDS slot, lanes without an output row store to an out-of-range offset.
  auto load_tile = [&](int tile_) {
    const int tile = tile_ < tile_last ? tile_ : tile_last;
    const bool live = tile_ <= tile_last;                         // (beyond the block's last tile: every offset out of range, no data moves)
    const int tc = tile & (tw - 1), tr = (tile >> (lgW - 4)) & (th - 1), n = tile >> (lgW - 4 + lgH - 2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ih = tr * 4 - 1 + spix_r[j], iw = tc * 16 - 1 + spix_c[j];
      const bool ok = live && sok[j] && (unsigned)ih < (unsigned)a.Hin && (unsigned)iw < (unsigned)a.Win;
      const unsigned off = ok ? (unsigned)((((n * a.Hin + ih) * a.Win + iw) * CIN + sch[j]) * 2) : DMA_OOB;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs0, (int)off, 0, 0);
      pre[j] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  int tile = blockIdx.x;
  load_tile(tile);
  __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsY, (int)DMA_OOB, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsY, (int)DMA_OOB, 0, 0);
  for (int it = my_n; it > 0; --it) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<uint4*>(stage + soff[j]) = pre[j];
    __syncthreads();
    load_tile(tile + gridDim.x);
    f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    int wl = lane;
    asm volatile("" : "+v"(wl));                                  // keep the weight image in LDS
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const char* px = stage + ((wv + u / 3) * 18 + i + u % 3) * PIXB + g * 16;
#pragma unroll
      for (int k = 0; k < SPT; ++k) {
        const uint4 b = *reinterpret_cast<const uint4*>(px + k * 64);
        acc0 = mma16<bf16>(wfrag[(u * SPT + k) * 64 + wl], b, acc0);
        acc1 = mma16<bf16>(wfrag[(S + u * SPT + k) * 64 + wl], b, acc1);
      }
    }
    const int tl = tile < tile_last ? tile : tile_last;
    const int tc = tl & (tw - 1), tr = (tl >> (lgW - 4)) & (th - 1), n = tl >> (lgW - 4 + lgH - 2);
    const int q = tr * 4 + wv, r = tc * 16 + i;
#pragma unroll
    for (int T = 0; T < 2; ++T) {
      const f32x4 acc = T ? acc1 : acc0;
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = acc[e]; v[4 + e] = __shfl(acc[e], (lane + 16) & 63); }
      const int cls = 2 * T + (g >> 1);
      const unsigned yo = (g & 1) == 0 ? (unsigned)((((n * a.Hof + 2 * q + (cls >> 1)) * a.Wof + 2 * r + (cls & 1)) * a.ldY) * 2) : DMA_OOB;
      const uint4 pk = Elem<bf16>::pack(v);
      __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk.x, pk.y, pk.z, pk.w}, rsY, (int)yo, 0, 0);
    }
    tile += gridDim.x;
  }
}

// 8-channel (padded image) inputs, 64 outputs: what conv_cin8_kernel handles
bool conv_cin8_eligible(const IgemmArgs& a, int is_bf16) {
  const bool pow2 = (a.Wg & (a.Wg - 1)) == 0 && (a.Hg & (a.Hg - 1)) == 0;
  return is_bf16 && a.zeros && a.Cin == 8 && a.x.C[0] == 8 && a.x.C[1] == 0 && a.Cout == 64 && a.ldY == 64 && a.nclass == 1 && a.splitk == 1 && a.os == 1 &&
         a.Hof == a.Hg && a.Wof == a.Wg && pow2 && !a.ref && !a.accumulate && !a.y_f32 && !a.bn_part && !a.x.aff_a[0] && a.x.act == ACT_NONE &&
         a.ntaps <= 16 && (a.Kpad == 96 || a.Kpad == 128) && (size_t)a.N * a.Hin * a.Win * 16 < 0x70000000ull &&
         (((long long)a.N * a.Hg * a.Wg) & 15) == 0 && (a.out_act == ACT_NONE || a.out_act == ACT_RELU) &&
         (a.Kpad == 128 || !(a.xa_lrelu || a.xa_relu)) && !(a.xa_relu && !a.xa_lrelu);      // (the instantiated output combinations: conv_cin8_kernel)
}

// 3x3 stride-1 conv from 64 to <= 8 channels with the kernel's plain epilogue: what conv3x3_cout8_tile_kernel handles
bool conv_cout8_eligible(const IgemmArgs& a, int is_bf16) {
  bool near = a.ntaps == 9;
  for (int t = 0; near && t < 9; ++t) near = a.taps[0].dh[t] >= -1 && a.taps[0].dh[t] <= 1 && a.taps[0].dw[t] >= -1 && a.taps[0].dw[t] <= 1;
  return is_bf16 && near && a.zeros && a.nclass == 1 && a.sh == 1 && a.sw == 1 && a.os == 1 && a.Cin == 64 && a.x.C[0] == 64 && a.x.C[1] == 0 &&
         a.CoutPad == 16 && a.Cout <= 8 && a.ldY == 8 && a.splitk == 1 && !a.rowperm && !a.bn_part && !a.x.aff_a[0] && a.x.act == ACT_NONE &&
         (a.Wg & (a.Wg - 1)) == 0 && (a.Hg & (a.Hg - 1)) == 0 && a.Wg >= 16 && a.Hg >= 4 && a.Hof == a.Hg && a.Wof == a.Wg && a.Hin == a.Hg &&
         a.Win == a.Wg && !a.y_f32 && (size_t)a.N * a.Hin * a.Win * 64 * 2 < 0x70000000ull &&
         !a.bias && a.out_act == ACT_NONE && !a.ref && !a.accumulate && !a.split_c;
}

// 4x4 stride-2 transposed conv from 64 to <= 8 channels with the kernel's plain epilogue: what deconv_cout8_tile_kernel handles
bool conv_dcout8_eligible(const IgemmArgs& a, int is_bf16) {
  return is_bf16 && a.zeros && a.nclass == 4 && a.os == 2 && a.ntaps == 4 && a.Cin == 64 && a.x.C[0] == 64 && a.x.C[1] == 0 && a.CoutPad == 16 &&
         a.Cout <= 8 && a.ldY == 8 && !a.y_f32 && a.splitk == 1 && !a.rowperm && !a.bn_part && !a.x.aff_a[0] && a.x.act == ACT_NONE &&
         (a.Wg & (a.Wg - 1)) == 0 && (a.Hg & (a.Hg - 1)) == 0 && a.Wg >= 16 && a.Hg >= 4 && a.Hof == 2 * a.Hg && a.Wof == 2 * a.Wg && a.Hin == a.Hg &&
         a.Win == a.Wg && (size_t)a.N * a.Hin * a.Win * 64 * 2 < 0x70000000ull && (size_t)a.N * a.Hof * a.Wof * 8 * 2 < 0x70000000ull &&
         !a.bias && a.out_act == ACT_NONE && !a.ref && !a.accumulate && !a.split_c;
}

// 4-channel float32 transposed conv from two equally wide sources (decoder_1's concat): what deconv_cout4_tile_kernel handles
bool conv_cout4_eligible(const IgemmArgs& a, int is_bf16) {
  const bool pow2 = (a.Wg & (a.Wg - 1)) == 0 && (a.Hg & (a.Hg - 1)) == 0;
  const int spt = a.Cin / 32;
  return is_bf16 && a.zeros && a.nclass == 4 && a.os == 2 && a.ntaps == 4 && a.Cout == 4 && a.y_f32 && a.ldY == 4 && a.splitk == 1 && pow2 &&
         a.Wg >= 16 && a.Hg >= 4 && a.Cin % 32 == 0 && (spt == 2 || spt == 4) && a.x.C[1] == a.x.C[0] && a.x.C[0] + a.x.C[1] == a.Cin &&
         !a.ref && !a.accumulate && a.out_act == ACT_NONE && !a.x.aff_a[0] && !a.x.aff_a[1] && a.x.act == ACT_NONE && a.Hof == 2 * a.Hg &&
         a.Wof == 2 * a.Wg && (size_t)a.N * a.Hin * a.Win * a.Cin * 2 < 0x70000000ull && (size_t)a.N * a.Hof * a.Wof * 16 < 0x70000000ull;
}

// The launch geometry all four share: log2 of the (power-of-two: eligibility) pixel grid's sides, and one persistent block per 64
// pixels - a 4 x 16 tile of the tile kernels, a 16-pixel tile for each of conv_cin8_kernel's four waves - up to the kernel's grid cap
// (thin_blocks_knob, conv_ops.h)
struct ThinGrid { int lgW, lgH, blocks; };
static ThinGrid thin_grid(const IgemmArgs& a, int knob) {
  ThinGrid g{ilog2(a.Wg), ilog2(a.Hg), 0};
  g.blocks = ((a.N << (g.lgW + g.lgH)) + 63) >> 6;
  if (g.blocks > thin_blocks_knob(knob)) g.blocks = thin_blocks_knob(knob);
  return g;
}

// a tile kernel with `smem` bytes of dynamic LDS (the weight image of the transposed convolutions takes it beyond the default limit)
template <typename K> static hipError_t launch_thin_tile(K kern, const IgemmArgs& a, int knob, int smem, hipStream_t st) {
  const ThinGrid g = thin_grid(a, knob);
  if (smem > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(256), (size_t)smem, st, a, g.lgW, g.lgH);
  return hipGetLastError();
}

hipError_t launch_conv_cin8(const IgemmArgs& a, hipStream_t st) {
  const ThinGrid g = thin_grid(a, 3);
  // which outputs exist is a template parameter (bit 0 raw output, 1 lrelu copy, 2 relu copy): the tile loop has no branch
  const int outs = (a.Y ? 1 : 0) | (a.xa_lrelu ? 2 : 0) | (a.xa_relu ? 4 : 0);
  void (*kern)(const IgemmArgs, int, int) = nullptr;
  if (a.Kpad == 96) kern = outs == 1 ? conv_cin8_kernel<3, 1> : nullptr;
  else switch (outs) {
    case 1: kern = conv_cin8_kernel<4, 1>; break;
    case 2: kern = conv_cin8_kernel<4, 2>; break;
    case 3: kern = conv_cin8_kernel<4, 3>; break;
    case 6: kern = conv_cin8_kernel<4, 6>; break;
    case 7: kern = conv_cin8_kernel<4, 7>; break;
    default: break;
  }
  if (!kern) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(256), 0, st, a, g.lgW, g.lgH);
  return hipGetLastError();
}

hipError_t launch_conv_cout8(const IgemmArgs& a, hipStream_t st) {
  return launch_thin_tile(conv3x3_cout8_tile_kernel, a, 0, ThinHalo<64>::LDS_BYTES, st);
}

hipError_t launch_conv_dcout8(const IgemmArgs& a, hipStream_t st) {
  return launch_thin_tile(deconv_cout8_tile_kernel<2>, a, 1, thin_weight_image_bytes<2, 2> + ThinHalo<64>::LDS_BYTES, st);
}

hipError_t launch_conv_cout4(const IgemmArgs& a, hipStream_t st) {
  if (a.Cin == 64) return launch_thin_tile(deconv_cout4_tile_kernel<2, 1>, a, 2, thin_weight_image_bytes<2, 1> + ThinHalo<64>::LDS_BYTES, st);
  return launch_thin_tile(deconv_cout4_tile_kernel<4, 1>, a, 2, thin_weight_image_bytes<4, 1> + ThinHalo<128>::LDS_BYTES, st);
}

}  // namespace vp

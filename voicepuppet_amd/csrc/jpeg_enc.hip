// Baseline JPEG encoding of uint8 RGB frames on the device (vp_jpeg_*): what the reference does per frame on the host with cv2.imwrite
// (infer_bfmvid.py:243-244), for the frames of a whole launch at once and without a host wait.
//
// The stream (ITU T.81 baseline, JFIF 1.01): SOI, APP0, DQT x 2, SOF0 (4:2:0), DHT x 4 (the Annex K tables, fixed), DRI, SOS, entropy-coded
// data, EOI.  The restart interval is one MCU row, so an interval is byte aligned and depends on nothing outside its 16 pixel rows: that
// is the unit of parallel work.
//
//   jpeg_interval_kernel   one workgroup per (frame, MCU row):
//     1. transform: one thread per 8 x 8 block.  The thread reads its pixels straight from the frame (24 or 48 contiguous bytes per image
//        row, as dwords; the 24 KB of an MCU row are read once for luminance and once for chrominance and stay in cache between), converts
//        to full-range YCbCr in float32 without rounding, averages 2 x 2 for chroma, runs the separable float32 DCT in registers (even / odd
//        halves: 32 multiplies per 8-point pass), divides by the quantisation step, rounds to nearest with ties away from zero and stores
//        int16 in zig-zag order to LDS.  Luminance blocks take the first 4 * mcus work items and chrominance the rest, so a wave runs one
//        of the two code paths; in LDS the blocks lie in scan order.  A block is 66 int16 apart from the next (33 dwords): the threads of a
//        wave, each walking its own block, hit 32 different banks.
//     2. bit lengths: one thread per block walks its 63 AC coefficients (run lengths, ZRL, EOB) and adds up the code lengths; the DC
//        difference needs only the previous block of the same component, which is in LDS.  A wave scans the lengths into bit offsets.
//     3. deposit: the same walk again, every code OR-ed into the interval's bit buffer in LDS at its offset (big-endian dwords, LDS
//        atomics: neighbouring blocks share a dword).  The last byte is padded with 1 bits.
//     4. byte stuffing: the packed bytes are walked in tiles of 256; a ballot counts the 0xFF bytes below each lane, the waves exchange
//        their totals, and every byte (and the 0x00 behind a 0xFF) goes to its final place in the interval's slot of the workspace.
//        Every store is guarded by the slot capacity; an interval that does not fit records -1 as its length.
//   jpeg_gather_kernel     one workgroup per (frame, MCU row): sums the interval lengths of its frame (before it: its offset; all: the file
//        size), and, when every interval fitted and the file fits the caller's row, copies its interval behind the header and the intervals
//        before it, followed by its RSTn marker (or EOI).  Interval 0 also copies the header and writes out_bytes[frame]; on a misfit it
//        writes -1 there and nothing is copied.
//
// Only vector loads / stores, LDS atomics and plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "workspace.h"

namespace vp {

// ---- ITU T.81 Annex K -------------------------------------------------------------------------------------------------------------------
static const unsigned char kQLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                         69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                         81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
// zig-zag position -> row-major index (T.81 Figure A.6)
static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// row-major index -> zig-zag position, for the unrolled store of a block
struct ZigzagInv {
  int pos[64];
  constexpr ZigzagInv() : pos() {
    constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    for (int i = 0; i < 64; ++i) pos[zz[i]] = i;
  }
};
static constexpr ZigzagInv kZigzagInv{};

// ---- device tables and geometry ---------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kBlockStride = 66;       // int16 per block in LDS: 33 dwords, so the threads of a wave (one block each) spread over 32 banks
constexpr int kHuffWords = 2 * 256 + 2 * 16;   // AC luma, AC chroma [256] then DC luma, DC chroma [16]: (length << 16) | code

struct JpegTables {                    // in the workspace, filled at create
  float quant[2][64];                  // quantisation steps, row-major: luminance, chrominance
  uint32_t huff[kHuffWords];
};

struct IntervalArgs {
  const unsigned char* rgb;            // [frames][H][W][3]
  const JpegTables* tab;
  unsigned char* slots;                // [max_frames * rows][cap]
  int* lens;                           // [max_frames * rows]
  short* coef;                         // [max_frames][rows][nblk][64] or null
  int W, H, rows, mcus, nblk, cap;
};

struct GatherArgs {
  const unsigned char* slots;
  const int* lens;
  const unsigned char* header;
  unsigned char* out;
  int* out_bytes;
  size_t out_row_bytes;
  int rows, cap, header_len;
};

// 0.5 * cos(m * pi / 16), m = 0 .. 7
__device__ __forceinline__ constexpr float dct_cos(int m) {
  return m == 0 ? 0.5f : m == 1 ? 0.49039264020161522f : m == 2 ? 0.46193976625564337f : m == 3 ? 0.41573480615127262f
       : m == 4 ? 0.35355339059327379f : m == 5 ? 0.27778511650980114f : m == 6 ? 0.19134171618254489f : 0.09754516100806417f;
}
// the DCT matrix entry c(u) / 2 * cos((2x + 1) u pi / 16)
__device__ __forceinline__ constexpr float dct_c(int u, int x) {
  if (u == 0) return 0.35355339059327379f;
  int m = ((2 * x + 1) * u) % 32;
  if (m > 16) m = 32 - m;
  if (m == 8) return 0.0f;
  return m < 8 ? dct_cos(m) : -dct_cos(16 - m);
}

// 8-point pass over v[0], v[S], .. v[7 S]: even outputs from the sums, odd outputs from the differences of mirrored inputs
template <int S>
__device__ __forceinline__ void dct8(float* v) {
  float s[4], d[4], o[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = v[j * S] + v[(7 - j) * S]; d[j] = v[j * S] - v[(7 - j) * S]; }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float* h = (u & 1) ? d : s;
    o[u] = dct_c(u, 0) * h[0] + dct_c(u, 1) * h[1] + dct_c(u, 2) * h[2] + dct_c(u, 3) * h[3];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u * S] = o[u];
}

// v: the level-shifted samples of one block, row-major -> quantised zig-zag int16 at dst
__device__ __forceinline__ void transform_store(float* v, const float* q, short* dst) {
#pragma unroll
  for (int y = 0; y < 8; ++y) dct8<1>(v + 8 * y);
#pragma unroll
  for (int x = 0; x < 8; ++x) dct8<8>(v + x);
#pragma unroll
  for (int n = 0; n < 64; ++n) dst[kZigzagInv.pos[n]] = (short)(int)roundf(v[n] / q[n]);    // roundf: nearest, ties away from zero
}

__device__ __forceinline__ int byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255; }

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }      // bits of |v|, 0 for 0

// One block's codes.  WRITE == false: returns their total length.  WRITE: ORs them into `bits` from bit `pos` on.
template <bool WRITE>
__device__ __forceinline__ int code_block(const short* c, int prev_dc, const uint32_t* ac, const uint32_t* dc, uint32_t* bits, int pos) {
  int n = 0;
  auto put = [&](uint32_t v, int len) {
    if (WRITE) {
      const int at = pos + n, off = at & 31;
      const unsigned long long x = (unsigned long long)v << (64 - off - len);     // len <= 26: off + len <= 57
      atomicOr(&bits[at >> 5], (uint32_t)(x >> 32));
      if (off + len > 32) atomicOr(&bits[(at >> 5) + 1], (uint32_t)x);
    }
    n += len;
  };
  const int diff = (int)c[0] - prev_dc;
  int s = category(diff);
  uint32_t h = dc[s];
  put(((h & 0xffffu) << s) | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << s) - 1)), (int)(h >> 16) + s);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = c[k];
    if (v == 0) { ++run; continue; }
    while (run > 15) { h = ac[0xf0]; put(h & 0xffffu, (int)(h >> 16)); run -= 16; }
    s = category(v);
    h = ac[(run << 4) | s];
    put(((h & 0xffffu) << s) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(h >> 16) + s);
    run = 0;
  }
  if (run) { h = ac[0]; put(h & 0xffffu, (int)(h >> 16)); }
  return n;
}

__global__ __launch_bounds__(kThreads) void jpeg_interval_kernel(const IntervalArgs a) {
  extern __shared__ uint32_t lds[];
  // carve: tables, per-block lengths / offsets, coefficients, bit buffer
  float* quant = reinterpret_cast<float*>(lds);                       // [2][64]
  uint32_t* huff = lds + 128;                                         // [kHuffWords]
  int* blen = reinterpret_cast<int*>(huff + kHuffWords);              // [nblk + 1]
  short* coef = reinterpret_cast<short*>(blen + ((a.nblk + 2) & ~1)); // [nblk][kBlockStride]
  uint32_t* bits = reinterpret_cast<uint32_t*>(coef + a.nblk * kBlockStride);   // [cap / 4 + 1]
  __shared__ int wsum[2][kThreads / 64];
  __shared__ int s_total;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x, frame = blockIdx.y;
  const int W = a.W, M = a.mcus, nblk = a.nblk;
  for (int i = t; i < 128; i += kThreads) quant[i] = a.tab->quant[0][i];
  for (int i = t; i < kHuffWords; i += kThreads) huff[i] = a.tab->huff[i];
  for (int i = t; i < a.cap / 4 + 1; i += kThreads) bits[i] = 0;
  __syncthreads();

  // 1. transform
  const unsigned char* src = a.rgb + ((size_t)frame * a.H + (size_t)row * 16) * W * 3;
  for (int j = t; j < nblk; j += kThreads) {
    float v[64];
    if (j < 4 * M) {
      const int mcu = j >> 2, b = j & 3;
      const unsigned char* p = src + ((size_t)(b >> 1) * 8 * W + mcu * 16 + (b & 1) * 8) * 3;
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        uint32_t w[6];
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + (size_t)y * W * 3);
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = pw[i];
#pragma unroll
        for (int x = 0; x < 8; ++x)
          v[8 * y + x] = 0.299f * (float)byte_of(w, 3 * x) + 0.587f * (float)byte_of(w, 3 * x + 1) + 0.114f * (float)byte_of(w, 3 * x + 2) - 128.0f;
      }
      transform_store(v, quant, coef + (mcu * 6 + b) * kBlockStride);
    } else {
      const int cr = j >= 5 * M, mcu = j - (4 + cr) * M;
      const float kr = cr ? 0.5f : -0.168736f, kg = cr ? -0.418688f : -0.331264f, kb = cr ? -0.081312f : 0.5f;
      const unsigned char* p = src + (size_t)mcu * 16 * 3;
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        uint32_t w0[12], w1[12];
        const uint32_t* p0 = reinterpret_cast<const uint32_t*>(p + (size_t)(2 * y) * W * 3);
        const uint32_t* p1 = reinterpret_cast<const uint32_t*>(p + (size_t)(2 * y + 1) * W * 3);
#pragma unroll
        for (int i = 0; i < 12; ++i) { w0[i] = p0[i]; w1[i] = p1[i]; }
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          // the 2 x 2 sums are exact integers; the mean of the four conversions is the conversion of the mean
          const float r = (float)(byte_of(w0, 6 * x) + byte_of(w0, 6 * x + 3) + byte_of(w1, 6 * x) + byte_of(w1, 6 * x + 3));
          const float g = (float)(byte_of(w0, 6 * x + 1) + byte_of(w0, 6 * x + 4) + byte_of(w1, 6 * x + 1) + byte_of(w1, 6 * x + 4));
          const float bl = (float)(byte_of(w0, 6 * x + 2) + byte_of(w0, 6 * x + 5) + byte_of(w1, 6 * x + 2) + byte_of(w1, 6 * x + 5));
          v[8 * y + x] = 0.25f * (kr * r + kg * g + kb * bl);
        }
      }
      transform_store(v, quant + 64, coef + (mcu * 6 + 4 + cr) * kBlockStride);
    }
  }
  __syncthreads();

  if (a.coef) {       // tests: the quantised coefficients, scan order
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.coef + ((size_t)frame * a.rows + row) * nblk * 64);
    const uint32_t* c32 = reinterpret_cast<const uint32_t*>(coef);
    for (int e = t; e < nblk * 32; e += kThreads) dst[e] = c32[(e >> 5) * (kBlockStride / 2) + (e & 31)];
  }

  // 2. bit length of every block, then their exclusive scan (wave 0: a run of consecutive blocks per lane, a shuffle scan over the lanes)
  auto prev_dc = [&](int bi) -> int {
    const int mcu = bi / 6, b = bi - 6 * mcu;
    if (b >= 4) return mcu ? coef[(bi - 6) * kBlockStride] : 0;
    if (b) return coef[(bi - 1) * kBlockStride];
    return mcu ? coef[(bi - 3) * kBlockStride] : 0;
  };
  for (int bi = t; bi < nblk; bi += kThreads) {
    const int ch = (bi % 6) >= 4;
    blen[bi] = code_block<false>(coef + bi * kBlockStride, prev_dc(bi), huff + 256 * ch, huff + 512 + 16 * ch, nullptr, 0);
  }
  __syncthreads();
  if (wave == 0) {
    const int per = (nblk + 63) / 64, b0 = lane * per;
    int sum = 0;
    for (int i = b0; i < b0 + per && i < nblk; ++i) sum += blen[i];
    int inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    int at = inc - sum;
    for (int i = b0; i < b0 + per && i < nblk; ++i) { const int l = blen[i]; blen[i] = at; at += l; }
    if (lane == 63) s_total = inc;
  }
  __syncthreads();
  const int total_bits = s_total;
  int* len_out = a.lens + (size_t)frame * a.rows + row;
  if (total_bits > a.cap * 8) {            // does not fit the bit buffer: nothing is written
    if (t == 0) *len_out = -1;
    return;
  }

  // 3. deposit
  for (int bi = t; bi < nblk; bi += kThreads) {
    const int ch = (bi % 6) >= 4;
    code_block<true>(coef + bi * kBlockStride, prev_dc(bi), huff + 256 * ch, huff + 512 + 16 * ch, bits, blen[bi]);
  }
  if (t == 0 && (total_bits & 7)) {        // pad the last byte with 1 bits
    const int pad = 8 - (total_bits & 7), off = total_bits & 31;
    atomicOr(&bits[total_bits >> 5], ((1u << pad) - 1u) << (32 - off - pad));
  }
  __syncthreads();

  // 4. byte stuffing into the slot
  const int nbytes = (total_bits + 7) >> 3;
  unsigned char* dst = a.slots + ((size_t)frame * a.rows + row) * a.cap;
  int base = 0;
  for (int i0 = 0, par = 0; i0 < nbytes; i0 += kThreads, par ^= 1) {
    const int i = i0 + t;
    const bool valid = i < nbytes;
    const int b = valid ? (int)((bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) : 0;
    const bool ff = b == 255;
    const unsigned long long m = __ballot(ff);
    if (lane == 0) wsum[par][wave] = __popcll(m);
    __syncthreads();           // wsum[par] is next written two tiles on, behind the barrier of the tile between
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { const int c = wsum[par][w]; all += c; if (w < wave) before += c; }
    const int pos = i + base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (valid && pos < a.cap) dst[pos] = (unsigned char)b;
    if (valid && ff && pos + 1 < a.cap) dst[pos + 1] = 0;
    base += all;
  }
  if (t == 0) *len_out = nbytes + base <= a.cap ? nbytes + base : -1;
}

__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(const GatherArgs a) {
  __shared__ int s_before, s_all, s_bad;
  const int t = threadIdx.x, row = blockIdx.x, frame = blockIdx.y;
  if (t == 0) { s_before = 0; s_all = 0; s_bad = 0; }
  __syncthreads();
  const int* lens = a.lens + (size_t)frame * a.rows;
  for (int i = t; i < a.rows; i += kThreads) {
    const int l = lens[i];
    if (l < 0 || l > a.cap) { s_bad = 1; continue; }
    atomicAdd(&s_all, l);
    if (i < row) atomicAdd(&s_before, l);
  }
  __syncthreads();
  const size_t size = (size_t)a.header_len + (size_t)s_all + 2 * (size_t)a.rows;      // RSTn behind every interval but the last, then EOI
  if (s_bad || size > a.out_row_bytes) {
    if (row == 0 && t == 0) a.out_bytes[frame] = -1;
    return;
  }
  unsigned char* out = a.out + (size_t)frame * a.out_row_bytes;
  if (row == 0) {
    for (int i = t; i < a.header_len; i += kThreads) out[i] = a.header[i];
    if (t == 0) a.out_bytes[frame] = (int)size;
  }
  const int len = lens[row];
  const unsigned char* src = a.slots + ((size_t)frame * a.rows + row) * a.cap;
  unsigned char* dst = out + a.header_len + s_before + 2 * row;
  for (int i = t; i < len; i += kThreads) dst[i] = src[i];
  if (t == 0) {
    dst[len] = 0xff;
    dst[len + 1] = row + 1 < a.rows ? (unsigned char)(0xd0 + (row & 7)) : (unsigned char)0xd9;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxLds = 64 * 1024 - 64;      // the kernel's few static words beside the dynamic carve

// libjpeg's jpeg_quality_scaling and jpeg_add_quant_table with force_baseline
static void scaled_quant(const unsigned char* base, int quality, unsigned char* out) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * scale + 50) / 100;
    out[i] = (unsigned char)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
}

// T.81 Annex C: (length << 16) | code by symbol
static void huff_codes(const unsigned char* bits, const unsigned char* vals, uint32_t* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

static std::vector<unsigned char> jpeg_header(const vp_jpeg_desc* d, const unsigned char* ql, const unsigned char* qc) {
  std::vector<unsigned char> h;
  auto put = [&](std::initializer_list<int> b) { for (int v : b) h.push_back((unsigned char)v); };
  auto put16 = [&](int v) { h.push_back((unsigned char)(v >> 8)); h.push_back((unsigned char)(v & 255)); };
  put({0xff, 0xd8});
  put({0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00});
  for (int i = 0; i < 2; ++i) {
    put({0xff, 0xdb, 0x00, 0x43, i});
    for (int k = 0; k < 64; ++k) h.push_back((i ? qc : ql)[kZigzag[k]]);
  }
  put({0xff, 0xc0, 0x00, 0x11, 0x08});
  put16(d->height); put16(d->width);
  put({0x03, 0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01});
  struct { int id; const unsigned char* bits; const unsigned char* vals; int n; } tabs[4] = {
      {0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162}, {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
  for (const auto& t : tabs) {
    put({0xff, 0xc4});
    put16(19 + t.n);
    h.push_back((unsigned char)t.id);
    h.insert(h.end(), t.bits, t.bits + 16);
    h.insert(h.end(), t.vals, t.vals + t.n);
  }
  put({0xff, 0xdd, 0x00, 0x04});
  put16(d->width / 16);
  put({0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00});
  return h;
}

}  // namespace vp

struct vp_jpeg {
  vp_jpeg_desc d;
  int rows, mcus, nblk, cap, lds_bytes;
  vp::JpegTables* tables;
  unsigned char *header_dev, *slots;
  int* lens;
  short* coef;
  std::vector<unsigned char> header;
  bool keep_coef;         // set by the first vp_jpeg_tensor("coefficients"): encodes from then on also store them
};

using namespace vp;

static int jpeg_check(const vp_jpeg_desc* d, vp_jpeg* h) {
  if (const int rc = check_desc(d, "vp_jpeg")) return rc;
  if (d->max_frames < 1 || d->max_frames > VP_JPEG_MAX_FRAMES) { set_err("vp_jpeg: bad descriptor (max_frames %d, 1 .. %d)", d->max_frames, VP_JPEG_MAX_FRAMES); return VP_ERR_ARG; }
  if (d->height < 16 || d->height % 16 || d->width < 16 || d->width % 16) {
    set_err("vp_jpeg: bad descriptor (%d x %d: height and width must be multiples of 16, 4:2:0 MCUs)", d->height, d->width);
    return VP_ERR_ARG;
  }
  if (d->quality < 1 || d->quality > 100) { set_err("vp_jpeg: bad descriptor (quality %d, 1 .. 100)", d->quality); return VP_ERR_ARG; }
  if (d->height > 4096) { set_err("vp_jpeg: bad descriptor (height %d, up to 4096)", d->height); return VP_ERR_ARG; }
  h->d = *d;
  h->rows = d->height / 16; h->mcus = d->width / 16; h->nblk = 6 * h->mcus;
  h->cap = VP_JPEG_SLOT_BYTES(d->width);
  // the kernel's carve of dynamic LDS: tables, block offsets, coefficients, bit buffer
  h->lds_bytes = 4 * (128 + kHuffWords + ((h->nblk + 2) & ~1)) + 2 * h->nblk * kBlockStride + 4 * (h->cap / 4 + 1);
  if (h->lds_bytes > kMaxLds) {
    set_err("vp_jpeg: bad descriptor (width %d: an MCU row's coefficients and bit buffer need %d bytes of LDS, 65536 at most; up to 832)", d->width, h->lds_bytes);
    return VP_ERR_ARG;
  }
  return VP_OK;
}

static size_t jpeg_carve(vp_jpeg* h, void* base) {
  Arena ar(base);
  const size_t n = (size_t)h->d.max_frames * h->rows;
  h->tables = ar.take<JpegTables>(1);
  h->header_dev = ar.take<unsigned char>(1024);
  h->lens = ar.take<int>(n);
  h->slots = ar.take<unsigned char>(n * h->cap);
  h->coef = ar.take<short>(n * h->nblk * 64);
  return align256(ar.total());
}

extern "C" {

size_t vp_jpeg_desc_size(void) { return sizeof(vp_jpeg_desc); }

size_t vp_jpeg_workspace_bytes(const vp_jpeg_desc* d) {
  vp_jpeg h;
  return jpeg_check(d, &h) ? 0 : jpeg_carve(&h, nullptr);
}

size_t vp_jpeg_frame_capacity(const vp_jpeg_desc* d) {
  vp_jpeg h;
  if (jpeg_check(d, &h)) return 0;
  unsigned char q[64] = {1};
  const size_t header = jpeg_header(d, q, q).size();
  return align256(header + (size_t)h.rows * (h.cap + 2));
}

int vp_jpeg_create(const vp_jpeg_desc* d, void* workspace, size_t bytes, void* stream, vp_jpeg_t** out) {
  if (const int rc = open_handle("vp_jpeg_create", d, jpeg_check, jpeg_carve, workspace, bytes, out)) return rc;
  vp_jpeg* h = *out;
  h->keep_coef = false;
  unsigned char ql[64], qc[64];
  scaled_quant(kQLuma, d->quality, ql);
  scaled_quant(kQChroma, d->quality, qc);
  h->header = jpeg_header(d, ql, qc);
  JpegTables tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 0; i < 64; ++i) { tab.quant[0][i] = (float)ql[i]; tab.quant[1][i] = (float)qc[i]; }
  huff_codes(kAcLumaBits, kAcLumaVals, tab.huff);
  huff_codes(kAcChromaBits, kAcChromaVals, tab.huff + 256);
  huff_codes(kDcLumaBits, kDcVals, tab.huff + 512);
  huff_codes(kDcChromaBits, kDcVals, tab.huff + 528);
  hipStream_t st = (hipStream_t)stream;
  // create is not an encode: it may wait (pageable sources), once per encoder
  hipError_t e = hipMemcpyAsync(h->tables, &tab, sizeof(tab), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->header_dev, h->header.data(), h->header.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_err("vp_jpeg_create: table upload -> %s", hipGetErrorString(e)); delete h; *out = nullptr; return VP_ERR_HIP; }
  return VP_OK;
}

void vp_jpeg_destroy(vp_jpeg_t* h) { delete h; }

int vp_jpeg_encode(vp_jpeg_t* h, const unsigned char* rgb, int frames, unsigned char* out, size_t out_row_bytes, int* out_bytes, void* stream) {
  if (!h || !rgb || !out || !out_bytes || frames < 1 || frames > h->d.max_frames) {
    set_err("vp_jpeg_encode: bad argument (1 .. max_frames frames, device buffers)");
    return VP_ERR_ARG;
  }
  if ((uintptr_t)rgb & 3) { set_err("vp_jpeg_encode: the frames must start on a 4-byte boundary (the kernel reads them as dwords)"); return VP_ERR_ARG; }
  IntervalArgs a{};
  a.rgb = rgb;
  a.tab = h->tables;
  a.slots = h->slots;
  a.lens = h->lens;
  a.coef = h->keep_coef ? h->coef : nullptr;
  a.W = h->d.width; a.H = h->d.height; a.rows = h->rows; a.mcus = h->mcus; a.nblk = h->nblk; a.cap = h->cap;
  hipLaunchKernelGGL(jpeg_interval_kernel, dim3(h->rows, frames), dim3(kThreads), (size_t)h->lds_bytes, (hipStream_t)stream, a);
  VP_HIP_CHECK(hipGetLastError());
  GatherArgs g{};
  g.slots = a.slots; g.lens = a.lens;
  g.header = h->header_dev;
  g.out = out; g.out_bytes = out_bytes; g.out_row_bytes = out_row_bytes;
  g.rows = h->rows; g.cap = h->cap; g.header_len = (int)h->header.size();
  hipLaunchKernelGGL(jpeg_gather_kernel, dim3(h->rows, frames), dim3(kThreads), 0, (hipStream_t)stream, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_jpeg_tensor(vp_jpeg_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_jpeg_tensor: bad argument"); return VP_ERR_ARG; }
  if (std::string(name) != "coefficients") { set_err("vp_jpeg_tensor: no tensor '%s' (coefficients)", name); return VP_ERR_ARG; }
  h->keep_coef = true;
  *ptr = h->coef;
  if (shape) { shape[0] = h->d.max_frames; shape[1] = h->rows; shape[2] = h->nblk; shape[3] = 64; }
  return VP_OK;
}

int vp_jpeg_header(const vp_jpeg_t* h, unsigned char* host_out, size_t cap, size_t* n) {
  if (!h || !n) { set_err("vp_jpeg_header: bad argument"); return VP_ERR_ARG; }
  *n = h->header.size();
  if (host_out) {
    if (cap < h->header.size()) { set_err("vp_jpeg_header: %zu bytes needed, %zu given", h->header.size(), cap); return VP_ERR_ARG; }
    memcpy(host_out, h->header.data(), h->header.size());
  }
  return VP_OK;
}

}  // extern "C"

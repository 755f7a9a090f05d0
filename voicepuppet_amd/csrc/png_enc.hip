// PNG encoding of device tensors (vp_png_*): what the reference's five tf.summary.image calls (train_pixrefer.py:105-118) do on the host
// with zlib, for the frames of a whole launch at once and without a host wait.  tests/png_ref.py restates the byte stream.
//
// The file (PNG 1.2, bit depth 8, colour type 0 / 2 / 6, no interlace): signature, IHDR, IDAT(78 01), one IDAT per strip, IDAT(03 00,
// Adler-32), IEND.  A strip is R image rows (R from width * channels, so that the raw rows, the filtered bytes and the bit buffer fit the
// workgroup's LDS); it is filtered against the raw row above it, coded as one deflate block and closed with an empty stored block, so it
// is byte aligned and depends on nothing outside itself: the unit of parallel work.
//
//   png_strip_kernel    one workgroup per (frame, strip):
//     1. raw: the strip's rows and the row above it, uint8 or float32 (-> uint8: trunc(x * 255.5f), saturated) from the caller's
//        [frames, H, W, pixel_stride] tensor, channels [channel_offset, channel_offset + C), to LDS.
//     2. filter: a wave per row.  Adaptive: the five filters' sums of absolute signed residuals, the smallest wins, the lowest number on a
//        tie.  The filter byte and the residuals go to the strip's filtered bytes in LDS.
//     3. tokens: a maximal stretch of equal bytes is a literal and then runs (distance 1) of up to 258; pieces shorter than 3 are
//        literals.  Every thread owns a contiguous piece of the strip and the tokens that start in it; what it needs from outside its
//        piece is where the stretch around its first byte starts and where the one around its last byte ends (a max / min over the
//        threads' first and last breaks).  The tokens are never stored: the same walk runs for the histogram, the bit count and the deposit.
//     4. codes: histogram by LDS atomics; the used symbols ranked by (count, symbol); Huffman's two-queue merge by one thread; leaf depths
//        by walking up; the depth counts cut to the limit (15, code-length code 7) and repaired until Kraft's sum fits; lengths handed
//        out along the ranking; canonical codes, bit-reversed.
//     5. the coded size decides: coded bits are OR-ed into the bit buffer (LDS atomics, little-endian dwords) at offsets from a scan of
//        the threads' bit counts, or the strip is stored (00 LEN NLEN, the filtered bytes).
//     6. the chunk: length and 'IDAT' in front, the CRC-32 behind.  Every thread runs a table CRC over its share of the chunk and
//        multiplies it by x^(8 * bytes behind it) mod P (zlib's crc32_combine); the XOR of the products is the chunk's CRC.  The finished
//        chunk goes to the strip's slot of the workspace as dwords; its length, its Adler-32 pair and the stored flag to the strip table.
//   png_gather_kernel   one workgroup per (frame, strip): sums the chunk lengths of its frame (before it: its offset; all: the file size)
//        and copies its chunk behind the header and the chunks before it.  Strip 0 also copies the header, combines the Adler-32 pairs,
//        writes the last IDAT and IEND, and out_bytes[frame].
//
// Only vector loads / stores, LDS atomics and plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "workspace.h"

namespace vp {

namespace png {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = 16;
constexpr int kLdsBudget = 53248;      // raw rows + filtered strip (tests/png_ref.py LDS_BUDGET); the kernel's static tables take 10 KB more
constexpr int kSyms = 286;
constexpr int kSymsPad = 288;
constexpr int kHeaderBytes = 47;       // signature 8, IHDR 25, IDAT(78 01) 14
constexpr int kTrailerBytes = 30;      // IDAT(03 00, Adler-32) 18, IEND 12
constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr uint32_t kAdlerMod = 65521u;

struct StripArgs {
  const void* src;
  unsigned char* slots;                // [max_frames * strips][slot_bytes]
  int* meta;                           // [max_frames * strips][4]: chunk bytes, Adler a, Adler b, stored flag
  int f32, pixel_stride, channel_offset;
  int H, W, C, R, strips, filter, slot_bytes, region_a;
};

struct GatherArgs {
  const unsigned char* slots;
  const int* meta;
  const unsigned char* header;
  unsigned char* out;
  int* out_bytes;
  size_t out_row_bytes;
  int H, R, row_bytes, strips, slot_bytes;
};

struct CodeScratch {                   // build_code's working set
  int sorted[kSymsPad];
  int weight[2 * kSymsPad];
  short parent[2 * kSymsPad];
  int count[32];
  int next[32];
  int n;
};

__device__ __forceinline__ int to_u8(float x) {
  const float v = x * 255.5f;
  return v >= 255.0f ? 255 : (v > 0.0f ? (int)v : 0);        // NaN fails both comparisons: 0
}

__device__ __forceinline__ int abs_signed(int r) { r &= 255; return r < 128 ? r : 256 - r; }

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int residual(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (x - pred) & 255;
}

// (a * b) mod P over GF(2), reflected: bit 31 is x^0 (zlib's multmodp, fixed trip count)
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
  }
  return p;
}

__device__ __forceinline__ uint32_t crc_pow(uint32_t base, unsigned n) {
  uint32_t p = 0x80000000u;
  while (n) {
    if (n & 1u) p = crc_mul(p, base);
    base = crc_mul(base, base);
    n >>= 1;
  }
  return p;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sum over the workgroup; red: kWaves words nobody else uses until the next barrier after this call
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
  v = (uint32_t)wave_sum((int)v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s ^= red[w];
  return s;
}

// run length 3 .. 258 -> length symbol, its extra bits and their value (RFC 1951 3.2.5)
__device__ __forceinline__ void length_symbol(int n, int* sym, int* eb, int* val) {
  const int l = n - 3;
  if (n == 258) { *sym = 285; *eb = 0; *val = 0; return; }
  if (l < 8) { *sym = 257 + l; *eb = 0; *val = 0; return; }
  const int e = (31 - __clz(l)) - 2;
  *sym = 261 + 4 * e + ((l >> e) & 3);
  *eb = e;
  *val = l & ((1 << e) - 1);
}

// OR `n` bits of v (n <= 32) into the little-endian bit buffer at bit `at`
__device__ __forceinline__ void put_bits(uint32_t* buf, int at, uint32_t v, int n) {
  const int off = at & 31;
  const unsigned long long x = (unsigned long long)v << off;
  atomicOr(&buf[at >> 5], (uint32_t)x);
  if (off + n > 32) atomicOr(&buf[(at >> 5) + 1], (uint32_t)(x >> 32));
}

// The tokens that start in [a, b) of data[0, N): emit(position, run) with run 0 for a literal.  seg_start: where the stretch of equal
// bytes around `a` starts; next_break: the first break at or after b (N when there is none).
template <class Emit>
__device__ __forceinline__ void walk_tokens(const unsigned char* data, int a, int b, int seg_start, int next_break, Emit emit) {
  int p = a, s = seg_start;
  while (p < b) {
    int q = p + 1;
    while (q < b && data[q] == data[q - 1]) ++q;
    const int e = q < b ? q : next_break;
    const int L = e - s, pe = e < b ? e : b;
    for (int pos = p; pos < pe; ++pos) {
      const int k = pos - s;
      if (k == 0) { emit(pos, 0); continue; }
      const int j = k - 1, m = j / 258, r = j - 258 * m;
      const int rest = L - 1 - 258 * m, piece = rest < 258 ? rest : 258;
      if (piece < 3) emit(pos, 0);
      else if (r == 0) emit(pos, piece);
    }
    p = pe;
    s = pe;
  }
}

// Length-limited Huffman code of freq[0, nsym) (tests/png_ref.py huff_lengths, canonical_codes): lens and bit-reversed codes.  Called by
// the whole workgroup; freq is not changed.
__device__ void build_code(const int* freq, int nsym, int limit, int* lens, int* codes, CodeScratch& S) {
  const int t = threadIdx.x;
  if (t < 32) { S.count[t] = 0; S.next[t] = 0; }
  if (t == 0) S.n = 0;
  __syncthreads();
  for (int s = t; s < nsym; s += kThreads) {
    lens[s] = 0;
    codes[s] = 0;
    const int f = freq[s];
    if (f > 0) {
      int rank = 0;
      for (int u = 0; u < nsym; ++u) {
        const int fu = freq[u];
        rank += (fu > 0 && (fu < f || (fu == f && u < s))) ? 1 : 0;
      }
      S.sorted[rank] = s;
      S.weight[rank] = f;
      atomicAdd(&S.n, 1);
    }
  }
  __syncthreads();
  const int n = S.n;
  if (t == 0) {
    if (n == 1) S.count[1] = 1;
    int a = 0, b = n;
    for (int node = n; node < 2 * n - 1; ++node) {      // two queues: the ranked leaves, the internal nodes in the order made
      int w = 0;
      for (int i = 0; i < 2; ++i) {
        int pick;
        if (a < n && (b >= node || S.weight[a] <= S.weight[b])) pick = a++; else pick = b++;
        S.parent[pick] = (short)node;
        w += S.weight[pick];
      }
      S.weight[node] = w;
    }
  }
  __syncthreads();
  if (n > 1) {
    for (int j = t; j < n; j += kThreads) {
      int d = 0, x = j;
      while (x != 2 * n - 2) { x = S.parent[x]; ++d; }
      atomicAdd(&S.count[d < limit ? d : limit], 1);
    }
  }
  __syncthreads();
  if (t == 0) {
    int total = 0;
    for (int d = 1; d <= limit; ++d) total += S.count[d] << (limit - d);
    while (total > (1 << limit)) {
      S.count[limit] -= 1;
      for (int d = limit - 1; d > 0; --d)
        if (S.count[d]) { S.count[d] -= 1; S.count[d + 1] += 2; break; }
      --total;
    }
    int code = 0;
    for (int l = 1; l <= limit; ++l) { code = (code + S.count[l - 1]) << 1; S.next[l] = code; }
  }
  __syncthreads();
  for (int j = t; j < n; j += kThreads) {
    int c = 0, len = 1;
    for (int d = limit; d > 0; --d) { c += S.count[d]; if (j < c) { len = d; break; } }
    lens[S.sorted[j]] = len;
  }
  __syncthreads();
  for (int s = t; s < nsym; s += kThreads) {
    const int l = lens[s];
    if (l) {
      int idx = 0;
      for (int u = 0; u < s; ++u) idx += lens[u] == l ? 1 : 0;
      codes[s] = (int)(__brev((uint32_t)(S.next[l] + idx)) >> (32 - l));
    }
  }
  __syncthreads();
}

__constant__ unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__global__ __launch_bounds__(kThreads) void png_strip_kernel(const StripArgs a) {
  extern __shared__ uint32_t lds[];
  unsigned char* raw = reinterpret_cast<unsigned char*>(lds);          // [rows + 1][W C], row 0 the row above; later the chunk
  uint32_t* out32 = lds;
  unsigned char* out8 = raw;
  unsigned char* filt = raw + a.region_a;                              // [rows][1 + W C]
  __shared__ uint32_t crc_tab[256];
  __shared__ int hist[kSymsPad], ll_len[kSymsPad], ll_code[kSymsPad];
  __shared__ int cl_freq[20], cl_len[20], cl_code[20];
  __shared__ int first_break[kThreads], last_break[kThreads];
  __shared__ CodeScratch S;
  __shared__ uint32_t red[kWaves];
  __shared__ int s_nll, s_hdr_bits, s_ncl;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int strip = blockIdx.x, frame = blockIdx.y;
  const int WC = a.W * a.C, RB = WC + 1;
  const int y0 = strip * a.R;
  const int rows = a.H - y0 < a.R ? a.H - y0 : a.R;
  const int N = rows * RB;

  {
    uint32_t c = (uint32_t)t;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
    crc_tab[t] = c;
  }
  for (int s = t; s < kSymsPad; s += kThreads) hist[s] = 0;
  if (t < 20) cl_freq[t] = 0;
  if (t == 0) s_nll = 0;

  // 1. the raw rows
  for (int e = t; e < (rows + 1) * WC; e += kThreads) {
    const int r = e / WC, i = e - r * WC, y = y0 + r - 1;
    int v = 0;
    if (y >= 0) {
      const int px = i / a.C, c = i - px * a.C;
      const size_t at = (((size_t)frame * a.H + y) * a.W + px) * a.pixel_stride + a.channel_offset + c;
      v = a.f32 ? to_u8(static_cast<const float*>(a.src)[at]) : (int)static_cast<const unsigned char*>(a.src)[at];
    }
    raw[e] = (unsigned char)v;
  }
  __syncthreads();

  // 2. filter, a wave per row
  for (int r = wave; r < rows; r += kWaves) {
    const unsigned char* cur = raw + (r + 1) * WC;
    const unsigned char* up = raw + r * WC;
    int f = a.filter;
    if (f < 0) {
      int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
      for (int i = lane; i < WC; i += 64) {
        const int x = cur[i], b = up[i], l = i >= a.C ? cur[i - a.C] : 0, c = i >= a.C ? up[i - a.C] : 0;
        s0 += abs_signed(x);
        s1 += abs_signed(x - l);
        s2 += abs_signed(x - b);
        s3 += abs_signed(x - ((l + b) >> 1));
        s4 += abs_signed(x - paeth(l, b, c));
      }
      s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
      f = 0;
      int best = s0;
      if (s1 < best) { best = s1; f = 1; }
      if (s2 < best) { best = s2; f = 2; }
      if (s3 < best) { best = s3; f = 3; }
      if (s4 < best) { best = s4; f = 4; }
    }
    unsigned char* dst = filt + r * RB;
    if (lane == 0) dst[0] = (unsigned char)f;
    for (int i = lane; i < WC; i += 64) {
      const int x = cur[i], b = up[i], l = i >= a.C ? cur[i - a.C] : 0, c = i >= a.C ? up[i - a.C] : 0;
      dst[1 + i] = (unsigned char)residual(f, x, l, b, c);
    }
  }
  __syncthreads();

  // the raw rows are done with: their place becomes the chunk (length, 'IDAT', data, CRC), zeroed for the bit deposit
  const int out_words = (8 + N + 10 + 4 + 3) / 4 + 1;
  for (int i = t; i < out_words; i += kThreads) out32[i] = 0;

  // 3. every thread's piece of the strip, and the breaks around it
  const int per = (N + kThreads - 1) / kThreads;
  const int pa = t * per < N ? t * per : N, pb = pa + per < N ? pa + per : N;
  {
    int fb = N, lb = -1;
    for (int p = pa; p < pb; ++p)
      if (p == 0 || filt[p] != filt[p - 1]) { if (fb == N) fb = p; lb = p; }
    first_break[t] = fb;
    last_break[t] = lb;
  }
  __syncthreads();
  int seg_start = 0, next_break = N;
  for (int u = 0; u < t; ++u) { const int v = last_break[u]; seg_start = v > seg_start ? v : seg_start; }
  for (int u = kThreads - 1; u > t; --u) { const int v = first_break[u]; next_break = v < next_break ? v : next_break; }
  if (pa < pb && (pa == 0 || filt[pa] != filt[pa - 1])) seg_start = pa;

  // 4. histogram and the two codes
  walk_tokens(filt, pa, pb, seg_start, next_break, [&](int pos, int run) {
    int sym = filt[pos], eb, val;
    if (run) length_symbol(run, &sym, &eb, &val);
    atomicAdd(&hist[sym], 1);
  });
  if (t == 0) atomicAdd(&hist[256], 1);
  __syncthreads();
  build_code(hist, kSyms, 15, ll_len, ll_code, S);
  for (int s = t; s < kSyms; s += kThreads)
    if (ll_len[s]) atomicMax(&s_nll, s + 1);
  __syncthreads();
  const int n_ll = s_nll;
  for (int s = t; s < n_ll; s += kThreads) atomicAdd(&cl_freq[ll_len[s]], 1);
  if (t == 0) atomicAdd(&cl_freq[1], 1);                 // the one distance code, length 1
  __syncthreads();
  build_code(cl_freq, 19, 7, cl_len, cl_code, S);
  if (t == 0) {
    int n_cl = 4;
    for (int i = 4; i < 19; ++i) if (cl_len[kClOrder[i]]) n_cl = i + 1;
    int bits = 17 + 3 * n_cl;
    for (int v = 0; v < 16; ++v) bits += cl_freq[v] * cl_len[v];
    s_ncl = n_cl;
    s_hdr_bits = bits;
  }

  // 5. bit counts, their scan, and the decision
  int my_bits = 0;
  walk_tokens(filt, pa, pb, seg_start, next_break, [&](int pos, int run) {
    int sym = filt[pos], eb = 0, val;
    if (run) { length_symbol(run, &sym, &eb, &val); eb += 1; }
    my_bits += ll_len[sym] + eb;
  });
  int inc = my_bits;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();
  if (lane == 63) red[wave] = (uint32_t)inc;
  __syncthreads();
  int before = inc - my_bits, token_bits = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) { const int c = (int)red[w]; token_bits += c; if (w < wave) before += c; }
  const int hdr_bits = s_hdr_bits, n_cl = s_ncl;
  const int block_bits = hdr_bits + token_bits + ll_len[256];
  const int coded_bytes = (block_bits + 3 + 7) / 8 + 4;
  const int stored_bytes = N + 10;
  const bool stored = coded_bytes >= stored_bytes;
  const int D = stored ? stored_bytes : coded_bytes;
  __syncthreads();                                       // red is free again

  const int base = 64;                                   // the data starts behind the chunk's length and type
  if (!stored) {
    if (t == 0) {
      put_bits(out32, base, 0u | (2u << 1) | ((uint32_t)(n_ll - 257) << 3) | (0u << 8) | ((uint32_t)(n_cl - 4) << 13), 17);
      for (int i = 0; i < n_cl; ++i) put_bits(out32, base + 17 + 3 * i, (uint32_t)cl_len[kClOrder[i]], 3);
    }
    for (int s = t; s < n_ll + 1; s += kThreads) {
      int at = base + 17 + 3 * n_cl;
      for (int u = 0; u < s; ++u) at += cl_len[ll_len[u]];
      const int l = s < n_ll ? ll_len[s] : 1;
      put_bits(out32, at, (uint32_t)cl_code[l], cl_len[l]);
    }
    int at = base + hdr_bits + before;
    walk_tokens(filt, pa, pb, seg_start, next_break, [&](int pos, int run) {
      int sym = filt[pos], eb = 0, val = 0;
      if (run) { length_symbol(run, &sym, &eb, &val); }
      const int l = ll_len[sym];
      const int n = l + eb + (run ? 1 : 0);              // the distance code is one 0 bit above the extra bits
      put_bits(out32, at, (uint32_t)ll_code[sym] | ((uint32_t)val << l), n);
      at += n;
    });
    if (t == kThreads - 1) put_bits(out32, base + hdr_bits + token_bits, (uint32_t)ll_code[256], ll_len[256]);
    __syncthreads();
    if (t == 0) { out8[8 + D - 2] = 0xff; out8[8 + D - 1] = 0xff; }      // 000, padding, 00 00 FF FF
  } else {
    if (t == 0) {
      out8[8] = 0;
      out8[9] = (unsigned char)(N & 255); out8[10] = (unsigned char)(N >> 8);
      out8[11] = (unsigned char)(~N & 255); out8[12] = (unsigned char)((~N >> 8) & 255);
      out8[8 + D - 2] = 0xff; out8[8 + D - 1] = 0xff;                    // 00 00 00 FF FF
    }
    for (int i = t; i < N; i += kThreads) out8[13 + i] = filt[i];
  }
  if (t == 0) {
    out8[0] = (unsigned char)(D >> 24); out8[1] = (unsigned char)(D >> 16); out8[2] = (unsigned char)(D >> 8); out8[3] = (unsigned char)D;
    out8[4] = 'I'; out8[5] = 'D'; out8[6] = 'A'; out8[7] = 'T';
  }
  __syncthreads();

  // 6. CRC-32 of type and data: equal shares counted from the end, thread t has (255 - t) shares behind it
  const int T = D + 4;
  const int share = (T + kThreads - 1) / kThreads;
  int lo = T - (kThreads - t) * share, hi = lo + share;
  uint32_t state = (lo <= 0 && hi > 0) ? 0xffffffffu : 0u;
  if (lo < 0) lo = 0;
  for (int i = lo; i < hi; ++i) state = crc_tab[(state ^ out8[4 + i]) & 255u] ^ (state >> 8);
  uint32_t part = 0;
  if (state) {
    const uint32_t m0 = crc_pow(0x00800000u, (unsigned)share);           // x^(8 share)
    part = crc_mul(crc_pow(m0, (unsigned)(kThreads - 1 - t)), state);
  }
  const uint32_t crc = block_xor(part, red) ^ 0xffffffffu;
  if (t == 0) {
    out8[8 + D] = (unsigned char)(crc >> 24); out8[9 + D] = (unsigned char)(crc >> 16);
    out8[10 + D] = (unsigned char)(crc >> 8); out8[11 + D] = (unsigned char)crc;
  }

  // Adler-32 of the filtered bytes: a = 1 + sum d, b = N + sum (N - i) d[i]
  uint32_t s1 = 0, s2 = 0;
  for (int i = pa; i < pb; ++i) { const uint32_t d = filt[i]; s1 += d; s2 += (uint32_t)(N - i) * d; }     // < 2^32: 113 * 28672 * 255
  s2 %= kAdlerMod;
  const uint32_t sum1 = block_sum(s1, red);
  const uint32_t sum2 = block_sum(s2, red);              // its barriers also order the CRC bytes before the copy
  const size_t slot = (size_t)frame * a.strips + strip;
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.slots + slot * a.slot_bytes);
  for (int i = t; i < (12 + D + 3) / 4; i += kThreads) dst[i] = out32[i];
  if (t == 0) {
    int* m = a.meta + slot * 4;
    m[0] = 12 + D;
    m[1] = (int)((1u + sum1) % kAdlerMod);
    m[2] = (int)(((uint32_t)N + sum2) % kAdlerMod);
    m[3] = stored ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void png_gather_kernel(const GatherArgs a) {
  __shared__ int s_before, s_all;
  const int t = threadIdx.x, strip = blockIdx.x, frame = blockIdx.y;
  if (t == 0) { s_before = 0; s_all = 0; }
  __syncthreads();
  const int* meta = a.meta + (size_t)frame * a.strips * 4;
  for (int i = t; i < a.strips; i += kThreads) {
    const int l = meta[4 * i];
    atomicAdd(&s_all, l);
    if (i < strip) atomicAdd(&s_before, l);
  }
  __syncthreads();
  const size_t size = (size_t)kHeaderBytes + (size_t)s_all + kTrailerBytes;
  if (size > a.out_row_bytes) return;                    // cannot happen: vp_png_encode refuses a row below vp_png_frame_capacity
  unsigned char* out = a.out + (size_t)frame * a.out_row_bytes;
  const int len = meta[4 * strip];
  const unsigned char* src = a.slots + ((size_t)frame * a.strips + strip) * a.slot_bytes;
  unsigned char* dst = out + kHeaderBytes + s_before;
  for (int i = t; i < len; i += kThreads) dst[i] = src[i];
  if (strip != 0) return;
  for (int i = t; i < kHeaderBytes; i += kThreads) out[i] = a.header[i];
  if (t == 0) {
    unsigned long long A = 1, B = 0;
    for (int i = 0; i < a.strips; ++i) {
      const int rows = a.H - i * a.R < a.R ? a.H - i * a.R : a.R;
      const unsigned long long a2 = (unsigned)meta[4 * i + 1], b2 = (unsigned)meta[4 * i + 2], len2 = (unsigned long long)rows * a.row_bytes;
      B = (B + b2 + (len2 % kAdlerMod) * (A + kAdlerMod - 1)) % kAdlerMod;
      A = (A + a2 + kAdlerMod - 1) % kAdlerMod;
    }
    unsigned char tail[kTrailerBytes] = {0, 0, 0, 6, 'I', 'D', 'A', 'T', 0x03, 0x00, (unsigned char)(B >> 8), (unsigned char)B, (unsigned char)(A >> 8),
                                         (unsigned char)A, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    uint32_t c = 0xffffffffu;
    for (int i = 4; i < 14; ++i) {
      c ^= tail[i];
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
    }
    c ^= 0xffffffffu;
    tail[14] = (unsigned char)(c >> 24); tail[15] = (unsigned char)(c >> 16); tail[16] = (unsigned char)(c >> 8); tail[17] = (unsigned char)c;
    unsigned char* end = out + kHeaderBytes + s_all;
    for (int i = 0; i < kTrailerBytes; ++i) end[i] = tail[i];
    a.out_bytes[frame] = (int)size;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
static size_t align_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

static uint32_t host_crc(const unsigned char* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
  }
  return c ^ 0xffffffffu;
}

static std::vector<unsigned char> file_header(const vp_png_desc* d) {
  std::vector<unsigned char> h = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  auto put32 = [&](uint32_t v) { for (int s = 24; s >= 0; s -= 8) h.push_back((unsigned char)(v >> s)); };
  auto chunk = [&](const char* kind, const std::vector<unsigned char>& data) {
    put32((uint32_t)data.size());
    const size_t at = h.size();
    h.insert(h.end(), kind, kind + 4);
    h.insert(h.end(), data.begin(), data.end());
    put32(host_crc(h.data() + at, h.size() - at));
  };
  std::vector<unsigned char> ihdr;
  for (int s = 24; s >= 0; s -= 8) ihdr.push_back((unsigned char)((uint32_t)d->width >> s));
  for (int s = 24; s >= 0; s -= 8) ihdr.push_back((unsigned char)((uint32_t)d->height >> s));
  ihdr.push_back(8);
  ihdr.push_back(d->channels == 1 ? 0 : d->channels == 3 ? 2 : 6);
  ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
  chunk("IHDR", ihdr);
  chunk("IDAT", {0x78, 0x01});
  return h;
}

}  // namespace png
}  // namespace vp

struct vp_png {
  vp_png_desc d;
  int R, strips, WC, RB, slot_bytes, region_a, lds_bytes;
  size_t capacity;
  unsigned char *header_dev, *slots;
  int* meta;
  std::vector<unsigned char> header;
};

using namespace vp;
using namespace vp::png;

static int png_check(const vp_png_desc* d, vp_png* h) {
  if (const int rc = check_desc(d, "vp_png")) return rc;
  if (d->max_frames < 1 || d->max_frames > VP_PNG_MAX_FRAMES) { set_err("vp_png: bad descriptor (max_frames %d, 1 .. %d)", d->max_frames, VP_PNG_MAX_FRAMES); return VP_ERR_ARG; }
  if (d->height < 1 || d->height > VP_PNG_MAX_HEIGHT) { set_err("vp_png: bad descriptor (height %d, 1 .. %d)", d->height, VP_PNG_MAX_HEIGHT); return VP_ERR_ARG; }
  if (d->channels != 1 && d->channels != 3 && d->channels != 4) { set_err("vp_png: bad descriptor (channels %d: 1, 3 or 4)", d->channels); return VP_ERR_ARG; }
  if (d->filter < -1 || d->filter > 4) { set_err("vp_png: bad descriptor (filter %d: -1 adaptive, 0 .. 4 forced)", d->filter); return VP_ERR_ARG; }
  if (d->width < 1 || (long long)d->width * d->channels > VP_PNG_MAX_ROW_BYTES) {
    set_err("vp_png: bad descriptor (width %d x %d channels: 1 .. %d bytes per row, a strip lives in one workgroup's LDS)", d->width, d->channels, VP_PNG_MAX_ROW_BYTES);
    return VP_ERR_ARG;
  }
  h->d = *d;
  h->WC = d->width * d->channels;
  h->RB = h->WC + 1;
  int R = (kLdsBudget - 32 - h->WC) / (2 * h->WC + 1);
  h->R = R > kMaxRows ? kMaxRows : R;                                     // >= 1 up to VP_PNG_MAX_ROW_BYTES
  h->strips = (d->height + h->R - 1) / h->R;
  const int chunk = 12 + h->R * h->RB + 10;
  h->slot_bytes = (int)align_up((size_t)chunk + 4, 16);
  const int raw = (h->R + 1) * h->WC;
  h->region_a = (int)align_up((size_t)(raw > chunk + 12 ? raw : chunk + 12), 16);
  h->lds_bytes = h->region_a + (int)align_up((size_t)h->R * h->RB, 16);
  h->capacity = kHeaderBytes + kTrailerBytes;
  for (int y = 0; y < d->height; y += h->R) h->capacity += 12 + (size_t)(d->height - y < h->R ? d->height - y : h->R) * h->RB + 10;
  if (h->capacity > 0x7fffffffu) { set_err("vp_png: bad descriptor (%d x %d x %d: a file of up to %zu bytes, lengths are 31 bits)", d->height, d->width, d->channels, h->capacity); return VP_ERR_ARG; }
  return VP_OK;
}

static size_t png_carve(vp_png* h, void* base) {
  Arena ar(base);
  const size_t n = (size_t)h->d.max_frames * h->strips;
  h->header_dev = ar.take<unsigned char>(kHeaderBytes);
  h->meta = ar.take<int>(n * 4);
  h->slots = ar.take<unsigned char>(n * h->slot_bytes);
  return align256(ar.total());
}

extern "C" {

size_t vp_png_desc_size(void) { return sizeof(vp_png_desc); }

size_t vp_png_workspace_bytes(const vp_png_desc* d) {
  vp_png h;
  return png_check(d, &h) ? 0 : png_carve(&h, nullptr);
}

size_t vp_png_frame_capacity(const vp_png_desc* d) {
  vp_png h;
  return png_check(d, &h) ? 0 : align256(h.capacity);
}

int vp_png_rows_per_strip(const vp_png_desc* d) {
  vp_png h;
  return png_check(d, &h) ? 0 : h.R;
}

int vp_png_create(const vp_png_desc* d, void* workspace, size_t bytes, void* stream, vp_png_t** out) {
  if (const int rc = open_handle("vp_png_create", d, png_check, png_carve, workspace, bytes, out)) return rc;
  vp_png* h = *out;
  h->header = file_header(d);
  hipStream_t st = (hipStream_t)stream;
  // create is not an encode: it may wait (a pageable source), once per encoder
  hipError_t e = hipMemcpyAsync(h->header_dev, h->header.data(), h->header.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_err("vp_png_create: header upload -> %s", hipGetErrorString(e)); delete h; *out = nullptr; return VP_ERR_HIP; }
  return VP_OK;
}

void vp_png_destroy(vp_png_t* h) { delete h; }

int vp_png_encode(vp_png_t* h, const void* src, int src_dtype, int pixel_stride, int channel_offset, int frames, unsigned char* out,
                  size_t out_row_bytes, int* out_bytes, void* stream) {
  if (!h || !src || !out || !out_bytes || frames < 1 || frames > h->d.max_frames) {
    set_err("vp_png_encode: bad argument (1 .. max_frames frames, device buffers)");
    return VP_ERR_ARG;
  }
  if (src_dtype != VP_PNG_U8 && src_dtype != VP_PNG_F32) { set_err("vp_png_encode: src_dtype %d (VP_PNG_U8 or VP_PNG_F32)", src_dtype); return VP_ERR_ARG; }
  if (channel_offset < 0 || pixel_stride < 1 || pixel_stride > VP_PNG_MAX_PIXEL_STRIDE || channel_offset + h->d.channels > pixel_stride) {
    set_err("vp_png_encode: channels [%d, %d) of a pixel of %d (up to %d)", channel_offset, channel_offset + h->d.channels, pixel_stride, VP_PNG_MAX_PIXEL_STRIDE);
    return VP_ERR_ARG;
  }
  if (src_dtype == VP_PNG_F32 && ((uintptr_t)src & 3)) { set_err("vp_png_encode: a float32 source must start on a 4-byte boundary"); return VP_ERR_ARG; }
  if (out_row_bytes < h->capacity) { set_err("vp_png_encode: out_row_bytes %zu, a file may take %zu (vp_png_frame_capacity)", out_row_bytes, h->capacity); return VP_ERR_ARG; }
  StripArgs a{};
  a.src = src;
  a.slots = h->slots;
  a.meta = h->meta;
  a.f32 = src_dtype == VP_PNG_F32; a.pixel_stride = pixel_stride; a.channel_offset = channel_offset;
  a.H = h->d.height; a.W = h->d.width; a.C = h->d.channels; a.R = h->R; a.strips = h->strips; a.filter = h->d.filter;
  a.slot_bytes = h->slot_bytes; a.region_a = h->region_a;
  hipLaunchKernelGGL(png_strip_kernel, dim3(h->strips, frames), dim3(kThreads), (size_t)h->lds_bytes, (hipStream_t)stream, a);
  VP_HIP_CHECK(hipGetLastError());
  GatherArgs g{};
  g.slots = a.slots; g.meta = a.meta;
  g.header = h->header_dev;
  g.out = out; g.out_bytes = out_bytes; g.out_row_bytes = out_row_bytes;
  g.H = a.H; g.R = h->R; g.row_bytes = h->RB; g.strips = h->strips; g.slot_bytes = h->slot_bytes;
  hipLaunchKernelGGL(png_gather_kernel, dim3(h->strips, frames), dim3(kThreads), 0, (hipStream_t)stream, g);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_png_tensor(vp_png_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_png_tensor: bad argument"); return VP_ERR_ARG; }
  if (std::string(name) != "strips") { set_err("vp_png_tensor: no tensor '%s' (strips)", name); return VP_ERR_ARG; }
  *ptr = h->meta;
  if (shape) { shape[0] = h->d.max_frames; shape[1] = h->strips; shape[2] = 4; shape[3] = 1; }
  return VP_OK;
}

int vp_png_header(const vp_png_t* h, unsigned char* host_out, size_t cap, size_t* n) {
  if (!h || !n) { set_err("vp_png_header: bad argument"); return VP_ERR_ARG; }
  *n = h->header.size();
  if (host_out) {
    if (cap < h->header.size()) { set_err("vp_png_header: %zu bytes needed, %zu given", h->header.size(), cap); return VP_ERR_ARG; }
    memcpy(host_out, h->header.data(), h->header.size());
  }
  return VP_OK;
}

}  // extern "C"

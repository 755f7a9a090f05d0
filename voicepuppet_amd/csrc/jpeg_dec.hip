// Baseline JPEG decoding of a batch of files on the device (vp_jpegdec_*): what the reference does per sample on the host with two
// cv2.imread calls (generator/generator.py:956-1019) and in ImageLoader (generator/loader.py).  The host parses the headers and packs, per
// file, a meta blob (quantisation tables, Huffman look-up tables, segment table: include/vp_hip.h) and the file itself into one buffer.
//
//   jpegdec_entropy_kernel  one lane per segment, the 64 lanes of a workgroup on one file (its four Huffman tables in LDS).  A lane runs a
//        64-bit bit buffer refilled bytewise (stuffed 0x00 dropped; from a marker or the end of the file on it feeds zeros and counts
//        them), decodes a symbol by a 9-bit look-up or, for longer codes, the canonical maxcode walk, and stores every block's int16
//        coefficients row-major to the workspace (the block zeroed first).  At every MCU-row start it records where it stands (byte, bit,
//        predictors) in `entries`.  Reads are bounded by the file's length, writes by the segment's MCU range clamped to the file's MCU
//        count, both taken from the kernel arguments the host validated against the descriptor, never from the blob.
//   jpegdec_scan_kernel     (opt-in, vp_jpegdec_enable_scan) one workgroup per file without restart markers and without an index: finds the
//        file's MCU-row entry points in parallel, chunk by chunk, by the self-synchronisation of Huffman streams, and writes `entries`
//        before the entropy kernel of the same call runs, which then takes one lane per MCU row.  See the comment at the kernel.
//   jpegdec_planes_kernel   one thread per 8 x 8 block: dequantise, libjpeg's "islow" inverse DCT in registers, uint8 to the padded plane.
//   jpegdec_rgb_kernel      one thread per 4 pixels of a row: fancy up-sampling of chroma (4:2:0 both ways, 4:2:2 along the row), YCbCr -> RGB,
//        three dword stores where the row is dword aligned (a wave writes 768 contiguous bytes), bytes at a ragged right edge or on an
//        unaligned row.
//
// Three layouts (vp_jpegdec_file.sampling): 1, 4:4:4, an MCU of 8 x 8 pixels and the blocks Y Cb Cr; 2, 4:2:0, 16 x 16 and Y00 Y01 Y10 Y11
// Cb Cr; 3, 4:2:2, 16 wide and 8 high and Y0 (left) Y1 (right) Cb Cr.  blocks_per_mcu() and block_component() are the only places that
// know the block sequences.
//
// Only vector loads / stores and plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "workspace.h"

namespace vp {

constexpr int kLookupBits = 9;
constexpr int kHuffBytes = 1424;             // uint16 lut[512], int32 maxcode[18], int32 valoff[18], uint8 vals[256]
constexpr int kQuantAt = 128, kHuffAt = 640, kSegAt = VP_JPEGDEC_META_BYTES;
constexpr int kLanes = 64;
constexpr int kScanLanes = 1024;             // chunks of one sweep of the index scan

struct DecFile {                             // one file of a launch, as kernel argument
  uint32_t meta, file;                       // offsets in the blob
  uint32_t bytes, nseg, dri;
  uint16_t W, H, mcux, mcuy;
  uint8_t sampling, tq[3], td[3], ta[3];
  uint8_t scan, pad;                         // scan: the index scan runs on this file and the entropy kernel asks scan_ok
};

struct DecArgs {
  const unsigned char* blob;
  short* coef;                               // [slot][blocks_cap][64]
  int* entries;                              // [slot][rows_cap][4]
  unsigned char* planes;                     // [slot][3][Hp][Wp]
  unsigned char* out;
  int* status;
  size_t row_pitch, frame_stride;
  int first;                                 // slot of f[0]
  int blocks_cap, rows_cap, Hp, Wp, bgr;
  uint2* scan_state;                         // [file of the launch][chunks_cap]: exit state per chunk (null: no scan)
  int* scan_ok;                              // [slot]
  int* scan_rounds;                          // [slot]
  int chunk_bytes, chunks_cap, max_rounds;
  DecFile f[VP_JPEGDEC_FILES_PER_LAUNCH];
};

// blocks of one MCU, and the component of its block j, per layout
__host__ __device__ __forceinline__ int blocks_per_mcu(int sampling) { return sampling == 2 ? 6 : (sampling == 3 ? 4 : 3); }
__device__ __forceinline__ int block_component(int bpm, int j) { return bpm == 6 ? (j < 4 ? 0 : j - 3) : (bpm == 4 ? (j < 2 ? 0 : j - 1) : j); }

struct HuffLds {
  uint16_t lut[512];
  int maxcode[18];
  int valoff[18];
  unsigned char vals[256];
};
static_assert(sizeof(HuffLds) == kHuffBytes, "meta blob layout");

struct ZigzagNat {
  unsigned char at[64];
  constexpr ZigzagNat() : at() {
    constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    for (int i = 0; i < 64; ++i) at[i] = zz[i];
  }
};
__device__ __constant__ ZigzagNat kZigzagNat{};      // zig-zag position -> row-major index

struct BitReader {
  const unsigned char* p;        // the file
  uint32_t pos, end;             // next byte to fetch; the file's length
  uint64_t buf;                  // left aligned
  int nbits;                     // valid bits in buf
  int real;                      // of them from the file (the zeros fed behind the data are the last); negative: zeros were consumed
  bool stopped;

  __device__ __forceinline__ void start(uint32_t at, int bit) {
    pos = at < end ? at : end; buf = 0; nbits = 0; real = 0; stopped = false;
    refill();
    take(bit & 7);
  }
  __device__ __forceinline__ void refill() {
    while (nbits <= 56) {
      uint32_t b = 0;
      bool got = false;
      if (!stopped && pos < end) {
        b = p[pos];
        if (b != 0xff) { ++pos; got = true; }
        else if (pos + 1 < end && p[pos + 1] == 0) { pos += 2; got = true; }
      }
      if (got) real += 8; else { stopped = true; b = 0; }
      buf |= (uint64_t)b << (56 - nbits);
      nbits += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }     // 1 <= n <= 32
  __device__ __forceinline__ void skip(int n) { buf <<= n; nbits -= n; real -= n; }
  __device__ __forceinline__ uint32_t take(int n) {
    if (n == 0) return 0;
    const uint32_t v = peek(n);
    skip(n);
    return v;
  }
  // where the next unread bit lies in the file: walks back over the data bytes still in the buffer (a 0x00 behind a 0xff is stuffing)
  __device__ __forceinline__ void where(int* byte, int* bit) const {
    uint32_t at = pos;
    const int k = real > 0 ? (real + 7) >> 3 : 0;
    for (int i = 0; i < k && at > 0; ++i) {
      --at;
      if (at > 0 && p[at] == 0 && p[at - 1] == 0xff) --at;
    }
    *byte = (int)at;
    *bit = real > 0 ? (8 - (real & 7)) & 7 : 0;
  }
};

// -1: no code of up to 16 bits starts the buffer
__device__ __forceinline__ int huff_symbol(BitReader& r, const HuffLds& t) {
  r.refill();
  const uint32_t e = t.lut[r.peek(kLookupBits)];
  if (e) { r.skip((int)(e >> 8)); return (int)(e & 255u); }
  const int look = (int)r.peek(16);
  for (int l = kLookupBits + 1; l <= 16; ++l) {
    const int code = look >> (16 - l);
    if (code <= t.maxcode[l]) { r.skip(l); return t.vals[(code + t.valoff[l]) & 255]; }
  }
  return -1;
}

__device__ __forceinline__ int extend(uint32_t v, int s) { return s == 0 || v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1; }

__global__ __launch_bounds__(kLanes) void jpegdec_entropy_kernel(const DecArgs a) {
  __shared__ HuffLds huff[4];
  const DecFile& f = a.f[blockIdx.y];
  const int seg = blockIdx.x * kLanes + threadIdx.x;
  // a scanned file whose scan held: one lane per MCU row from `entries`; one that did not hold: its single segment, as without the scan
  const bool by_row = f.scan && a.scan_ok[a.first + blockIdx.y] == 1;
  const uint32_t nseg = by_row ? (uint32_t)f.mcuy : f.nseg;
  if ((uint32_t)(blockIdx.x * kLanes) >= nseg) return;          // the whole workgroup
  const unsigned char* meta = a.blob + f.meta;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(meta + kHuffAt);
    uint32_t* dst = reinterpret_cast<uint32_t*>(huff);
    for (int i = threadIdx.x; i < 4 * kHuffBytes / 4; i += kLanes) dst[i] = src[i];
  }
  __syncthreads();
  if ((uint32_t)seg >= nseg) return;
  const int slot = a.first + blockIdx.y;
  int* entries = a.entries + (size_t)slot * a.rows_cap * 4;    // mcuy <= rows_cap: checked by the host against the descriptor
  int sg[6];
  if (by_row) {
    const int4 e = *reinterpret_cast<const int4*>(entries + 4 * seg);
    sg[0] = e.x; sg[1] = e.y; sg[2] = e.z; sg[3] = e.w; sg[4] = seg * (int)f.mcux; sg[5] = f.mcux;
  } else {
    const int* src = reinterpret_cast<const int*>(meta + kSegAt) + 6 * seg;
#pragma unroll
    for (int i = 0; i < 6; ++i) sg[i] = src[i];
  }
  const int bpm = blocks_per_mcu(f.sampling);
  const int total = (int)f.mcux * f.mcuy;
  int mcu0 = sg[4], count = sg[5];
  if (mcu0 < 0 || mcu0 >= total || count < 1) return;           // nothing this lane may write
  if (count > total - mcu0) count = total - mcu0;
  int pred[3] = {(int)(short)(sg[2] & 0xffff), (int)(short)((uint32_t)sg[2] >> 16), (int)(short)(sg[3] & 0xffff)};

  BitReader r;
  r.p = a.blob + f.file;
  r.end = f.bytes;
  r.start((uint32_t)sg[0], sg[1]);
  // total * bpm <= blocks_cap = 3 (Hp / 8) (Wp / 8): likewise.  4:2:2: 4 mcux mcuy <= 4 (Wp / 16) (Hp / 8) = 2 (Hp / 8) (Wp / 8), and
  // mcuy = ceil(H / 8) <= Hp / 8 = rows_cap for `entries` above
  short* coef = a.coef + (size_t)slot * a.blocks_cap * 64;
  bool bad = false;
  for (int mcu = mcu0; mcu < mcu0 + count && !bad; ++mcu) {
    if (f.dri && mcu > mcu0 && mcu % (int)f.dri == 0) {         // a restart inside the segment: the marker, predictors zero
      r.refill();
      const uint32_t m = r.pos;
      if (r.real < 8 && m + 1 < r.end && r.p[m] == 0xff && (r.p[m + 1] & 0xf8) == 0xd0) {
        r.start(m + 2, 0);
        pred[0] = pred[1] = pred[2] = 0;
      } else { bad = true; break; }
    }
    if (mcu % (int)f.mcux == 0) {
      int byte, bit;
      r.where(&byte, &bit);
      int4 e;
      e.x = byte; e.y = bit;
      e.z = (int)(((uint32_t)pred[0] & 0xffffu) | ((uint32_t)pred[1] << 16));
      e.w = (int)((uint32_t)pred[2] & 0xffffu);
      *reinterpret_cast<int4*>(entries + 4 * (mcu / (int)f.mcux)) = e;
    }
    for (int j = 0; j < bpm && !bad; ++j) {
      const int c = block_component(bpm, j);
      short* blk = coef + ((size_t)mcu * bpm + j) * 64;
      uint4* z = reinterpret_cast<uint4*>(blk);
#pragma unroll
      for (int i = 0; i < 8; ++i) z[i] = make_uint4(0, 0, 0, 0);
      int s = huff_symbol(r, huff[f.td[c]]);
      if (s < 0 || s > 15) { bad = true; break; }
      pred[c] += extend(r.take(s), s);
      blk[0] = (short)pred[c];
      const HuffLds& ac = huff[2 + f.ta[c]];
      int k = 1;
      while (k < 64) {
        const int rs = huff_symbol(r, ac);
        if (rs < 0) { bad = true; break; }
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
          if (run == 15) { k += 16; continue; }
          break;                                               // EOB
        }
        k += run;
        if (k > 63) { bad = true; break; }
        blk[kZigzagNat.at[k]] = (short)extend(r.take(s), s);
        ++k;
      }
      if (k > 64 || r.real < 0) bad = true;                     // ZRL past the block; bits taken from behind the data
    }
  }
  if (bad) a.status[slot] = -1;
}


// ---- index scan ------------------------------------------------------------------------------------------------------------------------
// The entropy-coded segment of a file, from the byte its one segment starts at to the end of the file, is cut into chunks of chunk_bytes
// raw file bytes; lane i of the workgroup owns chunk i (a file with more than kScanLanes chunks is handled in sweeps of kScanLanes).  A
// decoder state is (position of the next symbol as BitReader::where() names it, block-in-MCU j, zig-zag position k; k == 0: a DC
// symbol comes next), packed as (byte, bit | j << 3 | k << 8).  decode(chunk, state) decodes symbols from `state` while the next symbol
// starts in front of the chunk's end and returns the state it then stands in.
//
//   cold pass   exit[i] = decode(chunk i, guess): the guess of lane 0 is the true state (the segment's start; in a later sweep the settled
//               exit of the chunk before), the guess of every other lane its chunk's first byte - one further if that byte is the stuffed
//               0x00 of an 0xff 0x00 pair - bit 0, j = 0, k = 0.
//   rounds      exit[i] = decode(chunk i, exit[i - 1]) for all i >= 1 at once (every lane reads its neighbour's state of the round before),
//               until a round changes nothing or max_rounds is reached.  A lane whose input did not change since it last decoded does
//               not decode again: decode() is a function of its input.
//   Why the fixed point is the serial decode: in a round without change exit[i] == decode(chunk i, exit[i - 1]) holds for every i >= 1,
//   and exit[-1], lane 0's input, is the true state.  The serial decoder's state at the end of chunk 0 is decode(chunk 0, true) = exit[0];
//   if its state at the end of chunk i - 1 is exit[i - 1], its state at the end of chunk i is decode(chunk i, exit[i - 1]) = exit[i].  By
//   induction every exit[i] is the serial decoder's state.  That it is reached in few rounds is the self-synchronisation of Huffman
//   codes (Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018); that it was reached is checked, never assumed.
//   count pass  from its settled input every lane counts the blocks that start in its chunk and sums their DC differences per component;
//               an exclusive prefix sum over the workgroup, carried across sweeps, gives the block index and the three predictors
//               (modulo 2^16 in the end, as `entries` stores them) at every chunk start.
//   entry pass  one more walk; where a block with index % (blocks per MCU) == 0 and MCU % mcux == 0 starts, entries[row] is written from
//               BitReader::where(), the form the entropy kernel records.
//
// Rules for states no valid stream reaches (only determinism matters, a wrong guess is only ever a starting point):
//   - a symbol (code and extra bits) that takes bits from behind the data (the end of the file or a marker) is void, and so is an
//     invalid code with fewer than 16 bits of data left (zeros fed behind the data took part in calling it invalid): the walk ends in the
//     state in front of it.  The padding behind the last block, up to seven ones, ends the true walk this way: no code of a table built
//     by the standard's procedure is all ones, so the padding either starts a code that runs into the zeros or starts none;
//   - an invalid code, a DC category above 15, a run past coefficient 63: the reader goes back in front of the symbol, drops one bit, and
//     a DC symbol of the same block-in-MCU is expected (k = 0).
// scan_ok = the rounds of every sweep settled, no lane met the second rule from its settled input, every counted block's j agreed with
// its index, and the block total is mcux * mcuy * blocks per MCU.  Reads are bounded by the file's length (BitReader), the walk by the
// chunk's end (every step consumes at least one bit), the writes to `entries` by mcuy, the state writes by the chunk count of the file's
// length, which the host checked against the descriptor the workspace was sized for.
__device__ __forceinline__ bool same(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }

// MODE 0: states only.  1: acc += (blocks, DC differences per component).  2: acc runs as (block index, predictors), entries are written.
// -> the exit state; *err: the drop-one-bit rule was used (MODE 2: or a block's j disagrees with its index)
template <int MODE>
__device__ __forceinline__ uint2 scan_walk(const unsigned char* file, uint32_t bytes, const HuffLds* huff, const DecFile& f, int bpm, uint2 in,
                                           uint32_t chunk_end, int4& acc, bool& err, int* entries) {
  BitReader r;
  r.p = file;
  r.end = bytes;
  r.start(in.x, (int)(in.y & 7u));
  int j = (int)(in.y >> 3) & 7, k = (int)(in.y >> 8);
  for (;;) {
    const BitReader s = r;                                      // in front of the next symbol
    int byte = 0, bit = 0;
    bool stop = false;
    // where() lies at least the buffer's data bytes in front of pos: only then can it have reached the chunk's end (and is worth its walk)
    if (r.pos >= chunk_end + (uint32_t)(r.real > 0 ? (r.real + 7) >> 3 : 0)) {
      s.where(&byte, &bit);
      stop = (uint32_t)byte >= chunk_end;
    }
    bool bad = false;
    int c = 0, diff = 0;
    if (!stop) {
      if (k == 0) {
        c = block_component(bpm, j);
        const int sy = huff_symbol(r, huff[f.td[c]]);
        if (sy < 0 || sy > 15) bad = true;
        else diff = extend(r.take(sy), sy);
        c = sy < 0 ? -1 : c;
      } else {
        const int rs = huff_symbol(r, huff[2 + f.ta[block_component(bpm, j)]]);
        if (rs < 0) bad = true;
        else if (rs & 15) r.take(rs & 15);
        c = rs;
      }
      if (r.real < 0 || (c < 0 && r.real < 16)) {               // void: bits from behind the data
        stop = true;
        s.where(&byte, &bit);
      }
    }
    if (stop) return make_uint2((uint32_t)byte, (uint32_t)(bit | (j << 3) | (k << 8)));
    if (!bad) {
      if (k == 0) {
        if (MODE == 1) {
          acc.x += 1;
          if (c == 0) acc.y += diff; else if (c == 1) acc.z += diff; else acc.w += diff;
        }
        if (MODE == 2) {
          const int mcu = acc.x / bpm;
          if (acc.x - mcu * bpm != j) err = true;
          else if (j == 0 && mcu % (int)f.mcux == 0 && mcu / (int)f.mcux < (int)f.mcuy) {
            int4 e;
            s.where(&e.x, &e.y);
            e.z = (int)(((uint32_t)acc.y & 0xffffu) | ((uint32_t)acc.z << 16));
            e.w = (int)((uint32_t)acc.w & 0xffffu);
            *reinterpret_cast<int4*>(entries + 4 * (mcu / (int)f.mcux)) = e;
          }
          acc.x += 1;
          if (c == 0) acc.y += diff; else if (c == 1) acc.z += diff; else acc.w += diff;
        }
        k = 1;
      } else {
        const int run = c >> 4;
        if ((c & 15) == 0) {
          if (run == 15) { k += 16; bad = k > 64; }
          else k = 64;                                          // EOB
        } else {
          k += run;
          if (k > 63) bad = true; else ++k;
        }
      }
    }
    if (bad) {
      err = true;
      r = s;
      r.refill();
      r.skip(1);
      k = 0;
    } else if (k >= 64) {
      k = 0;
      j = j + 1 == bpm ? 0 : j + 1;
    }
  }
}

__global__ __launch_bounds__(kScanLanes) void jpegdec_scan_kernel(const DecArgs a) {
  __shared__ HuffLds huff[4];
  __shared__ int4 pre[kScanLanes];
  __shared__ int4 carry;                                        // block index and predictors at the sweep's first chunk
  __shared__ int changed, failed;
  const DecFile& f = a.f[blockIdx.x];
  if (!f.scan) return;
  const int lane = threadIdx.x, slot = a.first + blockIdx.x;
  const unsigned char* meta = a.blob + f.meta;
  const unsigned char* file = a.blob + f.file;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(meta + kHuffAt);
    uint32_t* dst = reinterpret_cast<uint32_t*>(huff);
    for (int i = lane; i < 4 * kHuffBytes / 4; i += kScanLanes) dst[i] = src[i];
  }
  const int* sg = reinterpret_cast<const int*>(meta + kSegAt);
  const int bpm = blocks_per_mcu(f.sampling);
  const int total = (int)f.mcux * f.mcuy;
  const uint32_t start = (uint32_t)sg[0];
  // the one segment must be the whole scan from MCU 0, and start inside the file behind its first byte (the cold start looks one back)
  bool ok = sg[4] == 0 && sg[5] >= total && sg[0] >= 1 && start < f.bytes && (uint32_t)sg[1] < 8u;
  const uint32_t shift = 31 - __clz(a.chunk_bytes);
  const int nchunks = ok ? (int)((f.bytes - start + (uint32_t)a.chunk_bytes - 1) >> shift) : 0;
  if (nchunks > a.chunks_cap) ok = false;
  if (lane == 0) {
    carry = make_int4(0, (int)(short)(sg[2] & 0xffff), (int)(short)((uint32_t)sg[2] >> 16), (int)(short)(sg[3] & 0xffff));
    changed = 0;
    failed = 0;
  }
  __syncthreads();
  uint2* state = a.scan_state + (size_t)blockIdx.x * a.chunks_cap;
  int* entries = a.entries + (size_t)slot * a.rows_cap * 4;
  int rounds_max = 0;
  for (int base = 0; ok && base < nchunks; base += kScanLanes) {
    const int chunk = base + lane;
    const bool active = chunk < nchunks;
    const uint32_t first = start + ((uint32_t)chunk << shift);
    const uint32_t chunk_end = active && first + (uint32_t)a.chunk_bytes < f.bytes ? first + (uint32_t)a.chunk_bytes : f.bytes;
    uint2 in = make_uint2(0, 0), mine = make_uint2(0, 0);
    if (active) {
      if (lane == 0) in = base == 0 ? make_uint2(start, (uint32_t)sg[1]) : state[chunk - 1];
      else in = make_uint2(first + (file[first] == 0 && file[first - 1] == 0xff ? 1u : 0u), 0u);
    }
    int4 acc = make_int4(0, 0, 0, 0);
    bool err = false, redo = active;
    int round = 0;
    for (;; ++round) {                                          // round 0 is the cold pass
      if (redo) {
        bool e = false;
        const uint2 out = scan_walk<0>(file, f.bytes, huff, f, bpm, in, chunk_end, acc, e, entries);
        if (round == 0 || !same(out, mine)) {
          state[chunk] = out;
          mine = out;
          if (round) changed = 1;
        }
      }
      __syncthreads();
      const bool ch = changed != 0;
      if (round > 0 && (!ch || round >= a.max_rounds)) {
        if (ch) ok = false;                                     // max_rounds rounds and the last still changed a state
        break;
      }
      __syncthreads();
      if (lane == 0) changed = 0;
      redo = false;
      if (active && lane > 0) {
        const uint2 n = state[chunk - 1];
        redo = !same(n, in);
        in = n;
      }
      __syncthreads();
    }
    if (round > rounds_max) rounds_max = round;
    if (!ok) break;
    // every lane's `in` is now the serial decoder's state at its chunk's start
    if (active) scan_walk<1>(file, f.bytes, huff, f, bpm, in, chunk_end, acc, err, entries);
    pre[lane] = acc;
    __syncthreads();
    for (int d = 1; d < kScanLanes; d <<= 1) {
      int4 v = make_int4(0, 0, 0, 0);
      if (lane >= d) v = pre[lane - d];
      __syncthreads();
      int4 w = pre[lane];
      w.x += v.x; w.y += v.y; w.z += v.z; w.w += v.w;
      pre[lane] = w;
      __syncthreads();
    }
    const int4 incl = pre[lane], c0 = carry;
    int4 at = make_int4(c0.x + incl.x - acc.x, c0.y + incl.y - acc.y, c0.z + incl.z - acc.z, c0.w + incl.w - acc.w);
    __syncthreads();
    if (lane == kScanLanes - 1) carry = make_int4(c0.x + incl.x, c0.y + incl.y, c0.z + incl.z, c0.w + incl.w);
    if (active) scan_walk<2>(file, f.bytes, huff, f, bpm, in, chunk_end, at, err, entries);
    if (err) failed = 1;
    __syncthreads();                                            // carry, failed and this sweep's states are in place
  }
  if (lane == 0) {
    a.scan_ok[slot] = ok && !failed && carry.x == total * bpm ? 1 : 0;
    a.scan_rounds[slot] = rounds_max;
  }
}

// ---- pixels ------------------------------------------------------------------------------------------------------------------------------
// libjpeg's jidctint.c pass over v[0], v[S], .. v[7 S]; uint32 arithmetic wraps like the restatement's int32
template <int S, int SHIFT>
__device__ __forceinline__ void idct8(int* v) {
  typedef uint32_t u;
  const u i0 = v[0], i1 = v[S], i2 = v[2 * S], i3 = v[3 * S], i4 = v[4 * S], i5 = v[5 * S], i6 = v[6 * S], i7 = v[7 * S];
  u z1 = (i2 + i6) * 4433u;
  u tmp2 = z1 + i6 * (u)(-15137);
  u tmp3 = z1 + i2 * 6270u;
  u tmp0 = (i0 + i4) << 13, tmp1 = (i0 - i4) << 13;
  const u t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  tmp0 = i7; tmp1 = i5; tmp2 = i3; tmp3 = i1;
  z1 = tmp0 + tmp3;
  u z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const u z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
  z1 *= (u)(-7373); z2 *= (u)(-20995);
  z3 = z3 * (u)(-16069) + z5; z4 = z4 * (u)(-3196) + z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const u r = 1u << (SHIFT - 1);
  v[0] = (int)(t10 + tmp3 + r) >> SHIFT;     v[7 * S] = (int)(t10 - tmp3 + r) >> SHIFT;
  v[S] = (int)(t11 + tmp2 + r) >> SHIFT;     v[6 * S] = (int)(t11 - tmp2 + r) >> SHIFT;
  v[2 * S] = (int)(t12 + tmp1 + r) >> SHIFT; v[5 * S] = (int)(t12 - tmp1 + r) >> SHIFT;
  v[3 * S] = (int)(t13 + tmp0 + r) >> SHIFT; v[4 * S] = (int)(t13 - tmp0 + r) >> SHIFT;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpegdec_planes_kernel(const DecArgs a) {
  const DecFile& f = a.f[blockIdx.y];
  const int bpm = blocks_per_mcu(f.sampling);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= (int)f.mcux * f.mcuy * bpm) return;
  const int slot = a.first + blockIdx.y;
  const int mcu = b / bpm, j = b - mcu * bpm;
  const int my = mcu / (int)f.mcux, mx = mcu - my * (int)f.mcux;
  int c, by, bx;
  if (bpm == 6 && j < 4) { c = 0; by = 2 * my + (j >> 1); bx = 2 * mx + (j & 1); }
  else if (bpm == 4 && j < 2) { c = 0; by = my; bx = 2 * mx + j; }          // 4:2:2: two luma blocks side by side
  else { c = block_component(bpm, j); by = my; bx = mx; }
  const uint4* src = reinterpret_cast<const uint4*>(a.coef + ((size_t)slot * a.blocks_cap + b) * 64);
  const uint4* q4 = reinterpret_cast<const uint4*>(a.blob + f.meta + kQuantAt + 128 * f.tq[c]);
  int v[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 w = src[i], q = q4[i];
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w}, qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[8 * i + 2 * e] = (int)(short)(ww[e] & 0xffffu) * (int)(qq[e] & 0xffffu);
      v[8 * i + 2 * e + 1] = (int)(short)(ww[e] >> 16) * (int)(qq[e] >> 16);
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) idct8<8, 11>(v + x);
#pragma unroll
  for (int y = 0; y < 8; ++y) idct8<1, 18>(v + 8 * y);
  // 8 by < Hp, 8 bx < Wp by the padded sizes of the descriptor (multiples of 16, at least the file's H and W).  4:2:2: bx <= 2 mcux - 1
  // and 16 mcux = 16 ceil(W / 16) <= Wp; by <= mcuy - 1 and 8 mcuy = 8 ceil(H / 8) <= Hp.  Its chroma fills the left half of its plane
  unsigned char* plane = a.planes + ((size_t)slot * 3 + c) * a.Hp * a.Wp;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (uint32_t)clamp255(v[8 * y + x] + 128) << (8 * x);
      hi |= (uint32_t)clamp255(v[8 * y + 4 + x] + 128) << (8 * x);
    }
    *reinterpret_cast<uint2*>(plane + (size_t)(8 * by + y) * a.Wp + 8 * bx) = make_uint2(lo, hi);
  }
}

__global__ __launch_bounds__(256) void jpegdec_rgb_kernel(const DecArgs a) {
  const DecFile& f = a.f[blockIdx.y];
  const int W = f.W, H = f.H, groups = (W + 3) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= groups * H) return;
  const int slot = a.first + blockIdx.y;
  const int y = t / groups, x0 = 4 * (t - y * groups);
  const unsigned char* Y = a.planes + (size_t)slot * 3 * a.Hp * a.Wp;
  const unsigned char* Cb = Y + (size_t)a.Hp * a.Wp;
  const unsigned char* Cr = Cb + (size_t)a.Hp * a.Wp;
  int cb[4], cr[4];
  if (f.sampling == 2) {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int r = y >> 1;
    int rn = (y & 1) ? r + 1 : r - 1;
    rn = rn < 0 ? 0 : (rn > ch - 1 ? ch - 1 : rn);
    const int c0 = x0 >> 1;
    int sb[4], sr[4];                          // column sums 3 * near row + far row at columns c0 - 1 .. c0 + 2, clamped to the component
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int c = c0 - 1 + i;
      c = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c);
      sb[i] = 3 * Cb[(size_t)r * a.Wp + c] + Cb[(size_t)rn * a.Wp + c];
      sr[i] = 3 * Cr[(size_t)r * a.Wp + c] + Cr[(size_t)rn * a.Wp + c];
    }
    // (3 this + this + 8) >> 4 at a replicated edge is libjpeg's (4 this + 8) >> 4
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      cb[2 * i] = (3 * sb[1 + i] + sb[i] + 8) >> 4;     cb[2 * i + 1] = (3 * sb[1 + i] + sb[2 + i] + 7) >> 4;
      cr[2 * i] = (3 * sr[1 + i] + sr[i] + 8) >> 4;     cr[2 * i + 1] = (3 * sr[1 + i] + sr[2 + i] + 7) >> 4;
    }
  } else if (f.sampling == 3) {
    // libjpeg's h2v1 triangle filter along the row, none down the column: chroma row y, columns c0 - 1 .. c0 + 2 clamped to the
    // component's own cw = ceil(W / 2) samples (cw <= 8 mcux <= Wp / 2: every read lies in the plane's left half)
    const int cw = (W + 1) >> 1, c0 = x0 >> 1;
    int sb[4], sr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int c = c0 - 1 + i;
      c = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c);
      sb[i] = Cb[(size_t)y * a.Wp + c];
      sr[i] = Cr[(size_t)y * a.Wp + c];
    }
    // (3 this + this + 1) >> 2 and (3 this + this + 2) >> 2 at a replicated edge are libjpeg's unfiltered first and last samples
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      cb[2 * i] = (3 * sb[1 + i] + sb[i] + 1) >> 2;     cb[2 * i + 1] = (3 * sb[1 + i] + sb[2 + i] + 2) >> 2;
      cr[2 * i] = (3 * sr[1 + i] + sr[i] + 1) >> 2;     cr[2 * i + 1] = (3 * sr[1 + i] + sr[2 + i] + 2) >> 2;
    }
  } else {
    const uint32_t wb = *reinterpret_cast<const uint32_t*>(Cb + (size_t)y * a.Wp + x0);
    const uint32_t wr = *reinterpret_cast<const uint32_t*>(Cr + (size_t)y * a.Wp + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { cb[i] = (wb >> (8 * i)) & 255; cr[i] = (wr >> (8 * i)) & 255; }
  }
  const uint32_t wy = *reinterpret_cast<const uint32_t*>(Y + (size_t)y * a.Wp + x0);      // x0 + 3 < Wp: Wp is a multiple of 8
  unsigned char px[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int l = (wy >> (8 * i)) & 255, u = cb[i] - 128, v = cr[i] - 128;
    const int R = clamp255(l + ((91881 * v + 32768) >> 16));
    const int G = clamp255(l + ((-22554 * u - 46802 * v + 32768) >> 16));
    const int B = clamp255(l + ((116130 * u + 32768) >> 16));
    px[3 * i] = (unsigned char)(a.bgr ? B : R);
    px[3 * i + 1] = (unsigned char)G;
    px[3 * i + 2] = (unsigned char)(a.bgr ? R : B);
  }
  unsigned char* dst = a.out + (size_t)slot * a.frame_stride + (size_t)y * a.row_pitch + (size_t)x0 * 3;
  if (x0 + 4 <= W && ((uintptr_t)dst & 3) == 0) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      d[i] = (uint32_t)px[4 * i] | ((uint32_t)px[4 * i + 1] << 8) | ((uint32_t)px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
  } else {
    const int n = 3 * (W - x0 < 4 ? W - x0 : 4);
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < n) dst[i] = px[i];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
}  // namespace vp

struct vp_jpegdec {
  vp_jpegdec_desc d;
  int Hp, Wp, blocks_cap, rows_cap;
  short* coef;
  int* entries;
  unsigned char* planes;
  // the index scan: scan_state null until vp_jpegdec_enable_scan
  int chunk_bytes, max_rounds, chunks_cap, scan_slots;      // chunks of the largest file; files of one launch group
  uint2* scan_state;
  int *scan_ok, *scan_rounds;
};

using namespace vp;

static int dec_check(const vp_jpegdec_desc* d, vp_jpegdec* h) {
  if (const int rc = check_desc(d, "vp_jpegdec")) return rc;
  if (d->max_files < 1 || d->max_files > VP_JPEGDEC_MAX_FILES) { set_err("vp_jpegdec: bad descriptor (max_files %d, 1 .. %d)", d->max_files, VP_JPEGDEC_MAX_FILES); return VP_ERR_ARG; }
  if (d->max_height < 1 || d->max_height > 8192) { set_err("vp_jpegdec: bad descriptor (max_height %d, 1 .. 8192)", d->max_height); return VP_ERR_ARG; }
  if (d->max_width < 1 || d->max_width > 8192) { set_err("vp_jpegdec: bad descriptor (max_width %d, 1 .. 8192)", d->max_width); return VP_ERR_ARG; }
  if (d->max_file_bytes < 1 || d->max_file_bytes > (1 << 30)) { set_err("vp_jpegdec: bad descriptor (max_file_bytes %d, 1 .. 2^30)", d->max_file_bytes); return VP_ERR_ARG; }
  if (d->max_segments_per_file < 1 || d->max_segments_per_file > (1 << 20)) {
    set_err("vp_jpegdec: bad descriptor (max_segments_per_file %d, 1 .. 2^20)", d->max_segments_per_file);
    return VP_ERR_ARG;
  }
  if (d->bgr != 0 && d->bgr != 1) { set_err("vp_jpegdec: bad descriptor (bgr %d, 0 or 1)", d->bgr); return VP_ERR_ARG; }
  h->d = *d;
  h->Hp = (d->max_height + 15) & ~15;
  h->Wp = (d->max_width + 15) & ~15;
  h->blocks_cap = 3 * (h->Hp / 8) * (h->Wp / 8);         // 4:4:4; 4:2:0 needs half of it, 4:2:2 two thirds
  h->rows_cap = h->Hp / 8;
  return VP_OK;
}

static size_t dec_carve(vp_jpegdec* h, void* base) {
  Arena ar(base);
  const size_t files = h->d.max_files;
  h->coef = ar.take<short>(files * h->blocks_cap * 64);
  h->entries = ar.take<int>(files * h->rows_cap * 4);
  h->planes = ar.take<unsigned char>(files * 3 * h->Hp * h->Wp);
  return align256(ar.total());
}

static int scan_check(const vp_jpegdec_desc* d, int chunk_bytes, vp_jpegdec* h) {
  if (const int rc = dec_check(d, h)) return rc;
  if (chunk_bytes < 32 || chunk_bytes > 4096 || (chunk_bytes & (chunk_bytes - 1))) {
    set_err("vp_jpegdec: bad scan chunk_bytes %d (a power of two, 32 .. 4096)", chunk_bytes);
    return VP_ERR_ARG;
  }
  h->chunk_bytes = chunk_bytes;
  h->chunks_cap = (d->max_file_bytes + chunk_bytes - 1) / chunk_bytes;
  h->scan_slots = d->max_files < VP_JPEGDEC_FILES_PER_LAUNCH ? d->max_files : VP_JPEGDEC_FILES_PER_LAUNCH;
  return VP_OK;
}

static size_t scan_carve(vp_jpegdec* h, void* base) {
  Arena ar(base);
  h->scan_state = ar.take<uint2>((size_t)h->scan_slots * h->chunks_cap);     // launch groups run one after another on the stream
  h->scan_ok = ar.take<int>(h->d.max_files);
  h->scan_rounds = ar.take<int>(h->d.max_files);
  return align256(ar.total());
}

extern "C" {

size_t vp_jpegdec_desc_size(void) { return sizeof(vp_jpegdec_desc); }

size_t vp_jpegdec_workspace_bytes(const vp_jpegdec_desc* d) {
  vp_jpegdec h;
  return dec_check(d, &h) ? 0 : dec_carve(&h, nullptr);
}

int vp_jpegdec_create(const vp_jpegdec_desc* d, void* workspace, size_t bytes, vp_jpegdec_t** out) {
  return open_handle("vp_jpegdec_create", d, dec_check, dec_carve, workspace, bytes, out);
}

size_t vp_jpegdec_scan_workspace_bytes(const vp_jpegdec_desc* d, int chunk_bytes) {
  vp_jpegdec h;
  return scan_check(d, chunk_bytes, &h) ? 0 : scan_carve(&h, nullptr);
}

int vp_jpegdec_enable_scan(vp_jpegdec_t* h, void* scan_workspace, size_t bytes, int chunk_bytes, int max_rounds) {
  if (!h) { set_err("vp_jpegdec_enable_scan: bad argument"); return VP_ERR_ARG; }
  vp_jpegdec s = *h;                                        // (a refusal leaves the handle as it was)
  if (const int rc = scan_check(&h->d, chunk_bytes, &s)) return rc;
  if (max_rounds < 1 || max_rounds > 1024) { set_err("vp_jpegdec_enable_scan: bad max_rounds %d (1 .. 1024)", max_rounds); return VP_ERR_ARG; }
  const size_t need = scan_carve(&s, nullptr);
  if (!scan_workspace || bytes < need) { set_err("vp_jpegdec_enable_scan: workspace too small (%zu of %zu bytes)", bytes, need); return VP_ERR_WORKSPACE; }
  scan_carve(&s, scan_workspace);
  s.max_rounds = max_rounds;
  *h = s;
  return VP_OK;
}

void vp_jpegdec_destroy(vp_jpegdec_t* h) { delete h; }

int vp_jpegdec_decode(vp_jpegdec_t* h, const unsigned char* blob, const vp_jpegdec_file* files, int n, unsigned char* out, size_t row_pitch,
                      size_t frame_stride, int* status, void* stream) {
  if (!h || !blob || !files || !out || !status || n < 1 || n > h->d.max_files) {
    set_err("vp_jpegdec_decode: bad argument (1 .. max_files files, device blob, output and status, host file table)");
    return VP_ERR_ARG;
  }
  if ((uintptr_t)blob & 15) { set_err("vp_jpegdec_decode: the blob must start on a 16-byte boundary"); return VP_ERR_ARG; }
  const vp_jpegdec_desc& d = h->d;
  for (int i = 0; i < n; ++i) {
    const vp_jpegdec_file& f = files[i];
    const char* what = nullptr;
    if (f.n_segments == 0) continue;              // a gap: nothing is read or written for this position
    if (f.width < 1 || f.width > d.max_width || f.height < 1 || f.height > d.max_height) what = "width / height outside 1 .. the descriptor's maxima";
    else if (f.sampling != 1 && f.sampling != 2 && f.sampling != 3) what = "sampling (1: 4:4:4, 2: 4:2:0, 3: 4:2:2)";
    else if (f.file_bytes < 1 || f.file_bytes > d.max_file_bytes) what = "file_bytes outside 1 .. max_file_bytes";
    else if (f.n_segments < 1 || f.n_segments > d.max_segments_per_file) what = "n_segments outside 1 .. max_segments_per_file";
    else if (f.restart_interval < 0) what = "restart_interval";
    else if (f.meta_offset & 15) what = "meta_offset is not a multiple of 16";
    else if (f.meta_offset >> 32 || f.file_offset >> 32 || (f.file_offset + (uint64_t)f.file_bytes) >> 32) what = "offsets past 4 GiB";
    else if ((size_t)f.width * 3 > row_pitch || (size_t)(f.height - 1) * row_pitch + (size_t)f.width * 3 > frame_stride) what = "the image does not fit row_pitch / frame_stride";
    for (int c = 0; c < 3 && !what; ++c)
      if (f.tq[c] > 3 || f.td[c] > 1 || f.ta[c] > 1) what = "table selector (tq 0 .. 3, td / ta 0 .. 1)";
    if (what) { set_err("vp_jpegdec_decode: file %d: %s", i, what); return VP_ERR_ARG; }
  }
  hipStream_t st = (hipStream_t)stream;
  VP_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)n * sizeof(int), st));
  if (h->scan_state) {                             // 0 for every file the scan does not run on
    VP_HIP_CHECK(hipMemsetAsync(h->scan_ok, 0, (size_t)n * sizeof(int), st));
    VP_HIP_CHECK(hipMemsetAsync(h->scan_rounds, 0, (size_t)n * sizeof(int), st));
  }
  for (int i0 = 0; i0 < n; i0 += VP_JPEGDEC_FILES_PER_LAUNCH) {
    const int m = n - i0 < VP_JPEGDEC_FILES_PER_LAUNCH ? n - i0 : VP_JPEGDEC_FILES_PER_LAUNCH;
    DecArgs a;
    memset(&a, 0, sizeof(a));
    a.blob = blob;
    a.coef = h->coef;
    a.entries = h->entries;
    a.planes = h->planes;
    a.out = out; a.status = status; a.row_pitch = row_pitch; a.frame_stride = frame_stride;
    a.first = i0; a.blocks_cap = h->blocks_cap; a.rows_cap = h->rows_cap; a.Hp = h->Hp; a.Wp = h->Wp; a.bgr = d.bgr;
    if (h->scan_state) {
      a.scan_state = h->scan_state;
      a.scan_ok = h->scan_ok;
      a.scan_rounds = h->scan_rounds;
      a.chunk_bytes = h->chunk_bytes; a.chunks_cap = h->chunks_cap; a.max_rounds = h->max_rounds;
    }
    int max_seg = 1, max_blocks = 1, max_groups = 1, scans = 0;
    for (int i = 0; i < m; ++i) {
      const vp_jpegdec_file& f = files[i0 + i];
      DecFile& g = a.f[i];
      if (f.n_segments == 0) continue;            // all zero: every kernel's bound check ends its workgroups
      const int sx = f.sampling == 1 ? 8 : 16, sy = f.sampling == 2 ? 16 : 8;      // the MCU in pixels; 4:2:2 is 16 wide, 8 high
      g.meta = (uint32_t)f.meta_offset; g.file = (uint32_t)f.file_offset; g.bytes = (uint32_t)f.file_bytes;
      g.nseg = (uint32_t)f.n_segments; g.dri = (uint32_t)f.restart_interval;
      g.W = (uint16_t)f.width; g.H = (uint16_t)f.height;
      g.mcux = (uint16_t)((f.width + sx - 1) / sx); g.mcuy = (uint16_t)((f.height + sy - 1) / sy);
      g.sampling = (uint8_t)f.sampling;
      for (int c = 0; c < 3; ++c) { g.tq[c] = f.tq[c]; g.td[c] = f.td[c]; g.ta[c] = f.ta[c]; }
      const int blocks = (int)g.mcux * g.mcuy * blocks_per_mcu(f.sampling);
      const int groups = ((f.width + 3) / 4) * f.height;
      if (h->scan_state && f.n_segments == 1 && f.restart_interval == 0 && g.mcuy >= 2) {      // whether its segment is the whole scan: the kernel
        g.scan = 1;
        ++scans;
        if (g.mcuy > max_seg) max_seg = g.mcuy;
      }
      if (f.n_segments > max_seg) max_seg = f.n_segments;
      if (blocks > max_blocks) max_blocks = blocks;
      if (groups > max_groups) max_groups = groups;
    }
    if (scans) {
      hipLaunchKernelGGL(jpegdec_scan_kernel, dim3(m), dim3(kScanLanes), 0, st, a);
      VP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((max_seg + kLanes - 1) / kLanes, m), dim3(kLanes), 0, st, a);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_planes_kernel, dim3((max_blocks + 255) / 256, m), dim3(256), 0, st, a);
    VP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_rgb_kernel, dim3((max_groups + 255) / 256, m), dim3(256), 0, st, a);
    VP_HIP_CHECK(hipGetLastError());
  }
  return VP_OK;
}

int vp_jpegdec_tensor(vp_jpegdec_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_jpegdec_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string s(name);
  int64_t shp[4] = {h->d.max_files, 0, 0, 1};
  if (s == "coefficients") { *ptr = h->coef; shp[1] = h->blocks_cap; shp[2] = 64; }
  else if (s == "entries") { *ptr = h->entries; shp[1] = h->rows_cap; shp[2] = 4; }
  else if (s == "planes") { *ptr = h->planes; shp[1] = 3; shp[2] = h->Hp; shp[3] = h->Wp; }
  else if (s == "scan_ok" || s == "scan_rounds") {
    if (!h->scan_state) { set_err("vp_jpegdec_tensor: '%s' needs vp_jpegdec_enable_scan", name); return VP_ERR_ARG; }
    *ptr = s == "scan_ok" ? h->scan_ok : h->scan_rounds; shp[1] = 1; shp[2] = 1;
  }
  else { set_err("vp_jpegdec_tensor: no tensor '%s' (coefficients, entries, planes, scan_ok, scan_rounds)", name); return VP_ERR_ARG; }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = shp[i];
  return VP_OK;
}

}  // extern "C"

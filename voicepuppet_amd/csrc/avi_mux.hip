// AVI (Motion-JPEG + 16-bit PCM) segments built on the device: include/vp_hip.h vp_avimux_*.
//
// A call lays the JPEG rows of vp_jpeg_encode and the float32 samples of a push out as RIFF chunks, slot by slot: per slot one `01wb`
// chunk (when it has samples) and one `00dc` chunk per frame, in row order.  The blob starts with a table (per-slot offset, byte count,
// chunk count, status; one AVIOLDINDEX entry per chunk) that the host reads; the chunk bytes behind it are written to a file as they are.
//
//   avi_layout_kernel  one workgroup: rows -> slots (frame_slot is non-decreasing: a lower bound per slot), the chunk sizes in segment
//                      order, an exclusive scan over them, the table, and a chunk list for the second kernel in the workspace
//   avi_gather_kernel  one workgroup per chunk and slice of 16 KB (a workgroup walks its chunk's slices with the grid's y stride): 16-byte
//                      copies where source and destination agree modulo 16, 4- or 2-byte copies where they agree modulo 4 or 2, bytes
//                      at the ragged ends and otherwise; the samples converted to int16 in the same launch
//
// No atomics, no grid-wide barrier: the gather launch follows the layout launch on the stream.  Every read of a row ends at
// min(lengths[r], row_bytes), every read of the samples inside [0, samples), every write inside [0, out_capacity).
#include <stdint.h>
#include <string.h>

#include "workspace.h"

namespace vp {

constexpr int kAviLanes = 256;
constexpr uint32_t kAviSlice = 16384;      // payload bytes one workgroup copies at a time
constexpr int kAviMaxSlices = 16;          // grid y: a longer chunk is walked with this stride
constexpr int kAviMaxChunks = VP_AVIMUX_MAX_FRAMES + VP_AVIMUX_MAX_SLOTS;
constexpr uint32_t kFcc00dc = 0x63643030u, kFcc01wb = 0x62773130u;       // little-endian fourccs
constexpr uint32_t kAviKeyframe = 0x10u;   // AVIIF_KEYFRAME: every MJPEG frame and every PCM chunk

enum { kAviSkip = 0, kAviFrame = 1, kAviAudio = 2 };

struct AviChunk {
  uint32_t dst;        // chunk header, bytes from the start of the blob
  uint32_t payload;    // bytes after the 8-byte header, without the pad
  int32_t src;         // row of `data` (frame) or first sample of `pcm` (audio)
  uint32_t kind;       // kAviSkip: nothing is written (the slot's status is not 0)
};

struct AviArgs {
  const unsigned char* data;
  size_t row_bytes;
  const int* lengths;
  const int* frame_slot;
  const float* pcm;
  const int* s_off;
  const int* s_cnt;
  unsigned char* out;
  AviChunk* chunks;
  uint32_t* nchunks;
  uint32_t cap, table_bytes;
  int K, samples, slots;
};

// the slot whose row range [lb[s], lb[s + 1]) holds row r, or -1 (lb is non-decreasing)
__device__ inline int avi_slot_of(const int* lb, int S, int r) {
  int lo = 0, hi = S + 1;                  // first j with lb[j] > r
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (lb[m] > r) hi = m; else lo = m + 1;
  }
  return (lo >= 1 && lo <= S) ? lo - 1 : -1;
}

__global__ __launch_bounds__(kAviLanes) void avi_layout_kernel(AviArgs a) {
  __shared__ int lb[VP_AVIMUX_MAX_SLOTS + 1];
  __shared__ int cnt[VP_AVIMUX_MAX_SLOTS], soff[VP_AVIMUX_MAX_SLOTS], status[VP_AVIMUX_MAX_SLOTS];
  __shared__ int cbase[VP_AVIMUX_MAX_SLOTS + 1];
  __shared__ uint32_t segoff[VP_AVIMUX_MAX_SLOTS];
  __shared__ uint32_t off[kAviMaxChunks];            // chunk sizes, then their exclusive scan
  __shared__ uint32_t part[kAviLanes];
  const int t = threadIdx.x, S = a.slots, K = a.K;
  uint32_t* table = (uint32_t*)a.out;

  for (int s = t; s <= S; s += kAviLanes) {          // rows of slots < s
    int lo = 0, hi = K;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (a.frame_slot[m] < s) lo = m + 1; else hi = m;
    }
    lb[s] = lo;
    if (s < S) status[s] = 0;
  }
  __syncthreads();
  if (t == 0) {
    // an unsorted frame_slot may not overlap two slots' rows; the samples of all slots together stay inside what the host passed
    int rem = a.samples;
    for (int s = 0; s < S; ++s) {
      if (lb[s + 1] < lb[s]) lb[s + 1] = lb[s];
      int c = a.samples > 0 ? a.s_cnt[s] : 0;
      c = min(max(c, 0), rem);
      int o = a.samples > 0 ? a.s_off[s] : 0;
      o = min(max(o, 0), a.samples - c);
      cnt[s] = c;
      soff[s] = o;
      rem -= c;
    }
  }
  __syncthreads();
  for (int r = t; r < K; r += kAviLanes) {
    if (a.lengths[r] < 0) {
      const int s = avi_slot_of(lb, S, r);
      if (s >= 0) status[s] = 1;                     // every writer stores the same value
    }
  }
  __syncthreads();
  if (t == 0) {
    int c = 0;
    for (int s = 0; s < S; ++s) {
      cbase[s] = c;
      if (status[s] == 0) c += (lb[s + 1] - lb[s]) + (cnt[s] > 0 ? 1 : 0);
    }
    cbase[S] = c;
  }
  __syncthreads();
  const int n = cbase[S];
  for (int r = t; r < K; r += kAviLanes) {
    const int s = avi_slot_of(lb, S, r);
    if (s < 0 || status[s]) continue;
    const uint32_t L = (uint32_t)min((size_t)a.lengths[r], a.row_bytes);
    off[cbase[s] + (cnt[s] > 0 ? 1 : 0) + (r - lb[s])] = 8u + L + (L & 1u);
  }
  for (int s = t; s < S; s += kAviLanes)
    if (status[s] == 0 && cnt[s] > 0) off[cbase[s]] = 8u + 2u * (uint32_t)cnt[s];
  __syncthreads();

  // exclusive scan of the n sizes: a run per lane, a scan over the lanes' sums, the run again
  const int per = (n + kAviLanes - 1) / kAviLanes;
  const int b = min(t * per, n), e = min(b + per, n);
  uint32_t sum = 0;
  for (int i = b; i < e; ++i) sum += off[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kAviLanes; d <<= 1) {
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = t ? part[t - 1] : 0u;
  for (int i = b; i < e; ++i) {
    const uint32_t v = off[i];
    off[i] = run;
    run += v;
  }
  const uint32_t total = part[kAviLanes - 1];
  __syncthreads();

  const uint32_t room = a.cap - a.table_bytes;       // the host refused cap < table_bytes
  for (int s = t; s < S; s += kAviLanes) {
    const int first = cbase[s], nch = cbase[s + 1] - first;
    const uint32_t begin = first < n ? off[first] : total;
    const uint32_t end = cbase[s + 1] < n ? off[cbase[s + 1]] : total;
    if (nch > 0 && end > room) status[s] = 2;
    segoff[s] = begin;
    table[4 + 4 * s + 0] = a.table_bytes + begin;
    table[4 + 4 * s + 1] = end - begin;
    table[4 + 4 * s + 2] = (uint32_t)nch;
    table[4 + 4 * s + 3] = (uint32_t)status[s];
  }
  __syncthreads();
  if (t == 0) {
    uint32_t used = 0, worst = 0;
    for (int s = 0; s < S; ++s) {
      worst = max(worst, (uint32_t)status[s]);
      if (status[s] == 0 && cbase[s + 1] > cbase[s]) used = cbase[s + 1] < n ? off[cbase[s + 1]] : total;
    }
    table[0] = a.table_bytes;
    table[1] = a.table_bytes + used;                 // the blob's used prefix
    table[2] = (uint32_t)n;
    table[3] = worst;
    *a.nchunks = (uint32_t)n;
  }
  uint32_t* entries = table + 4 + 4 * S;
  for (int r = t; r < K; r += kAviLanes) {
    const int s = avi_slot_of(lb, S, r);
    if (s < 0 || status[s] == 1) continue;
    const int p = cbase[s] + (cnt[s] > 0 ? 1 : 0) + (r - lb[s]);
    const uint32_t L = (uint32_t)min((size_t)a.lengths[r], a.row_bytes);
    entries[4 * p + 0] = kFcc00dc;
    entries[4 * p + 1] = kAviKeyframe;
    entries[4 * p + 2] = off[p] - segoff[s];
    entries[4 * p + 3] = L;
    a.chunks[p] = AviChunk{a.table_bytes + off[p], L, r, status[s] == 0 ? (uint32_t)kAviFrame : (uint32_t)kAviSkip};
  }
  for (int s = t; s < S; s += kAviLanes) {
    if (status[s] == 1 || cnt[s] <= 0) continue;
    const int p = cbase[s];
    entries[4 * p + 0] = kFcc01wb;
    entries[4 * p + 1] = kAviKeyframe;
    entries[4 * p + 2] = 0u;
    entries[4 * p + 3] = 2u * (uint32_t)cnt[s];
    a.chunks[p] = AviChunk{a.table_bytes + off[p], 2u * (uint32_t)cnt[s], soff[s], status[s] == 0 ? (uint32_t)kAviAudio : (uint32_t)kAviSkip};
  }
}

// bytes [0, len) from src to dst, both offset alike: units of W bytes where dst (and so src) is on a W-byte boundary, bytes before and after
template <int W, typename T>
__device__ inline void avi_copy(unsigned char* dst, const unsigned char* src, uint32_t len, int t) {
  const uint32_t head = min(len, (uint32_t)((W - ((uintptr_t)dst & (W - 1))) & (W - 1)));
  const uint32_t body = (len - head) / W;
  const uint32_t tail0 = head + body * W;
  for (uint32_t i = t; i < head; i += kAviLanes) dst[i] = src[i];
  const T* s = (const T*)(src + head);
  T* d = (T*)(dst + head);
  for (uint32_t i = t; i < body; i += kAviLanes) d[i] = s[i];
  for (uint32_t i = tail0 + t; i < len; i += kAviLanes) dst[i] = src[i];
}

__device__ inline short avi_s16(float x) {
  float v = rintf(x * 32768.0f);                     // round half to even
  v = fminf(fmaxf(v, -32768.0f), 32767.0f);
  if (!(x == x)) v = 0.0f;
  return (short)(int)v;
}

__global__ __launch_bounds__(kAviLanes) void avi_gather_kernel(AviArgs a) {
  const uint32_t c = blockIdx.x;
  if (c >= *a.nchunks) return;
  const AviChunk ch = a.chunks[c];
  if (ch.kind == kAviSkip) return;
  const int t = threadIdx.x;
  const uint32_t n = ch.payload;
  unsigned char* head = a.out + ch.dst;
  unsigned char* dst = head + 8;
  if (blockIdx.y == 0 && t == 0) {
    const uint32_t fcc = ch.kind == kAviFrame ? kFcc00dc : kFcc01wb;
    for (int i = 0; i < 4; ++i) {
      head[i] = (unsigned char)(fcc >> (8 * i));
      head[4 + i] = (unsigned char)(n >> (8 * i));
    }
  }
  const uint32_t stride = gridDim.y * kAviSlice;
  if (ch.kind == kAviFrame) {
    const unsigned char* src = a.data + (size_t)ch.src * a.row_bytes;
    const uintptr_t x = (uintptr_t)src ^ (uintptr_t)dst;
    for (uint32_t b0 = blockIdx.y * kAviSlice; b0 < n; b0 += stride) {
      const uint32_t len = min(kAviSlice, n - b0);   // a slice starts a multiple of 16 bytes into both
      if ((x & 15) == 0) avi_copy<16, uint4>(dst + b0, src + b0, len, t);
      else if ((x & 3) == 0) avi_copy<4, uint32_t>(dst + b0, src + b0, len, t);
      else if ((x & 1) == 0) avi_copy<2, unsigned short>(dst + b0, src + b0, len, t);
      else avi_copy<1, unsigned char>(dst + b0, src + b0, len, t);
      if ((n & 1u) && b0 + len == n && t == kAviLanes - 1) dst[n] = 0;       // the pad byte of an odd length
    }
  } else {
    const float* src = a.pcm + ch.src;
    short* d = (short*)dst;                          // chunk offsets are even and the blob is on a 4-byte boundary
    for (uint32_t b0 = blockIdx.y * kAviSlice; b0 < n; b0 += stride) {
      const uint32_t i1 = min(b0 + kAviSlice, n) / 2;
      for (uint32_t i = b0 / 2 + t; i < i1; i += kAviLanes) d[i] = avi_s16(src[i]);
    }
  }
}

static size_t avi_table_bytes(int slots, int frames) { return 16 + 16 * (size_t)slots + 16 * ((size_t)frames + slots); }

}  // namespace vp

struct vp_avimux {
  vp_avimux_desc d;
  uint32_t* nchunks;
  vp::AviChunk* chunks;
};

using namespace vp;

// (this family's refusals name the entry point, `who`)
static int avi_check(const vp_avimux_desc* d, const char* who, vp_avimux* h) {
  if (const int rc = check_desc(d, "vp_avimux", who)) return rc;
  if (d->max_frames < 1 || d->max_frames > VP_AVIMUX_MAX_FRAMES) {
    set_err("%s: bad descriptor (max_frames %d, 1 .. %d)", who, d->max_frames, VP_AVIMUX_MAX_FRAMES);
    return VP_ERR_ARG;
  }
  if (d->slots < 1 || d->slots > VP_AVIMUX_MAX_SLOTS) { set_err("%s: bad descriptor (slots %d, 1 .. %d)", who, d->slots, VP_AVIMUX_MAX_SLOTS); return VP_ERR_ARG; }
  if (d->row_bytes < 1) { set_err("%s: bad descriptor (row_bytes %d, at least 1)", who, d->row_bytes); return VP_ERR_ARG; }
  if (d->max_samples < 0) { set_err("%s: bad descriptor (max_samples %d, at least 0)", who, d->max_samples); return VP_ERR_ARG; }
  const unsigned long long cap = avi_table_bytes(d->slots, d->max_frames) + (unsigned long long)d->max_frames * (8ull + (unsigned long long)d->row_bytes + 1ull) +
                                 8ull * d->slots + 2ull * (unsigned long long)d->max_samples;
  if (cap > 0xFFFFFFFFull) {
    set_err("%s: bad descriptor (%d frames of %d bytes and %d samples are %llu bytes: offsets are 32 bits)", who, d->max_frames, d->row_bytes, d->max_samples, cap);
    return VP_ERR_ARG;
  }
  h->d = *d;
  return VP_OK;
}

static size_t avi_carve(vp_avimux* h, void* base) {
  Arena ar(base);
  h->nchunks = ar.take<uint32_t>(1);
  h->chunks = ar.take<AviChunk>((size_t)h->d.max_frames + h->d.slots);
  return ar.total();
}

extern "C" {

size_t vp_avimux_desc_size(void) { return sizeof(vp_avimux_desc); }

size_t vp_avimux_workspace_bytes(const vp_avimux_desc* d) {
  vp_avimux h;
  return avi_check(d, "vp_avimux_workspace_bytes", &h) ? 0 : avi_carve(&h, nullptr);
}

size_t vp_avimux_table_bytes(const vp_avimux_desc* d, int frames) {
  vp_avimux h;
  if (avi_check(d, "vp_avimux_table_bytes", &h)) return 0;
  if (frames < 0 || frames > d->max_frames) { set_err("vp_avimux_table_bytes: frames %d outside 0 .. max_frames %d", frames, d->max_frames); return 0; }
  return avi_table_bytes(d->slots, frames);
}

size_t vp_avimux_out_capacity(const vp_avimux_desc* d) {
  vp_avimux h;
  if (avi_check(d, "vp_avimux_out_capacity", &h)) return 0;
  return avi_table_bytes(d->slots, d->max_frames) + (size_t)d->max_frames * (8 + (size_t)d->row_bytes + 1) + 8 * (size_t)d->slots + 2 * (size_t)d->max_samples;
}

int vp_avimux_create(const vp_avimux_desc* d, void* workspace, size_t workspace_bytes, vp_avimux_t** out) {
  const auto check = [](const vp_avimux_desc* d, vp_avimux* h) { return avi_check(d, "vp_avimux_create", h); };
  return open_handle("vp_avimux_create", d, check, avi_carve, workspace, workspace_bytes, out);
}

void vp_avimux_destroy(vp_avimux_t* h) { delete h; }

int vp_avimux_segment(vp_avimux_t* h, const unsigned char* data, size_t row_bytes, const int* lengths, const int* frame_slot, int frames,
                      const float* pcm, const int* sample_offset, const int* sample_count, int samples, unsigned char* out, size_t out_capacity,
                      void* stream) {
  const char* who = "vp_avimux_segment";
  if (!h || !out) { set_err("%s: bad argument (handle, device out)", who); return VP_ERR_ARG; }
  const vp_avimux_desc& d = h->d;
  if ((uintptr_t)out & 3) { set_err("%s: out must be on a 4-byte boundary", who); return VP_ERR_ARG; }
  if (frames < 0 || frames > d.max_frames) { set_err("%s: frames %d outside 0 .. max_frames %d", who, frames, d.max_frames); return VP_ERR_ARG; }
  if (frames > 0 && (!data || !lengths || !frame_slot)) { set_err("%s: %d frames without data, lengths or frame_slot", who, frames); return VP_ERR_ARG; }
  if (frames > 0 && (row_bytes < 1 || row_bytes > (size_t)d.row_bytes)) {
    set_err("%s: row_bytes %zu outside 1 .. the descriptor's %d", who, row_bytes, d.row_bytes);
    return VP_ERR_ARG;
  }
  if (samples < 0 || samples > d.max_samples) { set_err("%s: samples %d outside 0 .. max_samples %d", who, samples, d.max_samples); return VP_ERR_ARG; }
  if (samples > 0 && (!pcm || !sample_offset || !sample_count)) { set_err("%s: %d samples without pcm, sample_offset or sample_count", who, samples); return VP_ERR_ARG; }
  if ((uintptr_t)pcm & 3) { set_err("%s: pcm must be on a 4-byte boundary", who); return VP_ERR_ARG; }
  const size_t table = avi_table_bytes(d.slots, frames);
  if (out_capacity < table) { set_err("%s: out_capacity %zu is smaller than the table of %zu bytes", who, out_capacity, table); return VP_ERR_ARG; }
  AviArgs a;
  memset(&a, 0, sizeof(a));
  a.data = data; a.row_bytes = frames > 0 ? row_bytes : 1; a.lengths = lengths; a.frame_slot = frame_slot; a.K = frames;
  a.pcm = pcm; a.s_off = sample_offset; a.s_cnt = sample_count; a.samples = samples;
  a.out = out; a.cap = (uint32_t)(out_capacity > 0xFFFFFFFFull ? 0xFFFFFFFFull : out_capacity); a.table_bytes = (uint32_t)table; a.slots = d.slots;
  a.nchunks = h->nchunks;
  a.chunks = h->chunks;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(avi_layout_kernel, dim3(1), dim3(kAviLanes), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  const size_t longest = frames > 0 ? (row_bytes > 2 * (size_t)samples ? row_bytes : 2 * (size_t)samples) : 2 * (size_t)samples;
  size_t slices = (longest + kAviSlice - 1) / kAviSlice;
  slices = slices < 1 ? 1 : (slices > (size_t)kAviMaxSlices ? (size_t)kAviMaxSlices : slices);
  hipLaunchKernelGGL(avi_gather_kernel, dim3(frames + d.slots, (unsigned)slices), dim3(kAviLanes), 0, st, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

}  // extern "C"

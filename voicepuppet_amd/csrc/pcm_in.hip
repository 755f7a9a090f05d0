// Stream ingest (vp_pcmin_*): client PCM as it arrives - interleaved int16 or float32, 1 .. 8 channels, any common rate - to the mono float32
// 16 kHz signal vp_bfmstream_group_push takes, on the device and chunk by chunk.  What WavLoader.get_data (generator/loader.py:39-54) does
// for a whole file on the host: convert, mean over the channels, scipy.signal.resample_poly(x, up, down) with its default Kaiser design.
//
//   y[m] = sum_k h[m * down - k * up + half] * x[k]        h = float32(firwin(2 half + 1, 1 / max(up, down), ('kaiser', 5.0))) * up
//
// Polyphase form: q = m * down + half, phase p = q % up, newest input k1 = q / up, y[m] = sum_{t < T} bank[p][t] * x[k1 - t] with
// bank[p][t] = h[p + t * up] (0 past the end of h), T = ceil((2 half + 1) / up).  Every output is ONE float32 fma chain over t = 0 .. T-1,
// inputs outside the clip entering as zeros: its bits depend on the clip alone, not on where pushes cut it or which slots share a launch.
//
// Per slot the handle keeps the last Hn >= T mono frames (two buffers; a push reads one and writes the other, so one launch does both)
// and, on the host, the input / output counters.  All counts are host arithmetic; a push never waits and never allocates.
//
//   pcmin_kernel   one workgroup per (slot, tile of 256 outputs), plus one per slot that received frames (its new history).
//     A tile stages its span of [history ++ new frames ++ zeros] in LDS once: history and zeros by dword, the new frames by 16-byte loads
//     of the interleaved samples where a frame's size divides 16 (the slot's segment starts on a 16-byte boundary), converted and mixed
//     down on the way.  Then one output per thread: T fmas from LDS and the slot's bank (global, L2-resident: 244 bytes at 48 kHz, 35 KB at
//     44.1 kHz).  up == down copies (no filter, no delay).  The table of the launch (7 dwords per slot) travels by value.
//
// Only vector loads / stores and plain C++.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "workspace.h"

namespace vp {

constexpr int kPcmThreads = 256;               // outputs per tile
constexpr int kPcmSpan = 4096;                 // floats of LDS per tile: ceil(255 down / up) + T + 1 input frames must fit
constexpr size_t kPcmBankCap = 1u << 20;       // bytes of one rate's polyphase bank
constexpr int kPcmMaxIn = 1 << 22;             // frames per slot and push (32-bit lane offsets: 8 channels x 4 bytes x 4 M frames = 128 MB)

struct PcmRate {                               // device copy, one per accepted rate
  int up, down, half, T, Hn, bank_off;         // bank_off: floats from the start of the banks
};

struct PcmEntry {                              // one participating slot of a launch
  uint32_t raw_off16;                          // its segment of raw, in 16-byte units
  int n_new;                                   // new input frames
  int n_out;                                   // outputs of this push
  int out_off;                                 // where they go in the packed output
  int tile0;                                   // first workgroup
  int kbase;                                   // index of k1(first output) in the virtual signal [history(Hn) ++ new ++ zeros]
  uint32_t cfg;                                // p0 (phase of the first output) | rate << 16 | (channels - 1) << 19 | format << 22 | parity << 23 | slot << 24
};

struct PcmArgs {
  const unsigned char* raw;
  float* out;
  float* hist;                                 // [slots][2][hist_stride]
  const float* banks;
  const PcmRate* rates;
  int hist_stride, entries, tiles;             // workgroups >= tiles write histories: entry (block - tiles) of those with n_new > 0, in hist_entry
  PcmEntry e[VP_PCMIN_MAX_SLOTS];
  unsigned char hist_entry[VP_PCMIN_MAX_SLOTS];
};
static_assert(sizeof(PcmArgs) <= 4096, "the launch table travels as kernel arguments");

// one frame -> mono float32: WavLoader's expressions (int16 / 32768; mean over the channels in float32, left to right)
template <typename S>
__device__ __forceinline__ float pcm_sample(S v);
template <>
__device__ __forceinline__ float pcm_sample<short>(short v) { return (float)v * (1.0f / 32768.0f); }
template <>
__device__ __forceinline__ float pcm_sample<float>(float v) { return v; }

template <typename S>
__device__ __forceinline__ float pcm_mix(const S* s, int c) {
  float a = pcm_sample<S>(s[0]);
  if (c == 1) return a;
  for (int i = 1; i < c; ++i) a += pcm_sample<S>(s[i]);
  return c == 2 ? a * 0.5f : a / (float)c;
}

// frames [f_a, f_b) of a slot's segment -> dst[f - f_a + dst0] (dst: LDS or the new history)
template <typename S>
__device__ __forceinline__ void pcm_stage(const unsigned char* seg, int n_new, int c, int f_a, int f_b, float* dst, int dst0) {
  const int fb = c * (int)sizeof(S);           // bytes per frame
  if (16 % fb == 0) {
    const int fpv = 16 / fb;
    for (int v = f_a / fpv + (int)threadIdx.x; v * fpv < f_b; v += kPcmThreads) {
      const int f0 = v * fpv;
      if (f0 + fpv <= n_new) {
        union { uint4 q; S s[16 / sizeof(S)]; } u;
        u.q = *reinterpret_cast<const uint4*>(seg + (size_t)v * 16);
#pragma unroll
        for (int j = 0; j < 16 / (int)sizeof(S); ++j) {
          if (j < fpv) {
            const int f = f0 + j;
            if (f >= f_a && f < f_b) dst[f - f_a + dst0] = pcm_mix<S>(u.s + j * c, c);
          }
        }
      } else {                                 // the last, partial vector of the segment: nothing is read past its frames
        for (int f = max(f0, f_a); f < min(f_b, n_new); ++f) dst[f - f_a + dst0] = pcm_mix<S>(reinterpret_cast<const S*>(seg + (size_t)f * fb), c);
      }
    }
  } else {
    for (int f = f_a + (int)threadIdx.x; f < f_b; f += kPcmThreads) dst[f - f_a + dst0] = pcm_mix<S>(reinterpret_cast<const S*>(seg + (size_t)f * fb), c);
  }
}

__global__ __launch_bounds__(kPcmThreads) void pcmin_kernel(const PcmArgs a) {
  __shared__ float x[kPcmSpan];
  const int b = (int)blockIdx.x;
  const bool is_hist = b >= a.tiles;
  int ei;
  if (is_hist) {
    ei = a.hist_entry[b - a.tiles];
  } else {
    ei = 0;
    while (ei + 1 < a.entries && b >= a.e[ei + 1].tile0) ++ei;
  }
  const PcmEntry& e = a.e[ei];
  const uint32_t cfg = e.cfg;
  const int p0 = (int)(cfg & 0xffffu), ri = (int)((cfg >> 16) & 7u), c = (int)((cfg >> 19) & 7u) + 1, fmt = (int)((cfg >> 22) & 1u);
  const int parity = (int)((cfg >> 23) & 1u), slot = (int)(cfg >> 24);
  const PcmRate r = a.rates[ri];
  const unsigned char* seg = a.raw + (size_t)e.raw_off16 * 16;
  const float* hist = a.hist + ((size_t)slot * 2 + parity) * a.hist_stride;
  const int n_new = e.n_new, Hn = r.Hn;

  if (is_hist) {
    // the last Hn frames of [history ++ new]: virtual indices n_new .. n_new + Hn - 1
    float* nh = a.hist + ((size_t)slot * 2 + (parity ^ 1)) * a.hist_stride;
    const int keep = max(Hn - n_new, 0);       // frames that stay from the old history
    for (int i = (int)threadIdx.x; i < keep; i += kPcmThreads) nh[i] = hist[i + n_new];
    const int f_a = max(n_new - Hn, 0);
    if (fmt == 0) pcm_stage<short>(seg, n_new, c, f_a, n_new, nh, keep);
    else pcm_stage<float>(seg, n_new, c, f_a, n_new, nh, keep);
    return;
  }

  const int i0 = (b - e.tile0) * kPcmThreads;  // first output of the tile, within the push
  const int i = i0 + (int)threadIdx.x;
  float* out = a.out + e.out_off;
  if (r.up == r.down) {                        // pass-through: output i is new frame i
    const int f_b = min(i0 + kPcmThreads, e.n_out);
    if (fmt == 0) pcm_stage<short>(seg, n_new, c, i0, f_b, out, i0);
    else pcm_stage<float>(seg, n_new, c, i0, f_b, out, i0);
    return;
  }
  const int T = r.T;
  // virtual index of the newest input of output j of the push: kbase + (p0 + j * down) / up
  const unsigned long long q_lo = (unsigned long long)p0 + (unsigned long long)i0 * (unsigned)r.down;
  const int i_last = min(i0 + kPcmThreads, e.n_out) - 1;
  const unsigned long long q_hi = (unsigned long long)p0 + (unsigned long long)i_last * (unsigned)r.down;
  const int r_lo = e.kbase + (int)(q_lo / (unsigned)r.up) - (T - 1);
  const int r_hi = e.kbase + (int)(q_hi / (unsigned)r.up);
  const int span = r_hi - r_lo + 1;            // <= kPcmSpan (checked per rate at create); r_lo >= 0 (Hn >= T)
  for (int j = (int)threadIdx.x; j < span; j += kPcmThreads) {
    const int rr = r_lo + j;
    if (rr < Hn) x[j] = hist[rr];
    else if (rr >= Hn + n_new) x[j] = 0.0f;
  }
  const int f_a = max(r_lo - Hn, 0), f_b = min(r_hi + 1 - Hn, n_new);
  if (f_b > f_a) {
    if (fmt == 0) pcm_stage<short>(seg, n_new, c, f_a, f_b, x, f_a + Hn - r_lo);
    else pcm_stage<float>(seg, n_new, c, f_a, f_b, x, f_a + Hn - r_lo);
  }
  __syncthreads();
  if (i < e.n_out) {
    const unsigned long long q = (unsigned long long)p0 + (unsigned long long)i * (unsigned)r.down;
    const int k1 = e.kbase + (int)(q / (unsigned)r.up) - r_lo;       // in x
    const int p = (int)(q % (unsigned)r.up);
    const float* bank = a.banks + r.bank_off + (size_t)p * T;
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) acc = fmaf(bank[t], x[k1 - t], acc);
    out[i] = acc;
  }
}

// ---- host: ratio, filter design, counts --------------------------------------------------------------------------------------------------
static long long gcd_ll(long long a, long long b) { while (b) { long long t = a % b; a = b; b = t; } return a; }

struct PcmRatio { int up, down, half, T; };

static int pcm_ratio(int in_rate, int out_rate, PcmRatio* r) {
  if (in_rate < 1 || out_rate < 1 || in_rate > 1000000 || out_rate > 1000000) return VP_ERR_ARG;
  const long long g = gcd_ll(in_rate, out_rate);
  r->up = (int)(out_rate / g);
  r->down = (int)(in_rate / g);
  if (r->up == r->down) { r->half = 0; r->T = 1; return VP_OK; }
  const long long half = 10LL * (r->up > r->down ? r->up : r->down);
  if (half > (1 << 26)) return VP_ERR_ARG;
  r->half = (int)half;
  r->T = (int)((2 * half + 1 + r->up - 1) / r->up);
  return VP_OK;
}

// modified Bessel function I0 by its power series (x <= 5 here: 30 terms reach 1e-17 relative)
static double bessel_i0(double x) {
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 60; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) in double, then resample_poly's float32 cast and h *= up
static void pcm_bank(const PcmRatio& r, float* h) {
  const int N = 2 * r.half + 1;
  const double kPi = 3.14159265358979323846, beta = 5.0;
  const double c = 1.0 / (double)(r.up > r.down ? r.up : r.down), alpha = 0.5 * (N - 1), i0b = bessel_i0(beta);
  std::vector<double> d(N);
  double s = 0.0;
  for (int i = 0; i < N; ++i) {
    const double m = (double)i - alpha;
    const double y = kPi * (m == 0.0 ? 1.0e-20 : c * m);
    const double u = m / alpha;
    const double w = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - u * u))) / i0b;
    d[i] = c * (sin(y) / y) * w;
    s += d[i];
  }
  const float fup = (float)r.up;
  for (int i = 0; i < N; ++i) h[i] = (float)(d[i] / s) * fup;
}

static long long pcm_samples_after(const PcmRatio& r, long long n, int finished) {
  // n * up stays far below 2^63: n < 2^40 (checked by the callers), up <= 10^6
  const long long total = (n * r.up + r.down - 1) / r.down;
  if (finished) return total;
  const long long a = n * r.up - 1 - r.half;
  const long long cnt = a < 0 ? 0 : a / r.down + 1;
  return cnt < total ? cnt : total;
}

struct PcmSlot { int rate, channels, format, parity; bool open, finished; long long n_in, n_out; };

}  // namespace vp

struct vp_pcmin {
  vp_pcmin_desc d;
  vp::PcmRatio ratio[8];
  int Hn[8], bank_off[8];
  int hist_stride;
  size_t bank_floats;
  vp::PcmRate* rates;
  float *banks, *hist;
  vp::PcmSlot slot[VP_PCMIN_MAX_SLOTS];
};

using namespace vp;

// (this family's null and struct_bytes refusals keep their own wording, which is older than check_desc's)
static int pcm_check(const vp_pcmin_desc* d, vp_pcmin* h) {
  if (!d) { set_err("vp_pcmin: null descriptor"); return VP_ERR_ARG; }
  if (d->struct_bytes != (int)sizeof(vp_pcmin_desc)) {
    set_err("vp_pcmin_desc: struct_bytes is %d, this library's descriptor has %zu (the struct grows at the tail only)", d->struct_bytes, sizeof(vp_pcmin_desc));
    return VP_ERR_ARG;
  }
  if (d->slots < 1 || d->slots > VP_PCMIN_MAX_SLOTS) { set_err("vp_pcmin_desc: slots = %d, 1 .. %d", d->slots, VP_PCMIN_MAX_SLOTS); return VP_ERR_ARG; }
  if (d->out_rate < 1000 || d->out_rate > 1000000) { set_err("vp_pcmin_desc: out_rate = %d, 1000 .. 1000000 (the model's is 16000)", d->out_rate); return VP_ERR_ARG; }
  if (d->max_in_frames < 1 || d->max_in_frames > kPcmMaxIn) { set_err("vp_pcmin_desc: max_in_frames = %d, 1 .. %d", d->max_in_frames, kPcmMaxIn); return VP_ERR_ARG; }
  if (d->n_rates < 1 || d->n_rates > 8) { set_err("vp_pcmin_desc: n_rates = %d, 1 .. 8", d->n_rates); return VP_ERR_ARG; }
  h->d = *d;
  h->bank_floats = 0;
  h->hist_stride = 4;
  for (int i = 0; i < d->n_rates; ++i) {
    PcmRatio& r = h->ratio[i];
    if (pcm_ratio(d->rates[i], d->out_rate, &r)) { set_err("vp_pcmin_desc: rates[%d] = %d is no sample rate (1 .. 1000000 Hz)", i, d->rates[i]); return VP_ERR_ARG; }
    for (int j = 0; j < i; ++j)
      if (d->rates[j] == d->rates[i]) { set_err("vp_pcmin_desc: rates[%d] = %d is listed twice", i, d->rates[i]); return VP_ERR_ARG; }
    const size_t bytes = (size_t)r.up * r.T * sizeof(float);
    const long long span = ((long long)(kPcmThreads - 1) * r.down) / r.up + r.T + 1;
    if (r.up != r.down && (bytes > kPcmBankCap || r.up > 65535 || span > kPcmSpan)) {
      set_err("vp_pcmin_desc: rates[%d] = %d Hz is over the cap: up / down = %d / %d needs a bank of %zu bytes (cap %zu) and %lld frames of LDS per tile (cap %d)",
              i, d->rates[i], r.up, r.down, bytes, kPcmBankCap, span, kPcmSpan);
      return VP_ERR_ARG;
    }
    h->Hn[i] = (r.T + 3) & ~3;
    h->bank_off[i] = (int)h->bank_floats;
    h->bank_floats += (r.up == r.down) ? 4 : (((size_t)r.up * r.T + 3) & ~(size_t)3);
    if (h->Hn[i] > h->hist_stride) h->hist_stride = h->Hn[i];
  }
  return VP_OK;
}

static size_t pcm_carve(vp_pcmin* h, void* base) {
  Arena ar(base);
  h->rates = ar.take<PcmRate>(8);
  h->banks = ar.take<float>(h->bank_floats);
  h->hist = ar.take<float>((size_t)h->d.slots * 2 * h->hist_stride);
  return align256(ar.total());
}

// the counts of one push, host only: 0, or VP_ERR_ARG with the message set
static int pcm_counts(const vp_pcmin_t* h, const char* who, const long long* in_frames, const int* finish, long long* out_samples, long long* total) {
  *total = 0;
  for (int s = 0; s < h->d.slots; ++s) {
    const long long n = in_frames ? in_frames[s] : 0;
    const int fin = finish ? finish[s] != 0 : 0;
    long long k = 0;
    if (n < 0 || n > h->d.max_in_frames) { set_err("%s: in_frames[%d] = %lld, 0 .. max_in_frames = %d per push", who, s, n, h->d.max_in_frames); return VP_ERR_ARG; }
    if (n || fin) {
      const PcmSlot& S = h->slot[s];
      if (!S.open) { set_err("%s: slot %d is not open (vp_pcmin_open_slot)", who, s); return VP_ERR_ARG; }
      if (S.finished) { set_err("%s: slot %d has finished its clip (vp_pcmin_open_slot restarts it)", who, s); return VP_ERR_ARG; }
      if (S.n_in + n > (1LL << 40)) { set_err("%s: slot %d: more than 2^40 frames in one clip", who, s); return VP_ERR_ARG; }
      k = pcm_samples_after(h->ratio[S.rate], S.n_in + n, fin) - S.n_out;
    }
    if (out_samples) out_samples[s] = k;
    *total += k;
  }
  return VP_OK;
}

extern "C" {

size_t vp_pcmin_desc_size(void) { return sizeof(vp_pcmin_desc); }

int vp_pcmin_ratio(int in_rate, int out_rate, int* up, int* down, int* half, int* taps_per_phase) {
  PcmRatio r;
  if (pcm_ratio(in_rate, out_rate, &r)) { set_err("vp_pcmin_ratio: in_rate = %d, out_rate = %d: 1 .. 1000000 Hz", in_rate, out_rate); return VP_ERR_ARG; }
  if (up) *up = r.up;
  if (down) *down = r.down;
  if (half) *half = r.half;
  if (taps_per_phase) *taps_per_phase = r.T;
  return VP_OK;
}

int vp_pcmin_bank(int in_rate, int out_rate, float* h) {
  PcmRatio r;
  if (!h || pcm_ratio(in_rate, out_rate, &r)) { set_err("vp_pcmin_bank: bad argument (in_rate = %d, out_rate = %d)", in_rate, out_rate); return VP_ERR_ARG; }
  if (r.up == r.down) { h[0] = 1.0f; return VP_OK; }
  pcm_bank(r, h);
  return VP_OK;
}

long long vp_pcmin_samples_after(int in_rate, int out_rate, long long in_frames, int finished) {
  PcmRatio r;
  if (in_frames < 0 || in_frames > (1LL << 40) || pcm_ratio(in_rate, out_rate, &r)) {
    set_err("vp_pcmin_samples_after: bad argument (in_rate = %d, out_rate = %d, in_frames = %lld)", in_rate, out_rate, in_frames);
    return -1;
  }
  return pcm_samples_after(r, in_frames, finished);
}

size_t vp_pcmin_workspace_bytes(const vp_pcmin_desc* d) {
  vp_pcmin h;
  return pcm_check(d, &h) ? 0 : pcm_carve(&h, nullptr);
}

int vp_pcmin_create(const vp_pcmin_desc* d, void* workspace, size_t bytes, void* stream, vp_pcmin_t** out) {
  if (const int rc = open_handle("vp_pcmin_create", d, pcm_check, pcm_carve, workspace, bytes, out)) return rc;
  vp_pcmin* h = *out;
  memset(h->slot, 0, sizeof(h->slot));
  // the rate table and the polyphase banks [phase][tap], from the float32 filter: bank[p][t] = h[p + t up]
  PcmRate rates[8];
  memset(rates, 0, sizeof(rates));
  std::vector<float> banks(align256(h->bank_floats * sizeof(float)) / sizeof(float), 0.0f), hf;      // (zeros up to the end of the carve)
  for (int i = 0; i < d->n_rates; ++i) {
    const PcmRatio& r = h->ratio[i];
    rates[i] = PcmRate{r.up, r.down, r.half, r.T, h->Hn[i], h->bank_off[i]};
    if (r.up == r.down) continue;
    const int N = 2 * r.half + 1;
    hf.assign(N, 0.0f);
    pcm_bank(r, hf.data());
    float* b = banks.data() + h->bank_off[i];
    for (int p = 0; p < r.up; ++p)
      for (int t = 0; t < r.T; ++t) {
        const long long j = (long long)p + (long long)t * r.up;
        b[(size_t)p * r.T + t] = j < N ? hf[j] : 0.0f;
      }
  }
  hipStream_t st = (hipStream_t)stream;
  // create is not a push: it may wait (pageable sources), once per handle
  hipError_t e = hipMemcpyAsync(h->rates, rates, sizeof(rates), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->banks, banks.data(), banks.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(h->hist, 0, (size_t)d->slots * 2 * h->hist_stride * sizeof(float), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_err("vp_pcmin_create: table upload -> %s", hipGetErrorString(e)); delete h; *out = nullptr; return VP_ERR_HIP; }
  return VP_OK;
}

void vp_pcmin_destroy(vp_pcmin_t* h) { delete h; }

int vp_pcmin_open_slot(vp_pcmin_t* h, int slot, int in_rate, int channels, int format, void* stream) {
  if (channels < 1 || channels > VP_PCMIN_MAX_CHANNELS) { set_err("vp_pcmin_open_slot: channels = %d, 1 .. %d", channels, VP_PCMIN_MAX_CHANNELS); return VP_ERR_ARG; }
  if (format != VP_PCM_S16 && format != VP_PCM_F32) { set_err("vp_pcmin_open_slot: format = %d (VP_PCM_S16 or VP_PCM_F32)", format); return VP_ERR_ARG; }
  if (!h) { set_err("vp_pcmin_open_slot: null handle"); return VP_ERR_ARG; }
  if (slot < 0 || slot >= h->d.slots) { set_err("vp_pcmin_open_slot: slot = %d of %d", slot, h->d.slots); return VP_ERR_ARG; }
  int ri = -1;
  for (int i = 0; i < h->d.n_rates; ++i)
    if (h->d.rates[i] == in_rate) ri = i;
  if (ri < 0) { set_err("vp_pcmin_open_slot: in_rate = %d is not among the rates of the descriptor", in_rate); return VP_ERR_ARG; }
  PcmSlot& S = h->slot[slot];
  // an empty clip has a zero history; the buffer the next push reads is zeroed in stream order
  VP_HIP_CHECK(hipMemsetAsync(h->hist + ((size_t)slot * 2 + S.parity) * h->hist_stride, 0, h->hist_stride * sizeof(float), (hipStream_t)stream));
  S.rate = ri; S.channels = channels; S.format = format;
  S.open = true; S.finished = false; S.n_in = 0; S.n_out = 0;
  return VP_OK;
}

long long vp_pcmin_ready(const vp_pcmin_t* h, const long long* in_frames, const int* finish, long long* out_samples) {
  if (!h) { set_err("vp_pcmin_ready: bad argument"); return -1; }
  long long total;
  return pcm_counts(h, "vp_pcmin_ready", in_frames, finish, out_samples, &total) ? -1 : total;
}

int vp_pcmin_push(vp_pcmin_t* h, const void* raw, const long long* in_frames, const int* finish, float* pcm_out, void* stream) {
  if (!h) { set_err("vp_pcmin_push: bad argument"); return VP_ERR_ARG; }
  long long k[VP_PCMIN_MAX_SLOTS], total;
  const int rc = pcm_counts(h, "vp_pcmin_push", in_frames, finish, k, &total);
  if (rc) return rc;
  if (total > 0x7fffffffLL) { set_err("vp_pcmin_push: %lld output samples in one push", total); return VP_ERR_ARG; }
  PcmArgs a;
  a.raw = (const unsigned char*)raw; a.out = pcm_out;
  a.hist = h->hist;
  a.banks = h->banks;
  a.rates = h->rates;
  a.hist_stride = h->hist_stride;
  int ne = 0, tiles = 0, nh = 0;
  size_t raw_bytes = 0;
  long long out_off = 0, in_total = 0;
  for (int s = 0; s < h->d.slots; ++s) {
    const long long n = in_frames ? in_frames[s] : 0;
    if (n == 0 && k[s] == 0) continue;
    const PcmSlot& S = h->slot[s];
    const PcmRatio& r = h->ratio[S.rate];
    PcmEntry& e = a.e[ne];
    raw_bytes = (raw_bytes + 15) & ~(size_t)15;
    if ((raw_bytes >> 4) > 0xffffffffull) { set_err("vp_pcmin_push: more than 64 GB of raw samples in one push"); return VP_ERR_ARG; }
    e.raw_off16 = (uint32_t)(raw_bytes >> 4);
    raw_bytes += (size_t)n * S.channels * (S.format == VP_PCM_S16 ? 2 : 4);
    e.n_new = (int)n; e.n_out = (int)k[s]; e.out_off = (int)out_off; e.tile0 = tiles;
    // first output m0 = n_out so far: q = m0 down + half, newest input k1 = q / up, as an index into [history (n_in - Hn ..) ++ new]
    const long long q = S.n_out * r.down + r.half;
    e.kbase = (int)(q / r.up - (S.n_in - h->Hn[S.rate]));
    e.cfg = (uint32_t)(q % r.up) | (uint32_t)S.rate << 16 | (uint32_t)(S.channels - 1) << 19 | (uint32_t)S.format << 22 | (uint32_t)S.parity << 23 | (uint32_t)s << 24;
    tiles += (int)((k[s] + kPcmThreads - 1) / kPcmThreads);
    if (n) a.hist_entry[nh++] = (unsigned char)ne;
    out_off += k[s]; in_total += n;
    ++ne;
  }
  if (in_total && !raw) { set_err("vp_pcmin_push: raw is NULL with frames to read"); return VP_ERR_ARG; }
  if (total && !pcm_out) { set_err("vp_pcmin_push: pcm_out is NULL with samples to write"); return VP_ERR_ARG; }
  if (((uintptr_t)raw & 15) != 0) { set_err("vp_pcmin_push: raw must start on a 16-byte boundary (the kernel reads it in 16-byte vectors)"); return VP_ERR_ARG; }
  a.entries = ne; a.tiles = tiles;
  if (tiles + nh) {
    hipLaunchKernelGGL(pcmin_kernel, dim3(tiles + nh), dim3(kPcmThreads), 0, (hipStream_t)stream, a);
    VP_HIP_CHECK(hipGetLastError());
  }
  for (int s = 0; s < h->d.slots; ++s) {
    const long long n = in_frames ? in_frames[s] : 0;
    PcmSlot& S = h->slot[s];
    if (n) S.parity ^= 1;
    S.n_in += n; S.n_out += k[s];
    if (finish && finish[s]) S.finished = true;
  }
  return VP_OK;
}

}  // extern "C"

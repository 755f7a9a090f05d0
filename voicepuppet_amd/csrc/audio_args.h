// Launchers of audio_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vp {
hipError_t launch_frame_window(const float* pcm, const float* window, float* frames, int B, int L, int F, int win, int hop, hipStream_t st);
// 512-sample frames, <= 80 mel bins: the whole log-mel front-end in one launch (FFT form)
hipError_t launch_logmel512(const float* pcm, const float* window, const float* w256, const float* w512, const float* mel, float* out, int B, int L, int F, int hop,
                            int nmel, hipStream_t st);
hipError_t launch_mag_mel_log(const float* spec, int ld, int nb, const float* mel, int nmel, float* out, int nframes, hipStream_t st);
// TF 'SAME': out = ceil(size / s), total pad = max((out - 1) s + k - size, 0), the odd unit goes to the end; *pb is the leading pad
inline void same_pad(int size, int k, int s, int* pb, int* out) {
  const int o = (size + s - 1) / s;
  int total = (o - 1) * s + k - size;
  if (total < 0) total = 0;
  *pb = total / 2; *out = o;
}
hipError_t launch_conv_first(const float* x, const float* w, const float* bias, void* y, int out_bf16, int B, int H, int W, int Wo, int Cout, int pt, int pl, hipStream_t st);
hipError_t launch_dwconv7x3(const void* x, const float* w, const float* bias, void* y, int is_bf16, int B, int H, int W, int C, hipStream_t st, int rev = 0);
// bfm_dwproj.hip: depthwise 7x3 + ReLU6 + 1x1 projection (+ residual) of an inverted-residual block in one kernel (float32, mel widths <= 20);
// wdw22: the 21 folded taps followed by the folded bias row [22][Ce]; Wp: PackDesc-packed projection weights WITHOUT row permutation
inline int& bfm_dwproj_knob() { static int v = 1; return v; }
bool dwproj_eligible(int W, int Ce, int cout);
hipError_t launch_dwproj(const float* ex, const float* wdw22, const float* Wp, int rows_pad, const float* bias, float* y, int add, int B, int H, int W,
                         int Ce, int cout, hipStream_t st);
hipError_t launch_cvt_f32_bf16(const float* x, void* y, size_t n, hipStream_t st);
hipError_t launch_maxpool_same(const void* x, void* y, int in_bf16, int out_bf16, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int pt, int pl, int Ho, int Wo, hipStream_t st);
hipError_t launch_fold_bn(const float* w, const float* beta, const float* mean, const float* var, float eps, size_t n, int C, float* wf, float* bf, hipStream_t st);
hipError_t launch_gru_seq(const float* xg, const float* xc, const float* whg, const float* whc, const int* seq_len, float* out, int B, int T, hipStream_t st);
// gru_fwd_state_kernel: rows [t0, t0 + n) of each sequence's T rows, state in / out in hstate [B][256]
hipError_t launch_gru_state(const float* xg, const float* xc, const float* whg, const float* whc, float* hstate, float* out, int B, int T, int t0, int n,
                            hipStream_t st);
hipError_t launch_add_ears(float* out, const float* ears, int n, hipStream_t st);
// Streaming groups (vp_bfmstream_group, plan_bfmnet.hip).  The per-launch tables travel BY VALUE as kernel arguments (a push never waits
// on the device, so there is no host buffer whose reuse would need a fence): at most kGroupMaxSlots entries (<= 4 KB of arguments).
constexpr int kGroupMaxSlots = 128;
constexpr int kGroupCarry = 512;      // floats per carry buffer (the carried samples of a stream are fewer than one 512-sample frame)
// one stream's log-mel piece: carry[slot][cur][0, carry_n) ++ (zeros ? 0 : pcm[pcm_off ..]), F * hop + keep samples, staged in row e
// of stage [entries][stage_len] -> logmel512_kernel -> frames [entries][max_frames][nmel] -> F frames at ring rows ring_row .. (mod cap)
// of ring[slot]; the `keep` samples from F * hop on -> carry[slot][cur ^ 1].  Three launches; max_samples: the longest piece
struct LmGroupEntry { int pcm_off, ring_row; short slot, carry_n, F, keep; unsigned char cur, zeros; };
struct LmGroupTable { LmGroupEntry e[kGroupMaxSlots]; };
hipError_t launch_logmel512_group(const float* pcm, float* carry, float* stage, int stage_len, float* frames, float* ring, int cap, const float* window,
                                  const float* w256, const float* w512, const float* mel, int nmel, int hop, const LmGroupTable& tab, int nentries,
                                  int max_frames, int max_samples, hipStream_t st);
// window rows of one active stream: ring[slot] rows r0 (mod cap) .., the first `valid` received
struct WinGroupEntry { int slot, r0, valid; };
struct WinGroupTable { WinGroupEntry e[kGroupMaxSlots]; };
hipError_t launch_mel_window_group(const float* ring, int cap, int nmel, int rows, int A, int B, const WinGroupTable& tab, float* out, hipStream_t st);
// the emitted rows [t0, t0 + n) of one active stream's window; row: where they go in the packed output
struct RowsGroupEntry { int slot, t0, n, row; };
struct RowsGroupTable { RowsGroupEntry e[kGroupMaxSlots]; };
hipError_t launch_gru_state_group(const float* xg, const float* xc, const float* whg, const float* whc, float* hstate, float* out, int T, const RowsGroupTable& tab,
                                  int A, hipStream_t st);
hipError_t launch_rows_scatter_group(const float* src, int T, float* dst, const RowsGroupTable& tab, int A, int max_rows, hipStream_t st);

hipError_t launch_mul_inplace(float* x, const float* m, size_t n, hipStream_t st);
}  // namespace vp

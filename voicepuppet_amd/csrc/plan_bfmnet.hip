// Audio front-end executors: log-mel (DataGenerator.extract_mfcc, generator/generator.py:60-80) and
// BFMNet inference (voicepuppet/bfmnet/bfmnet.py:189-213,325-333 + tinynet.py:159-212), f32.
//   * STFT = framing kernel + ONE f32-MFMA GEMM against a [512 x 514] cos/-sin matrix (the DFT of a 512
//     window is 0.26 MMAC per frame; a GEMM keeps it on the matrix cores and bit-stable), then a fused
//     |.| -> mel(257x80) -> log kernel.
//   * MfccNet: inference batch-norm (contrib, no gamma, eps 1e-3) is folded into the conv weights on the
//     device whenever the parameters change; every 1x1 conv / dense layer is the implicit-GEMM kernel with
//     bias + activation (+ residual accumulate) in its epilogue; depthwise 7x3, the 9x5 stem and the SAME
//     max-pools are VALU kernels; the GRU is one persistent block per sequence.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "audio_args.h"
#include "conv_ops.h"
#include "errors.h"
#include "launch.h"
#include "vp_common.h"
#include "workspace.h"

using namespace vp;

namespace {

// a 1x1 conv / dense layer as an igemm over `pixels` rows
struct Gemm {
  int cin = 0, cout = 0;
  size_t w_src = 0;      // float offset of the [cin, cout] matrix in its source arena
  int src_ld = 0;        // row stride (cout of the full TF kernel; GRU kernels are read partially)
  int which = 0;         // 0: folded arena, 1: raw parameter arena
  size_t bias = 0;       // float offset of the bias (folded arena or raw arena, same `which`)
  size_t pk = 0;         // BYTE offset in the packed arena
  int bf = 0;            // bf16 operands / output (the MfccNet trunk in bf16-storage mode), f32 accumulation
  IgemmPlan plan;
};

}  // namespace

// ------------------------------------------------------------------------------------------------
// log-mel
// ------------------------------------------------------------------------------------------------
struct vp_logmel {
  vp_logmel_desc d;
  int frames, nb, ncol;
  float *window, *dft, *mel, *frames_buf, *spec;
  float *w256, *w512;      // FFT twiddles of the one-launch form (audio_kernels.hip logmel512_kernel)
  bool fused;              // 512-sample frames, <= 80 mel bins: one launch; other shapes: framing + DFT matrix product + mel (three)
  char* packed;
  char* scratch;
  void* zeros;
  IgemmPlan plan;
};

static size_t logmel_carve(vp_logmel* h, char* base) {
  Arena ar(base);
  const vp_logmel_desc& d = h->d;
  h->frames = 1 + (d.samples - d.win_length) / d.hop_step;
  h->nb = d.fft_length / 2 + 1;
  h->ncol = round_up(2 * h->nb, 8);
  const size_t P = (size_t)d.batch * h->frames;
  h->window = (float*)ar.alloc(d.win_length * sizeof(float));
  h->dft = (float*)ar.alloc((size_t)d.win_length * h->ncol * sizeof(float));
  h->mel = (float*)ar.alloc((size_t)h->nb * d.num_mel_bins * sizeof(float));
  h->w256 = (float*)ar.alloc(256 * 2 * sizeof(float));
  h->w512 = (float*)ar.alloc(257 * 2 * sizeof(float));
  h->fused = d.win_length == 512 && d.num_mel_bins <= 80;
  h->frames_buf = (float*)ar.alloc(P * d.win_length * sizeof(float));
  h->spec = (float*)ar.alloc(P * h->ncol * sizeof(float));
  ConvGeomX g = make_geom(0, 1, 1, 0, 1, (int)P, 1, d.win_length, d.win_length, h->ncol);
  h->plan = plan_fwd(g, 0, 0);
  h->packed = (char*)ar.alloc(h->plan.pack_elems * sizeof(float));
  h->scratch = (char*)ar.alloc(h->plan.partial_bytes + 256);
  h->zeros = ar.alloc(256);
  return ar.total();
}

static bool logmel_ok(const vp_logmel_desc* d) {
  return d && d->batch >= 1 && d->win_length == d->fft_length && d->win_length % 16 == 0 && d->win_length <= 4096 &&
         d->hop_step >= 1 && d->samples >= d->win_length && d->num_mel_bins >= 1 && d->num_mel_bins <= 128 && d->sample_rate > 0;
}

extern "C" {

size_t vp_logmel_workspace_bytes(const vp_logmel_desc* d) {
  if (!logmel_ok(d)) return 0;
  vp_logmel h{};
  h.d = *d;
  return logmel_carve(&h, nullptr);
}

int vp_logmel_frames(const vp_logmel_desc* d) { return logmel_ok(d) ? 1 + (d->samples - d->win_length) / d->hop_step : 0; }

int vp_logmel_create(const vp_logmel_desc* d, void* workspace, size_t bytes, void* stream, vp_logmel_t** out) {
  if (!logmel_ok(d) || !workspace || !out) { set_err("vp_logmel_create: bad argument"); return VP_ERR_ARG; }
  vp_logmel* h = new vp_logmel{};
  h->d = *d;
  if (bytes < logmel_carve(h, nullptr)) { delete h; set_err("vp_logmel_create: workspace too small"); return VP_ERR_WORKSPACE; }
  logmel_carve(h, (char*)workspace);
  hipStream_t st = (hipStream_t)stream;
  const int n = d->win_length, nb = h->nb;
  // constants in double, stored as f32: periodic Hann, DFT matrix [n][cos 0..nb-1 | -sin 0..nb-1 | 0], HTK mel matrix
  std::vector<float> win(n), dft((size_t)n * h->ncol, 0.f), mel((size_t)nb * d->num_mel_bins, 0.f);
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < n; ++i) win[i] = (float)(0.5 - 0.5 * cos(2.0 * PI * i / n));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < nb; ++k) {
      const double ang = 2.0 * PI * (double)(((long long)i * k) % n) / n;
      dft[(size_t)i * h->ncol + k] = (float)cos(ang);
      dft[(size_t)i * h->ncol + nb + k] = (float)(-sin(ang));
    }
  // tf.signal.linear_to_mel_weight_matrix (HTK mel, DC row zero, triangles in the mel domain)
  auto hz2mel = [](double f) { return 1127.0 * log1p(f / 700.0); };
  const double lo = hz2mel(d->lower_hz), hi = hz2mel(d->upper_hz);
  for (int k = 1; k < nb; ++k) {
    const double m = hz2mel((double)k * (d->sample_rate / 2.0) / (nb - 1));
    for (int j = 0; j < d->num_mel_bins; ++j) {
      const double e0 = lo + (hi - lo) * j / (d->num_mel_bins + 1), e1 = lo + (hi - lo) * (j + 1) / (d->num_mel_bins + 1),
                   e2 = lo + (hi - lo) * (j + 2) / (d->num_mel_bins + 1);
      const double v = fmin((m - e0) / (e1 - e0), (e2 - m) / (e2 - e1));
      mel[(size_t)k * d->num_mel_bins + j] = (float)(v > 0 ? v : 0);
    }
  }
  std::vector<float> t256(512), t512(514);
  for (int i = 0; i < 256; ++i) { t256[2 * i] = (float)cos(2.0 * PI * i / 256); t256[2 * i + 1] = (float)(-sin(2.0 * PI * i / 256)); }
  for (int i = 0; i < 257; ++i) { t512[2 * i] = (float)cos(2.0 * PI * i / 512); t512[2 * i + 1] = (float)(-sin(2.0 * PI * i / 512)); }
  VP_HIP_CHECK(hipMemcpyAsync(h->w256, t256.data(), t256.size() * 4, hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->w512, t512.data(), t512.size() * 4, hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->window, win.data(), win.size() * 4, hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->dft, dft.data(), dft.size() * 4, hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->mel, mel.data(), mel.size() * 4, hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipMemsetAsync(h->zeros, 0, 256, st));
  VP_HIP_CHECK(hipStreamSynchronize(st));   // host staging vectors die here
  VP_HIP_CHECK(launch_pack_weights_one(h->plan.pack, h->dft, h->packed, 0, st));
  *out = h;
  return VP_OK;
}

void vp_logmel_destroy(vp_logmel_t* h) { delete h; }

int vp_logmel_forward(vp_logmel_t* h, const float* pcm, float* out, void* stream) {
  if (!h || !pcm || !out) { set_err("vp_logmel_forward: null argument"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const vp_logmel_desc& d = h->d;
  const int P = d.batch * h->frames;
  if (h->fused) {
    VP_HIP_CHECK(launch_logmel512(pcm, h->window, h->w256, h->w512, h->mel, out, d.batch, d.samples, h->frames, d.hop_step, d.num_mel_bins, st));
    return VP_OK;
  }
  VP_HIP_CHECK(launch_frame_window(pcm, h->window, h->frames_buf, d.batch, d.samples, h->frames, d.win_length, d.hop_step, st));
  IgemmArgs a = h->plan.a;
  set_single_src(a.x, h->frames_buf, d.win_length, nullptr, nullptr, ACT_NONE, 0);
  a.Wp = h->packed; a.Y = h->spec; a.ldY = h->ncol; a.partial = (float*)h->scratch; a.zeros = h->zeros;
  VP_HIP_CHECK(launch_igemm(a, 0, h->plan.cfg, st));
  VP_HIP_CHECK(launch_mag_mel_log(h->spec, h->ncol, h->nb, h->mel, d.num_mel_bins, out, P, st));
  return VP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// BFMNet inference
// ------------------------------------------------------------------------------------------------
namespace {

struct PInfo { std::string name; size_t off; int ndim; int64_t shape[4]; };

struct ConvBN {            // conv (or depthwise) + contrib batch_norm
  size_t w, beta, mean, var;   // offsets in the parameter arena
  size_t wn;                   // number of weights
  int C;                       // output channels
  size_t wf, bf;               // offsets in the folded arena
};

struct Block {
  int cin, cexp, cout;
  bool pool, shortcut;
  bool fusable;          // depthwise + projection in one kernel (bfm_dwproj.hip): float32 trunk, mel width <= 20
  ConvBN expand, dw, project, sc;
  Gemm g_expand, g_project, g_sc;
};

struct BfmModel {
  std::vector<PInfo> manifest;
  size_t nparams = 0, nfolded = 0;
  ConvBN stem, last;
  Gemm g_last;
  std::vector<Block> blocks;
  std::vector<ConvBN*> folds;
  size_t enc_w, enc_b, rnn_w, rnn_b, gk, gb, ck, cb, d0w, d0b, d1w, d1b, d2w, d2b;
  Gemm g_enc, g_rnn, g_xg, g_xc, g_d0, g_d1, g_d2;
};

size_t add_p(BfmModel& m, const std::string& name, std::initializer_list<int64_t> shape) {
  PInfo p;
  p.name = name; p.off = m.nparams; p.ndim = (int)shape.size();
  size_t cnt = 1; int i = 0;
  for (auto s : shape) { p.shape[i++] = s; cnt *= (size_t)s; }
  for (; i < 4; ++i) p.shape[i] = 1;
  m.nparams += cnt;
  m.manifest.push_back(p);
  return p.off;
}

ConvBN add_conv_bn(BfmModel& m, const std::string& scope, const char* wname, std::initializer_list<int64_t> wshape, int C) {
  ConvBN c{};
  c.w = add_p(m, scope + "/" + wname, wshape);
  c.wn = 1;
  for (auto s : wshape) c.wn *= (size_t)s;
  const std::string bn = scope.substr(0, scope.rfind('/')) + "/BatchNorm/";
  c.beta = add_p(m, bn + "beta", {C});
  c.mean = add_p(m, bn + "moving_mean", {C});
  c.var = add_p(m, bn + "moving_variance", {C});
  c.C = C;
  c.wf = m.nfolded; m.nfolded += c.wn;
  c.bf = m.nfolded; m.nfolded += (size_t)C;
  return c;
}

void build_model(BfmModel& m) {
  const std::string P = "mfcc_encoder/MfccNet/";
  m.stem = add_conv_bn(m, P + "block0_0/conv2d/conv2d", "kernel", {9, 5, 1, 32}, 32);
  struct Spec { const char* scope; int cout, exp; bool pool; };
  static const Spec specs[] = {{"block1_0", 64, 1, false}, {"block2_0", 64, 6, true}, {"block2_1", 64, 6, false},
                               {"block3_0", 128, 6, true}, {"block3_1", 128, 6, false}, {"block3_2", 128, 6, false},
                               {"block4_0", 192, 6, true}, {"block4_1", 192, 6, false}, {"block4_2", 192, 6, false}, {"block4_3", 192, 6, false},
                               {"block5_0", 256, 6, false}, {"block5_1", 256, 6, false}, {"block5_2", 256, 6, false},
                               {"block6_0", 256, 6, true}, {"block6_1", 256, 6, false}, {"block6_2", 256, 6, false},
                               {"block7_0", 256, 6, false}};
  int cin = 32;
  m.blocks.reserve(32);
  for (const Spec& s : specs) {
    Block b{};
    b.cin = cin; b.cexp = cin * s.exp; b.cout = s.cout; b.pool = s.pool; b.shortcut = s.cout != cin;
    const std::string B = P + s.scope;
    b.expand = add_conv_bn(m, B + "/expansion_1x1_conv2d/conv2d", "kernel", {1, 1, cin, b.cexp}, b.cexp);
    // depthwise: variable scope .../depthwise_conv2d/SeparableConv2d/depthwise_weights, BN at .../depthwise_conv2d/BatchNorm
    b.dw = add_conv_bn(m, B + "/depthwise_conv2d/SeparableConv2d", "depthwise_weights", {7, 3, b.cexp, 1}, b.cexp);
    b.project = add_conv_bn(m, B + "/projection_1x1_conv2d/conv2d", "kernel", {1, 1, b.cexp, s.cout}, s.cout);
    if (b.shortcut) b.sc = add_conv_bn(m, B + "/1x1_conv2d/conv2d", "kernel", {1, 1, cin, s.cout}, s.cout);
    m.blocks.push_back(b);
    cin = s.cout;
  }
  m.last = add_conv_bn(m, P + "block8_0/conv2d/conv2d", "kernel", {1, 1, cin, 256}, 256);
  m.enc_w = add_p(m, "mfcc_encoder/dense/kernel", {256, 256}); m.enc_b = add_p(m, "mfcc_encoder/dense/bias", {256});
  m.rnn_w = add_p(m, "rnn_module/dense/kernel", {256, 256}); m.rnn_b = add_p(m, "rnn_module/dense/bias", {256});
  const std::string G = "rnn_module/rnn/multi_rnn_cell/cell_0/gru_cell/";
  m.gk = add_p(m, G + "gates/kernel", {512, 512}); m.gb = add_p(m, G + "gates/bias", {512});
  m.ck = add_p(m, G + "candidate/kernel", {512, 256}); m.cb = add_p(m, G + "candidate/bias", {256});
  m.d0w = add_p(m, "bfm_coeff_decoder/dense/kernel", {256, 128}); m.d0b = add_p(m, "bfm_coeff_decoder/dense/bias", {128});
  m.d1w = add_p(m, "bfm_coeff_decoder/dense_1/kernel", {128, 64}); m.d1b = add_p(m, "bfm_coeff_decoder/dense_1/bias", {64});
  m.d2w = add_p(m, "bfm_coeff_decoder/dense_2/kernel", {64, 64}); m.d2b = add_p(m, "bfm_coeff_decoder/dense_2/bias", {64});
}

}  // namespace

struct vp_bfmnet {
  vp_bfmnet_desc d;
  BfmModel m;
  const float* params;
  float* folded;
  char* packed;
  size_t packed_elems;
  void* nb16;            // bf16 copy of the current narrow trunk tensor (bf16-trunk mode: operand of the expansion / shortcut convs)
  float *mf, *n0, *n1, *ex, *dwb, *pooled, *enc, *c1, *xg, *xc, *rnn, *dd0, *dd1;
  char* scratch;
  size_t scratch_bytes;
  void* zeros;
  bool dirty;
  int T5, Wm[6];
  const float *drop0, *drop1;   // opt-in: the reference's unconditional decoder dropout (bfmnet.py:114,116) as explicit masks
  const vp_bfmnet* like;        // streaming-group bucket plans: every GEMM reduces its rows as this plan's does (IgemmPin); null otherwise
};

namespace {

void plan_gemm(vp_bfmnet* h, Gemm& g, int pixels, int cin, int cout, int which, size_t w_src, int src_ld, size_t bias, int bf = 0, const Gemm* like = nullptr) {
  g.cin = cin; g.cout = cout; g.which = which; g.w_src = w_src; g.src_ld = src_ld; g.bias = bias; g.bf = bf;
  ConvGeomX geo = make_geom(0, 1, 1, 0, 1, pixels, 1, cin, cin, cout);
  const IgemmPin pin = like ? IgemmPin{like->plan.cfg, like->plan.a.splitk} : IgemmPin{};
  g.plan = plan_fwd(geo, w_src, bf, like ? &pin : nullptr);
  g.plan.pack.s_ch = src_ld;      // row stride of the [cin, cout] source matrix (HWIO with H = W = 1)
  g.pk = h->packed_elems;         // (bytes: the arena mixes bf16 and f32 blocks; every block is packed relative to its own base)
  g.plan.pack.dst_off = 0;
  h->packed_elems += align256(g.plan.pack_elems * (bf ? 2 : 4));
  if (g.plan.partial_bytes > h->scratch_bytes) h->scratch_bytes = g.plan.partial_bytes;
}

size_t bfm_carve(vp_bfmnet* h, char* base) {
  Arena ar(base);
  const int B = h->d.batch, T = h->d.frames;
  h->T5 = 5 * T;
  BfmModel& m = h->m;
  h->packed_elems = 0; h->scratch_bytes = 0;
  // mel widths: 80 -> 40 (stem stride 2) -> 20 -> 10 -> 5 -> 3 (SAME pools after block2_0, 3_0, 4_0, 6_0)
  int W = (h->d.num_mel_bins + 1) / 2;
  size_t max_net = 0, max_exp = 0;
  const int tb = h->d.trunk_dtype == VP_BF16 ? 1 : 0;      // MfccNet activations / 1x1-conv operands in bf16 (f32 accumulation)
  const size_t tes = tb ? 2 : 4;
  const BfmModel* lm = h->like ? &h->like->m : nullptr;     // (same layer table: the i-th GEMM of both plans is the same layer)
  for (size_t bi = 0; bi < m.blocks.size(); ++bi) {
    Block& b = m.blocks[bi];
    const Block* lb = lm ? &lm->blocks[bi] : nullptr;
    const int P = B * h->T5 * W;
    plan_gemm(h, b.g_expand, P, b.cin, b.cexp, 0, b.expand.wf, b.cexp, b.expand.bf, tb, lb ? &lb->g_expand : nullptr);
    plan_gemm(h, b.g_project, P, b.cexp, b.cout, 0, b.project.wf, b.cout, b.project.bf, tb, lb ? &lb->g_project : nullptr);
    // (the fused kernel addresses the expanded tensor with 32-bit lane offsets - launch_dwproj refuses 0xF0000000 bytes and more: very long
    // clips fall back to the depthwise kernel + the GEMM here, at plan time, instead of failing at run time: ADVICE r5)
    b.fusable = !tb && dwproj_eligible(W, b.cexp, b.cout) && (size_t)P * b.cexp * sizeof(float) < 0xF0000000ull;
    if (b.fusable) { b.g_project.plan.pack.perm = 0; b.g_project.plan.a.rowperm = 0; }     // (the fused kernel reads plain packed rows; the GEMM kernels take either)
    if (b.shortcut) plan_gemm(h, b.g_sc, P, b.cin, b.cout, 0, b.sc.wf, b.cout, b.sc.bf, tb, lb ? &lb->g_sc : nullptr);
    if ((size_t)P * b.cexp > max_exp) max_exp = (size_t)P * b.cexp;
    if ((size_t)P * (b.cin > b.cout ? b.cin : b.cout) > max_net) max_net = (size_t)P * (b.cin > b.cout ? b.cin : b.cout);
    if (b.pool) W = (W + 1) / 2;
  }
  plan_gemm(h, m.g_last, B * h->T5 * W, 256, 256, 0, m.last.wf, 256, m.last.bf, tb, lm ? &lm->g_last : nullptr);
  const int BT = B * T;
  plan_gemm(h, m.g_enc, BT, 256, 256, 1, m.enc_w, 256, m.enc_b, 0, lm ? &lm->g_enc : nullptr);
  plan_gemm(h, m.g_rnn, BT, 256, 256, 1, m.rnn_w, 256, m.rnn_b, 0, lm ? &lm->g_rnn : nullptr);
  plan_gemm(h, m.g_xg, BT, 256, 512, 1, m.gk, 512, m.gb, 0, lm ? &lm->g_xg : nullptr);       // rows 0..255 of the [512,512] gate kernel (the x part)
  plan_gemm(h, m.g_xc, BT, 256, 256, 1, m.ck, 256, m.cb, 0, lm ? &lm->g_xc : nullptr);
  plan_gemm(h, m.g_d0, BT, 256, 128, 1, m.d0w, 128, m.d0b, 0, lm ? &lm->g_d0 : nullptr);
  plan_gemm(h, m.g_d1, BT, 128, 64, 1, m.d1w, 64, m.d1b, 0, lm ? &lm->g_d1 : nullptr);
  plan_gemm(h, m.g_d2, BT, 64, 64, 1, m.d2w, 64, m.d2b, 0, lm ? &lm->g_d2 : nullptr);
  h->folded = (float*)ar.alloc(m.nfolded * sizeof(float));
  h->packed = (char*)ar.alloc(h->packed_elems);
  h->n0 = (float*)ar.alloc(max_net * sizeof(float));      // the residual stream stays f32 in both modes
  h->n1 = (float*)ar.alloc(max_net * sizeof(float));
  h->nb16 = ar.alloc(max_net * 2);
  h->ex = (float*)ar.alloc(max_exp * tes);
  h->dwb = (float*)ar.alloc(max_exp * tes);
  h->pooled = (float*)ar.alloc((size_t)BT * 256 * 4);
  h->enc = (float*)ar.alloc((size_t)BT * 256 * 4);
  h->c1 = (float*)ar.alloc((size_t)BT * 256 * 4);
  h->xg = (float*)ar.alloc((size_t)BT * 512 * 4);
  h->xc = (float*)ar.alloc((size_t)BT * 256 * 4);
  h->rnn = (float*)ar.alloc((size_t)BT * 256 * 4);
  h->dd0 = (float*)ar.alloc((size_t)BT * 128 * 4);
  h->dd1 = (float*)ar.alloc((size_t)BT * 64 * 4);
  h->scratch = (char*)ar.alloc(h->scratch_bytes + 256);
  h->zeros = ar.alloc(256);
  return ar.total();
}

bool bfm_ok(const vp_bfmnet_desc* d) {
  return d && d->batch >= 1 && d->frames >= 1 && d->num_mel_bins == 80 && (d->trunk_dtype == VP_F32 || d->trunk_dtype == VP_BF16);
}

int run_gemm(vp_bfmnet* h, Gemm& g, const void* x, void* y, int act, int accumulate, hipStream_t st, int y_f32 = 0) {
  IgemmArgs a = g.plan.a;
  a.y_f32 = (g.bf && y_f32) ? 1 : 0;           // bf16 operands, f32 result (residual stream / head inputs)
  set_single_src(a.x, x, g.cin, nullptr, nullptr, ACT_NONE, 0);
  a.Wp = h->packed + g.pk;
  a.Y = y; a.ldY = g.cout;
  a.bias = (g.which == 0 ? h->folded : h->params) + g.bias;
  a.out_act = act; a.accumulate = accumulate;
  a.partial = (float*)h->scratch; a.zeros = h->zeros;
  VP_HIP_CHECK(launch_igemm(a, g.bf, g.plan.cfg, st));
  return VP_OK;
}

int prepare_weights(vp_bfmnet* h, hipStream_t st) {
  BfmModel& m = h->m;
  auto fold = [&](const ConvBN& c) -> hipError_t {
    return launch_fold_bn(h->params + c.w, h->params + c.beta, h->params + c.mean, h->params + c.var, 1e-3f, c.wn, c.C,
                          h->folded + c.wf, h->folded + c.bf, st);
  };
  VP_HIP_CHECK(fold(m.stem));
  for (Block& b : m.blocks) {
    VP_HIP_CHECK(fold(b.expand)); VP_HIP_CHECK(fold(b.dw)); VP_HIP_CHECK(fold(b.project));
    if (b.shortcut) VP_HIP_CHECK(fold(b.sc));
  }
  VP_HIP_CHECK(fold(m.last));
  auto pack = [&](Gemm& g) -> hipError_t {
    return launch_pack_weights_one(g.plan.pack, g.which == 0 ? h->folded : h->params, h->packed + g.pk, g.bf, st);
  };
  for (Block& b : m.blocks) {
    VP_HIP_CHECK(pack(b.g_expand)); VP_HIP_CHECK(pack(b.g_project));
    if (b.shortcut) VP_HIP_CHECK(pack(b.g_sc));
  }
  for (Gemm* g : {&m.g_last, &m.g_enc, &m.g_rnn, &m.g_xg, &m.g_xc, &m.g_d0, &m.g_d1, &m.g_d2}) VP_HIP_CHECK(pack(*g));
  h->dirty = false;
  return VP_OK;
}

}  // namespace

extern "C" {

size_t vp_bfmnet_param_count(void) { BfmModel m; build_model(m); return m.nparams; }

int vp_bfmnet_param_info(int index, char* name, int name_cap, size_t* offset, int* ndim, int64_t shape[4]) {
  BfmModel m;
  build_model(m);
  if (index < 0 || index >= (int)m.manifest.size()) return VP_ERR_ARG;
  const PInfo& p = m.manifest[index];
  if (name && name_cap > 0) { strncpy(name, p.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = p.off;
  if (ndim) *ndim = p.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  return VP_OK;
}

size_t vp_bfmnet_workspace_bytes(const vp_bfmnet_desc* d) {
  if (!bfm_ok(d)) return 0;
  vp_bfmnet* h = new vp_bfmnet{};
  h->d = *d;
  build_model(h->m);
  const size_t n = bfm_carve(h, nullptr);
  delete h;
  return n;
}

int vp_bfmnet_create(const vp_bfmnet_desc* d, void* workspace, size_t bytes, const float* params, void* stream, vp_bfmnet_t** out) {
  if (!bfm_ok(d) || !workspace || !params || !out) { set_err("vp_bfmnet_create: bad argument"); return VP_ERR_ARG; }
  vp_bfmnet* h = new vp_bfmnet{};
  h->d = *d;
  build_model(h->m);
  if (bytes < bfm_carve(h, nullptr)) { delete h; set_err("vp_bfmnet_create: workspace too small"); return VP_ERR_WORKSPACE; }
  bfm_carve(h, (char*)workspace);
  h->params = params;
  h->dirty = true;
  VP_HIP_CHECK(hipMemsetAsync(h->zeros, 0, 256, (hipStream_t)stream));
  *out = h;
  return VP_OK;
}

void vp_bfmnet_destroy(vp_bfmnet_t* h) { delete h; }

int vp_bfmnet_params_changed(vp_bfmnet_t* h) { if (!h) return VP_ERR_ARG; h->dirty = true; return VP_OK; }

}  // extern "C"

// The forward in stages (the streaming executor below runs the same stages on a window plan, with its own recurrence between them):
// bfm_trunk: mfccs [B,5T,80] -> MfccNet -> MfccEncoder -> RNNModule dense -> the GRU's input projections h->xg / h->xc
static int bfm_trunk(vp_bfmnet* h, const float* mfccs, hipStream_t st) {
  int rc;
  if (h->dirty && (rc = prepare_weights(h, st))) return rc;
  BfmModel& m = h->m;
  const int B = h->d.batch, T = h->d.frames, H = h->T5;
  int W = h->d.num_mel_bins, pl, Wo;
  // stem: conv [9,5] stride [1,2] SAME on [B, 5T, 80, 1]
  same_pad(W, 5, 2, &pl, &Wo);
  // bf16-trunk mode: the 6x-expanded tensors (ex, dwb: the bytes of this network) and every 1x1-conv operand are bf16; the narrow
  // residual stream (block inputs / outputs) stays f32 so that rounding does not compound over the 17 blocks - an expansion conv
  // reads a bf16 COPY of it (nb16), the projection conv adds its f32 result into it
  const int tb = h->d.trunk_dtype == VP_BF16 ? 1 : 0;
  VP_HIP_CHECK(launch_conv_first(mfccs, h->folded + m.stem.wf, h->folded + m.stem.bf, h->n0, 0, B, H, W, Wo, 32, 4, pl, st));
  W = Wo;
  float* cur = h->n0;
  float* alt = h->n1;
  auto operand = [&](const float* t, int c) -> const void* {      // what a trunk GEMM reads for the narrow tensor t
    if (!tb) return t;
    (void)launch_cvt_f32_bf16(t, h->nb16, (size_t)B * H * W * c, st);
    return h->nb16;
  };
  for (Block& b : m.blocks) {
    const void* xin = operand(cur, b.cin);
    if ((rc = run_gemm(h, b.g_expand, xin, h->ex, ACT_RELU6, 0, st))) return rc;
    // depthwise + projection: one kernel where the block is fusable (the depthwise result never reaches HBM), else two
    const bool fused = b.fusable && bfm_dwproj_knob();
    auto dw_project = [&](float* dst) -> int {
      if (fused) {
        VP_HIP_CHECK(launch_dwproj(h->ex, h->folded + b.dw.wf, (const float*)(h->packed + b.g_project.pk), b.g_project.plan.a.wp_rows, h->folded + b.project.bf, dst, 1,
                                   B, H, W, b.cexp, b.cout, st));
        return VP_OK;
      }
      VP_HIP_CHECK(launch_dwconv7x3(h->ex, h->folded + b.dw.wf, h->folded + b.dw.bf, h->dwb, tb, B, H, W, b.cexp, st));
      return run_gemm(h, b.g_project, h->dwb, dst, ACT_NONE, 1, st, 1);
    };
    if (b.shortcut) {
      if ((rc = run_gemm(h, b.g_sc, xin, alt, ACT_NONE, 0, st, 1))) return rc;
      if ((rc = dw_project(alt))) return rc;
      float* t = cur; cur = alt; alt = t;
    } else {
      if ((rc = dw_project(cur))) return rc;   // residual add in place
    }
    if (b.pool) {   // max_pooling2d([2,2], strides [1,2], 'same'): time pad (0,1), mel pad (0, W odd)
      const int Wn = (W + 1) / 2;
      VP_HIP_CHECK(launch_maxpool_same(cur, alt, 0, 0, B, H, W, b.cout, 2, 2, 1, 2, 0, 0, H, Wn, st));
      float* t = cur; cur = alt; alt = t;
      W = Wn;
    }
  }
  if ((rc = run_gemm(h, m.g_last, operand(cur, 256), alt, ACT_RELU, 0, st, 1))) return rc;
  // MfccEncoder pool [5,3] stride [5,3] SAME -> [B, T, 1, 256]  (bfmnet.py:35)
  {
    int pt, ph, pw2, wo2;
    same_pad(H, 5, 5, &pt, &ph);
    same_pad(W, 3, 3, &pw2, &wo2);
    if (ph != T || wo2 != 1) { set_err("vp_bfmnet_forward: unexpected pooled size %dx%d", ph, wo2); return VP_ERR_STATE; }
    VP_HIP_CHECK(launch_maxpool_same(alt, h->pooled, 0, 0, B, H, W, 256, 5, 3, 5, 3, pt, pw2, ph, wo2, st));
  }
  if ((rc = run_gemm(h, m.g_enc, h->pooled, h->enc, ACT_LEAKY, 0, st))) return rc;
  if ((rc = run_gemm(h, m.g_rnn, h->enc, h->c1, ACT_LEAKY, 0, st))) return rc;
  if ((rc = run_gemm(h, m.g_xg, h->c1, h->xg, ACT_NONE, 0, st))) return rc;
  if ((rc = run_gemm(h, m.g_xc, h->c1, h->xc, ACT_NONE, 0, st))) return rc;
  return VP_OK;
}

// recurrent halves of the GRU's gate / candidate kernels (rows 256..511 of each)
static const float* gru_whg(vp_bfmnet* h) { return h->params + h->m.gk + (size_t)256 * 512; }
static const float* gru_whc(vp_bfmnet* h) { return h->params + h->m.ck + (size_t)256 * 256; }

// bfm_decode: h->rnn [B,T,256] -> BFMCoeffDecoder -> out [B,T,64] (+ ears [B,T,1] when given)
static int bfm_decode(vp_bfmnet* h, const float* ears, float* out, hipStream_t st) {
  int rc;
  BfmModel& m = h->m;
  const int B = h->d.batch, T = h->d.frames;
  if ((rc = run_gemm(h, m.g_d0, h->rnn, h->dd0, ACT_LEAKY, 0, st))) return rc;
  if (h->drop0) VP_HIP_CHECK(launch_mul_inplace(h->dd0, h->drop0, (size_t)B * T * 128, st));
  if ((rc = run_gemm(h, m.g_d1, h->dd0, h->dd1, ACT_LEAKY, 0, st))) return rc;
  if (h->drop1) VP_HIP_CHECK(launch_mul_inplace(h->dd1, h->drop1, (size_t)B * T * 64, st));
  if ((rc = run_gemm(h, m.g_d2, h->dd1, out, ACT_NONE, 0, st))) return rc;
  if (ears) VP_HIP_CHECK(launch_add_ears(out, ears, B * T, st));
  return VP_OK;
}

extern "C" {

int vp_bfmnet_forward(vp_bfmnet_t* h, const float* ears, const float* mfccs, const int* seq_len, float* out, void* stream) {
  if (!h || !ears || !mfccs || !seq_len || !out) { set_err("vp_bfmnet_forward: null argument"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = bfm_trunk(h, mfccs, st))) return rc;
  VP_HIP_CHECK(launch_gru_seq(h->xg, h->xc, gru_whg(h), gru_whc(h), seq_len, h->rnn, h->d.batch, h->d.frames, st));
  return bfm_decode(h, ears, out, st);
}

int vp_bfmnet_set_decoder_dropout(vp_bfmnet_t* h, const float* mask0, const float* mask1) {
  if (!h) { set_err("vp_bfmnet_set_decoder_dropout: null handle"); return VP_ERR_ARG; }
  h->drop0 = mask0; h->drop1 = mask1;
  return VP_OK;
}

int vp_bfmnet_tensor(vp_bfmnet_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) return VP_ERR_ARG;
  const std::string s(name);
  const int B = h->d.batch, T = h->d.frames;
  float* p = nullptr; int c = 256;
  if (s == "MfccEncoder") p = h->enc;
  else if (s == "RNNModule") p = h->rnn;
  else if (s == "pooled") p = h->pooled;
  else return VP_ERR_ARG;
  *ptr = p;
  if (shape) { shape[0] = B; shape[1] = T; shape[2] = c; shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Streaming BFMNet inference (include/vp_hip.h, vp_bfmstream_group_* and vp_bfmstream_*).  One executor: a group of S independent
// sessions ("slots") behind one handle; a vp_bfmstream is a group of one slot.  A push runs, per round, ONE launch chain for all the
// slots that take part in it:
//   pieces:  each slot's next piece of samples (at most 5 max_chunk_frames mel frames' worth) behind its carried samples (< 512: the
//            start of its next mel frame) -> a staging matrix -> logmel512_kernel (batch = the pieces) -> mel_scatter_group_kernel ->
//            each slot's mel ring
//   windows: the slots with frames ready, compacted to batch rows 0..A-1 -> mel_window_group_kernel (rows not received yet are zero)
//            -> bfm_trunk on the bucket plan of batch >= A (1, 2, 4, .., S) -> gru_state_group_kernel (each slot's state, over the
//            emitted frames only) -> bfm_decode -> rows_scatter_group_kernel -> the packed output; the ears are added once per push
// A frame f is emitted before finish once mel rows up to 5f + 4 + R have arrived; its window starts Lf frames before the first emitted
// frame (or at the clip start) and reaches Rf frames past the last, so every emitted frame sees exactly what the offline forward shows
// it.  At finish the window's right edge sits at pad_len, where the offline sequence ends (its SAME padding); a finished clip shorter
// than T_win runs its last frames on an exact-size plan instead, in rounds of its own (A = B = 1).
// Every kernel of the chain computes a batch row as the batch-1 window plan computes its one row: the bucket plans pin each GEMM's tile
// and K split to the batch-1 plan's (IgemmPin), the stem, depthwise, depthwise + projection and pooling kernels are per pixel.  So a
// slot's coefficients do not depend on the slots that share its rounds: they are those of a one-slot group, a vp_bfmstream, fed the
// same chunks.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int kHop = 128, kWin = 512, kMelPerFrame = 5, kSamplesPerFrame = kHop * kMelPerFrame;
constexpr int kMaxChunkFrames = 1024;

struct StreamGeo { int L, R, Lf, Rf, Tw, cap, piece; };

// receptive field of a pooled frame's mel rows, from the layer table: the stem's SAME time padding, each block's depthwise SAME
// padding, each SAME max-pool's (stride 1 in time: pads (0, k - 1)); the MfccEncoder pool is aligned to frames (5 rows, stride 5)
void receptive_field(const BfmModel& m, int* L, int* R) {
  auto kt = [&](size_t off) {
    for (const PInfo& p : m.manifest) if (p.off == off) return (int)p.shape[0];
    return 1;
  };
  int l = 0, r = 0, pb, o;
  int k = kt(m.stem.w);
  same_pad(1 << 20, k, 1, &pb, &o); l += pb; r += k - 1 - pb;
  for (const Block& b : m.blocks) {
    k = kt(b.dw.w);
    same_pad(1 << 20, k, 1, &pb, &o); l += pb; r += k - 1 - pb;
    if (b.pool) { same_pad(1 << 20, 2, 1, &pb, &o); l += pb; r += 2 - 1 - pb; }
  }
  *L = l; *R = r;
}

bool stream_ok(const vp_bfmstream_desc* d) {
  return d && d->struct_bytes == (int)sizeof(vp_bfmstream_desc) && d->max_chunk_frames >= 1 && d->max_chunk_frames <= kMaxChunkFrames &&
         d->num_mel_bins == 80 && (d->trunk_dtype == VP_F32 || d->trunk_dtype == VP_BF16) && d->sample_rate > 0 && d->lower_hz >= 0.f &&
         d->upper_hz > d->lower_hz && d->upper_hz <= d->sample_rate * 0.5f;
}

StreamGeo stream_geo(const vp_bfmstream_desc* d, const BfmModel& m) {
  StreamGeo g{};
  receptive_field(m, &g.L, &g.R);
  g.Lf = (g.L + kMelPerFrame - 1) / kMelPerFrame;
  g.Rf = (g.R + kMelPerFrame - 1) / kMelPerFrame;
  g.Tw = d->max_chunk_frames + g.Lf + g.Rf;
  g.piece = kMelPerFrame * d->max_chunk_frames;            // most mel frames one staging buffer yields
  // the ring keeps rows [5 w0, mel_done): before a piece that is < 5 Lf + R + 5 rows (the unemitted tail + the left context), a piece
  // adds `piece`; at finish the last window reads 5 Tw rows
  const int during = kMelPerFrame * g.Lf + g.R + kMelPerFrame + g.piece;
  // (finish appends its <= 8 rows of padding without emitting: the kMelPerFrame + 16 rows of slack cover them)
  g.cap = (during > kMelPerFrame * g.Tw ? during : kMelPerFrame * g.Tw) + 24;
  return g;
}

long long mel_avail(long long n) { return n >= kWin ? (n - kWin) / kHop + 1 : 0; }
long long pad_len_of(long long n) { return 1 + n / kSamplesPerFrame; }
long long emitted_after(const StreamGeo& g, long long n, bool fin) {
  if (fin) return pad_len_of(n);
  const long long M = mel_avail(n);
  return M >= kMelPerFrame + g.R ? (M - kMelPerFrame - g.R) / kMelPerFrame + 1 : 0;
}

size_t bfm_plan_bytes(vp_bfmnet* scratch, int frames) {
  scratch->d.frames = frames;
  return bfm_carve(scratch, nullptr);
}

struct GroupSlot { int cur, carry; long long samples, mel_done, emitted; bool finished; };

bool group_ok(const vp_bfmstream_group_desc* d, vp_bfmstream_desc* sd) {
  if (!d || d->struct_bytes != (int)sizeof(vp_bfmstream_group_desc) || d->slots < 1 || d->slots > kGroupMaxSlots) return false;
  *sd = vp_bfmstream_desc{(int)sizeof(vp_bfmstream_desc), d->max_chunk_frames, d->num_mel_bins, d->trunk_dtype, d->sample_rate, d->lower_hz, d->upper_hz};
  return stream_ok(sd);
}

std::vector<int> group_buckets(int S) {
  std::vector<int> b;
  for (int x = 1; x < S; x *= 2) b.push_back(x);
  b.push_back(S);
  return b;
}

void model_gemms(const BfmModel& m, std::vector<const Gemm*>& v) {
  for (const Block& b : m.blocks) {
    v.push_back(&b.g_expand); v.push_back(&b.g_project);
    if (b.shortcut) v.push_back(&b.g_sc);
  }
  for (const Gemm* g : {&m.g_last, &m.g_enc, &m.g_rnn, &m.g_xg, &m.g_xc, &m.g_d0, &m.g_d1, &m.g_d2}) v.push_back(g);
}

// the bucket plans (not carved yet) and the bytes of their shared region.  Refuses (VP_ERR_ARG) a group whose larger buckets would leave
// the batch-1 plan's kernels: the depthwise + projection kernel's and the GEMM loader's 32-bit lane offsets (bfm_dwproj.hip, conv_kernels.hip)
int group_plans(const vp_bfmstream_desc& sd, int S, const StreamGeo& g, std::vector<vp_bfmnet*>& plans, size_t* bytes) {
  *bytes = 0;
  for (int B : group_buckets(S)) {
    vp_bfmnet* p = new vp_bfmnet{};
    p->d = vp_bfmnet_desc{B, g.Tw, sd.num_mel_bins, sd.trunk_dtype};
    build_model(p->m);
    p->like = plans.empty() ? nullptr : plans[0];
    const size_t n = bfm_carve(p, nullptr);
    plans.push_back(p);
    if (n > *bytes) *bytes = n;
    const vp_bfmnet* r = plans[0];
    std::vector<const Gemm*> ga, gr;
    model_gemms(p->m, ga);
    model_gemms(r->m, gr);
    // the lane-offset limits first (a larger batch outgrowing them is the expected way to fail), then anything else that would make a
    // bucket run other kernels or another weight image than the batch-1 plan, named
    const char* lim = nullptr;
    int at = -1;
    auto big = [](const Gemm* x) { const IgemmArgs& a = x->plan.a; return (size_t)a.N * a.Hin * a.Win * a.Cin * (x->bf ? 2 : 4) >= 0x70000000ull; };
    for (size_t i = 0; !lim && i < ga.size() && i < gr.size(); ++i)
      if (big(ga[i]) != big(gr[i])) { lim = "the implicit-GEMM loader"; at = (int)i; }
    for (size_t i = 0; !lim && i < p->m.blocks.size(); ++i)
      if (p->m.blocks[i].fusable != r->m.blocks[i].fusable) { lim = "launch_dwproj"; at = (int)i; }
    if (lim) {
      set_err("vp_bfmstream_group: %d slots of %d-frame windows need a batch-%d plan whose tensors exceed the 32-bit lane offsets of %s "
              "(%s %d); use fewer slots or a smaller max_chunk_frames", S, g.Tw, B, lim, lim[0] == 'l' ? "block" : "GEMM", at);
      return VP_ERR_ARG;
    }
    const char* what = p->packed_elems != r->packed_elems || ga.size() != gr.size() ? "packed weight image" : nullptr;
    for (size_t i = 0; !what && i < ga.size(); ++i) {
      const IgemmPlan &a = ga[i]->plan, &b = gr[i]->plan;
      at = (int)i;
      if (a.cfg != b.cfg) what = "tile";
      else if (a.a.splitk != b.a.splitk) what = "K split";
      else if (a.a.kern != b.a.kern) what = "kernel";
      else if (ga[i]->pk != gr[i]->pk || memcmp(&a.pack, &b.pack, sizeof(PackDesc))) what = "weight packing";
    }
    if (what) {
      set_err("vp_bfmstream_group: the batch-%d plan of %d slots x %d-frame windows differs from the batch-1 plan in the %s (GEMM %d): its "
              "rows would not be the one-stream plan's", B, S, g.Tw, what, at);
      return VP_ERR_ARG;
    }
  }
  return VP_OK;
}

void free_plans(std::vector<vp_bfmnet*>& plans) {
  for (vp_bfmnet* p : plans) delete p;
  plans.clear();
}

}  // namespace

struct vp_bfmstream_group {
  vp_bfmstream_group_desc d;
  vp_bfmstream_desc sd;            // one slot's session descriptor
  StreamGeo g;
  const float* params;
  vp_logmel_t* lm;                 // constants of the log-mel kernel
  std::vector<vp_bfmnet*> plans;   // bucket plans of batch 1, 2, 4, .., S: carved on ONE region (they run in stream order), so they also
                                   // share one folded / packed weight image (same offsets, same packing: group_plans checks it)
  vp_bfmnet* shrt;                 // exact-size plan of a clip shorter than T_win, carved at finish
  char *lm_base, *plan_base, *short_base;
  size_t lm_bytes, plan_bytes, short_bytes;
  float *carry, *stage, *frames, *ring, *mwin, *hstate, *dout;   // [S][2][kGroupCarry], [S][stage_len], [S][piece][nmel], [S][cap][nmel],
                                   // [S][5 T_win][nmel], [S][256], [S][T_win][64]
  int stage_len;                   // kWin + kHop * piece: a piece with its carried samples
  void* zeros;                     // the bucket plans' 256 zero bytes (their own `zeros` lie in the shared region, overwritten by others)
  std::vector<GroupSlot> slot;
  bool dirty;
};

static size_t group_carve(vp_bfmstream_group* G, char* base, vp_logmel_desc* lmd) {
  Arena ar(base);
  const StreamGeo& g = G->g;
  const size_t S = G->d.slots, nmel = G->d.num_mel_bins;
  G->carry = (float*)ar.alloc(S * 2 * kGroupCarry * 4);
  G->stage_len = kWin + kHop * g.piece;
  G->stage = (float*)ar.alloc(S * G->stage_len * 4);
  G->frames = (float*)ar.alloc(S * g.piece * nmel * 4);
  G->ring = (float*)ar.alloc(S * g.cap * nmel * 4);
  G->mwin = (float*)ar.alloc(S * kMelPerFrame * g.Tw * nmel * 4);
  G->hstate = (float*)ar.alloc(S * 256 * 4);
  G->dout = (float*)ar.alloc(S * g.Tw * 64 * 4);
  G->zeros = ar.alloc(256);
  *lmd = vp_logmel_desc{G->d.sample_rate, G->d.num_mel_bins, kWin, kHop, kWin, G->d.lower_hz, G->d.upper_hz, 1, kWin};
  G->lm_bytes = vp_logmel_workspace_bytes(lmd);
  G->lm_base = (char*)ar.alloc(G->lm_bytes);
  G->plan_base = (char*)ar.alloc(G->plan_bytes);
  vp_bfmnet tmp{};
  tmp.d = vp_bfmnet_desc{1, g.Tw, G->d.num_mel_bins, G->d.trunk_dtype};
  build_model(tmp.m);
  size_t sb = 0;
  for (int t = 1; t < g.Tw; ++t) { const size_t b = bfm_plan_bytes(&tmp, t); if (b > sb) sb = b; }
  G->short_bytes = sb;
  G->short_base = (char*)ar.alloc(sb);
  return ar.total();
}

// the layout of a descriptor's group (plans made, nothing carved on memory); VP_ERR_ARG with the reason on a refused descriptor
static int group_layout(vp_bfmstream_group* G, const vp_bfmstream_group_desc* d, size_t* bytes) {
  if (!group_ok(d, &G->sd)) { set_err("vp_bfmstream_group: bad descriptor"); return VP_ERR_ARG; }
  G->d = *d;
  BfmModel m;
  build_model(m);
  G->g = stream_geo(&G->sd, m);
  int rc;
  if ((rc = group_plans(G->sd, d->slots, G->g, G->plans, &G->plan_bytes))) return rc;
  vp_logmel_desc lmd;
  *bytes = group_carve(G, nullptr, &lmd);
  return VP_OK;
}

static int group_prepare(vp_bfmstream_group* G, hipStream_t st) {
  if (!G->dirty) return VP_OK;
  int rc;
  if ((rc = prepare_weights(G->plans[0], st))) return rc;       // (the image every bucket plan reads)
  for (vp_bfmnet* p : G->plans) p->dirty = false;
  G->dirty = false;
  return VP_OK;
}

// one piece for each slot in `who` (left[s] samples still to go, from pcm + pos[s], or zeros when pcm is null) -> mel rows; one launch
static int group_pieces(vp_bfmstream_group* G, const float* pcm, std::vector<long long>& pos, std::vector<long long>& left, std::vector<int>& who,
                        hipStream_t st) {
  const long long most = (long long)kHop * G->g.piece;
  LmGroupTable tab;
  int ne = 0, maxF = 0, maxN = 0;
  who.clear();
  for (int s = 0; s < G->d.slots; ++s) {
    if (left[s] <= 0) continue;
    GroupSlot& z = G->slot[s];
    const int q = (int)(left[s] < most ? left[s] : most);
    const int ls = z.carry + q;
    const int F = ls >= kWin ? (ls - kWin) / kHop + 1 : 0;
    LmGroupEntry& e = tab.e[ne++];
    e.pcm_off = pcm ? (int)pos[s] : 0;
    e.ring_row = (int)(z.mel_done % G->g.cap);
    e.slot = (short)s; e.carry_n = (short)z.carry; e.F = (short)F; e.keep = (short)(ls - kHop * F);
    e.cur = (unsigned char)z.cur; e.zeros = pcm ? 0 : 1;
    if (F > maxF) maxF = F;
    if (ls > maxN) maxN = ls;
    z.mel_done += F; z.carry = ls - kHop * F; z.cur ^= 1; z.samples += q;
    pos[s] += q; left[s] -= q;
    who.push_back(s);
  }
  if (!ne) return VP_OK;
  const vp_logmel* lm = G->lm;
  VP_HIP_CHECK(launch_logmel512_group(pcm, G->carry, G->stage, G->stage_len, G->frames, G->ring, G->g.cap, lm->window, lm->w256, lm->w512, lm->mel,
                                      G->d.num_mel_bins, kHop, tab, ne, maxF, maxN, st));
  return VP_OK;
}

// the exact-size plan of a finished clip of pad frames (shorter than T_win), carved on its region of the workspace
static int short_plan(vp_bfmstream_group* G, int pad, hipStream_t st) {
  if (G->shrt && G->shrt->d.frames == pad) return VP_OK;
  delete G->shrt;
  G->shrt = new vp_bfmnet{};
  G->shrt->d = vp_bfmnet_desc{1, pad, G->d.num_mel_bins, G->d.trunk_dtype};
  build_model(G->shrt->m);
  if (bfm_carve(G->shrt, nullptr) > G->short_bytes) { set_err("vp_bfmstream_group: short plan outgrew its region"); return VP_ERR_STATE; }
  bfm_carve(G->shrt, G->short_base);
  G->shrt->params = G->params;
  G->shrt->dirty = true;
  VP_HIP_CHECK(hipMemsetAsync(G->shrt->zeros, 0, 256, st));
  return VP_OK;
}

// the window of Tw frames that emits slot s's frames [f0, f0 + n): it starts Lf frames before f0 (or at the clip start) and, at finish,
// ends at pad_len at the latest.  *w0: its first frame
static int place_window(const vp_bfmstream_group* G, int s, long long f0, int n, int Tw, bool fin, long long* w0) {
  const GroupSlot& z = G->slot[s];
  const long long pad = pad_len_of(z.samples);
  long long w = f0 - G->g.Lf > 0 ? f0 - G->g.Lf : 0;
  if (fin && w + Tw > pad) w = pad - Tw > 0 ? pad - Tw : 0;
  if ((long long)kMelPerFrame * w < z.mel_done - G->g.cap) { set_err("vp_bfmstream_group: slot %d window %lld left the mel history", s, w); return VP_ERR_STATE; }
  if (f0 < w || f0 + n > w + Tw) { set_err("vp_bfmstream_group: slot %d frames [%lld, %lld) outside window %lld + %d", s, f0, f0 + n, w, Tw); return VP_ERR_STATE; }
  *w0 = w;
  return VP_OK;
}

// one round on plan p (batch >= act.size()): the next (at most max_chunk_frames) frames up to target[s] of every slot s in act, out rows of
// slot s from row[s] on
static int group_round(vp_bfmstream_group* G, vp_bfmnet* p, const std::vector<int>& act, const std::vector<long long>& target, bool fin, float* out,
                       std::vector<long long>& row, hipStream_t st) {
  const StreamGeo& g = G->g;
  const int A = (int)act.size(), Tw = p->d.frames;
  WinGroupTable win;
  RowsGroupTable rows;
  int most = 0, rc;
  for (int b = 0; b < A; ++b) {
    const int s = act[b];
    GroupSlot& z = G->slot[s];
    const long long f0 = z.emitted;
    const int n = (int)(target[s] - f0 < G->d.max_chunk_frames ? target[s] - f0 : G->d.max_chunk_frames);
    long long w0;
    if ((rc = place_window(G, s, f0, n, Tw, fin, &w0))) return rc;
    const long long r0 = (long long)kMelPerFrame * w0, got = z.mel_done - r0;
    win.e[b] = WinGroupEntry{s, (int)(r0 % g.cap), (int)(got < 0 ? 0 : got > kMelPerFrame * Tw ? kMelPerFrame * Tw : got)};
    rows.e[b] = RowsGroupEntry{s, (int)(f0 - w0), n, (int)row[s]};
    if (n > most) most = n;
    z.emitted += n; row[s] += n;
  }
  VP_HIP_CHECK(launch_mel_window_group(G->ring, g.cap, G->d.num_mel_bins, kMelPerFrame * Tw, A, p->d.batch, win, G->mwin, st));
  if ((rc = bfm_trunk(p, G->mwin, st))) return rc;
  VP_HIP_CHECK(launch_gru_state_group(p->xg, p->xc, gru_whg(p), gru_whc(p), G->hstate, p->rnn, Tw, rows, A, st));
  if ((rc = bfm_decode(p, nullptr, G->dout, st))) return rc;
  VP_HIP_CHECK(launch_rows_scatter_group(G->dout, Tw, out, rows, A, most, st));
  return VP_OK;
}

// everything ready now for the slots in `who`, in rounds of at most max_chunk_frames per slot; out rows of slot s from row[s] on
static int group_emit(vp_bfmstream_group* G, const std::vector<int>& who, bool fin, float* out, std::vector<long long>& row, hipStream_t st) {
  const int S = G->d.slots;
  std::vector<long long> target(S, 0);
  std::vector<int> live;
  int rc;
  for (int s : who) {
    GroupSlot& z = G->slot[s];
    target[s] = emitted_after(G->g, z.samples, fin);
    if (z.emitted >= target[s]) continue;
    const long long pad = pad_len_of(z.samples);
    if (!fin || pad >= G->g.Tw) { live.push_back(s); continue; }
    // a finished clip shorter than T_win: its frames alone, on the exact-size plan
    if ((rc = short_plan(G, (int)pad, st))) return rc;
    while (z.emitted < target[s])
      if ((rc = group_round(G, G->shrt, {s}, target, fin, out, row, st))) return rc;
  }
  const std::vector<int> buckets = group_buckets(S);
  while (true) {
    std::vector<int> act;
    for (int s : live) if (G->slot[s].emitted < target[s]) act.push_back(s);
    if (act.empty()) return VP_OK;
    size_t bi = 0;
    while (buckets[bi] < (int)act.size()) ++bi;
    if ((rc = group_round(G, G->plans[bi], act, target, fin, out, row, st))) return rc;
  }
}

extern "C" {

size_t vp_bfmstream_group_desc_size(void) { return sizeof(vp_bfmstream_group_desc); }

size_t vp_bfmstream_group_workspace_bytes(const vp_bfmstream_group_desc* d) {
  vp_bfmstream_group G{};
  size_t n = 0;
  const int rc = group_layout(&G, d, &n);
  free_plans(G.plans);
  return rc ? 0 : n;
}

int vp_bfmstream_group_plan_info(const vp_bfmstream_group_desc* d, int bucket, int gemm, int info[8]) {
  vp_bfmstream_group G{};
  size_t n = 0;
  int rc = group_layout(&G, d, &n);
  if (!rc) {
    std::vector<const Gemm*> gs;
    if (bucket < 0 || bucket >= (int)G.plans.size()) rc = VP_ERR_ARG;
    else {
      model_gemms(G.plans[bucket]->m, gs);
      if (gemm < 0 || gemm >= (int)gs.size() || !info) rc = VP_ERR_ARG;
      else {
        const IgemmPlan& p = gs[gemm]->plan;
        info[0] = G.plans[bucket]->d.batch; info[1] = p.cfg; info[2] = p.a.splitk; info[3] = p.a.kern;
        info[4] = p.a.N * p.a.Hg * p.a.Wg; info[5] = gs[gemm]->cin; info[6] = gs[gemm]->cout; info[7] = gs[gemm]->bf;
      }
    }
  }
  free_plans(G.plans);
  return rc;
}

int vp_bfmstream_group_create(const vp_bfmstream_group_desc* d, void* workspace, size_t bytes, const float* params, void* stream,
                              vp_bfmstream_group_t** out) {
  if (!workspace || !params || !out) { set_err("vp_bfmstream_group_create: null argument"); return VP_ERR_ARG; }
  vp_bfmstream_group* G = new vp_bfmstream_group{};
  size_t need = 0;
  int rc;
  if ((rc = group_layout(G, d, &need))) { vp_bfmstream_group_destroy(G); return rc; }
  if (bytes < need) { vp_bfmstream_group_destroy(G); set_err("vp_bfmstream_group_create: workspace too small"); return VP_ERR_WORKSPACE; }
  vp_logmel_desc lmd;
  group_carve(G, (char*)workspace, &lmd);
  G->params = params;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = vp_logmel_create(&lmd, G->lm_base, G->lm_bytes, stream, &G->lm))) { vp_bfmstream_group_destroy(G); return rc; }
  for (vp_bfmnet* p : G->plans) {
    bfm_carve(p, G->plan_base);
    p->params = params;
    p->zeros = G->zeros;
  }
  G->dirty = true;
  G->slot.assign(d->slots, GroupSlot{});
  hipError_t e = hipMemsetAsync(G->zeros, 0, 256, st);
  if (e == hipSuccess) e = hipMemsetAsync(G->hstate, 0, (size_t)d->slots * 256 * 4, st);
  if (e != hipSuccess) { set_err("vp_bfmstream_group_create: %s", hipGetErrorString(e)); vp_bfmstream_group_destroy(G); return VP_ERR_HIP; }
  *out = G;
  return VP_OK;
}

void vp_bfmstream_group_destroy(vp_bfmstream_group_t* h) {
  if (!h) return;
  vp_logmel_destroy(h->lm);
  free_plans(h->plans);
  delete h->shrt;
  delete h;
}

int vp_bfmstream_group_params_changed(vp_bfmstream_group_t* h) {
  if (!h) return VP_ERR_ARG;
  h->dirty = true;
  if (h->shrt) h->shrt->dirty = true;
  return VP_OK;
}

int vp_bfmstream_group_reset_slot(vp_bfmstream_group_t* h, int slot, void* stream) {
  if (!h || slot < 0 || slot >= h->d.slots) { set_err("vp_bfmstream_group_reset_slot: bad handle or slot"); return VP_ERR_ARG; }
  h->slot[slot] = GroupSlot{};
  VP_HIP_CHECK(hipMemsetAsync(h->hstate + (size_t)slot * 256, 0, 256 * 4, (hipStream_t)stream));
  return VP_OK;
}

long long vp_bfmstream_group_ready(const vp_bfmstream_group_t* h, const long long* n, const int* finish, int* k) {
  if (!h || !n) return -1;
  long long total = 0;
  for (int s = 0; s < h->d.slots; ++s) {
    const GroupSlot& z = h->slot[s];
    const bool fin = finish && finish[s];
    long long ks = 0;
    if (n[s] < 0 || (z.finished && (n[s] > 0 || fin))) return -1;
    if (!z.finished) ks = (fin ? pad_len_of(z.samples + n[s]) : emitted_after(h->g, z.samples + n[s], false)) - z.emitted;
    if (k) k[s] = (int)ks;
    total += ks;
  }
  return total;
}

int vp_bfmstream_group_push(vp_bfmstream_group_t* h, const float* pcm, const long long* n, const int* finish, const float* ears, float* coeff_out,
                            void* stream) {
  if (!h || !n) { set_err("vp_bfmstream_group_push: null handle / n"); return VP_ERR_ARG; }
  const int S = h->d.slots;
  long long total = 0;
  for (int s = 0; s < S; ++s) {
    if (n[s] < 0) { set_err("vp_bfmstream_group_push: n[%d] < 0", s); return VP_ERR_ARG; }
    if (h->slot[s].finished && (n[s] > 0 || (finish && finish[s]))) {
      set_err("vp_bfmstream_group_push: slot %d is finished (vp_bfmstream_group_reset_slot)", s);
      return VP_ERR_STATE;
    }
    total += n[s];
  }
  if (total > 0 && !pcm) { set_err("vp_bfmstream_group_push: samples and no pcm"); return VP_ERR_ARG; }
  if (total >= (1ll << 31)) { set_err("vp_bfmstream_group_push: %lld samples in one push (at most 2^31 - 1)", total); return VP_ERR_ARG; }
  const long long K = vp_bfmstream_group_ready(h, n, finish, nullptr);
  if (K > 0 && (!ears || !coeff_out)) { set_err("vp_bfmstream_group_push: frames are ready and ears / coeff_out is NULL"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = group_prepare(h, st))) return rc;
  std::vector<long long> pos(S), left(S), row(S), clip(S);
  std::vector<int> who;
  {
    std::vector<int> k(S);
    vp_bfmstream_group_ready(h, n, finish, k.data());
    long long p = 0, r = 0;
    for (int s = 0; s < S; ++s) { pos[s] = p; p += n[s]; row[s] = r; r += k[s]; left[s] = n[s]; }
  }
  // the samples, piece by piece, emitting behind each piece
  while (true) {
    if ((rc = group_pieces(h, pcm, pos, left, who, st))) return rc;
    if (who.empty()) break;
    if ((rc = group_emit(h, who, false, coeff_out, row, st))) return rc;
  }
  // then the finishing slots: prepare_pcm's zero padding without emitting, then every pending frame by the finish rule
  std::vector<int> fin;
  for (int s = 0; s < S; ++s) {
    left[s] = 0;
    if (!finish || !finish[s]) continue;
    GroupSlot& z = h->slot[s];
    clip[s] = z.samples;
    left[s] = (long long)kHop * (kMelPerFrame * pad_len_of(z.samples) - 1) + kWin - z.samples;
    fin.push_back(s);
  }
  if (!fin.empty()) {
    while (true) {
      if ((rc = group_pieces(h, nullptr, pos, left, who, st))) return rc;
      if (who.empty()) break;
    }
    for (int s : fin) {
      GroupSlot& z = h->slot[s];
      z.samples = clip[s];
      if (z.mel_done != (long long)kMelPerFrame * pad_len_of(z.samples)) { set_err("vp_bfmstream_group_push: slot %d: %lld mel frames", s, z.mel_done); return VP_ERR_STATE; }
    }
    if ((rc = group_emit(h, fin, true, coeff_out, row, st))) return rc;
    for (int s : fin) h->slot[s].finished = true;
  }
  if (K > 0) VP_HIP_CHECK(launch_add_ears(coeff_out, ears, (int)K, st));
  return VP_OK;
}

int vp_bfmstream_group_tensor(vp_bfmstream_group_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) return VP_ERR_ARG;
  if (std::string(name) != "mel") return VP_ERR_ARG;
  *ptr = h->ring;
  if (shape) { shape[0] = h->d.slots; shape[1] = h->g.cap; shape[2] = h->d.num_mel_bins; shape[3] = 1; }
  return VP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// vp_bfmstream_*: one session = a group of one slot (its one bucket is the batch-1 window plan, which group_plans never refuses)
// ------------------------------------------------------------------------------------------------
struct vp_bfmstream { vp_bfmstream_group* G; };

static bool one_slot(const vp_bfmstream_desc* d, vp_bfmstream_group_desc* gd) {
  if (!stream_ok(d)) return false;
  *gd = vp_bfmstream_group_desc{(int)sizeof(vp_bfmstream_group_desc), 1, d->max_chunk_frames, d->num_mel_bins, d->trunk_dtype, d->sample_rate,
                                d->lower_hz, d->upper_hz};
  return true;
}

extern "C" {

size_t vp_bfmstream_desc_size(void) { return sizeof(vp_bfmstream_desc); }

int vp_bfmstream_context(const vp_bfmstream_desc* d, int* left_mel, int* right_mel, int* left_frames, int* right_frames, int* window_frames) {
  if (!stream_ok(d)) { set_err("vp_bfmstream_context: bad descriptor"); return VP_ERR_ARG; }
  BfmModel m;
  build_model(m);
  const StreamGeo g = stream_geo(d, m);
  if (left_mel) *left_mel = g.L;
  if (right_mel) *right_mel = g.R;
  if (left_frames) *left_frames = g.Lf;
  if (right_frames) *right_frames = g.Rf;
  if (window_frames) *window_frames = g.Tw;
  return VP_OK;
}

long long vp_bfmstream_frames_after(const vp_bfmstream_desc* d, long long samples, int finished) {
  if (!stream_ok(d) || samples < 0) return -1;
  BfmModel m;
  build_model(m);
  return emitted_after(stream_geo(d, m), samples, finished != 0);
}

size_t vp_bfmstream_workspace_bytes(const vp_bfmstream_desc* d) {
  vp_bfmstream_group_desc gd;
  return one_slot(d, &gd) ? vp_bfmstream_group_workspace_bytes(&gd) : 0;
}

int vp_bfmstream_create(const vp_bfmstream_desc* d, void* workspace, size_t bytes, const float* params, void* stream, vp_bfmstream_t** out) {
  vp_bfmstream_group_desc gd;
  if (!one_slot(d, &gd) || !workspace || !params || !out) { set_err("vp_bfmstream_create: bad argument"); return VP_ERR_ARG; }
  vp_bfmstream_group* G;
  int rc;
  if ((rc = vp_bfmstream_group_create(&gd, workspace, bytes, params, stream, &G))) return rc;
  *out = new vp_bfmstream{G};
  return VP_OK;
}

void vp_bfmstream_destroy(vp_bfmstream_t* h) {
  if (!h) return;
  vp_bfmstream_group_destroy(h->G);
  delete h;
}

int vp_bfmstream_params_changed(vp_bfmstream_t* h) { return h ? vp_bfmstream_group_params_changed(h->G) : VP_ERR_ARG; }

int vp_bfmstream_reset(vp_bfmstream_t* h, void* stream) {
  if (!h) { set_err("vp_bfmstream_reset: null handle"); return VP_ERR_ARG; }
  return vp_bfmstream_group_reset_slot(h->G, 0, stream);
}

int vp_bfmstream_ready(const vp_bfmstream_t* h, long long n) {
  int k = 0;
  return h && vp_bfmstream_group_ready(h->G, &n, nullptr, &k) >= 0 ? k : 0;
}

int vp_bfmstream_ready_finish(const vp_bfmstream_t* h) {
  const long long n = 0;
  const int fin = 1;
  int k = 0;
  return h && vp_bfmstream_group_ready(h->G, &n, &fin, &k) >= 0 ? k : 0;
}

int vp_bfmstream_push(vp_bfmstream_t* h, const float* pcm, long long n, const float* ears, float* coeff_out, void* stream) {
  if (!h || n < 0 || (n > 0 && !pcm)) { set_err("vp_bfmstream_push: bad argument"); return VP_ERR_ARG; }
  if (h->G->slot[0].finished) { set_err("vp_bfmstream_push: the session is finished (vp_bfmstream_reset)"); return VP_ERR_STATE; }
  if (vp_bfmstream_ready(h, n) > 0 && (!ears || !coeff_out)) { set_err("vp_bfmstream_push: frames are ready and ears / coeff_out is NULL"); return VP_ERR_ARG; }
  // a group push takes fewer than 2^31 samples: a longer push runs as several, cut at whole pieces (the piece sizes, and so the windows,
  // stay those of the uncut push)
  const long long piece = (long long)kHop * h->G->g.piece, most = ((1ll << 31) - 1) / piece * piece;
  while (n > 0) {
    long long q = n < most ? n : most;
    const int k = vp_bfmstream_ready(h, q);
    int rc;
    if ((rc = vp_bfmstream_group_push(h->G, pcm, &q, nullptr, ears, coeff_out, stream))) return rc;
    pcm += q; n -= q;
    if (k) { ears += k; coeff_out += (size_t)k * 64; }
  }
  return VP_OK;
}

int vp_bfmstream_finish(vp_bfmstream_t* h, const float* ears, float* coeff_out, void* stream) {
  if (!h) { set_err("vp_bfmstream_finish: null handle"); return VP_ERR_ARG; }
  if (h->G->slot[0].finished) { set_err("vp_bfmstream_finish: the session is finished (vp_bfmstream_reset)"); return VP_ERR_STATE; }
  if (!ears || !coeff_out) { set_err("vp_bfmstream_finish: null ears / coeff_out"); return VP_ERR_ARG; }
  const long long n = 0;
  const int fin = 1;
  return vp_bfmstream_group_push(h->G, nullptr, &n, &fin, ears, coeff_out, stream);
}

int vp_bfmstream_tensor(vp_bfmstream_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h) return VP_ERR_ARG;
  int64_t gs[4];
  const int rc = vp_bfmstream_group_tensor(h->G, name, ptr, gs);
  if (!rc && shape) { shape[0] = gs[1]; shape[1] = gs[2]; shape[2] = 1; shape[3] = 1; }
  return rc;
}

}  // extern "C"

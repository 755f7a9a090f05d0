// Stand-alone op entry points of the C ABI (parity tests drive the same kernels the step executor uses).
#include <string.h>

#include <string>

#include "conv_ops.h"
#include "errors.h"
#include "audio_args.h"
#include "launch.h"
#include "vp_common.h"
#include "workspace.h"

using namespace vp;

namespace {

bool conv_desc_ok(const vp_conv_desc* d) {
  if (!d || d->n < 1 || d->h < 1 || d->w < 1) return false;
  if (d->cin < 8 || (d->cin & (d->cin - 1))) return false;
  if (d->kind == 1 && (d->ksize != 4 || d->stride != 2 || d->pad != 1)) return false;
  if (d->kind != 0 && d->kind != 1) return false;
  if (d->ksize < 1 || d->ksize > 4 || d->stride < 1 || d->stride > 2) return false;
  if (d->kind == 0 && d->stride == 2 && (d->ksize != 4 || d->pad != 1 || (d->h & 1) || (d->w & 1))) return false;
  return d->dtype == VP_F32 || d->dtype == VP_BF16;
}

ConvGeomX geom_of(const vp_conv_desc* d) {
  return make_geom(d->kind, d->ksize, d->stride, d->pad, d->n, d->h, d->w, d->cin, d->cin, d->cout);
}

// 256 zero bytes behind the op's workspace use (padding source of the LDS-DMA loader)
const void* zero_page(char* ws, size_t used, hipStream_t st) {
  char* z = ws + align256(used);
  (void)hipMemsetAsync(z, 0, 256, st);
  return z;
}

}  // namespace

extern "C" {

int vp_pixrefer_pack_frames(const unsigned char* example_frames, const unsigned char* current_frames, const int* crops,
                            int n, int img_size, float* inputs, float* fg_inputs, float* targets, float* masks, void* stream) {
  if (!example_frames || !current_frames || !crops || !inputs || !fg_inputs || !targets || !masks || n < 1 || img_size < 2) {
    set_err("vp_pixrefer_pack_frames: bad argument");
    return VP_ERR_ARG;
  }
  FramePackArgs a;
  a.ex = example_frames; a.cur = current_frames; a.crops = crops;
  a.inputs = inputs; a.fg_inputs = fg_inputs; a.targets = targets; a.masks = masks;
  a.N = n; a.S = img_size;
  VP_HIP_CHECK(launch_frame_pack(a, (hipStream_t)stream));
  return VP_OK;
}

extern "C" void vp_phase_marks_enable(int on);   // plan_pixrefer.hip

// vp_tune: one row per key (the knobs and their defaults: conv_ops.h, audio_args.h)
enum TuneRule {
  TUNE_PLAIN,         // store any value
  TUNE_POSITIVE,      // a non-positive value is refused like an unknown key
  TUNE_NEG_RESETS,    // a negative value: back to the default
  TUNE_0_TO_4,        // a value outside 0 .. 4: back to the default
};
struct TuneRow { const char* key; int* knob; TuneRule rule; int dflt; };      // dflt: what a reset stores (the resetting rules only)

int vp_tune(const char* key, int value) {
  if (!key) return VP_ERR_ARG;
  static const TuneRow rows[] = {
      {"patch_tiles", &patch_tiles_knob(), TUNE_PLAIN},
      {"patch_min_blocks", &patch_minblk_knob(), TUNE_NEG_RESETS, PATCH_MIN_BLOCKS_DEFAULT},
      {"patch_small_tiles", &patch_small_knob(), TUNE_PLAIN},
      {"patch_long_k_on_256", &patch_longk_knob(), TUNE_PLAIN},
      {"wgrad_tr", &wgrad_tr_knob(), TUNE_PLAIN},
      {"patch3", &patch3_knob(), TUNE_PLAIN},
      {"c64", &c64_knob(), TUNE_PLAIN},
      {"dc64", &dc64_knob(), TUNE_PLAIN},
      {"pool_bwd_fused", &pool_bwd_fused_knob(), TUNE_0_TO_4, 1},
      {"cout1_wgrad_rows", &wgrad1_rows_knob(), TUNE_POSITIVE},
      {"cout1_bwd", &cout1_knob(), TUNE_NEG_RESETS, 256},
      {"s2c64", &s2c64_knob(), TUNE_PLAIN},
      {"wgrad_big", &wgrad_big_knob(), TUNE_PLAIN},
      {"patch4", &patch4_knob(), TUNE_PLAIN},
      {"s2c64_pair", &s2c64_pair_knob(), TUNE_PLAIN},
      {"bfm_dwproj", &bfm_dwproj_knob(), TUNE_PLAIN},
      {"patch2", &patch2_knob(), TUNE_PLAIN},
      {"patch_xcd", &patch_xcd_knob(), TUNE_PLAIN},
      {"smallp_max_pixels", &smallp_knob(), TUNE_PLAIN},
      {"igemm_splitk_target", &igemm_splitk_target_knob(), TUNE_NEG_RESETS, IGEMM_SPLITK_TARGET_DEFAULT},
      {"wgrad_fixed_x10", &wgrad_cost_knob(0), TUNE_PLAIN},
      {"wgrad_slab_x100", &wgrad_cost_knob(1), TUNE_PLAIN},
      {"wgrad_slab_tile_x1000", &wgrad_cost_knob(2), TUNE_NEG_RESETS, 150},
      {"smallp_split_target", &plan_misc_knob(0), TUNE_PLAIN},
      {"igemm_splitk_cap", &plan_misc_knob(1), TUNE_PLAIN},
      {"igemm_splitk_minchunk", &plan_misc_knob(2), TUNE_PLAIN},
      {"wgrad_resident_blocks", &plan_misc_knob(3), TUNE_PLAIN},
      {"igemm_small_grid", &igemm_small_grid_knob(), TUNE_PLAIN},
      {"thin_blocks_cout8", &thin_blocks_knob(0), TUNE_POSITIVE},
      {"thin_blocks_dcout8", &thin_blocks_knob(1), TUNE_POSITIVE},
      {"thin_blocks_cout4", &thin_blocks_knob(2), TUNE_POSITIVE},
      {"thin_blocks_cin8", &thin_blocks_knob(3), TUNE_POSITIVE},
  };
  if (!strcmp(key, "phase_marks")) { vp_phase_marks_enable(value); return VP_OK; }
  for (const TuneRow& r : rows) {
    if (strcmp(key, r.key)) continue;
    if (r.rule == TUNE_POSITIVE && value <= 0) break;
    const bool reset = (r.rule == TUNE_NEG_RESETS && value < 0) || (r.rule == TUNE_0_TO_4 && (value < 0 || value > 4));
    *r.knob = reset ? r.dflt : value;
    return VP_OK;
  }
  set_err("vp_tune: unknown key %s", key);
  return VP_ERR_ARG;
}

// the few-pixel kernel's arrival counters live behind the zero page of the op's workspace, zeroed per call
static unsigned* smallp_counter_page(char* ws, size_t used, const IgemmArgs& a, hipStream_t st) {
  unsigned* c = (unsigned*)(ws + align256(used) + 256);
  (void)hipMemsetAsync(c, 0, (size_t)smallp_counters(a) * sizeof(unsigned), st);
  return c;
}

size_t vp_conv_workspace_bytes(const vp_conv_desc* d) {
  if (!conv_desc_ok(d)) return 0;
  const int bf = d->dtype == VP_BF16, es = bf ? 2 : 4;
  const ConvGeomX g = geom_of(d);
  size_t best = 0;
  {
    IgemmPlan p = plan_fwd(g, 0, bf);      // (the patch-kernel plan of the same layer needs no more: same packed block, no split-K slab)
    best = align256(p.pack_elems * es) + p.partial_bytes;
    plan_kernel(p, g.Cout, bf, d->cin, 0, FAM_SMALLP, LaunchForm{});
    if (p.a.kern == CK_SMALLP) {
      const size_t b = align256(p.pack_elems * es) + align256(p.partial_bytes) + 512 + (size_t)smallp_counters(p.a) * sizeof(unsigned);
      if (b > best) best = b;
    }
  }
  if ((d->cout & (d->cout - 1)) == 0 && d->cout >= 8) {
    IgemmPlan p = plan_bwd_data(g, 0, 0, d->cin, d->cin, d->cin, bf);
    size_t b = align256(p.pack_elems * es) + p.partial_bytes;
    if (b > best) best = b;
    plan_kernel(p, d->cin, bf, d->cout, 0, FAM_SMALLP, LaunchForm{});
    if (p.a.kern == CK_SMALLP) {
      b = align256(p.pack_elems * es) + align256(p.partial_bytes) + 512 + (size_t)smallp_counters(p.a) * sizeof(unsigned);
      if (b > best) best = b;
    }
    for (int plain = 0; plain < 2; ++plain) {      // the LDS-DMA weight-gradient kernel (plain operands) tiles and splits differently
      WgradPlan w = plan_wgrad(g, bf, plain != 0);
      if (w.partial_bytes + 512 > best) best = w.partial_bytes + 512;
    }
  }
  return best + 1024;
}

int vp_conv_fwd(const vp_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                const float* w, const float* bias, void* y, void* workspace, void* stream) {
  if (!conv_desc_ok(d) || !x || !w || !y || !workspace) { set_err("vp_conv_fwd: bad argument"); return VP_ERR_ARG; }
  const int bf = d->dtype == VP_BF16, es = bf ? 2 : 4;
  hipStream_t st = (hipStream_t)stream;
  const ConvGeomX g = geom_of(d);
  IgemmPlan p = plan_fwd(g, 0, bf);
  p.a.out_act = d->out_act;
  LaunchForm f;
  f.bias = bias != nullptr; f.x_affine = in_scale != nullptr; f.x_act = d->in_act;
  // the patch kernel moves plain bytes (LDS-DMA): only inputs that need no deferred affine / activation
  const bool plain = d->in_act == ACT_NONE && !in_scale;
  plan_kernel(p, g.Cout, bf, d->cin, 0, plain ? (FAM_SMALLP | FAM_PATCH | FAM_PATCH2 | (d->out_act == ACT_NONE ? FAM_S2C64 : 0)) : 0, f);
  char* ws = (char*)workspace;
  VP_HIP_CHECK(launch_pack_weights_one(p.pack, w, ws, bf, st));
  IgemmArgs a = p.a;
  set_single_src(a.x, x, d->cin, in_scale, in_shift, d->in_act, 0);
  a.Wp = ws;
  a.partial = (float*)(ws + align256(p.pack_elems * es));
  a.Y = y; a.bias = bias;
  a.zeros = zero_page(ws, align256(p.pack_elems * es) + p.partial_bytes, st);
  if (a.kern == CK_SMALLP) a.sp_cnt = smallp_counter_page(ws, align256(p.pack_elems * es) + p.partial_bytes, a, st);
  VP_HIP_CHECK(launch_igemm(a, bf, p.cfg, st));
  return VP_OK;
}

int vp_conv_bwd_data(const vp_conv_desc* d, const void* dy, const float* w, void* dx, void* workspace, void* stream) {
  if (!conv_desc_ok(d) || !dy || !w || !dx || !workspace) { set_err("vp_conv_bwd_data: bad argument"); return VP_ERR_ARG; }
  if (d->cout < 8 || (d->cout & (d->cout - 1))) { set_err("vp_conv_bwd_data: cout must be a power of two >= 8"); return VP_ERR_ARG; }
  const int bf = d->dtype == VP_BF16, es = bf ? 2 : 4;
  hipStream_t st = (hipStream_t)stream;
  const ConvGeomX g = geom_of(d);
  IgemmPlan p = plan_bwd_data(g, 0, 0, d->cin, d->cin, d->cin, bf);
  plan_kernel(p, d->cin, bf, d->cout, 0, FAM_SMALLP | FAM_PATCH | FAM_PATCH2, LaunchForm{});
  char* ws = (char*)workspace;
  VP_HIP_CHECK(launch_pack_weights_one(p.pack, w, ws, bf, st));
  IgemmArgs a = p.a;
  set_single_src(a.x, dy, d->cout, nullptr, nullptr, ACT_NONE, 0);
  a.Wp = ws;
  a.partial = (float*)(ws + align256(p.pack_elems * es));
  a.Y = dx;
  a.zeros = zero_page(ws, align256(p.pack_elems * es) + p.partial_bytes, st);
  if (a.kern == CK_SMALLP) a.sp_cnt = smallp_counter_page(ws, align256(p.pack_elems * es) + p.partial_bytes, a, st);
  VP_HIP_CHECK(launch_igemm(a, bf, p.cfg, st));
  return VP_OK;
}

// Backward-data of a 3x3 / stride-1 / pad-1 convolution (64 -> 64 or 128 -> 128 channels, bf16) whose OUTPUT went through a 2x2 max pool,
// from the pool's gradient dy_pool [n][h/2][w/2][c] and its arg-max codes (IgemmArgs::pool_code layout), times relu'(ref): what the VGG
// backward pass of a step runs below pool1 / pool2.  fused = 0: maxpool_bwd_code_kernel expands the gradient into the workspace and
// conv_c64_kernel reads it back; fused = 1: the kernel's pooled-source loader expands it in LDS (IgemmArgs::pool_src).  Same kernel
// family, same arithmetic: the two results are bit-identical.  No other kernel is substituted: a shape outside conv_c64 is an error.
static bool pooled_desc_ok(const vp_conv_desc* d) {
  return conv_desc_ok(d) && d->kind == 0 && d->ksize == 3 && d->stride == 1 && d->pad == 1 && d->dtype == VP_BF16 && d->cin == d->cout &&
         (d->cin == 64 || d->cin == 128) && d->h % 4 == 0 && d->w % 16 == 0 && d->h >= 16;      // (the patch plans start at 16 x 16 pixels)
}

size_t vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(const vp_conv_desc* d) {
  if (!pooled_desc_ok(d)) return 0;
  return align256(vp_conv_workspace_bytes(d)) + align256((size_t)d->n * d->h * d->w * d->cout * 2) + 256;
}

int vp_conv3x3_c64_bwd_data_pooled(const vp_conv_desc* d, const void* dy_pool, const unsigned char* code, const float* w, const void* ref,
                                   void* dx, void* workspace, int fused, void* stream) {
  if (!pooled_desc_ok(d) || !dy_pool || !code || !w || !ref || !dx || !workspace) { set_err("vp_conv3x3_c64_bwd_data_pooled: bad argument"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const ConvGeomX g = geom_of(d);
  IgemmPlan p = plan_bwd_data(g, 0, 0, d->cin, d->cin, d->cin, 1);
  LaunchForm f;
  f.ref = true; f.ref_act = ACT_RELU;
  plan_kernel(p, d->cin, 1, d->cout, 0, FAM_PATCH, f);
  if (p.a.kern != CK_C64) {
    set_err("vp_conv3x3_c64_bwd_data_pooled: %d x %d x %d x %d is planned on kernel %s, not c64", d->n, d->h, d->w, d->cin, conv_kernel_name(p.a.kern));
    return VP_ERR_ARG;
  }
  char* ws = (char*)workspace;
  VP_HIP_CHECK(launch_pack_weights_one(p.pack, w, ws, 1, st));
  IgemmArgs a = p.a;
  a.Wp = ws;
  a.partial = (float*)(ws + align256(p.pack_elems * 2));
  a.Y = dx;
  a.ref = ref; a.ref_act = ACT_RELU;
  a.zeros = zero_page(ws, align256(p.pack_elems * 2) + p.partial_bytes, st);
  if (fused) {
    set_single_src(a.x, dy_pool, d->cout, nullptr, nullptr, ACT_NONE, 0);
    a.pool_code = const_cast<unsigned char*>(code);
    a.pool_src = 1;
  } else {
    char* full = ws + align256(vp_conv_workspace_bytes(d));
    VP_HIP_CHECK(launch_maxpool_bwd_code(code, dy_pool, full, d->n, d->h, d->w, d->cout, 1, st));
    set_single_src(a.x, full, d->cout, nullptr, nullptr, ACT_NONE, 0);
  }
  VP_HIP_CHECK(launch_igemm(a, 1, p.cfg, st));
  return VP_OK;
}

int vp_conv_bwd_weight(const vp_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                       const void* dy, float* dw, void* workspace, void* stream) {
  if (!conv_desc_ok(d) || !x || !dy || !dw || !workspace) { set_err("vp_conv_bwd_weight: bad argument"); return VP_ERR_ARG; }
  if (d->cout < 8 || (d->cout & (d->cout - 1))) { set_err("vp_conv_bwd_weight: cout must be a power of two >= 8"); return VP_ERR_ARG; }
  const int bf = d->dtype == VP_BF16;
  hipStream_t st = (hipStream_t)stream;
  const ConvGeomX g = geom_of(d);
  WgradPlan p = plan_wgrad(g, bf, !in_scale && d->in_act == ACT_NONE);
  WgradArgs a = p.a;
  PixSrc xs, ds;
  set_single_src(xs, x, d->cin, in_scale, in_shift, d->in_act, 0);
  set_single_src(ds, dy, d->cout, nullptr, nullptr, ACT_NONE, 0);
  if (d->kind == 0) { a.g = xs; a.d = ds; } else { a.g = ds; a.d = xs; }
  a.partial = (float*)workspace;
  a.dW = dw;
  a.zeros = zero_page((char*)workspace, p.partial_bytes, st);
  VP_HIP_CHECK(launch_wgrad(a, bf, p.cfg, st));
  return VP_OK;
}

size_t vp_bn_workspace_bytes(int pixels, int c, int dtype) {
  if (pixels < 1 || c < 8) return 0;
  const int nch = bn_nchunk(pixels, c, 1, dtype == VP_BF16);
  return (size_t)nch * 2 * c * sizeof(double) + 4 * (size_t)c * sizeof(float) + 1024;
}

static bool bn_ok(int pixels, int c, int dtype) {
  const int e = dtype == VP_BF16 ? 8 : 4;
  return pixels >= 1 && c >= e && c % e == 0 && 256 % (c / e) == 0 && (dtype == VP_F32 || dtype == VP_BF16);
}

int vp_bn_stats(const void* y, int pixels, int c, int dtype, const float* gamma, const float* beta, float eps,
                float* scale, float* shift, float* mean, float* rstd, void* workspace, void* stream) {
  if (!bn_ok(pixels, c, dtype) || !y || !gamma || !beta || !scale || !shift || !mean || !rstd || !workspace) {
    set_err("vp_bn_stats: bad argument");
    return VP_ERR_ARG;
  }
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = y; b.C = c; b.G = 1; b.Pg = pixels;
  b.nchunk = bn_nchunk(pixels, c, 1, dtype == VP_BF16);
  b.partial = (double*)workspace;
  b.gamma = gamma; b.beta = beta; b.aff_a = scale; b.aff_b = shift; b.mu = mean; b.rstd = rstd; b.eps = eps;
  VP_HIP_CHECK(launch_bn_stats(b, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_bn_bwd(const void* y, const void* dz, void* dy, int pixels, int c, int dtype, const float* gamma,
              const float* mean, const float* rstd, float* dgamma, float* dbeta, void* workspace, void* stream) {
  if (!bn_ok(pixels, c, dtype) || !y || !dz || !dy || !gamma || !mean || !rstd || !dgamma || !dbeta || !workspace) {
    set_err("vp_bn_bwd: bad argument");
    return VP_ERR_ARG;
  }
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = y; b.dz = dz; b.dy = dy; b.C = c; b.G = 1; b.Pg = pixels;
  b.nchunk = bn_nchunk(pixels, c, 1, dtype == VP_BF16);
  b.partial = (double*)workspace;
  float* f = (float*)((char*)workspace + (size_t)b.nchunk * 2 * c * sizeof(double));
  b.c1 = f; b.c2 = f + c;
  b.gamma = gamma; b.mu = const_cast<float*>(mean); b.rstd = const_cast<float*>(rstd);
  b.dgamma = dgamma; b.dbeta = dbeta;
  VP_HIP_CHECK(launch_bn_bwd(b, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

// ---- single pointwise / audio ops behind the step and BFMNet executors (SURVEY.md 8b list), exported for parity tests and reuse ----

int vp_maxpool2x2_fwd(const void* x, void* y, int n, int h, int w, int c, int dtype, void* stream) {
  const int e = dtype == VP_BF16 ? 8 : 4;
  if (!x || !y || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || c < e || c % e) { set_err("vp_maxpool2x2_fwd: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_maxpool_fwd(x, y, n, h, w, c, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int dtype, void* stream) {
  const int e = dtype == VP_BF16 ? 8 : 4;
  if (!x || !dy || !dx || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || c < e || c % e) { set_err("vp_maxpool2x2_bwd: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_maxpool_bwd(x, dy, dx, n, h, w, c, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_maxpool2x2_bwd_code(const void* code, const void* dy, void* dx, int n, int h, int w, int c, int dtype, void* stream) {
  const int e = dtype == VP_BF16 ? 8 : 4;
  if (!code || !dy || !dx || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || c < e || c % e) { set_err("vp_maxpool2x2_bwd_code: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_maxpool_bwd_code(code, dy, dx, n, h, w, c, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_composite_fwd(const float* gen_out4, const float* targets, float* out4, float* outputs, float* outputs_fg, int n, int hw,
                     void* stream) {
  if (!gen_out4 || !targets || !out4 || !outputs || !outputs_fg || n < 1 || hw < 1) { set_err("vp_composite_fwd: bad argument"); return VP_ERR_ARG; }
  CompositeArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.y4 = gen_out4; ca.targets = targets; ca.o4 = out4; ca.outputs = outputs; ca.outputs_fg = outputs_fg; ca.N = n; ca.HW = hw; ca.train = 0;
  VP_HIP_CHECK(launch_composite_fwd(ca, 0, (hipStream_t)stream));
  return VP_OK;
}

int vp_gan_loss(const float* logits, void* seed_d, void* seed_g, float* predict, float* losses, int m, float gan_weight, int dtype,
                void* stream) {
  if (!logits || !seed_d || !seed_g || !predict || !losses || m < 1) { set_err("vp_gan_loss: bad argument"); return VP_ERR_ARG; }
  GanLossArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.logits = logits; ga.dl_d = seed_d; ga.dl_g = seed_g; ga.predict = predict; ga.losses = losses; ga.M = m; ga.gan_weight = gan_weight;
  VP_HIP_CHECK(launch_gan_loss(ga, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

// ---- the PixReferNet step's pointwise kernels one at a time (tests/test_gpu_pixrefer_pointwise_ops.py): an argument check and the
// launcher the step executor calls, nothing else ----

static bool dtype_ok(int dtype) { return dtype == VP_F32 || dtype == VP_BF16; }
static int elem_of(int dtype) { return dtype == VP_BF16 ? 8 : 4; }
// channels a multiple of the element vector; reduce: the channel groups also divide the 256 threads of bn_reduce_kernel
static bool chan_ok(int c, int dtype, bool reduce) {
  if (!dtype_ok(dtype) || c < elem_of(dtype) || c % elem_of(dtype)) return false;
  return !reduce || 256 % (c / elem_of(dtype)) == 0;
}
static bool bn_one_launch(int path, int pg) {
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.Pg = pg;
  return path == VP_BN_PATH_ONE_LAUNCH || (path == VP_BN_PATH_PLANNER && bn_small(b));
}
static bool bn_groups_ok(int groups, int pg, int c, int dtype, int path) {
  if (groups < 1 || groups > 1024 || pg < 1 || path < VP_BN_PATH_PLANNER || path > VP_BN_PATH_ONE_LAUNCH) return false;
  return chan_ok(c, dtype, !bn_one_launch(path, pg));
}

size_t vp_bn_groups_workspace_bytes(int groups, int pixels_per_group, int c, int dtype) {
  if (groups < 1 || groups > 1024 || pixels_per_group < 1 || !chan_ok(c, dtype, true)) return 0;
  const int nch = bn_nchunk(pixels_per_group, c, groups, dtype == VP_BF16);
  return (size_t)groups * nch * 2 * c * sizeof(double) + 1024;
}

int vp_bn_groups_fwd(const void* y, int groups, int pixels_per_group, int c, int dtype, const float* gamma, const float* beta, float eps,
                     float* scale, float* shift, float* mean, float* rstd, void* out_lrelu, void* out_relu, int path, void* workspace,
                     void* stream) {
  if (!bn_groups_ok(groups, pixels_per_group, c, dtype, path) || !y || !gamma || !beta || !scale || !shift || !mean || !rstd ||
      (!workspace && !bn_one_launch(path, pixels_per_group))) {
    set_err("vp_bn_groups_fwd: bad argument");
    return VP_ERR_ARG;
  }
  const int bf = dtype == VP_BF16;
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = y; b.C = c; b.G = groups; b.Pg = pixels_per_group;
  b.gamma = gamma; b.beta = beta; b.aff_a = scale; b.aff_b = shift; b.mu = mean; b.rstd = rstd; b.eps = eps;
  if (bn_one_launch(path, pixels_per_group)) {
    b.nchunk = 1;
    VP_HIP_CHECK(launch_bn_small_fwd(b, out_lrelu, out_relu, bf, (hipStream_t)stream));
    return VP_OK;
  }
  b.nchunk = bn_nchunk(pixels_per_group, c, groups, bf);
  b.partial = (double*)workspace;
  VP_HIP_CHECK(launch_bn_stats(b, bf, (hipStream_t)stream));
  if (out_lrelu || out_relu)
    VP_HIP_CHECK(launch_act_apply(y, scale, shift, c, pixels_per_group, (size_t)groups * pixels_per_group, out_lrelu, out_relu, bf, (hipStream_t)stream));
  return VP_OK;
}

int vp_bn_groups_bwd(const void* y, const void* dz, void* dy, int groups, int pixels_per_group, int c, int dtype, const float* gamma,
                     const float* mean, const float* rstd, float* c1, float* c2, float* dgamma, float* dbeta, float* dbias_zero,
                     int accumulate, int path, void* workspace, void* stream) {
  if (!bn_groups_ok(groups, pixels_per_group, c, dtype, path) || !y || !dz || !dy || !gamma || !mean || !rstd || !c1 || !c2 || !dgamma ||
      !dbeta || (!workspace && !bn_one_launch(path, pixels_per_group))) {
    set_err("vp_bn_groups_bwd: bad argument");
    return VP_ERR_ARG;
  }
  const int bf = dtype == VP_BF16;
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = y; b.dz = dz; b.dy = dy; b.C = c; b.G = groups; b.Pg = pixels_per_group;
  b.c1 = c1; b.c2 = c2;
  b.gamma = gamma; b.mu = const_cast<float*>(mean); b.rstd = const_cast<float*>(rstd);
  b.dgamma = dgamma; b.dbeta = dbeta; b.dbias_zero = dbias_zero; b.accumulate = accumulate != 0;
  if (bn_one_launch(path, pixels_per_group)) {
    b.nchunk = 1;
    VP_HIP_CHECK(launch_bn_small_bwd(b, bf, (hipStream_t)stream));
    return VP_OK;
  }
  b.nchunk = bn_nchunk(pixels_per_group, c, groups, bf);
  b.partial = (double*)workspace;
  VP_HIP_CHECK(launch_bn_bwd(b, bf, (hipStream_t)stream));
  return VP_OK;
}

int vp_bn_groups_bwd_tail(const void* y, const void* dz, void* dy, int groups, int pixels_per_group, int c, int dtype, const float* gamma,
                          const float* mean, const float* rstd, const double* partial, int nchunk, int raw, float* c1, float* c2,
                          float* dgamma, float* dbeta, float* dbias_zero, int accumulate, void* stream) {
  if (groups < 1 || pixels_per_group < 1 || !chan_ok(c, dtype, false) || nchunk < 1 || (raw != 0 && raw != 1) || !y || !dz || !dy || !gamma ||
      !mean || !rstd || !partial || !c1 || !c2 || !dgamma || !dbeta) {
    set_err("vp_bn_groups_bwd_tail: bad argument");
    return VP_ERR_ARG;
  }
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = y; b.dz = dz; b.dy = dy; b.C = c; b.G = groups; b.Pg = pixels_per_group;
  b.nchunk = nchunk; b.partial = const_cast<double*>(partial); b.raw = raw;
  b.c1 = c1; b.c2 = c2;
  b.gamma = gamma; b.mu = const_cast<float*>(mean); b.rstd = const_cast<float*>(rstd);
  b.dgamma = dgamma; b.dbeta = dbeta; b.dbias_zero = dbias_zero; b.accumulate = accumulate != 0;
  VP_HIP_CHECK(launch_bn_bwd_tail(b, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_colsum_groups(const void* x, int groups, int pixels_per_group, int c, int creal, int dtype, float* out, int accumulate,
                     void* workspace, void* stream) {
  if (groups < 1 || groups > 1024 || pixels_per_group < 1 || !chan_ok(c, dtype, true) || creal < 1 || creal > c || !x || !out || !workspace) {
    set_err("vp_colsum_groups: bad argument");
    return VP_ERR_ARG;
  }
  BnArgs b;
  memset(&b, 0, sizeof(b));
  b.y = x; b.C = c; b.G = groups; b.Pg = pixels_per_group;
  b.nchunk = bn_nchunk(pixels_per_group, c, groups, dtype == VP_BF16);
  b.partial = (double*)workspace;
  VP_HIP_CHECK(launch_colsum(b, creal, out, accumulate != 0, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_act_apply(const void* y, const float* scale, const float* shift, int groups, int pixels_per_group, int c, int dtype,
                 void* out_lrelu, void* out_relu, void* stream) {
  if (groups < 1 || pixels_per_group < 1 || !chan_ok(c, dtype, false) || !y || (!scale) != (!shift) || (!out_lrelu && !out_relu)) {
    set_err("vp_act_apply: bad argument");
    return VP_ERR_ARG;
  }
  VP_HIP_CHECK(launch_act_apply(y, scale, shift, c, pixels_per_group, (size_t)groups * pixels_per_group, out_lrelu, out_relu, dtype == VP_BF16,
                                (hipStream_t)stream));
  return VP_OK;
}

int vp_relu_bwd(const void* y, void* d, size_t n, int dtype, void* stream) {
  if (!y || !d || n < 1 || !dtype_ok(dtype) || n % elem_of(dtype)) { set_err("vp_relu_bwd: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_relu_bwd(y, d, n, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_tap_gather(const float* s, const float* bias, float* y, int n, int hin, int win, int ksize, int pad, void* stream) {
  if (!s || !bias || !y || n < 1 || hin < 1 || win < 1 || ksize < 1 || ksize > 4 || pad < 0 || hin + 2 * pad - ksize + 1 < 1 ||
      win + 2 * pad - ksize + 1 < 1) {
    set_err("vp_tap_gather: bad argument");
    return VP_ERR_ARG;
  }
  TapArgs t;
  memset(&t, 0, sizeof(t));
  t.S = s; t.bias = bias; t.y = y; t.N = n; t.Hin = hin; t.Win = win; t.ks = ksize; t.pad = pad;
  t.Hout = hin + 2 * pad - ksize + 1; t.Wout = win + 2 * pad - ksize + 1;
  VP_HIP_CHECK(launch_tap_gather(t, (hipStream_t)stream));
  return VP_OK;
}

int vp_tap_spread(const void* dy, int ld_dy, void* dys, int n, int hin, int win, int pad, int dtype, void* stream) {
  if (!dy || !dys || ld_dy < 1 || n < 1 || hin < 1 || win < 1 || pad < 0 || hin + 2 * pad - 3 < 1 || win + 2 * pad - 3 < 1 || !dtype_ok(dtype)) {
    set_err("vp_tap_spread: bad argument");
    return VP_ERR_ARG;
  }
  TapArgs t;
  memset(&t, 0, sizeof(t));
  t.dy = dy; t.dyS = dys; t.ld_dy = ld_dy; t.N = n; t.Hin = hin; t.Win = win; t.ks = 4; t.pad = pad;
  t.Hout = hin + 2 * pad - 3; t.Wout = win + 2 * pad - 3;
  VP_HIP_CHECK(launch_tap_spread(t, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_pack_inputs(const float* inputs, const float* fg_inputs, int fg_c, void* gin, void* gfg, void* din, void* vin, int n, int hw,
                   int train, int dtype, void* stream) {
  if (!inputs || !fg_inputs || (fg_c != 3 && fg_c != 6) || !gin || !gfg || (train && (!din || !vin)) || n < 1 || hw < 1 || !dtype_ok(dtype)) {
    set_err("vp_pack_inputs: bad argument");
    return VP_ERR_ARG;
  }
  PackInputsArgs p;
  memset(&p, 0, sizeof(p));
  p.inputs = inputs; p.fg_inputs = fg_inputs; p.fg_c = fg_c; p.gin = gin; p.gfg = gfg; p.din = din; p.vin = vin;
  p.N = n; p.HW = hw; p.train = train != 0;
  VP_HIP_CHECK(launch_pack_inputs(p, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_composite_nblocks(int n, int hw) { return (n < 1 || hw < 1) ? 0 : composite_nblocks(n, hw); }

int vp_composite_fwd_train(const float* gen_out4, const float* targets, const float* masks, float* out4, float* outputs, float* outputs_fg,
                           void* din, void* vin, double* partial, int n, int hw, int dtype, void* stream) {
  if (!gen_out4 || !targets || !masks || !out4 || !outputs || !outputs_fg || !din || !vin || !partial || n < 1 || hw < 1 || !dtype_ok(dtype)) {
    set_err("vp_composite_fwd_train: bad argument");
    return VP_ERR_ARG;
  }
  CompositeArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.y4 = gen_out4; ca.targets = targets; ca.masks = masks; ca.o4 = out4; ca.outputs = outputs; ca.outputs_fg = outputs_fg;
  ca.din = din; ca.vin = vin; ca.partial = partial; ca.N = n; ca.HW = hw; ca.train = 1;
  VP_HIP_CHECK(launch_composite_fwd(ca, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_composite_bwd(const float* out4, const float* targets, const float* masks, const float* outputs, const void* d_din, const void* d_vin,
                     void* dy4, int n, int hw, float l1_weight, int dtype, void* stream) {
  if (!out4 || !targets || !masks || !outputs || !d_din || !d_vin || !dy4 || n < 1 || hw < 1 || !dtype_ok(dtype)) {
    set_err("vp_composite_bwd: bad argument");
    return VP_ERR_ARG;
  }
  CompositeArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.targets = targets; ca.masks = masks; ca.o4 = const_cast<float*>(out4); ca.outputs = const_cast<float*>(outputs);
  ca.d_din = d_din; ca.d_vin = d_vin; ca.dy4 = dy4; ca.N = n; ca.HW = hw; ca.train = 1; ca.l1_weight = l1_weight;
  VP_HIP_CHECK(launch_composite_bwd(ca, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_perceptual_nblocks(size_t half, int dtype) {
  return (half < 1 || !dtype_ok(dtype) || half % elem_of(dtype)) ? 0 : perceptual_nblocks(half, dtype == VP_BF16);
}

int vp_perceptual(const void* f3, void* df3, double* partial, size_t half, float l1_weight, int dtype, void* stream) {
  if (!f3 || !df3 || !partial || half < 1 || !dtype_ok(dtype) || half % elem_of(dtype)) { set_err("vp_perceptual: bad argument"); return VP_ERR_ARG; }
  PerceptualArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.f3 = f3; pa.df3 = df3; pa.partial = partial; pa.half = half; pa.l1_weight = l1_weight;
  VP_HIP_CHECK(launch_perceptual(pa, dtype == VP_BF16, (hipStream_t)stream));
  return VP_OK;
}

int vp_loss_final(const double* comp_partial, int n_comp, const double* perc_partial, int n_perc, double n_out, double n_feat,
                  float l1_weight, float gan_weight, float* losses, void* stream) {
  if (!comp_partial || !perc_partial || !losses || n_comp < 1 || n_perc < 1 || !(n_out > 0) || !(n_feat > 0)) {
    set_err("vp_loss_final: bad argument");
    return VP_ERR_ARG;
  }
  LossFinalArgs la;
  memset(&la, 0, sizeof(la));
  la.comp_partial = comp_partial; la.n_comp = n_comp; la.perc_partial = perc_partial; la.n_perc = n_perc;
  la.n_out = n_out; la.n_feat = n_feat; la.losses = losses; la.l1_weight = l1_weight; la.gan_weight = gan_weight;
  VP_HIP_CHECK(launch_loss_final(la, (hipStream_t)stream));
  return VP_OK;
}

int vp_dwconv7x3_bn_act(const float* x, const float* w, const float* bias, float* y, int b, int h, int wd, int c, void* stream) {
  if (!x || !w || !bias || !y || b < 1 || h < 1 || wd < 1 || c < 4 || (c & 3)) { set_err("vp_dwconv7x3_bn_act: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_dwconv7x3(x, w, bias, y, 0, b, h, wd, c, (hipStream_t)stream));
  return VP_OK;
}

int vp_dwconv7x3_bn_act_t(const void* x, const float* w, const float* bias, void* y, int dtype, int b, int h, int wd, int c, void* stream) {
  if (!x || !w || !bias || !y || b < 1 || h < 1 || wd < 1 || c < 4 || (c & 3) || (dtype != VP_F32 && dtype != VP_BF16)) {
    set_err("vp_dwconv7x3_bn_act_t: bad argument"); return VP_ERR_ARG;
  }
  VP_HIP_CHECK(launch_dwconv7x3(x, w, bias, y, dtype == VP_BF16, b, h, wd, c, (hipStream_t)stream));
  return VP_OK;
}

// the stem as bfm_trunk launches it: same_pad of the [9,5] kernel at stride [1,2] (4 time rows either side; mel: the odd unit goes to the end)
int vp_conv_first_fwd(const float* x, const float* w, const float* bias, float* y, int b, int h, int w_in, int cout, void* stream) {
  if (!x || !w || !bias || !y || b < 1 || h < 1 || w_in < 1 || cout < 1) { set_err("vp_conv_first_fwd: bad argument"); return VP_ERR_ARG; }
  int pt, ho, pl, wo;
  same_pad(h, 9, 1, &pt, &ho);
  same_pad(w_in, 5, 2, &pl, &wo);
  VP_HIP_CHECK(launch_conv_first(x, w, bias, y, 0, b, h, w_in, wo, cout, pt, pl, (hipStream_t)stream));
  return VP_OK;
}

// The fused depthwise + projection kernel on its own.  The projection weights go through the plan and the packing kernel that
// bfm_carve / prepare_weights use for a fusable block (plan_gemm's geometry, perm = rowperm = 0), so the packed layout and wp_rows the
// kernel reads are the ones of the forward.  Workspace: the [22][ce] tap + bias block, then the packed weights.
static IgemmPlan dwproj_pack_plan(int pixels, int ce, int cout) {
  IgemmPlan p = plan_fwd(make_geom(0, 1, 1, 0, 1, pixels, 1, ce, ce, cout), 0, 0);
  p.pack.s_ch = cout;
  p.pack.dst_off = 0;
  p.pack.perm = 0; p.a.rowperm = 0;
  return p;
}

size_t vp_dwproj_workspace_bytes(int ce, int cout) {
  if (ce < 16 || ce % 16 || cout < 1) return 0;
  return align256((size_t)22 * ce * sizeof(float)) + align256(dwproj_pack_plan(1, ce, cout).pack_elems * sizeof(float)) + 256;
}

int vp_dwproj_fwd(const float* ex, const float* w_dw, const float* b_dw, const float* w_proj, const float* b_proj, float* y, int add, int b, int h,
                  int w, int ce, int cout, void* workspace, void* stream) {
  if (!ex || !w_dw || !b_dw || !w_proj || !b_proj || !y || !workspace || b < 1 || h < 1 || w < 1) { set_err("vp_dwproj_fwd: bad argument"); return VP_ERR_ARG; }
  if (!dwproj_eligible(w, ce, cout)) {
    set_err("vp_dwproj_fwd: no kernel for mel width %d, %d expanded and %d output channels (dwproj_eligible)", w, ce, cout);
    return VP_ERR_ARG;
  }
  const size_t ex_bytes = (size_t)b * h * w * ce * sizeof(float);
  if (ex_bytes >= 0xF0000000ull) {
    set_err("vp_dwproj_fwd: the expanded tensor is %zu bytes, the kernel's 32-bit lane offsets stop below 0xF0000000 (%llu)", ex_bytes, 0xF0000000ull);
    return VP_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  float* wdw22 = (float*)workspace;
  float* packed = (float*)((char*)workspace + align256((size_t)22 * ce * sizeof(float)));
  VP_HIP_CHECK(hipMemcpyAsync(wdw22, w_dw, (size_t)21 * ce * sizeof(float), hipMemcpyDeviceToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(wdw22 + (size_t)21 * ce, b_dw, (size_t)ce * sizeof(float), hipMemcpyDeviceToDevice, st));
  const IgemmPlan p = dwproj_pack_plan(b * h * w, ce, cout);
  VP_HIP_CHECK(launch_pack_weights_one(p.pack, w_proj, packed, 0, st));
  VP_HIP_CHECK(launch_dwproj(ex, wdw22, packed, p.a.wp_rows, b_proj, y, add ? 1 : 0, b, h, w, ce, cout, st));
  return VP_OK;
}

int vp_maxpool_hw(const float* x, float* y, int b, int h, int w, int c, int kh, int kw, int sh, int sw, void* stream) {
  if (!x || !y || b < 1 || h < 1 || w < 1 || c < 4 || (c & 3) || kh < 1 || kw < 1 || sh < 1 || sw < 1) { set_err("vp_maxpool_hw: bad argument"); return VP_ERR_ARG; }
  // TF 'same': out = ceil(in / stride); total pad = max((out-1)*stride + k - in, 0), the odd unit goes to the end
  const int ho = (h + sh - 1) / sh, wo = (w + sw - 1) / sw;
  const int ph = (ho - 1) * sh + kh - h, pw = (wo - 1) * sw + kw - w;
  const int pt = ph > 0 ? ph / 2 : 0, pl = pw > 0 ? pw / 2 : 0;
  VP_HIP_CHECK(launch_maxpool_same(x, y, 0, 0, b, h, w, c, kh, kw, sh, sw, pt, pl, ho, wo, (hipStream_t)stream));
  return VP_OK;
}

int vp_gru_seq(const float* xg, const float* xc, const float* whg, const float* whc, const int* seq_len, float* out, int b, int t,
               void* stream) {
  if (!xg || !xc || !whg || !whc || !seq_len || !out || b < 1 || t < 1) { set_err("vp_gru_seq: bad argument"); return VP_ERR_ARG; }
  VP_HIP_CHECK(launch_gru_seq(xg, xc, whg, whc, seq_len, out, b, t, (hipStream_t)stream));
  return VP_OK;
}

int vp_gru_seq_state(const float* xg, const float* xc, const float* whg, const float* whc, float* hstate, float* out, int b, int t, int t0,
                     int n, void* stream) {
  if (!xg || !xc || !whg || !whc || !hstate || !out || b < 1 || t < 1 || t0 < 0 || n < 0 || t0 + n > t) {
    set_err("vp_gru_seq_state: bad argument"); return VP_ERR_ARG;
  }
  if (n == 0) return VP_OK;
  VP_HIP_CHECK(launch_gru_state(xg, xc, whg, whc, hstate, out, b, t, t0, n, (hipStream_t)stream));
  return VP_OK;
}

}  // extern "C"

// CRC-32C (Castagnoli) of a host buffer, continuing from `crc` (0 to start): what TensorFlow's checkpoint bundles checksum every tensor
// with.  The checkpoint reader / writer (voicepuppet_amd/utils/tf_checkpoint.py) verifies 160 MB per PixReferNet restore; its numpy
// lane-parallel form runs at 0.1 GB/s, the hardware instruction at several GB/s.  Host code only.
extern "C" __attribute__((target("sse4.2"))) unsigned vp_crc32c(const void* data, size_t n, unsigned crc) {
  const unsigned char* p = (const unsigned char*)data;
  unsigned long long c = (unsigned long long)(crc ^ 0xFFFFFFFFu);
  while (n && ((size_t)p & 7)) { c = __builtin_ia32_crc32qi((unsigned)c, *p++); --n; }
  while (n >= 8) { c = __builtin_ia32_crc32di(c, *(const unsigned long long*)p); p += 8; n -= 8; }
  while (n) { c = __builtin_ia32_crc32qi((unsigned)c, *p++); --n; }
  return (unsigned)c ^ 0xFFFFFFFFu;
}

// The convolution kernel table (conv_dispatch.h) and the launch path on it.  Adding a kernel: its ConvKernel id (conv_args.h, at the end:
// the values are visible outside the library), its eligibility function and launcher beside the kernel, and ONE row here, at its priority.
#include "conv_dispatch.h"

#include "conv_ops.h"
#include "conv_prof.h"
#include "errors.h"
#include "vp_common.h"

namespace vp {

// the kernels' own entry points, each pair defined beside its kernel
typedef const IgemmArgs& Args;
hipError_t launch_igemm_generic(Args, int is_bf16, int cfg, hipStream_t);                                              // conv_kernels.hip
hipError_t launch_igemm_patch(Args, int is_bf16, int bc, int bp, hipStream_t);                                         // conv_patch.hip
hipError_t launch_igemm_patch2(Args, int is_bf16, int bc, int bp, hipStream_t);                                        // conv_patch2.hip
bool patch3_eligible(Args, int is_bf16); hipError_t launch_igemm_patch3(Args, int is_bf16, int bc, int bp, hipStream_t);  // conv_patch3.hip
bool patch4_eligible(Args, int is_bf16); hipError_t launch_igemm_patch4(Args, hipStream_t);                               // conv_patch3.hip (KW = 4)
hipError_t launch_igemm_smallp(Args, int is_bf16, hipStream_t);                                                        // conv_smallp.hip (plain epilogue)
bool conv_s2c64_eligible(Args, int is_bf16); hipError_t launch_conv_s2c64(Args, hipStream_t);                             // conv_s2c64.hip
bool conv_cin8_eligible(Args, int is_bf16); hipError_t launch_conv_cin8(Args, hipStream_t);                               // conv_thin.hip
bool conv_cout8_eligible(Args, int is_bf16); hipError_t launch_conv_cout8(Args, hipStream_t);
bool conv_dcout8_eligible(Args, int is_bf16); hipError_t launch_conv_dcout8(Args, hipStream_t);
bool conv_cout4_eligible(Args, int is_bf16); hipError_t launch_conv_cout4(Args, hipStream_t);
bool conv_c64_eligible(Args, int is_bf16); hipError_t launch_conv_c64(Args, hipStream_t);                                 // conv_c64.hip
bool conv_dc256_eligible(Args, int is_bf16); hipError_t launch_conv_dc256(Args, hipStream_t);                             // conv_dc64.hip: 2 x 128 input channels (merged2_decoder_2)
bool conv_dc64_eligible(Args, int is_bf16); hipError_t launch_conv_dc64(Args, hipStream_t);

// launchers that take the plan's tile / no dtype, behind the rows' common signature
#define VP_TILED(fn) [](Args a, int bf, int cfg, hipStream_t st) { int bc, bp; igemm_tile(cfg, &bc, &bp); return fn(a, bf, bc, bp, st); }
#define VP_BF16(fn) [](Args a, int, int, hipStream_t st) { return fn(a, st); }

// In priority order: pick_conv_kernel takes the first row whose preconditions hold.  The few-pixel and s2c64 families have one kernel
// each; the specialised bf16 kernels check their plan family themselves; the other families' own kernels come last.
static const ConvKernelRow kTable[] = {
    // few-pixel layers (plain epilogue; the fused batch-norm forms are launched by the step executor: launch_smallp)
    {CK_SMALLP, "smallp", CK_SMALLP, false, nullptr, nullptr, [](Args a, int bf, int, hipStream_t st) { return launch_igemm_smallp(a, bf, st); },
     TILE_FROM_CFG, 0, BYTES_DEFAULT},
    // 4x4 stride-2 conv from 64 to 128 channels in front of a batch-norm (layer_2 / encoder_2 / encoder_fg_2 forward): weights resident in
    // registers, parity-split input patch, statistics per block
    {CK_S2C64, "s2c64", CK_S2C64, true, nullptr, conv_s2c64_eligible, VP_BF16(launch_conv_s2c64), 128, 64, BYTES_DEFAULT},
    // 8-channel (padded image) inputs, 64 outputs: the direct register-resident form
    {CK_CIN8, "cin8", CK_IGEMM, true, nullptr, conv_cin8_eligible, VP_BF16(launch_conv_cin8), 64, 16, BYTES_ONE_CLASS},
    // 3x3 stride-1 conv from 64 to <= 8 channels (conv1_1 backward-data): halo tile staged once
    {CK_COUT8, "cout8", CK_IGEMM, true, nullptr, conv_cout8_eligible, VP_BF16(launch_conv_cout8), 16, 64, BYTES_ONE_CLASS},
    // 4x4 stride-2 transposed conv from 64 to <= 8 channels (layer_1 backward-data)
    {CK_DCOUT8, "dcout8", CK_IGEMM, true, nullptr, conv_dcout8_eligible, VP_BF16(launch_conv_dcout8), 32, 64, BYTES_DEFAULT},
    // 4-channel f32 transposed conv (decoder_1): the four parity classes x four channels as one MFMA tile
    {CK_COUT4, "cout4", CK_IGEMM, true, nullptr, conv_cout4_eligible, VP_BF16(launch_conv_cout4), 16, 16, BYTES_F32_OUT},
    // 3x3 stride-1 conv from 64 to 64 / 128 channels (VGG conv1_2 forward / backward-data, conv2_1 forward): weights resident in registers,
    // 4 x 16-pixel tiles
    {CK_C64, "c64", CK_PATCH, true, c64_knob, conv_c64_eligible, VP_BF16(launch_conv_c64), TILE_ROWS_COUT, 64, BYTES_DEFAULT},
    // 4x4 stride-2 transposed conv from 2 x 128 to 64 channels (merged2_decoder_2 forward)
    {CK_DC256, "dc256", CK_PATCH2, true, dc64_knob, conv_dc256_eligible, VP_BF16(launch_conv_dc256), 64, 128, BYTES_DEFAULT},
    // 4x4 stride-2 transposed conv from 128 to 64 channels (backward-data of layer_2 / encoder_2 / encoder_fg_2): weights resident in
    // registers, two parity classes per block
    {CK_DC64, "dc64", CK_PATCH2, true, dc64_knob, conv_dc64_eligible, VP_BF16(launch_conv_dc64), 64, 128, BYTES_DEFAULT},
    // 4x4 / stride-1 taps (the discriminator's layer_4): the unrolled patch kernel with 16 tap steps per chunk, 128-row x 16 x 16-pixel tiles
    {CK_PATCH4, "patch4", CK_PATCH, true, patch4_knob, patch4_eligible, VP_BF16(launch_igemm_patch4), 128, 256, BYTES_DEFAULT},
    // stride-1 convs with the input patch staged once per channel chunk: unrolled 3x3, generic, parity classes
    {CK_PATCH3, "patch3", CK_PATCH, false, patch3_knob, patch3_eligible, VP_TILED(launch_igemm_patch3), TILE_FROM_CFG, 0, BYTES_DEFAULT},
    {CK_PATCH, "patch", CK_PATCH, false, nullptr, nullptr, VP_TILED(launch_igemm_patch), TILE_FROM_CFG, 0, BYTES_DEFAULT},
    {CK_PATCH2, "patch2", CK_PATCH2, false, nullptr, nullptr, VP_TILED(launch_igemm_patch2), TILE_FROM_CFG, 0, BYTES_DEFAULT},
    // generic implicit GEMM (IgemmPlan::cfg picks the tile)
    {CK_IGEMM, "igemm", CK_IGEMM, false, nullptr, nullptr, launch_igemm_generic, TILE_FROM_CFG, 0, BYTES_DEFAULT},
};
#undef VP_TILED
#undef VP_BF16

static const ConvKernelRow* conv_kernel_row(int kern) {      // null: no such kernel
  for (const ConvKernelRow& r : kTable) if (r.id == kern) return &r;
  return nullptr;
}
const char* conv_kernel_name(int kern) { const ConvKernelRow* r = conv_kernel_row(kern); return r ? r->name : "?"; }
int conv_staging(int kern) { const ConvKernelRow* r = conv_kernel_row(kern); return r ? r->family : CK_IGEMM; }

bool conv_kernel_ok(const IgemmArgs& a, int is_bf16) {
  if (a.pool_src && a.kern != CK_C64) return false;      // only conv_c64_kernel has the pooled-source loader
  const ConvKernelRow* r = conv_kernel_row(a.kern);
  if (!r || (r->bf16_only && !is_bf16)) return false;
  return !r->eligible || r->eligible(a, is_bf16);
}

int pick_conv_kernel(const IgemmArgs& v, int is_bf16) {
  const int fam = conv_staging(v.kern);
  for (const ConvKernelRow& r : kTable) {
    if (r.id == r.family) { if (r.id == fam) return fam; continue; }      // a family's own kernel
    if ((r.bf16_only && !is_bf16) || (r.knob && !r.knob())) continue;
    if (r.eligible(v, is_bf16)) return r.id;
  }
  return fam;
}

hipError_t launch_igemm(const IgemmArgs& a, int is_bf16, int cfg, hipStream_t st) {
  if (!conv_kernel_ok(a, is_bf16)) {
    set_err("launch_igemm: the arguments are outside the preconditions of the plan's kernel %s (%s, %d x %d x %d -> %d channels)",
            conv_kernel_name(a.kern), is_bf16 ? "bf16" : "f32", a.N, a.Hg, a.Wg, a.Cout);
    return hipErrorInvalidValue;
  }
  const ConvKernelRow& r = *conv_kernel_row(a.kern);
  int pbc = r.prof_bc, pbp = r.prof_bp;
  if (pbc == TILE_FROM_CFG) igemm_tile(cfg, &pbc, &pbp);
  else if (pbc == TILE_ROWS_COUT) pbc = a.Cout;
  // algorithmic cost: 2*MACs over real channels; bytes = X + W + Y each touched once
  const double Pn = (double)a.N * a.Hg * a.Wg * a.nclass;
  const double kreal = (double)a.ntaps * a.cin_real;
  const double es = is_bf16 ? 2 : 4;
  const double flops = 2.0 * Pn * a.Cout * kreal;
  const double xfull = (double)a.N * a.Hin * a.Win * a.cin_real;
  double bytes;
  if (r.prof_bytes == BYTES_ONE_CLASS) bytes = es * (xfull + kreal * a.Cout + Pn * a.Cout);
  else if (r.prof_bytes == BYTES_F32_OUT) bytes = es * (xfull + kreal * a.nclass * a.Cout) + 4.0 * Pn * a.Cout;
  else {
    // (IgemmArgs::pool_src: a quarter of the input pixels, each with one code byte per channel)
    const double xbytes = a.pool_src ? (es + 1) * ((double)a.N * (a.Hin / 2) * (a.Win / 2) * a.cin_real) : es * xfull;
    bytes = xbytes + es * (kreal * a.nclass * a.Cout + Pn * a.Cout);
  }
  ProfScope prof(r.name, is_bf16, pbc, pbp, flops, bytes, st);
  return r.launch(a, is_bf16, cfg, st);
}

}  // namespace vp

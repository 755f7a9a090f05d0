// Host-side launchers of the kernels: the convolution entry points (conv_dispatch.hip runs the plan's kernel through its table, the
// generic implicit GEMM is in conv_kernels.hip, the weight gradients in wgrad_kernels.hip), what the planner and the step executor call
// by name beside the kernel it belongs to, and the pointwise launchers (pointwise.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "conv_args.h"
#include "conv_dispatch.h"
#include "pointwise_args.h"

namespace vp {

// tile configs: IgemmPlan::cfg indexes igemm_tile, WgradPlan::cfg wgrad_tile.  The values are visible outside the library
// (vp_bfmstream_group_plan_info) and must not move; 8, 9 and wgrad 3, 4 are unused
enum IgemmCfg {
  IG_128x128 = 0, IG_64x128, IG_16x128, IG_128x32, IG_128x16, IG_64x32, IG_128x256, IG_256x256,                       // generic implicit GEMM (conv_kernels.hip)
  PATCH_256x256 = 10, PATCH_128x512, PATCH_64x512, PATCH_128x256, PATCH_64x256, PATCH_256x128,                       // patch kernels
  SMALLP_32x16 = 16, SMALLP_32x32, SMALLP_32x64,                                                                      // few-pixel kernel
};
enum WgradCfg { WG_128x128 = 0, WG_128x64, WG_128x16, WG_TR_256x128 = 5, WG_TR_128x128 = 6 };                        // WG_TR_*: wgrad_tr.hip
void igemm_tile(int cfg, int* bc, int* bp);                                                                          // conv_kernels.hip
void wgrad_tile(int cfg, int* bm, int* bn);                                                                          // wgrad_kernels.hip

// conv_dc64.hip / conv_s2c64.hip: the blocks of a launch = the partial rows its epilogue writes
int conv_dc64_grid(const IgemmArgs& a);                        // its blocks = partial rows of IgemmArgs::colsum_part
int conv_dc256_grid(const IgemmArgs& a);                       // its blocks; batch-norm partial rows = 2 per block
int conv_s2c64_grid(const IgemmArgs& a);                       // blocks of the launch = partial rows per batch-norm group
int conv_s2c64_tiles_per_image(const IgemmArgs& a);
// conv_cout1.hip (each launcher writes its own profile record)
bool conv_cout1_bwd_eligible(const Cout1Args& a);
hipError_t launch_conv_cout1_bwd(const Cout1Args& a, hipStream_t st);
bool conv_cout1_wgrad_eligible(const Cout1Args& a);
hipError_t launch_conv_cout1_wgrad(const Cout1Args& a, hipStream_t st);
// conv_smallp.hip: the fused batch-norm forms (with its profile record)
struct SmallPArgs;
hipError_t launch_smallp(const SmallPArgs& s, int is_bf16, hipStream_t st);
// wgrad_kernels.hip / wgrad_mm.hip / wgrad_tr.hip
hipError_t launch_wgrad(const WgradArgs& a, int is_bf16, int cfg, hipStream_t st);
bool wgrad_mm_eligible(const WgradArgs& a, int cfg);
hipError_t launch_wgrad_mm(const WgradArgs& a, int cfg, hipStream_t st);
hipError_t launch_wgrad_tr(const WgradArgs& a, hipStream_t st, const char** variant = nullptr, int* tile_cols = nullptr);

hipError_t launch_pack_weights(const PackDesc* d_descs, int ndesc, const float* master, void* packed, int is_bf16, hipStream_t st);
hipError_t launch_pack_weights_one(const PackDesc& d, const float* master, void* packed, int is_bf16, hipStream_t st);
int bn_nchunk(int Pg, int C, int G, int is_bf16);
hipError_t launch_bn_stats(const BnArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_bn_finalize(const BnArgs& a, hipStream_t st);
bool bn_small(const BnArgs& a);     // few pixels per group: statistics + finalize + per-pixel pass in one launch
hipError_t launch_bn_small_fwd(const BnArgs& a, void* out_lrelu, void* out_relu, int is_bf16, hipStream_t st);
hipError_t launch_bn_small_bwd(const BnArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_bn_bwd(const BnArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_bn_bwd_tail(const BnArgs& a, int is_bf16, hipStream_t st);     // finalize + apply from partial rows a conv epilogue wrote (IgemmArgs::bst_*)
hipError_t launch_colsum(const BnArgs& a, int creal, float* out, int accumulate, int is_bf16, hipStream_t st);
hipError_t launch_colsum_tail(const BnArgs& a, int creal, float* out, int accumulate, hipStream_t st);   // the finalize alone: partial rows from a conv epilogue (IgemmArgs::colsum_part)
hipError_t launch_act_apply(const void* y, const float* sc, const float* sh, int C, int Pg, size_t npix,
                            void* out_lrelu, void* out_relu, int is_bf16, hipStream_t st);
hipError_t launch_tap_gather(const TapArgs& a, hipStream_t st);
hipError_t launch_tap_spread(const TapArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_frame_pack(const FramePackArgs& a, hipStream_t st);
hipError_t launch_pack_inputs(const PackInputsArgs& a, int is_bf16, hipStream_t st);
int composite_nblocks(int N, int HW);
hipError_t launch_composite_fwd(const CompositeArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_composite_bwd(const CompositeArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_gan_loss(const GanLossArgs& a, int is_bf16, hipStream_t st);
int perceptual_nblocks(size_t half, int is_bf16);
hipError_t launch_perceptual(const PerceptualArgs& a, int is_bf16, hipStream_t st);
hipError_t launch_loss_final(const LossFinalArgs& a, hipStream_t st);
hipError_t launch_maxpool_fwd(const void* x, void* y, int B, int H, int W, int C, int is_bf16, hipStream_t st);
hipError_t launch_maxpool_bwd(const void* x, const void* dy, void* dx, int B, int H, int W, int C, int is_bf16, hipStream_t st);
hipError_t launch_maxpool_bwd_code(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int is_bf16, hipStream_t st);   // code: IgemmArgs::pool_code
hipError_t launch_relu_bwd(const void* y, void* d, size_t n, int is_bf16, hipStream_t st);
hipError_t launch_adam(const AdamArgs& a, hipStream_t st);
hipError_t launch_fetch(const FetchArgs& a, hipStream_t st);
hipError_t launch_grad_pack_bf16(const float* src, void* dst, size_t n, hipStream_t st);
hipError_t launch_grad_unpack_bf16(const void* src, float* dst, size_t n, float scale, hipStream_t st);

// ---- shape / tiling helpers shared by the plan and the single-op entry points ----
struct ConvGeom {
  int kind;           // 0 conv (HWIO), 1 deconv k4 s2 (HWOI)
  int ks, stride, pad;
  int N, Hin, Win, Hout, Wout;
  int Cin, Cin_real;  // Cin: padded (multiple of 8, power of two); Cin_real: channels in the TF kernel
  int Cout;           // real
};

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace vp

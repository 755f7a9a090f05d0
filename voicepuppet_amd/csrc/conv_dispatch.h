// The convolution kernel table: one row per ConvKernel (conv_args.h), in priority order.  Everything that is per kernel on the launch
// path - its name, its plan family, whether it is bf16-only, the knob that gates it, its preconditions, its launcher, its profile
// record - is a field of its row (conv_dispatch.hip); the functions below read the row or walk the table.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_args.h"

namespace vp {

enum ProfBytes {
  BYTES_DEFAULT,     // X + W + Y, each touched once, weights of every parity class (pool_src: a quarter of X plus its code bytes)
  BYTES_ONE_CLASS,   // ... the weights of one class (cin8 / cout8)
  BYTES_F32_OUT,     // ... Y in float32 (cout4)
};
constexpr int TILE_FROM_CFG = 0, TILE_ROWS_COUT = -1;

struct ConvKernelRow {
  int id;                    // ConvKernel
  const char* name;          // conv_kernel_name; also the kind of its profile class
  int family;                // the plan family it runs (conv_staging); id == family: the family's own kernel, run when no other row takes the launch
  bool bf16_only;
  int& (*knob)();            // vp_tune knob that gates it in pick_conv_kernel (0: off), or null
  bool (*eligible)(const IgemmArgs&, int is_bf16);      // its preconditions, or null: any plan of its family
  hipError_t (*launch)(const IgemmArgs&, int is_bf16, int cfg, hipStream_t);
  int prof_bc, prof_bp;      // tile of the profile class; TILE_FROM_CFG: igemm_tile(cfg); prof_bc == TILE_ROWS_COUT: IgemmArgs::Cout rows
  ProfBytes prof_bytes;
};

const char* conv_kernel_name(int kern);
int conv_staging(int kern);                           // plan family of a kernel: CK_IGEMM, CK_PATCH, CK_PATCH2, CK_SMALLP or CK_S2C64
bool conv_kernel_ok(const IgemmArgs& a, int is_bf16); // the preconditions of the plan's kernel (a.kern) hold for these arguments
// the kernel for a launch with arguments v of a plan of family conv_staging(v.kern): the first row, in table order, that takes it
int pick_conv_kernel(const IgemmArgs& v, int is_bf16);
// Runs the kernel the plan chose (IgemmArgs::kern, conv_ops.h plan_kernel).  A plan for one kernel runs on no other: arguments outside
// that kernel's preconditions fail loudly.
hipError_t launch_igemm(const IgemmArgs& a, int is_bf16, int cfg, hipStream_t st);

}  // namespace vp

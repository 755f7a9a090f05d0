// Optional per-launch timing of the convolution launchers (HIP events on the launch stream) for bench.py's roofline line: a launcher
// opens a ProfScope around its launches; vp_profile_collect aggregates the records by class name (conv_prof.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace vp {

void profile_enable(int on);          // 1: per kernel kind, 2: per layer tag
void profile_tag(const char* tag);
size_t profile_collect(char* out, size_t cap);

// which kernel family a launch ended up on ("ws" wave-specialised, "dma", "reg" register loader; "mm", the wgrad_tr variants): part of the
// class name of an "igemm" / "wgrad" record, so that a class is ONE kernel template (the names rocprofv3 reports are per kernel too).
// Cleared when a scope opens, set by the launcher inside it
extern const char* g_prof_family;

struct ProfRec { hipEvent_t e0, e1; std::string name; double flops, bytes; };

// one record, from construction to destruction, named kind[_family]_<bf16|f32>_<bc>x<bp>
struct ProfScope {
  bool on;
  ProfRec r;
  hipStream_t st;
  std::string kind;
  int bf, bc, bp;
  ProfScope(const char* kind_, int is_bf16, int bc_, int bp_, double flops, double bytes, hipStream_t s);
  ~ProfScope();
};

}  // namespace vp

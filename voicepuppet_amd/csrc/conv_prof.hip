// The per-launch profiler of the convolution launchers (conv_prof.h): event pool, records, aggregation.
#include "conv_prof.h"

#include <stdio.h>
#include <string.h>

#include <vector>

namespace vp {

static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_ev_pool;

static hipEvent_t prof_event() {
  hipEvent_t e;
  if (!g_ev_pool.empty()) { e = g_ev_pool.back(); g_ev_pool.pop_back(); return e; }
  hipEventCreate(&e);
  return e;
}

static std::string g_prof_tag;
static bool g_prof_detail = false;
void profile_enable(int on) { g_prof_on = on != 0; g_prof_detail = on > 1; }
void profile_tag(const char* tag) { if (g_prof_on && g_prof_detail) g_prof_tag = tag ? tag : ""; }

const char* g_prof_family = nullptr;

ProfScope::ProfScope(const char* kind_, int is_bf16, int bc_, int bp_, double flops, double bytes, hipStream_t s) : on(g_prof_on), st(s), kind(kind_), bf(is_bf16), bc(bc_), bp(bp_) {
  if (!on) return;
  g_prof_family = nullptr;
  r.flops = flops; r.bytes = bytes;
  r.e0 = prof_event(); r.e1 = prof_event();
  hipEventRecord(r.e0, st);
}
ProfScope::~ProfScope() {
  if (!on) return;
  hipEventRecord(r.e1, st);
  char buf[96];
  // classes follow the kernel template instances rocprofv3 lists (family / variant, operand type, tile)
  if ((kind == "igemm" || kind == "wgrad") && g_prof_family) snprintf(buf, sizeof(buf), "%s_%s_%s_%dx%d", kind.c_str(), g_prof_family, bf ? "bf16" : "f32", bc, bp);
  else snprintf(buf, sizeof(buf), "%s_%s_%dx%d", kind.c_str(), bf ? "bf16" : "f32", bc, bp);
  r.name = buf;
  if (g_prof_detail && !g_prof_tag.empty()) r.name = g_prof_tag + " " + r.name;
  g_prof.push_back(r);
}

// JSON array of {name, calls, ms, flops, bytes}; call after the stream has been synchronised
size_t profile_collect(char* out, size_t cap) {
  struct Agg { std::string name; int calls; double ms, flops, bytes; };
  static std::string cache = "[]";
  if (g_prof.empty()) {   // second call of the (size query, copy) pair
    if (out && cap > 0) { strncpy(out, cache.c_str(), cap - 1); out[cap - 1] = 0; }
    return cache.size() + 1;
  }
  std::vector<Agg> agg;
  for (ProfRec& r : g_prof) {
    float ms = 0.f;
    hipEventSynchronize(r.e1);
    hipEventElapsedTime(&ms, r.e0, r.e1);
    g_ev_pool.push_back(r.e0); g_ev_pool.push_back(r.e1);
    Agg* a = nullptr;
    for (Agg& x : agg) if (x.name == r.name) a = &x;
    if (!a) { agg.push_back({r.name, 0, 0, 0, 0}); a = &agg.back(); }
    a->calls++; a->ms += ms; a->flops += r.flops; a->bytes += r.bytes;
  }
  g_prof.clear();
  std::string js = "[";
  for (size_t i = 0; i < agg.size(); ++i) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s{\"name\":\"%s\",\"calls\":%d,\"ms\":%.6f,\"flops\":%.6e,\"bytes\":%.6e}", i ? "," : "",
             agg[i].name.c_str(), agg[i].calls, agg[i].ms, agg[i].flops, agg[i].bytes);
    js += buf;
  }
  js += "]";
  cache = js;
  if (out && cap > 0) { strncpy(out, js.c_str(), cap - 1); out[cap - 1] = 0; }
  return js.size() + 1;
}

}  // namespace vp

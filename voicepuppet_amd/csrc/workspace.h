// Workspaces and device handles of the C ABI, shared by its translation units (the C-side counterpart of _handle.py).  A handle module
// is xxx_check (the descriptor), xxx_carve (the workspace -> typed pointers in the handle) and its kernels:
//   *_workspace_bytes:  xxx_check, then xxx_carve on a stack handle with a null base;
//   *_create:           open_handle, which runs both, refuses a short workspace and carves the heap handle on the real base.
// The argument checks that the image families' descriptors and calls share (extents, pitch and stride, overlap) are in frame_args.h.
#pragma once
#include <stdint.h>

#include <new>
#include <utility>
#include <vector>

#include "errors.h"

namespace vp {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
template <class T>
inline T* align256(T* p) { return (T*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// Bump allocator over a caller's workspace.  A null workspace is the sizing pass: every carve returns null and only the offsets move.
// The base is rounded up to 256 here and every carve starts on a 256-byte line; total() charges the 256 bytes the rounding may cost.
struct Arena {
  char* base;
  size_t off = 0;
  std::vector<std::pair<size_t, size_t>>* track = nullptr;   // optional (offset, bytes) of every carve: vp_pixrefer_validate_plan
  explicit Arena(void* workspace) : base(align256((char*)workspace)) {}
  void* alloc(size_t bytes) {
    off = align256(off);
    void* p = base ? base + off : nullptr;
    if (track) track->push_back({off, bytes});
    off += bytes;
    return p;
  }
  template <class T>
  T* take(size_t count) { return (T*)alloc(count * sizeof(T)); }
  size_t total() const { return off + 256; }                 // (the planners publish this; the handle modules round it to whole lines)
};

// null and struct_bytes test of a descriptor whose first field is struct_bytes.  family: "vp_jpeg", of vp_jpeg_desc; who: what the
// message starts with, where that is not the family
template <class D>
int check_desc(const D* d, const char* family, const char* who = nullptr) {
  if (!who) who = family;
  if (!d) { set_err("%s: bad descriptor (null)", who); return VP_ERR_ARG; }
  if ((size_t)d->struct_bytes != sizeof(D)) {
    set_err("%s: bad descriptor (struct_bytes %u, this library's %s_desc is %d bytes)", who, (unsigned)d->struct_bytes, family, (int)sizeof(D));
    return VP_ERR_ARG;
  }
  return VP_OK;
}

// The front of every *_create, refusals in this order: a null `out` (*out is cleared from here on), the descriptor (check), a missing or
// short workspace (short_rc).  check(d, h) fills a handle's descriptor and derived integers and returns VP_OK or the refusal; carve(h, base)
// fills its pointers and returns the bytes needed.
template <class H, class D, class Check, class Carve>
int open_handle(const char* fn, const D* d, Check check, Carve carve, void* workspace, size_t bytes, H** out, int short_rc = VP_ERR_WORKSPACE) {
  if (!out) { set_err("%s: bad argument", fn); return VP_ERR_ARG; }
  *out = nullptr;
  H sized{};
  if (const int rc = check(d, &sized)) return rc;
  const size_t need = carve(&sized, nullptr);
  if (!workspace || bytes < need) { set_err("%s: workspace too small (%zu of %zu bytes)", fn, bytes, need); return short_rc; }
  H* h = new (std::nothrow) H(sized);
  if (!h) { set_err("%s: out of host memory", fn); return VP_ERR_STATE; }
  carve(h, workspace);
  *out = h;
  return VP_OK;
}

}  // namespace vp

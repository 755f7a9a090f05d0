// Argument checks the image handle families share (vp_keymatte, vp_matteclean, vp_mattesolve, vp_frame_metrics): the extents of a
// descriptor, a call's n, height and width against it, the row pitch and frame stride of a strided frame batch, and whether two
// buffers overlap.  One copy of every message; each function refuses in the order of its lines, so an entry point's order of refusals
// is the order of its calls.  Host only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "errors.h"

namespace vp {

// a descriptor's max_frames (1 .. frames_cap), max_height and max_width (min_side .. max_side).  family: "vp_keymatte"
inline int check_extents_desc(const char* family, int max_frames, int frames_cap, int max_height, int max_width, int min_side, int max_side) {
  if (max_frames < 1 || max_frames > frames_cap) {
    set_err("%s: bad descriptor (max_frames %d, 1 .. %d)", family, max_frames, frames_cap);
    return VP_ERR_ARG;
  }
  if (max_height < min_side || max_height > max_side) {
    set_err("%s: bad descriptor (max_height %d, %d .. %d)", family, max_height, min_side, max_side);
    return VP_ERR_ARG;
  }
  if (max_width < min_side || max_width > max_side) {
    set_err("%s: bad descriptor (max_width %d, %d .. %d)", family, max_width, min_side, max_side);
    return VP_ERR_ARG;
  }
  return VP_OK;
}

// a descriptor's max_radius (lo .. hi)
inline int check_radius_desc(const char* family, int max_radius, int lo, int hi) {
  if (max_radius < lo || max_radius > hi) {
    set_err("%s: bad descriptor (max_radius %d, %d .. %d)", family, max_radius, lo, hi);
    return VP_ERR_ARG;
  }
  return VP_OK;
}

// a call's n, height and width against the descriptor's three extents.  who: the entry point's name
inline int check_batch(const char* who, int n, int H, int W, int min_side, int max_frames, int max_height, int max_width) {
  if (n < 1 || n > max_frames) { set_err("%s: n %d outside 1 .. max_frames %d", who, n, max_frames); return VP_ERR_ARG; }
  if (H < min_side || H > max_height) { set_err("%s: height %d outside %d .. max_height %d", who, H, min_side, max_height); return VP_ERR_ARG; }
  if (W < min_side || W > max_width) { set_err("%s: width %d outside %d .. max_width %d", who, W, min_side, max_width); return VP_ERR_ARG; }
  return VP_OK;
}

// row pitch and frame stride, in bytes, of a batch of H rows of row_bytes: the bounds that keep every kernel's address arithmetic inside
// 64 bits, then rows and frames that do not overlap.  prefix: "", or "a_" / "b_" where a call takes two operands
inline int check_pitch(const char* who, const char* prefix, size_t pitch, size_t stride, int H, size_t row_bytes) {
  if (pitch > ((size_t)1 << 40)) { set_err("%s: %srow_pitch %zu is over 2^40 bytes", who, prefix, pitch); return VP_ERR_ARG; }
  if (stride > ((size_t)1 << 48)) { set_err("%s: %sframe_stride %zu is over 2^48 bytes", who, prefix, stride); return VP_ERR_ARG; }
  if (pitch < row_bytes) { set_err("%s: %srow_pitch %zu is smaller than a row of %zu bytes", who, prefix, pitch, row_bytes); return VP_ERR_ARG; }
  if (stride < (size_t)(H - 1) * pitch + row_bytes) {
    set_err("%s: %sframe_stride %zu is smaller than a frame ((height - 1) * row_pitch + %zu bytes)", who, prefix, stride, row_bytes);
    return VP_ERR_ARG;
  }
  return VP_OK;
}

// whether the `bytes` bytes at a and the `bytes` bytes at b share one
inline bool overlaps(const void* a, const void* b, size_t bytes) {
  return (uintptr_t)a < (uintptr_t)b + bytes && (uintptr_t)b < (uintptr_t)a + bytes;
}

}  // namespace vp

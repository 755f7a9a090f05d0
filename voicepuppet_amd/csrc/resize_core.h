// What csrc/resize.hip and csrc/triptych.hip share of cv2.resize(uint8, INTER_LINEAR): the coefficient tables (host, in OpenCV's own C
// float / double arithmetic - include from translation units compiled with -ffp-contract=off) and the integer arithmetic of one output
// byte (device).  See resize.hip for the algorithm and how it is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace vp {

struct ResizeTab { int ofs; short a0, a1; };      // source index, the two 11-bit coefficients (a1 = 0 and ofs clipped beyond xmax)

static void build_table(int ssize, int dsize, ResizeTab* tab) {
  const double inv_scale = (double)dsize / ssize;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= s;
    bool single = false;                             // beyond xmax: only S[s] is read (weight 2048)
    if (s < 0) { f = 0.f; s = 0; }
    if (s + 1 >= ssize) {
      single = true;
      if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    }
    const float c0 = 1.f - f, c1 = f;
    long a0 = lrintf(c0 * 2048.f), a1 = lrintf(c1 * 2048.f);
    a0 = a0 < -32768 ? -32768 : (a0 > 32767 ? 32767 : a0);
    a1 = a1 < -32768 ? -32768 : (a1 > 32767 ? 32767 : a1);
    tab[d].ofs = s;
    tab[d].a0 = single ? (short)2048 : (short)a0;
    tab[d].a1 = single ? (short)0 : (short)a1;
  }
}

// rows: OpenCV keeps the (possibly negative) floor and clips the two source ROWS instead of the coefficient
static void build_row_table(int ssize, int dsize, ResizeTab* tab, int* row1) {
  const double inv_scale = (double)dsize / ssize;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= s;
    const float c0 = 1.f - f, c1 = f;
    long b0 = lrintf(c0 * 2048.f), b1 = lrintf(c1 * 2048.f);
    b0 = b0 < -32768 ? -32768 : (b0 > 32767 ? 32767 : b0);
    b1 = b1 < -32768 ? -32768 : (b1 > 32767 ? 32767 : b1);
    const int r0 = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
    const int r1 = s + 1 < 0 ? 0 : (s + 1 > ssize - 1 ? ssize - 1 : s + 1);
    tab[d].ofs = r0; tab[d].a0 = (short)b0; tab[d].a1 = (short)b1;
    row1[d] = r1;
  }
}

// mode of a resize: 0 bilinear, 1 copy (equal sizes), 2 exact 2x reduction (INTER_AREA)
__host__ __device__ static inline int resize_mode(int src_h, int src_w, int dst_h, int dst_w) {
  return (dst_h == src_h && dst_w == src_w) ? 1 : ((src_h == 2 * dst_h && src_w == 2 * dst_w) ? 2 : 0);
}

// one output byte: s the source image [hs][ws][3], channel sc, destination pixel (dy, dx); xt / yt / yrow1 are read in mode 0 only
__device__ __forceinline__ int resize_px(const unsigned char* s, int ws, int mode, const ResizeTab* xt_, const ResizeTab* yt_, const int* yrow1,
                                         int dy, int dx, int sc) {
  if (mode == 1) return s[((size_t)dy * ws + dx) * 3 + sc];
  if (mode == 2) {
    const unsigned char* p = s + ((size_t)(2 * dy) * ws + 2 * dx) * 3 + sc;
    return (p[0] + p[3] + p[(size_t)ws * 3] + p[(size_t)ws * 3 + 3] + 2) >> 2;
  }
  const ResizeTab xt = xt_[dx], yt = yt_[dy];
  const int r1 = yrow1[dy];
  const int x1 = xt.a1 ? xt.ofs + 1 : xt.ofs;            // (a1 == 0: the second tap is never read by OpenCV either)
  const unsigned char* p0 = s + (size_t)yt.ofs * ws * 3;
  const unsigned char* p1 = s + (size_t)r1 * ws * 3;
  const int d0 = p0[xt.ofs * 3 + sc] * xt.a0 + p0[x1 * 3 + sc] * xt.a1;
  const int d1 = p1[xt.ofs * 3 + sc] * xt.a0 + p1[x1 * 3 + sc] * xt.a1;
  return ((((int)yt.a0 * (d0 >> 4)) >> 16) + (((int)yt.a1 * (d1 >> 4)) >> 16) + 2) >> 2;
}

}  // namespace vp

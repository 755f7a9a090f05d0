// Union-find core of the matte clean-up (include/vp_hip.h, vp_matteclean_*), __host__ __device__: csrc/matte_clean.hip runs it on LDS and
// on the global parent array, tests/matte_clean_core_host.cpp runs the same source on the host under sanitizers (mc_label_host).
//
// A parent array holds -1 outside the set and, inside it, the index of a pixel of the same component that is not larger than the pixel's
// own: the smaller index is always the root, so a component's root is its smallest index whatever the schedule.  mc_union links with an
// integer atomicMin on the larger root and retries from what it displaced when another lane got there first: lock free, nothing waits on
// another lane's progress.  Every loop counts its steps against `cap` (the frame's pixel count, which no path and no retry chain of a
// correct run can reach); a loop that gets there sets *hit and leaves, and mc_union then leaves too.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_HD __host__ __device__
#else
#define MC_HD
#endif

namespace vp {

MC_HD inline int mc_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
MC_HD inline void mc_store(int* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// *p = min(*p, v), returns what *p held
MC_HD inline int mc_atomic_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(p, v);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}

// the root of x (x inside the set)
MC_HD inline int mc_find(const int* parent, int x, int cap, int* hit) {
  for (int steps = 0;; ++steps) {
    const int up = mc_load(parent + x);
    if (up == x || up < 0) return x;
    if (steps >= cap) { *hit = 1; return x; }
    x = up;
  }
}

// joins the components of a and b (both inside the set)
MC_HD inline void mc_union(int* parent, int a, int b, int cap, int* hit) {
  for (int steps = 0;; ++steps) {
    a = mc_find(parent, a, cap, hit);
    b = mc_find(parent, b, cap, hit);
    if (a == b || *hit) return;
    if (steps >= cap) { *hit = 1; return; }
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = mc_atomic_min(parent + a, b);                 // a was a root: it now hangs below b
    if (old == a) return;
    a = old;                                                      // another lane linked a first: join what it linked to with b
  }
}

// Neighbours a pixel can be joined with: the ones before it in raster order, as (dx, dy): left, up, up-left, up-right (the last two for
// 8-connected components only).
struct McStep { int dx, dy; };
MC_HD inline McStep mc_back_neighbour(int j) {
  const McStep steps[4] = {{-1, 0}, {0, -1}, {-1, -1}, {1, -1}};
  return steps[j];
}

// Which of them a pixel has to be joined with, given which are in the set (in[j] as mc_back_neighbour(j)): not all.  Up, whenever it is
// in the set; then, by induction over the rows, pixels side by side in a row are connected once every pixel has applied the rule (either
// the right one picks the left one, or both pick their ups, which are side by side in the row above).  4-connected: also left, unless up
// and up-left are in the set too (left picks up-left, which is beside up).  8-connected: nothing more when up is in the set (left,
// up-left and up-right each touch up or a pixel beside it); otherwise left, or up-left when left is not in the set (left picks up-left
// itself), and up-right.  The rule may be applied with fewer neighbours visible (a tile's view): what it then picks inside the tile is a
// superset of what the full view picks there.
MC_HD inline void mc_pick(bool eight, const bool in[4], bool pick[4]) {
  pick[0] = pick[2] = pick[3] = false;
  pick[1] = in[1];
  if (!eight) { pick[0] = in[0] && !(in[1] && in[2]); return; }
  if (in[1]) return;
  if (in[0]) pick[0] = true; else pick[2] = in[2];
  pick[3] = in[3];
}

// Labels of one frame on the host, one pixel after the other: labels[i] = -1 outside the set, else the smallest index of i's component.
inline int mc_label_host(const unsigned char* in_set, int H, int W, bool eight, int* labels) {
  const int cap = H * W;
  int hit = 0;
  for (int i = 0; i < H * W; ++i) labels[i] = in_set[i] ? i : -1;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      if (!in_set[y * W + x]) continue;
      bool in[4], pick[4];
      for (int j = 0; j < 4; ++j) {
        const int nx = x + mc_back_neighbour(j).dx, ny = y + mc_back_neighbour(j).dy;
        in[j] = nx >= 0 && nx < W && ny >= 0 && in_set[ny * W + nx] != 0;
      }
      mc_pick(eight, in, pick);
      for (int j = 0; j < 4; ++j)
        if (pick[j]) mc_union(labels, y * W + x, (y + mc_back_neighbour(j).dy) * W + x + mc_back_neighbour(j).dx, cap, &hit);
    }
  for (int i = 0; i < H * W; ++i)
    if (labels[i] >= 0) labels[i] = mc_find(labels, i, cap, &hit);
  return hit;
}

}  // namespace vp

// The union-find core of the matte clean-up (voicepuppet_amd/csrc/matte_clean_core.h) on the host: the source the device kernels run,
// here one pixel after the other, built with -fsanitize=address,undefined by tests/test_matte_clean_host.py and run directly.
//   matte_clean_core_host IN OUT
// IN:  int32 count, then per case int32 height, width, eight and height * width bytes (nonzero: in the set).
// OUT: per case height * width int32 labels.  Prints "labelled <count> cases"; exit status 1 on a malformed file, 2 when a step cap was
// reached.  It also drives mc_find and mc_union by hand on a cycle, which no correct run produces: the cap must end both.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "matte_clean_core.h"

static bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 1; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 1; }
  int32_t count = 0;
  if (!read_exact(in, &count, 4) || count < 0) return 1;
  int capped = 0;
  for (int32_t c = 0; c < count; ++c) {
    int32_t hdr[3];
    if (!read_exact(in, hdr, sizeof(hdr)) || hdr[0] < 1 || hdr[0] > 1024 || hdr[1] < 1 || hdr[1] > 1024) return 1;
    const size_t pixels = (size_t)hdr[0] * hdr[1];
    std::vector<unsigned char> set(pixels);
    std::vector<int> labels(pixels);
    if (!read_exact(in, set.data(), pixels)) return 1;
    capped |= vp::mc_label_host(set.data(), hdr[0], hdr[1], hdr[2] != 0, labels.data());
    if (fwrite(labels.data(), sizeof(int), pixels, out) != pixels) return 1;
  }
  fclose(in);
  fclose(out);
  printf("labelled %d cases\n", (int)count);
  // a parent array with a cycle (2 -> 1 -> 2): find and union must stop at the cap and say so
  int cyc[4] = {0, 2, 1, 3}, hit = 0;
  vp::mc_find(cyc, 2, 4, &hit);
  printf("cycle: find %s\n", hit ? "capped" : "NOT-capped");
  hit = 0;
  vp::mc_union(cyc, 3, 2, 4, &hit);
  printf("cycle: union %s\n", hit ? "capped" : "NOT-capped");
  return capped ? 2 : 0;
}

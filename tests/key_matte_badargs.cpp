// Stand-alone caller of the host side of vp_keymatte_* (csrc/key_matte.hip), for the `make host-asan` build of the C-ABI layer.  The sizing
// query answers on the host; a null descriptor, struct_bytes - 4, sizes outside their ranges and a workspace one byte short are refused
// and leave *out null; a handle opened over a dummy pointer that is NOT 256-aligned names aligned tensors inside the workspace and
// refuses every bad argument of fit, apply, the model copies and the tensor query before any device call; vp_keymatte_solve_host runs
// on ordinary, degenerate, empty and extreme moments and returns finite numbers.  Prints one line per case; exits 1 when a case fails.
// Built and run by tests/test_key_matte_host.py under AddressSanitizer + UBSan; no GPU is touched.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "vp_hip.h"

static int failures = 0;
static void* const kFake = (void*)0x100010;      // never dereferenced by the host layer

static void expect(const char* what, bool ok, int rc) {
  const char* msg = vp_last_error();
  printf("%s vp_keymatte %s: rc %d, \"%s\"\n", ok ? "refused" : "NOT-REFUSED", what, rc, msg ? msg : "");
  if (!ok) ++failures;
}

static bool says(const char* word) { return strstr(vp_last_error(), word) != nullptr; }

static void solved(const char* what, const int64_t* S, double sigma_min, int want_status) {
  double m[VP_KEYMATTE_MODEL_DOUBLES + 1];
  m[VP_KEYMATTE_MODEL_DOUBLES] = -7.0;           // a canary behind the record
  const int rc = vp_keymatte_solve_host(S, sigma_min, m);
  bool ok = rc == VP_OK && m[VP_KEYMATTE_MODEL_DOUBLES] == -7.0 && (int)m[18] == want_status && m[16] == 1.0;
  for (int i = 0; i < VP_KEYMATTE_MODEL_DOUBLES; ++i) ok = ok && isfinite(m[i]);
  printf("%s vp_keymatte %s: rc %d, N %.0f, status %.0f, residual %.6g, inv00 %.6g\n", ok ? "solved" : "NOT-SOLVED", what, rc, m[15], m[18], m[17], m[9]);
  if (!ok) ++failures;
}

int main() {
  const vp_keymatte_desc good = {sizeof(vp_keymatte_desc), 2, 64, 48, 4};
  const size_t need = vp_keymatte_workspace_bytes(&good);
  if (need == 0 || need % 256) { printf("NOT-REFUSED vp_keymatte sizing: %zu, %s\n", need, vp_last_error()); ++failures; }
  if (vp_keymatte_desc_size() != sizeof(vp_keymatte_desc)) { printf("NOT-REFUSED vp_keymatte desc_size\n"); ++failures; }

  vp_keymatte_t* h = (vp_keymatte_t*)kFake;
  int rc = vp_keymatte_create(nullptr, kFake, need, &h);
  expect("null descriptor", vp_keymatte_workspace_bytes(nullptr) == 0 && rc == VP_ERR_ARG && !h && says("descriptor"), rc);
  vp_keymatte_desc bad = good;
  bad.struct_bytes -= 4;
  h = (vp_keymatte_t*)kFake;
  rc = vp_keymatte_create(&bad, kFake, need, &h);
  expect("struct_bytes - 4", vp_keymatte_workspace_bytes(&bad) == 0 && rc == VP_ERR_ARG && !h && says("struct_bytes"), rc);
  const struct { const char* field; vp_keymatte_desc d; } ranges[] = {
      {"max_frames", {sizeof(vp_keymatte_desc), 0, 64, 48, 4}},   {"max_frames", {sizeof(vp_keymatte_desc), -3, 64, 48, 4}},
      {"max_frames", {sizeof(vp_keymatte_desc), 4097, 64, 48, 4}}, {"max_height", {sizeof(vp_keymatte_desc), 2, 0, 48, 4}},
      {"max_height", {sizeof(vp_keymatte_desc), 2, 1025, 48, 4}}, {"max_width", {sizeof(vp_keymatte_desc), 2, 64, -48, 4}},
      {"max_width", {sizeof(vp_keymatte_desc), 2, 64, 15, 4}},    {"max_radius", {sizeof(vp_keymatte_desc), 2, 64, 48, 17}},
      {"max_radius", {sizeof(vp_keymatte_desc), 2, 64, 48, -1}}};
  for (const auto& r : ranges) {
    h = (vp_keymatte_t*)kFake;
    rc = vp_keymatte_create(&r.d, kFake, (size_t)1 << 30, &h);
    expect(r.field, vp_keymatte_workspace_bytes(&r.d) == 0 && rc == VP_ERR_ARG && !h && says(r.field), rc);
  }
  h = (vp_keymatte_t*)kFake;
  rc = vp_keymatte_create(&good, kFake, need - 1, &h);
  expect("one byte short", rc == VP_ERR_WORKSPACE && !h && says("workspace too small"), rc);
  h = (vp_keymatte_t*)kFake;
  rc = vp_keymatte_create(&good, nullptr, need, &h);
  expect("null workspace", rc == VP_ERR_WORKSPACE && !h && says("workspace too small"), rc);
  rc = vp_keymatte_create(&good, kFake, need, nullptr);
  expect("null out", rc == VP_ERR_ARG && says("bad argument"), rc);
  vp_keymatte_destroy(nullptr);
  // the largest descriptor is sized in 64 bits
  const vp_keymatte_desc huge = {sizeof(vp_keymatte_desc), VP_KEYMATTE_MAX_FRAMES, VP_KEYMATTE_MAX_SIZE, VP_KEYMATTE_MAX_SIZE, VP_KEYMATTE_MAX_RADIUS};
  if (vp_keymatte_workspace_bytes(&huge) < (size_t)VP_KEYMATTE_MAX_FRAMES * VP_KEYMATTE_MAX_SIZE * VP_KEYMATTE_MAX_SIZE * 16) {
    printf("NOT-REFUSED vp_keymatte sizing of the largest descriptor\n");
    ++failures;
  }

  rc = vp_keymatte_create(&good, kFake, need, &h);
  if (rc != VP_OK || !h) { printf("NOT-PLACED vp_keymatte create: rc %d\n", rc); return 1; }
  void* p = nullptr;
  int64_t shape[4];
  for (const char* t : {"moments", "model"}) {
    rc = vp_keymatte_tensor(h, t, &p, shape);
    const uintptr_t a = (uintptr_t)p, lo = (uintptr_t)kFake;
    const bool ok = rc == VP_OK && a % 256 == 0 && a >= lo && a < lo + need;
    printf("%s vp_keymatte tensor %s: rc %d at +%zu of %zu\n", ok ? "placed" : "NOT-PLACED", t, rc, (size_t)(a - lo), need);
    if (!ok) ++failures;
  }
  rc = vp_keymatte_tensor(h, "nothing", &p, shape);
  expect("tensor name", rc == VP_ERR_ARG && says("moments, model"), rc);
  rc = vp_keymatte_tensor(h, "model", nullptr, shape);
  expect("tensor null pointer", rc == VP_ERR_ARG, rc);

  const unsigned char* f = (const unsigned char*)kFake;
  unsigned char* o = (unsigned char*)kFake;
  const size_t pitch = 3 * 48, stride = 3 * 48 * 64;
  const double inf = INFINITY, nan = NAN;
  // fit
  rc = vp_keymatte_fit(nullptr, f, pitch, stride, 1, 64, 48, 0, 0, 16.0, 2.0, nullptr);  expect("fit null handle", rc == VP_ERR_ARG && says("handle"), rc);
  rc = vp_keymatte_fit(h, nullptr, pitch, stride, 1, 64, 48, 0, 0, 16.0, 2.0, nullptr);  expect("fit null frames", rc == VP_ERR_ARG && says("frames"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 3, 64, 48, 0, 0, 16.0, 2.0, nullptr);        expect("fit n", rc == VP_ERR_ARG && says("max_frames"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 65, 48, 0, 0, 16.0, 2.0, nullptr);        expect("fit height", rc == VP_ERR_ARG && says("max_height"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 15, 0, 0, 16.0, 2.0, nullptr);        expect("fit width", rc == VP_ERR_ARG && says("width 15"), rc);
  rc = vp_keymatte_fit(h, f, pitch - 1, stride, 1, 64, 48, 0, 0, 16.0, 2.0, nullptr);    expect("fit row_pitch", rc == VP_ERR_ARG && says("row_pitch"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride - 1, 2, 64, 48, 0, 0, 16.0, 2.0, nullptr);    expect("fit frame_stride", rc == VP_ERR_ARG && says("frame_stride"), rc);
  rc = vp_keymatte_fit(h, f, (size_t)1 << 41, (size_t)1 << 47, 1, 64, 48, 0, 0, 16.0, 2.0, nullptr);  expect("fit huge row_pitch", rc == VP_ERR_ARG && says("row_pitch"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, 25, 0, 16.0, 2.0, nullptr);       expect("fit band", rc == VP_ERR_ARG && says("band 25"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, INT32_MAX, 0, 16.0, 2.0, nullptr);  expect("fit band INT_MAX", rc == VP_ERR_ARG && says("band"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, -1, 0, 16.0, 2.0, nullptr);       expect("fit band -1", rc == VP_ERR_ARG && says("band -1"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, 4, 65, 16.0, 2.0, nullptr);       expect("fit side_rows", rc == VP_ERR_ARG && says("side_rows 65"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, 4, 3, 16.0, 2.0, nullptr);        expect("fit side_rows under band", rc == VP_ERR_ARG && says("side_rows 3"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, 0, 0, nan, 2.0, nullptr);         expect("fit trim", rc == VP_ERR_ARG && says("trim"), rc);
  rc = vp_keymatte_fit(h, f, pitch, stride, 1, 64, 48, 0, 0, 16.0, 0.0, nullptr);        expect("fit sigma_min", rc == VP_ERR_ARG && says("sigma_min"), rc);
  // apply
  rc = vp_keymatte_apply(nullptr, f, pitch, stride, 1, 64, 48, 4.0, 10.0, 4, 25.0, nullptr, o, nullptr);  expect("apply null handle", rc == VP_ERR_ARG && says("handle"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, 10.0, 4, 25.0, nullptr, nullptr, nullptr);  expect("apply null matte", rc == VP_ERR_ARG && says("matte"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 0, 64, 48, 4.0, 10.0, 4, 25.0, nullptr, o, nullptr);        expect("apply n", rc == VP_ERR_ARG && says("n 0"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 49, 4.0, 10.0, 4, 25.0, nullptr, o, nullptr);        expect("apply width", rc == VP_ERR_ARG && says("max_width"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 10.0, 10.0, 4, 25.0, nullptr, o, nullptr);       expect("apply lo >= hi", rc == VP_ERR_ARG && says("lo"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, inf, 4, 25.0, nullptr, o, nullptr);         expect("apply hi", rc == VP_ERR_ARG && says("hi"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, 10.0, 5, 25.0, nullptr, o, nullptr);        expect("apply radius", rc == VP_ERR_ARG && says("radius 5"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, 10.0, -1, 25.0, nullptr, o, nullptr);       expect("apply radius -1", rc == VP_ERR_ARG && says("radius -1"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, 10.0, 4, 0.0, nullptr, o, nullptr);         expect("apply eps", rc == VP_ERR_ARG && says("eps"), rc);
  rc = vp_keymatte_apply(h, f, pitch, stride, 1, 64, 48, 4.0, 10.0, 4, nan, nullptr, o, nullptr);         expect("apply eps nan", rc == VP_ERR_ARG && says("eps"), rc);
  // the model copies
  rc = vp_keymatte_get_model(h, nullptr, nullptr);                        expect("get_model null", rc == VP_ERR_ARG && says("model"), rc);
  rc = vp_keymatte_set_model(nullptr, (const double*)kFake, nullptr);     expect("set_model null handle", rc == VP_ERR_ARG && says("handle"), rc);
  rc = vp_keymatte_set_model(h, (const double*)0x100014, nullptr);        expect("set_model off an 8-byte boundary", rc == VP_ERR_ARG && says("8-byte"), rc);
  vp_keymatte_destroy(h);

  // SOLVE on the host
  double m[VP_KEYMATTE_MODEL_DOUBLES];
  int64_t S[21] = {0};
  rc = vp_keymatte_solve_host(nullptr, 2.0, m);  expect("solve null moments", rc == VP_ERR_ARG, rc);
  rc = vp_keymatte_solve_host(S, 2.0, nullptr);  expect("solve null model", rc == VP_ERR_ARG, rc);
  rc = vp_keymatte_solve_host(S, 0.0, m);        expect("solve sigma_min 0", rc == VP_ERR_ARG && says("sigma_min"), rc);
  rc = vp_keymatte_solve_host(S, nan, m);        expect("solve sigma_min nan", rc == VP_ERR_ARG && says("sigma_min"), rc);
  solved("no samples", S, 2.0, 1);
  // the 4 x 4 block x, y in 0 .. 3 of one colour (10, 20, 30), and the same with R = 10 + 2 x + y: a fit from 16 samples
  int64_t flat[21] = {0}, ramp[21] = {0};
  for (int y = 0; y < 4; ++y) {
    for (int x = 0; x < 4; ++x) {
      for (int k = 0; k < 2; ++k) {
        const int64_t v[6] = {x, y, k ? 10 + 2 * x + y : 10, 20, 30, 1};
        int64_t* dst = k ? ramp : flat;
        int at = 0;
        for (int i = 0; i < 6; ++i)
          for (int j = i; j < 6; ++j) dst[at++] += v[i] * v[j];
      }
    }
  }
  solved("16 samples of one colour", flat, 2.0, 0);
  solved("16 samples of a plane", ramp, 0.5, 0);
  flat[20] = 15;
  solved("15 samples", flat, 2.0, 1);
  // the largest sums a fit can produce: 4096 frames of 1024 x 1024 samples at x = y = 1023 and white
  int64_t big[21];
  const int64_t count = (int64_t)4096 * 1024 * 1024;
  {
    const int64_t v[6] = {1023, 1023, 255, 255, 255, 1};
    int at = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) big[at++] = count * v[i] * v[j];
  }
  solved("the largest moments", big, 2.0, 1);

  printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}

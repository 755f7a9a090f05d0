// Stand-alone caller of the eight handle families whose host code sits on csrc/workspace.h (jpeg, png, jpegdec and its scan, pcmin,
// frame_metrics, avimux, triptych, puppet), for the `make host-asan` build of the C-ABI layer.  Per family: the sizing query answers on
// the host; a null descriptor, struct_bytes - 4 and a workspace one byte short are refused with the family's code and a message, and
// leave *out null; *_destroy(nullptr) is harmless.  The three creates that make no device call (jpegdec, frame_metrics, avimux) are then
// opened over a dummy pointer that is NOT 256-aligned: the tensors they name must be aligned and inside the workspace.  Prints one line
// per case; exits 1 when a case fails.  Built and run by tests/test_workspace_host.py under AddressSanitizer + UBSan; no GPU is touched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "vp_hip.h"

static int failures = 0;
static void* const kFake = (void*)0x100010;      // never dereferenced by the host layer

static void expect(const char* family, const char* what, bool ok, int rc) {
  const char* msg = vp_last_error();
  printf("%s %s %s: rc %d, \"%s\"\n", ok ? "refused" : "NOT-REFUSED", family, what, rc, msg ? msg : "");
  if (!ok) ++failures;
}

// size(d): the family's *_workspace_bytes; create(d, workspace, bytes, out): its *_create; short_rc: what a short workspace returns
template <class D, class H, class Size, class Create>
static void family(const char* name, D good, Size size, Create create, void (*destroy)(H*), int short_rc = VP_ERR_WORKSPACE) {
  H* h = (H*)kFake;
  const size_t need = size(&good);
  if (need == 0) { printf("NOT-REFUSED %s sizing: %s\n", name, vp_last_error()); ++failures; }
  int rc = create((const D*)nullptr, kFake, need, &h);
  expect(name, "null descriptor", size((const D*)nullptr) == 0 && rc == VP_ERR_ARG && !h && strstr(vp_last_error(), "descriptor"), rc);
  D bad = good;
  bad.struct_bytes -= 4;
  h = (H*)kFake;
  rc = create(&bad, kFake, need, &h);
  expect(name, "struct_bytes - 4", size(&bad) == 0 && rc == VP_ERR_ARG && !h && strstr(vp_last_error(), "struct_bytes"), rc);
  h = (H*)kFake;
  rc = create(&good, kFake, need - 1, &h);
  expect(name, "one byte short", rc == short_rc && !h && strstr(vp_last_error(), "workspace too small"), rc);
  h = (H*)kFake;
  rc = create(&good, nullptr, need, &h);
  expect(name, "null workspace", rc == short_rc && !h && strstr(vp_last_error(), "workspace too small"), rc);
  rc = create(&good, kFake, need, (H**)nullptr);
  expect(name, "null out", rc == VP_ERR_ARG && strstr(vp_last_error(), "bad argument"), rc);
  destroy(nullptr);
}

static void inside(const char* family, const char* tensor, int rc, const void* p, size_t need) {
  const uintptr_t a = (uintptr_t)p, lo = (uintptr_t)kFake;
  const bool ok = rc == VP_OK && a % 256 == 0 && a >= lo && a < lo + need;
  printf("%s %s tensor %s: rc %d at +%zu of %zu\n", ok ? "placed" : "NOT-PLACED", family, tensor, rc, (size_t)(a - lo), need);
  if (!ok) ++failures;
}

int main() {
  family<vp_jpeg_desc, vp_jpeg_t>("vp_jpeg", {sizeof(vp_jpeg_desc), 4, 64, 64, 75}, vp_jpeg_workspace_bytes,
                                  [](const vp_jpeg_desc* d, void* w, size_t n, vp_jpeg_t** o) { return vp_jpeg_create(d, w, n, nullptr, o); }, vp_jpeg_destroy);
  family<vp_png_desc, vp_png_t>("vp_png", {sizeof(vp_png_desc), 3, 40, 36, 3, -1}, vp_png_workspace_bytes,
                                [](const vp_png_desc* d, void* w, size_t n, vp_png_t** o) { return vp_png_create(d, w, n, nullptr, o); }, vp_png_destroy);
  const vp_jpegdec_desc dec = {sizeof(vp_jpegdec_desc), 2, 64, 48, 1 << 16, 64, 1};
  family<vp_jpegdec_desc, vp_jpegdec_t>("vp_jpegdec", dec, vp_jpegdec_workspace_bytes, vp_jpegdec_create, vp_jpegdec_destroy);
  family<vp_pcmin_desc, vp_pcmin_t>("vp_pcmin", {(int)sizeof(vp_pcmin_desc), 4, 16000, 1 << 16, 2, {48000, 44100}}, vp_pcmin_workspace_bytes,
                                    [](const vp_pcmin_desc* d, void* w, size_t n, vp_pcmin_t** o) { return vp_pcmin_create(d, w, n, nullptr, o); },
                                    vp_pcmin_destroy);
  const vp_frame_metrics_desc fm = {sizeof(vp_frame_metrics_desc), 3, 40, 36};
  family<vp_frame_metrics_desc, vp_frame_metrics_t>("vp_frame_metrics", fm, vp_frame_metrics_workspace_bytes, vp_frame_metrics_create,
                                                    vp_frame_metrics_destroy);
  const vp_avimux_desc avi = {sizeof(vp_avimux_desc), 9, 260, 8, 1921};
  family<vp_avimux_desc, vp_avimux_t>("vp_avimux", avi, vp_avimux_workspace_bytes, vp_avimux_create, vp_avimux_destroy);
  family<vp_triptych_desc, vp_triptych_t>("vp_triptych", {sizeof(vp_triptych_desc), 2, 64, 224, 64}, vp_triptych_workspace_bytes,
                                          [](const vp_triptych_desc* d, void* w, size_t n, vp_triptych_t** o) { return vp_triptych_create(d, w, n, nullptr, o); },
                                          vp_triptych_destroy);
  // (a short workspace is VP_ERR_ARG in this family alone)
  family<vp_puppet_desc, vp_puppet_t>("vp_puppet", {(int)sizeof(vp_puppet_desc), 2, 8, 256, 224}, vp_puppet_workspace_bytes,
                                      [](const vp_puppet_desc* d, void* w, size_t n, vp_puppet_t** o) { return vp_puppet_create(d, w, n, nullptr, o); },
                                      vp_puppet_destroy, VP_ERR_ARG);

  // the scan workspace of a decoder: sized per chunk size, refused one byte short, carved on enable
  void* p = nullptr;
  int64_t shape[4];
  vp_jpegdec_t* jd = nullptr;
  size_t need = vp_jpegdec_workspace_bytes(&dec);
  int rc = vp_jpegdec_create(&dec, kFake, need, &jd);
  if (rc != VP_OK || !jd) { printf("NOT-PLACED vp_jpegdec create: rc %d\n", rc); return 1; }
  for (const char* t : {"coefficients", "entries", "planes"}) inside("vp_jpegdec", t, vp_jpegdec_tensor(jd, t, &p, shape), p, need);
  const size_t scan = vp_jpegdec_scan_workspace_bytes(&dec, 128);
  expect("vp_jpegdec", "scan null descriptor", vp_jpegdec_scan_workspace_bytes(nullptr, 128) == 0 && scan > 0 && scan % 256 == 0, 0);
  rc = vp_jpegdec_enable_scan(jd, kFake, scan - 1, 128, 32);
  expect("vp_jpegdec", "scan one byte short", rc == VP_ERR_WORKSPACE && strstr(vp_last_error(), "workspace too small"), rc);
  rc = vp_jpegdec_tensor(jd, "scan_ok", &p, shape);
  expect("vp_jpegdec", "scan tensor before enable_scan", rc == VP_ERR_ARG && strstr(vp_last_error(), "vp_jpegdec_enable_scan"), rc);
  rc = vp_jpegdec_enable_scan(jd, kFake, scan, 128, 32);
  if (rc != VP_OK) { printf("NOT-PLACED vp_jpegdec enable_scan: rc %d\n", rc); ++failures; }
  for (const char* t : {"scan_ok", "scan_rounds"}) inside("vp_jpegdec", t, vp_jpegdec_tensor(jd, t, &p, shape), p, scan);
  vp_jpegdec_destroy(jd);

  vp_frame_metrics_t* mh = nullptr;
  need = vp_frame_metrics_workspace_bytes(&fm);
  rc = vp_frame_metrics_create(&fm, kFake, need, &mh);
  if (rc != VP_OK || !mh) { printf("NOT-PLACED vp_frame_metrics create: rc %d\n", rc); return 1; }
  for (const char* t : {"abs_sum", "sq_sum"}) inside("vp_frame_metrics", t, vp_frame_metrics_tensor(mh, t, &p, shape), p, need);
  vp_frame_metrics_destroy(mh);

  vp_avimux_t* ah = nullptr;
  rc = vp_avimux_create(&avi, kFake, vp_avimux_workspace_bytes(&avi), &ah);
  if (rc != VP_OK || !ah) { printf("NOT-PLACED vp_avimux create: rc %d\n", rc); ++failures; }
  vp_avimux_destroy(ah);

  printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}

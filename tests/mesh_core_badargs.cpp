// Stand-alone caller of the dense mesh_core entry points (include/vp_hip.h) for the `make host-asan` build of the C-ABI layer:
// every call below must be refused with VP_ERR_ARG and a message before anything is enqueued, and the size queries must answer on
// the host.  Prints one line per case; exits 1 on the first case that is not refused.  Built and run by tests/test_mesh_core_host.py
// under AddressSanitizer + UBSan; no GPU is touched.
#include <stdio.h>
#include <string.h>

#include "vp_hip.h"

static int failures = 0;

static void refused(const char* what, int rc, const char* needle) {
  const char* msg = vp_last_error();
  const bool ok = rc == VP_ERR_ARG && msg && strstr(msg, needle);
  printf("%s %s: rc %d, \"%s\"\n", ok ? "refused" : "NOT-REFUSED", what, rc, msg ? msg : "");
  if (!ok) ++failures;
}

int main() {
  float* f = (float*)0x100000;   // never dereferenced by the host layer
  int* i = (int*)0x200000;
  void* ws = (void*)0x300000;

  if (vp_rasterize_triangles_workspace_bytes(2, 40, 36) < (size_t)2 * 40 * 36 * 8 || vp_rasterize_triangles_workspace_bytes(0, 40, 36) != 0 ||
      vp_rasterize_triangles_workspace_bytes(1, 65536, 65536) != 0 || vp_render_texture_workspace_bytes(2, 40, 36) < (size_t)2 * 40 * 36 * 8 ||
      vp_render_texture_workspace_bytes(1, 0, 36) != 0) {
    printf("NOT-REFUSED workspace queries\n");
    ++failures;
  }
  if (vp_vertex_adjacency_bytes(100, 200) < (size_t)(2 * 100 + 1 + 3 * 200) * 4 || vp_vertex_adjacency_bytes(0, 200) != 0 ||
      vp_vertex_adjacency_bytes(100, -1) != 0 || vp_vertex_adjacency_bytes(100, 0) == 0) {
    printf("NOT-REFUSED adjacency query\n");
    ++failures;
  }

  refused("rasterize null vertices", vp_rasterize_triangles(nullptr, i, f, i, f, 10, 5, 8, 8, 1, ws, nullptr), "vp_rasterize_triangles");
  refused("rasterize null triangles", vp_rasterize_triangles(f, nullptr, f, i, f, 10, 5, 8, 8, 1, ws, nullptr), "vp_rasterize_triangles");
  refused("rasterize null ids", vp_rasterize_triangles(f, i, f, nullptr, f, 10, 5, 8, 8, 1, ws, nullptr), "vp_rasterize_triangles");
  refused("rasterize null workspace", vp_rasterize_triangles(f, i, f, i, f, 10, 5, 8, 8, 1, nullptr, nullptr), "vp_rasterize_triangles");
  refused("rasterize ntri < 0", vp_rasterize_triangles(f, i, f, i, f, 10, -1, 8, 8, 1, ws, nullptr), "ntri -1");
  refused("rasterize h = 0", vp_rasterize_triangles(f, i, f, i, f, 10, 5, 0, 8, 1, ws, nullptr), "h 0");
  refused("rasterize h * w >= 2^31", vp_rasterize_triangles(f, i, f, i, f, 10, 5, 65536, 65536, 1, ws, nullptr), "h 65536");
  refused("rasterize batch = 0", vp_rasterize_triangles(f, i, f, i, f, 10, 5, 8, 8, 0, ws, nullptr), "batch 0");

  refused("texture null image", vp_render_texture(nullptr, f, i, f, f, i, f, 10, 10, 10, 5, 8, 8, 3, 16, 16, 3, 0, 1, ws, nullptr), "vp_render_texture");
  refused("texture null tex_coords", vp_render_texture(f, f, i, f, nullptr, i, f, 10, 10, 10, 5, 8, 8, 3, 16, 16, 3, 0, 1, ws, nullptr),
          "vp_render_texture");
  refused("texture c > tex_c", vp_render_texture(f, f, i, f, f, i, f, 10, 10, 10, 5, 8, 8, 4, 16, 16, 3, 0, 1, ws, nullptr), "c 4 > tex_c 3");
  refused("texture rows < nver", vp_render_texture(f, f, i, f, f, i, f, 10, 8, 9, 5, 8, 8, 3, 16, 16, 3, 0, 1, ws, nullptr), "tex_rows 9");
  refused("texture rows < tex_nver", vp_render_texture(f, f, i, f, f, i, f, 10, 12, 11, 5, 8, 8, 3, 16, 16, 3, 1, 1, ws, nullptr), "tex_rows 11");
  refused("texture tex_w = 0", vp_render_texture(f, f, i, f, f, i, f, 10, 10, 10, 5, 8, 8, 3, 16, 0, 3, 0, 1, ws, nullptr), "tex_w 0");

  refused("interpolate null out", vp_raster_interpolate(nullptr, i, f, i, f, 10, 5, 3, 8, 8, 1, nullptr), "vp_raster_interpolate");
  refused("interpolate k = 0", vp_raster_interpolate(f, i, f, i, f, 10, 5, 0, 8, 8, 1, nullptr), "k 0");
  refused("interpolate nver = 0", vp_raster_interpolate(f, i, f, i, f, 0, 5, 3, 8, 8, 1, nullptr), "nver 0");

  refused("adjacency null triangles", vp_vertex_adjacency_build(nullptr, 10, 5, ws, 1 << 20, nullptr), "vp_vertex_adjacency_build");
  refused("adjacency null buffer", vp_vertex_adjacency_build(i, 10, 5, nullptr, 1 << 20, nullptr), "vp_vertex_adjacency_build");
  refused("adjacency too small", vp_vertex_adjacency_build(i, 10, 5, ws, vp_vertex_adjacency_bytes(10, 5) - 1, nullptr), "needed");
  refused("normals null normal", vp_vertex_normals(nullptr, f, ws, 10, 5, 1, nullptr), "vp_vertex_normals");
  refused("normals null adjacency", vp_vertex_normals(f, f, nullptr, 10, 5, 1, nullptr), "vp_vertex_normals");
  refused("normals batch = 0", vp_vertex_normals(f, f, ws, 10, 5, 0, nullptr), "batch 0");

  printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}

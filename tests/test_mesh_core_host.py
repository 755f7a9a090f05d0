"""The dense half of mesh_core on the CPU: the numpy restatements of tests/mesh_core_ref.py against what the reference's compiled
mesh_core.cpp produced (tests/golden/mesh_core_dense.npz) and, when oracle/_ref is built, against that library itself; the conditions
that keep the fixture from going vacuous; the C ABI's declarations and its refusals.  Everything is equality of bits."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_core_ref as mr  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "mesh_core_dense.npz")
NAMES = ("vp_rasterize_triangles_workspace_bytes", "vp_rasterize_triangles", "vp_render_texture_workspace_bytes", "vp_render_texture",
         "vp_raster_interpolate", "vp_vertex_adjacency_bytes", "vp_vertex_adjacency_build", "vp_vertex_normals")


def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
  return dict(np.load(GOLD))


@pytest.mark.parametrize("tag", list(mr.MESHES))
def test_restatements_match_the_reference_goldens(gold, tag):
  v, t, h, w = mr.mesh(tag)
  assert np.array_equal(gold[tag + "_vertices"], v) and np.array_equal(gold[tag + "_triangles"], t)   # the mesh the golden was captured on
  depth, ids, bary, _ = mr.fresh_buffers(h, w)
  mr.rasterize_triangles_py(v, t, depth, ids, bary, h, w)
  assert np.array_equal(ids, gold[tag + "_ids"])
  assert np.array_equal(bits(depth), bits(gold[tag + "_depth"])) and np.array_equal(bits(bary), bits(gold[tag + "_weights"]))
  for mode in (0, 1):
    d, _, _, image = mr.fresh_buffers(h, w)
    mr.render_texture_py(image, v, t, gold[tag + "_texture"], gold[tag + "_tex_coords"], gold[tag + "_tex_triangles"], d, h, w, mode)
    assert np.array_equal(bits(image), bits(gold["%s_tex%d_image" % (tag, mode)])), mode
    assert np.array_equal(bits(d), bits(gold["%s_tex%d_depth" % (tag, mode)])), mode
    assert np.array_equal(bits(d), bits(gold[tag + "_depth"]))                   # one visibility rule for both rasterisers
  n = mr.get_normal_py(gold[tag + "_normal0"].copy(), gold[tag + "_tri_normal"], t)
  assert np.array_equal(bits(n), bits(gold[tag + "_normal"]))
  # the seeded inputs are the ones the maker draws
  for x, y in zip(mr.texture_inputs(v.shape[0], t.shape[0], 100 + list(mr.MESHES).index(tag)),
                  (gold[tag + "_texture"], gold[tag + "_tex_coords"], gold[tag + "_tex_triangles"])):
    assert np.array_equal(x, y)


def test_restatements_match_the_compiled_reference(gold):
  """The seed-17 mesh against oracle/_ref/libmesh_core_ref.so itself (make -C oracle), also from buffers a first pass has filled."""
  if not mr.have_compiled_reference():
    pytest.skip("oracle/_ref is not built: the goldens stand in for the compiled reference")
  tag = "m17"
  v, t, h, w = mr.mesh(tag)
  a, b = mr.fresh_buffers(h, w), mr.fresh_buffers(h, w)
  mr.rasterize_triangles_ref(v, t, a[0], a[1], a[2], h, w)
  mr.rasterize_triangles_py(v, t, b[0], b[1], b[2], h, w)
  assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], gold[tag + "_ids"])
  assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))
  v2 = v.copy()
  v2[:, 2] *= np.float32(1.5)                                    # a second mesh over the filled buffers: some pixels change, some stay
  mr.rasterize_triangles_ref(v2, t, a[0], a[1], a[2], h, w)
  mr.rasterize_triangles_py(v2, t, b[0], b[1], b[2], h, w)
  assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))
  for mode in (0, 1):
    d1, _, _, i1 = mr.fresh_buffers(h, w)
    d2, _, _, i2 = mr.fresh_buffers(h, w)
    mr.render_texture_ref(i1, v, t, gold[tag + "_texture"], gold[tag + "_tex_coords"], gold[tag + "_tex_triangles"], d1, h, w, mode)
    mr.render_texture_py(i2, v, t, gold[tag + "_texture"], gold[tag + "_tex_coords"], gold[tag + "_tex_triangles"], d2, h, w, mode)
    assert np.array_equal(bits(i1), bits(i2)) and np.array_equal(bits(d1), bits(d2))
  n1 = mr.get_normal_ref(gold[tag + "_normal0"].copy(), gold[tag + "_tri_normal"], t)
  assert np.array_equal(bits(n1), bits(gold[tag + "_normal"]))


def test_fixture_is_not_vacuous(gold):
  """Seed 17: background and coverage, covered pixels in the two-pixel border ring (no inside test there), weights outside [0, 1], an
  exact depth tie that went to the lower index, texture coordinates on both sides of the clamp."""
  tag = "m17"
  v, t, h, w = mr.mesh(tag)
  ids, bary = gold[tag + "_ids"], gold[tag + "_weights"]
  covered = ids >= 0
  assert 0.20 < covered.mean() < 0.95
  ring = np.ones((h, w), bool)
  ring[2:h - 2, 2:w - 2] = False
  assert (covered & ring).sum() > 0 and ring.sum() == 864
  assert (covered & ((bary < 0) | (bary > 1)).any(-1)).sum() >= 1
  # identical rows of the triangle list give identical arithmetic, hence equal depths wherever both are candidates: the lower index wins
  first = {}
  pairs = [(first.setdefault(tuple(row), k), k) for k, row in enumerate(t.tolist())]
  pairs = [(lo, hi) for lo, hi in pairs if lo != hi]
  assert len(pairs) >= 40
  assert sum(int((ids == lo).sum()) for lo, _ in pairs) > 0 and not any((ids == hi).any() for _, hi in pairs)
  assert np.array_equal(ids[~covered], np.full((~covered).sum(), -1)) and (gold[tag + "_depth"][~covered] == mr.DEPTH_INIT).all()
  tc = gold[tag + "_tex_coords"]
  assert (tc[:, :2] < 0).any() and (tc[:, :2] > 15).any()
  assert not np.array_equal(gold[tag + "_tex0_image"], gold[tag + "_tex1_image"])          # the two mapping modes differ
  assert not np.array_equal(gold[tag + "_normal"], gold[tag + "_normal0"]) and gold[tag + "_normal0"].any()


def test_interpolation_restatement_on_hand_values():
  tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
  attr = np.array([[1, 10], [2, 20], [4, 40], [8, 80]], np.float32)
  ids = np.array([[0, -1], [1, 0]], np.int32)
  bary = np.array([[[0.5, 0.25, 0.25], [9, 9, 9]], [[0, 1, 0], [1.5, -0.25, -0.25]]], np.float32)
  out = np.full((2, 2, 2), 7, np.float32)
  mr.interpolate_py(ids, bary, tri, attr, out)
  assert out[0, 0].tolist() == [2.0, 20.0] and out[0, 1].tolist() == [7.0, 7.0]
  assert out[1, 0].tolist() == [2.0, 20.0] and out[1, 1].tolist() == [0.0, 0.0]


def test_header_declares_the_dense_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  from voicepuppet_amd.utils import mesh_core                    # importable without a GPU
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  for name in NAMES:
    assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols(), name
  for cited in ("mesh_core.cpp:108-166", "mesh_core.cpp:234-333", "mesh_core.cpp:85-105", ":270-272", ":148"):
    assert cited in hdr, cited
  for name in ("render_colors_core", "rasterize_triangles_core", "render_texture_core", "get_normal_core", "rasterize_triangles",
               "render_texture", "interpolate", "vertex_normals", "vertex_adjacency"):
    assert callable(getattr(mesh_core, name)), name
  mk = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  assert "raster_dense.hip" in mk.split("SRCS =")[1].split("\n")[0]
  off = [l for l in mk.splitlines() if "-ffp-contract=off" in l]
  assert any("raster_dense.o" in l for l in off) and any("raster_dense.$(VAR).o" in l for l in off)      # the build and its variant form
  src = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "raster_dense.hip")).read()
  assert "#pragma clang fp contract(off)" in src


def test_library_refuses_bad_arguments():
  """The shipped library: refusals come back before any device call, so no GPU is needed."""
  from voicepuppet_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libvp_hip.so is not built: the refusals are unexercised")
  L = _lib.lib()
  p = ctypes.c_void_p(1 << 20)
  assert L.vp_rasterize_triangles_workspace_bytes(3, 40, 36) >= 3 * 40 * 36 * 8 and L.vp_rasterize_triangles_workspace_bytes(3, 0, 36) == 0
  assert L.vp_vertex_adjacency_bytes(480, 1000) >= (2 * 480 + 1 + 3000) * 4 and L.vp_vertex_adjacency_bytes(0, 5) == 0
  assert L.vp_rasterize_triangles(p, p, p, p, None, 10, 5, 8, 8, 1, p, None) == -1 and b"vp_rasterize_triangles" in L.vp_last_error()
  assert L.vp_rasterize_triangles(p, p, p, p, p, 10, 5, 8, 0, 1, p, None) == -1 and b"w 0" in L.vp_last_error()
  assert L.vp_render_texture(p, p, p, p, p, p, p, 10, 10, 10, 5, 8, 8, 4, 16, 16, 3, 0, 1, p, None) == -1 and b"c 4 > tex_c 3" in L.vp_last_error()
  assert L.vp_render_texture(p, p, p, p, p, p, p, 10, 12, 11, 5, 8, 8, 3, 16, 16, 3, 0, 1, p, None) == -1 and b"tex_rows 11" in L.vp_last_error()
  assert L.vp_raster_interpolate(p, p, p, p, p, 10, 5, 0, 8, 8, 1, None) == -1 and b"k 0" in L.vp_last_error()
  assert L.vp_vertex_adjacency_build(p, 10, 5, p, 8, None) == -1 and b"needed" in L.vp_last_error()
  assert L.vp_vertex_normals(p, p, None, 10, 5, 1, None) == -1 and b"vp_vertex_normals" in L.vp_last_error()


def test_refusals_through_the_host_build_under_sanitizers():
  """tests/mesh_core_badargs.cpp, a stand-alone program, against the `make host-asan` build of the C-ABI layer (AddressSanitizer + UBSan,
  kernels reduced to launch stubs): every bad call is refused with VP_ERR_ARG and a message, and the sanitizers stay silent."""
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  clang = "/opt/rocm/lib/llvm/bin/clang++"
  if not (os.path.exists(hipcc) and os.path.exists(clang)):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  csrc = os.path.join(ROOT, "voicepuppet_amd", "csrc")
  b = subprocess.run(["make", "-C", csrc, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  libdir = os.path.join(ROOT, "voicepuppet_amd")
  import tempfile
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "mesh_core_badargs")
    c = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mesh_core_badargs.cpp"),
                        "-L", libdir, "-l:libvp_host_asan.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "all refused" in r.stdout and "NOT-REFUSED" not in r.stdout and r.stdout.count("refused ") >= 20
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]

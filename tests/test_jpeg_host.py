"""The JPEG encoder's definition and host layer, without a GPU: the C ABI (include/vp_hip.h vp_jpeg_*) refuses what it must, and the numpy
restatement of the stream (tests/jpeg_ref.py), which the device encoder is compared with in tests/test_gpu_jpeg.py, is itself pinned
against libjpeg (PIL): same framing, same quantisation tables, quality and size within the margins of profiles/jpeg_encode.json."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as jr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Margins against PIL (quality=75, subsampling=2, restart_marker_rows=1), from the float64 restatement on the CPU (profiles/jpeg_encode.json,
# "quality"): worst PSNR deficit over the fixtures 0.086 dB (+ 0.1 dB), worst size ratio 0.9994 (+ 1 %).
PSNR_MARGIN_DB = 0.186
SIZE_MARGIN = 1.0094


def fixtures():
  z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_frames.npz"))
  fx = {k: z[k] for k in z.files}
  fx["sample22_256"] = np.load(os.path.join(ROOT, "tests", "golden", "sample22_256.npz"))["frame"]
  assert all(f.dtype == np.uint8 and f.shape[0] % 16 == 0 and f.shape[1] % 16 == 0 for f in fx.values())
  assert fx["sample22_panel"].shape == (512, 512, 3) and fx["sample22_256"].shape == (256, 256, 3)
  return fx


def pil_encode(frame, quality=75):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=2, restart_marker_rows=1)
  return buf.getvalue()


def pil_decode(data):
  from PIL import Image
  im = Image.open(io.BytesIO(data))
  im.load()
  return im


def test_header_declares_the_jpeg_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.jpeg  # noqa: F401  (importable without a GPU)
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  for name in ("vp_jpeg_desc_size", "vp_jpeg_workspace_bytes", "vp_jpeg_frame_capacity", "vp_jpeg_create", "vp_jpeg_encode", "vp_jpeg_tensor",
               "vp_jpeg_header", "vp_jpeg_destroy"):
    assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert name in _lib.exported_symbols()
  L = _lib.lib()
  assert L.vp_jpeg_desc_size() == ctypes.sizeof(_lib.JpegDesc) == 20
  body = hdr[hdr.index("typedef struct vp_jpeg_desc {"):hdr.index("} vp_jpeg_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.JpegDesc._fields_]


_REFUSALS = r"""
import ctypes, sys
sys.path.insert(0, %r)
from voicepuppet_amd import _lib
L = _lib.lib()
n = ctypes.sizeof(_lib.JpegDesc)
bad = 0
for mf, h, w, q in [(64, 512, 512, 75), (1, 256, 256, 1), (8, 16, 832, 100)]:
  d = _lib.JpegDesc(n, mf, h, w, q)
  ws, cap = L.vp_jpeg_workspace_bytes(ctypes.byref(d)), L.vp_jpeg_frame_capacity(ctypes.byref(d))
  print("ok", (mf, h, w, q), ws, cap)
  bad += ws == 0 or cap < (h // 16) * (24 * w + 2)
for what, d in [("multiples of 16", _lib.JpegDesc(n, 4, 500, 512, 75)), ("multiples of 16", _lib.JpegDesc(n, 4, 512, 520, 75)),
                ("quality", _lib.JpegDesc(n, 4, 512, 512, 0)), ("quality", _lib.JpegDesc(n, 4, 512, 512, 101)),
                ("max_frames", _lib.JpegDesc(n, 0, 512, 512, 75)), ("struct_bytes", _lib.JpegDesc(n - 4, 4, 512, 512, 75)),
                ("LDS", _lib.JpegDesc(n, 4, 512, 1024, 75))]:
  ws, msg = L.vp_jpeg_workspace_bytes(ctypes.byref(d)), L.vp_last_error().decode()
  cap = L.vp_jpeg_frame_capacity(ctypes.byref(d))
  h = ctypes.c_void_p()
  rc = L.vp_jpeg_create(ctypes.byref(d), None, 0, None, ctypes.byref(h))
  print("refused", what, ws, cap, rc, msg)
  bad += ws != 0 or cap != 0 or rc != -1 or what not in msg or h.value is not None
sys.exit(1 if bad else 0)
"""


def test_invalid_descriptors_are_refused_with_a_message():
  r = subprocess.run([sys.executable, "-c", _REFUSALS % ROOT], capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout + r.stderr


def test_invalid_descriptors_are_refused_by_the_host_build_under_sanitizers():
  """The same through `make host-asan` (the C-ABI layer under AddressSanitizer + UBSan, no GPU code), as tests/test_host_logic.py runs
  the planner."""
  import shutil
  csrc = os.path.join(ROOT, "voicepuppet_amd", "csrc")
  if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", csrc, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  so = os.path.join(ROOT, "voicepuppet_amd", "libvp_host_asan.so")
  rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
  assert os.path.exists(rt), rt
  env = dict(os.environ)
  env.update({"VP_LIB": so, "LD_PRELOAD": rt, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99", "UBSAN_OPTIONS": "halt_on_error=1:exitcode=98"})
  r = subprocess.run([sys.executable, "-c", _REFUSALS % ROOT], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name", ["sample22_panel", "background_1", "background_10", "sample22_256"])
def test_restatement_is_a_baseline_file_libjpeg_reads(name):
  frame = fixtures()[name]
  H, W = frame.shape[:2]
  coef, data = jr.encode(frame, 75)
  assert coef.shape == (H // 16, 6 * (W // 16), 64) and coef.dtype == np.int16
  im = pil_decode(data)
  assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG"
  info = jr.parse(data)
  assert info["size"] == (H, W) and info["dri"] == W // 16
  assert info["rst"] == [i % 8 for i in range(H // 16 - 1)]
  assert [m for m, _ in info["segments"]] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
  ref = pil_decode(pil_encode(frame))
  assert im.quantization == ref.quantization
  for q in (10, 100):
    assert pil_decode(jr.entropy_encode(jr.coefficients(frame[:32, :32], q), 32, 32, q)).quantization == pil_decode(pil_encode(frame[:32, :32], q)).quantization


@pytest.mark.parametrize("name", ["sample22_panel", "background_1", "background_10", "sample22_256"])
def test_restatement_quality_and_size_against_libjpeg(name):
  frame = fixtures()[name]
  data, pil = jr.encode(frame, 75)[1], pil_encode(frame)
  ours, theirs = jr.psnr(np.asarray(pil_decode(data)), frame), jr.psnr(np.asarray(pil_decode(pil)), frame)
  print("%s: %d bytes %.3f dB, PIL %d bytes %.3f dB" % (name, len(data), ours, len(pil), theirs))
  assert ours >= theirs - PSNR_MARGIN_DB, (ours, theirs)
  assert len(data) <= SIZE_MARGIN * len(pil), (len(data), len(pil))


def test_restatement_entropy_coder_corner_cases():
  """EOB-only blocks and zero DC differences (constant frame), ZRL runs, long codes and many stuffed bytes (noise): libjpeg decodes what
  the coder wrote (a code that does not match its table ends libjpeg's decode with an error or a wrong size)."""
  const = np.full((32, 48, 3), 77, np.uint8)
  coef, data = jr.encode(const, 75)
  assert np.count_nonzero(coef[:, :, 1:]) == 0
  assert np.abs(np.asarray(pil_decode(data)).astype(int) - 77).max() <= 1
  noise = np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8)
  coef, data = jr.encode(noise, 100)
  scan = data[len(jr.header(64, 64, 100)):]
  assert scan.count(b"\xff\x00") > 0
  assert pil_decode(data).size == (64, 64)
  sparse = np.zeros((1, 6, 64), np.int16)
  sparse[0, 0, 40], sparse[0, 1, 63], sparse[0, 4, 17] = 3, -1, 1023          # ZRL x 2, ZRL x 3, a 10-bit amplitude
  assert pil_decode(jr.entropy_encode(sparse, 16, 16, 75)).size == (16, 16)

"""The PNG format of vp_png_* without a GPU: the restatement (tests/png_ref.py) against PIL and zlib, its sizes, and the C ABI's
descriptor checks (include/vp_hip.h vp_png_*)."""
import ctypes
import io
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def goldens():
  out = {}
  for name in ("sample22_256.npz", "jpeg_frames.npz"):
    z = np.load(os.path.join(GOLDEN, name))
    for k in z.files:
      out[k] = z[k]
  return out


def cases():
  rng = np.random.default_rng(11)
  y, x = np.mgrid[0:40, 0:300]
  half = np.where(x + y < 170, 0, 255).astype(np.uint8)
  c = {"1x1": np.array([[[3, 200, 77]]], np.uint8),
       "17x5 grey": rng.integers(0, 256, (17, 5)).astype(np.uint8),
       "17x5 rgb": rng.integers(0, 256, (17, 5, 3)).astype(np.uint8),
       "17x5 rgba": rng.integers(0, 256, (17, 5, 4)).astype(np.uint8),
       "noise": rng.integers(0, 256, (48, 64, 3)).astype(np.uint8),
       "constant": np.full((40, 300, 3), 77, np.uint8),
       "half plane": np.stack([half, half, half], -1),
       "gradient": np.stack([(x * 255 // 299), (y * 255 // 39), (x + y) & 255], -1).astype(np.uint8),
       "frame": goldens()["frame"]}
  return c


def pil_pixels(data, shape):
  from PIL import Image
  im = Image.open(io.BytesIO(data))
  im.load()
  return np.asarray(im).reshape(shape)


@pytest.mark.parametrize("filter", [-1, 0, 1, 2, 3, 4])
def test_files_open_in_pil_and_inflate_to_the_filtered_rows(filter):
  """Every file: PIL's pixels are the input; the concatenated IDAT payload is a zlib stream of exactly the filtered rows; every chunk
  CRC and the Adler-32 hold against zlib's own."""
  for name, img in cases().items():
    data = png_ref.encode(img, filter=filter)
    assert np.array_equal(pil_pixels(data, img.shape), img), name
    chunks = png_ref.parse_chunks(data)
    assert [k for k, _, _ in chunks][:2] == [b"IHDR", b"IDAT"] and chunks[-1][0] == b"IEND", name
    for kind, payload, crc in chunks:
      assert crc == zlib.crc32(kind + payload) & 0xFFFFFFFF, (name, kind)
    idat = [p for k, p, _ in chunks if k == b"IDAT"]
    rows = png_ref.filtered_rows(img, filter)
    assert zlib.decompress(b"".join(idat)) == rows.tobytes(), name
    assert idat[0] == b"\x78\x01" and idat[-1][:2] == b"\x03\x00"
    assert struct.unpack(">I", idat[-1][2:])[0] == zlib.adler32(rows.tobytes()) & 0xFFFFFFFF, name
    if filter >= 0:
      assert set(rows[:, 0].tolist()) == {filter}
    h = img.shape[0]
    w, c = img.shape[1], (img.shape[2] if img.ndim == 3 else 1)
    assert len(idat) == 2 + -(-h // png_ref.rows_per_strip(w, c))


def test_strip_height_rule_and_to_u8():
  assert png_ref.rows_per_strip(512, 3) == 16 and png_ref.rows_per_strip(256, 3) == 16 and png_ref.rows_per_strip(512, 4) == 12
  assert png_ref.rows_per_strip(17738, 1) == 1 and png_ref.rows_per_strip(17739, 1) == 0
  x = np.array([-0.1, 0.0, 0.5 / 255.5, 1.0, 1.2, np.nan, 0.999 / 255.5, 1.0 / 255.5, 254.9 / 255.5, np.inf, -np.inf, 0.5], np.float32)
  assert png_ref.to_u8(x).tolist() == [0, 0, 0, 255, 255, 0, 0, int(np.float32(1.0 / 255.5) * np.float32(255.5)), 254, 255, 0, 127]


def test_tokens_and_length_limited_codes():
  d = np.array([5] + [9] * 600 + [1, 1, 1, 2, 2, 2, 2], np.uint8)
  assert png_ref.strip_tokens(d) == [("L", 5), ("L", 9), ("R", 258), ("R", 258), ("R", 83), ("L", 1), ("L", 1), ("L", 1), ("L", 2), ("R", 3)]
  assert png_ref.strip_tokens(np.array([7] * 261, np.uint8)) == [("L", 7), ("R", 258), ("L", 7), ("L", 7)]
  fib = [1, 1]
  while len(fib) < 24:
    fib.append(fib[-1] + fib[-2])
  lens = png_ref.huff_lengths(fib, 15)
  assert max(lens) == 15 and sum(2.0 ** -l for l in lens) <= 1.0
  assert max(png_ref.huff_lengths(fib, 32)) == 23                     # unlimited: deeper than 15
  assert png_ref.huff_lengths([0, 4, 0], 15) == [0, 1, 0]
  for seed in range(20):
    f = np.random.default_rng(seed).integers(0, 50, 19).tolist()
    lens = png_ref.huff_lengths(f, 7)
    assert max(lens) <= 7 and all((l > 0) == (c > 0) for l, c in zip(lens, f))
    if sum(c > 0 for c in f) > 1:
      assert sum(2.0 ** -l for l in lens if l) <= 1.0


def test_sizes_against_pil_level_1():
  """Over the seven golden images the files are together no larger than PIL's at compress_level=1 (zlib's fastest: what a host path in
  a hurry would use).  Per image it may lose: the matte has long diagonal edges that LZ77 matches and runs do not."""
  from PIL import Image
  ours = theirs = 0
  for name, img in goldens().items():
    data = png_ref.encode(img)
    assert np.array_equal(pil_pixels(data, img.shape), img)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG", compress_level=1)
    print("%-16s %4dx%-4d  restatement %7d  PIL level 1 %7d  ratio %.3f" % (name, img.shape[0], img.shape[1], len(data), len(buf.getvalue()),
                                                                           len(data) / len(buf.getvalue())))
    ours += len(data)
    theirs += len(buf.getvalue())
  print("sum %d against %d: %.3f" % (ours, theirs, ours / theirs))
  assert len(goldens()) == 7 and ours <= theirs


def test_constant_image_is_small_and_noise_is_bounded():
  const = np.full((64, 64, 3), 200, np.uint8)
  assert len(png_ref.encode(const)) < const.size / 20
  noise = np.random.default_rng(3).integers(0, 256, (100, 64, 3)).astype(np.uint8)
  data, info = png_ref.encode_strips(noise)
  assert all(stored for _, stored in info)
  strips = -(-100 // png_ref.rows_per_strip(64, 3))
  assert len(data) == png_ref.frame_capacity(100, 64, 3) == 47 + 30 + 100 * (1 + 64 * 3) + 22 * strips
  assert len(data) <= noise.size + 100 + 22 * strips + 77


def test_header_declares_the_png_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.png  # noqa: F401  (importable without a GPU)
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  L = _lib.lib()
  for name in ("vp_png_desc_size", "vp_png_workspace_bytes", "vp_png_frame_capacity", "vp_png_rows_per_strip", "vp_png_create", "vp_png_encode",
               "vp_png_tensor", "vp_png_header", "vp_png_destroy"):
    assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.exported_symbols(), name
  assert L.vp_png_desc_size() == ctypes.sizeof(_lib.PngDesc) == 24
  assert "png_enc.hip" in open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()


def test_png_descriptor_sizes_and_refusals():
  """Host-only entry points: the strip height and capacity rules of include/vp_hip.h as png_ref states them, and what is refused
  before anything is enqueued."""
  from voicepuppet_amd import _lib
  L = _lib.lib()

  def desc(max_frames=3, height=512, width=512, channels=3, filter=-1, struct_bytes=None):
    return _lib.PngDesc(ctypes.sizeof(_lib.PngDesc) if struct_bytes is None else struct_bytes, max_frames, height, width, channels, filter)
  for h, w, c in ((512, 512, 3), (1, 1, 3), (17, 5, 1), (17, 5, 4), (100, 2048, 4), (7, 17738, 1), (40, 300, 3)):
    d = desc(height=h, width=w, channels=c)
    assert L.vp_png_rows_per_strip(ctypes.byref(d)) == png_ref.rows_per_strip(w, c), (h, w, c)
    assert L.vp_png_frame_capacity(ctypes.byref(d)) == -(-png_ref.frame_capacity(h, w, c) // 256) * 256, (h, w, c)
    assert L.vp_png_workspace_bytes(ctypes.byref(d)) > 3 * png_ref.frame_capacity(h, w, c) - 3 * 77
  for bad, word in ((desc(struct_bytes=20), b"struct_bytes"), (desc(max_frames=0), b"max_frames"), (desc(max_frames=4097), b"max_frames"),
                    (desc(height=0), b"height"), (desc(height=65536), b"height"), (desc(width=0), b"width"), (desc(width=5913), b"width"),
                    (desc(width=17739, channels=1), b"width"), (desc(channels=2), b"channels"), (desc(channels=0), b"channels"),
                    (desc(filter=5), b"filter"), (desc(filter=-2), b"filter")):
    assert L.vp_png_workspace_bytes(ctypes.byref(bad)) == 0 and word in L.vp_last_error(), (word, L.vp_last_error())
    assert L.vp_png_frame_capacity(ctypes.byref(bad)) == 0 and L.vp_png_rows_per_strip(ctypes.byref(bad)) == 0
    h = ctypes.c_void_p()
    assert L.vp_png_create(ctypes.byref(bad), None, 0, None, ctypes.byref(h)) == -1 and not h.value
  h = ctypes.c_void_p()
  assert L.vp_png_create(ctypes.byref(desc()), None, 0, None, ctypes.byref(h)) == -3 and not h.value      # VP_ERR_WORKSPACE
  assert L.vp_png_encode(None, None, 0, 3, 0, 1, None, 0, None, None) == -1

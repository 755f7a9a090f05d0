"""The JPEG decoder's definition and host layer, without a GPU: the numpy restatement (tests/jpeg_dec_ref.py) the device decoder is compared
with in tests/test_gpu_jpeg_dec.py is pinned here against the encoder restatement (tests/jpeg_ref.py) coefficient for coefficient and against
libjpeg (PIL) byte for byte, and the product's parser (voicepuppet_amd/jpeg_dec.py::parse) against the restatement's plain loops."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_ref as dr  # noqa: E402
import jpeg_ref as jr  # noqa: E402


def _image(w, h, seed, noise=False):
  rng = np.random.default_rng(seed)
  if noise:
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
  yy, xx = np.mgrid[0:h, 0:w]
  img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 5) % 256], -1)
  return (img + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)


def _pil(img, **kw):
  from PIL import Image
  b = io.BytesIO()
  Image.fromarray(img).save(b, "JPEG", **kw)
  return b.getvalue()


def _pil_rgb(data):
  from PIL import Image
  return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# case 3: (name, width, height, PIL settings, noise)
PIL_CASES = [("16x16", 16, 16, {}, False), ("8x8", 8, 8, {}, False), ("17x33", 17, 33, {}, False), ("48x32", 48, 32, {}, False),
             ("40x24_444", 40, 24, {"subsampling": 0}, False), ("48x32_opt_q100", 48, 32, {"optimize": True, "quality": 100}, True),
             ("48x32_rst_rows", 48, 32, {"restart_marker_rows": 1}, False), ("48x32_rst_blocks", 48, 32, {"restart_marker_blocks": 1}, False)]


def pil_files():
  return {name: _pil(_image(w, h, i, noise), **kw) for i, (name, w, h, kw, noise) in enumerate(PIL_CASES)}


# case 1: (name, frame, quality)
def roundtrip_cases():
  ramp = np.repeat((np.arange(48) * 5)[None, :, None], 32, 0).repeat(3, 2).astype(np.uint8)
  return [("noise_q10", _image(48, 32, 20, True), 10), ("noise_q75", _image(48, 32, 21, True), 75), ("noise_q100", _image(32, 32, 22, True), 100),
          ("ramp", ramp, 75), ("zero_ac", np.full((32, 48, 3), 77, np.uint8), 75)]


# case 2: hand-made coefficient blocks (zig-zag order) -> files of 16 x 16 (one MCU); what each must contain
def handmade_cases():
  def blocks():
    return np.zeros((1, 6, 64), np.int16)
  c63 = blocks()
  c63[0, :, 63] = 5                              # 62 zeros: three ZRL, a run of 14, no EOB
  full = blocks()
  full[0, :, :] = np.where(np.arange(64) % 2, -1023, 1023)
  dc = blocks()
  dc[0, :4, 0] = [1023, -1024, 1023, -1024]      # Y differences 1023, -2047, 2047, -2047
  dc[0, 4, 0], dc[0, 5, 0] = 1023, -1024
  run16 = blocks()
  run16[0, :, 17] = 3                            # exactly 16 zeros in front: one ZRL, run 0
  return [("coef63", c63, ("zrl", "no_eob")), ("full_1023", full, ("no_eob", "stuffed", "long")), ("dc_2047", dc, ("long",)),
          ("run16", run16, ("zrl", "long"))]


def handmade_files():
  return {name: (c, jr.entropy_encode(c, 16, 16, 75), must) for name, c, must in handmade_cases()}


def all_files():
  """every file of cases 1-3 by name"""
  out = {"rt_" + n: jr.encode(img, q)[1] for n, img, q in roundtrip_cases()}
  out.update({"hm_" + n: f for n, (_, f, _) in handmade_files().items()})
  out.update({"pil_" + n: f for n, f in pil_files().items()})
  return out


@pytest.mark.parametrize("name", [c[0] for c in roundtrip_cases()])
def test_coefficient_round_trip_is_exact(name):
  img, q = next((i, q) for n, i, q in roundtrip_cases() if n == name)
  coef, data = jr.encode(img, q)
  got, _, _ = dr.entropy_decode(data)
  assert got.dtype == np.int16 and np.array_equal(got, coef.reshape(-1, 64))


@pytest.mark.parametrize("name", [c[0] for c in handmade_cases()])
def test_handmade_blocks_contain_their_subject_and_decode(name):
  coef, data, must = handmade_files()[name]
  got, _, stats = dr.entropy_decode(data)
  print(name, stats)
  for what in must:
    assert stats[what] > 0, "%s: the file has no %s" % (name, what)
  assert np.array_equal(got, coef.reshape(-1, 64))
  if name == "coef63":
    assert stats["zrl"] == 18 and stats["no_eob"] == 6 and stats["eob"] == 0
  if name == "run16":
    assert stats["zrl"] == 6


@pytest.mark.parametrize("name", [c[0] for c in PIL_CASES])
def test_pixels_equal_libjpeg(name):
  """Byte equality with np.asarray(Image.open(...).convert("RGB")) on every file: reached (maximum difference 0, share of differing
  pixels 0), with the up-sampling edge at the component's own ceil(W/2) x ceil(H/2) samples, which is where libjpeg replicates."""
  data = pil_files()[name]
  got, want = dr.decode(data), _pil_rgb(data)
  diff = np.abs(got.astype(int) - want.astype(int))
  print(name, "max", diff.max(), "share", (diff > 0).mean())
  assert got.shape == want.shape and np.array_equal(got, want)


def test_planes_equal_libjpeg_ycbcr():
  """The stage before up-sampling and colour: a 4:4:4 file's planes against PIL's mode YCbCr (no conversion, no up-sampling)."""
  from PIL import Image
  data = pil_files()["40x24_444"]
  info = dr.parse(data)
  pl = dr.planes(info, dr.entropy_decode(data, info)[0])
  im = Image.open(io.BytesIO(data))
  im.draft("YCbCr", im.size)
  want = np.asarray(im)
  assert want.shape == (24, 40, 3)
  for c in range(3):
    assert np.array_equal(pl[c][:24, :40], want[..., c])


def test_parse_refuses_what_is_outside_the_subset():
  from voicepuppet_amd.jpeg_dec import parse
  img = _image(32, 32, 3)
  from PIL import Image
  grey = io.BytesIO()
  Image.fromarray(img[..., 0]).save(grey, "JPEG")
  good = _pil(img)
  for what, data, kw in [("progressive", _pil(img, progressive=True), {}), ("components", grey.getvalue(), {}),
                         ("sampling", _pil(img, subsampling=1), {}), ("truncated header", good[:150], {}),
                         ("oversize", good, {"max_height": 16, "max_width": 64}), ("SOI", b"PNG" + good, {})]:
    r = parse(data, **kw)
    assert r.refused and what in r.refused, (what, r.refused)
    if what not in ("truncated header", "oversize", "SOI"):
      with pytest.raises(dr.Refused):
        dr.parse(data)
  assert parse(good).refused is None and parse(good, 32, 32).refused is None


@pytest.mark.parametrize("name", sorted(all_files()))
def test_parse_equals_the_restatement(name):
  """dimensions, sampling, table selectors, scan offset, the marker positions of the plain loop, the segment table, and the Huffman
  look-up form: every code of the file's tables, looked up the device's way, gives the restatement's symbol."""
  from voicepuppet_amd import jpeg_dec as jd
  data = all_files()[name]
  info, ref = jd.parse(data), dr.parse(data)
  assert info.refused is None
  assert (info.height, info.width) == ref["size"] and info.sampling == ref["sampling"] and info.scan == ref["scan"] and info.dri == ref["dri"]
  assert list(info.rst) == ref["rst"]
  assert [tuple(t) for t in zip(info.tq, info.td, info.ta)] == ref["tables"]
  want = dr.segments(ref)
  assert info.segments.shape == (len(want), 6)
  for row, (byte, bit, pred, mcu0, count) in zip(info.segments.tolist(), want):
    assert row == [byte, bit, 0, 0, mcu0, count]
  if ref["dri"]:
    assert len(want) == len(ref["rst"]) + 1 and [s[0] for s in want[1:]] == [r + 2 for r in ref["rst"]]
  blob = jd.meta_blob(info)
  assert len(blob) == jd.META_BYTES + 24 * len(want) and len(blob) % 8 == 0
  for comp in range(3):
    q = np.frombuffer(blob, np.uint16, 64, 128 + 128 * info.tq[comp])
    assert np.array_equal(q, ref["quant"][ref["tables"][comp][0]])
  for (tc, th), (bits, vals) in ref["huff"].items():
    at = 640 + 1424 * (2 * tc + th)
    lut = np.frombuffer(blob, np.uint16, 512, at)
    maxcode, valoff = np.frombuffer(blob, np.int32, 18, at + 1024), np.frombuffer(blob, np.int32, 18, at + 1096)
    v = np.frombuffer(blob, np.uint8, 256, at + 1168)
    for (length, code), sym in dr._decoder_table(bits, vals).items():
      look = (code << 16 >> length) | ((1 << (16 - length)) - 1)       # the code followed by ones
      e = int(lut[look >> 7])
      if length <= jd.LOOKUP_BITS:
        assert e == (length << 8) | sym
      else:
        assert e == 0
        hit = next(l for l in range(jd.LOOKUP_BITS + 1, 17) if (look >> (16 - l)) <= maxcode[l])
        assert hit == length and v[(code + valoff[length]) & 255] == sym


@pytest.mark.parametrize("name", [c[0] for c in PIL_CASES])
def test_index_segments_reproduce_the_whole_scan_decode(name):
  """The entries a decode records, fed back as one segment per MCU row, give the same coefficients segment by segment (a restart
  interval shorter than a row is crossed inside the segment)."""
  data = pil_files()[name]
  info = dr.parse(data)
  whole, entries, _ = dr.entropy_decode(data, info, [(info["scan"], 0, (0, 0, 0), 0, info["mcux"] * info["mcuy"])])
  assert sorted(entries) == list(range(info["mcuy"]))
  per_row = info["mcux"] * info["bpm"]
  for r, seg in enumerate(dr.entry_segments(info, entries)):
    out = np.full_like(whole, 12345)
    dr.decode_segment(data, info, seg, out)
    assert np.array_equal(out[r * per_row:(r + 1) * per_row], whole[r * per_row:(r + 1) * per_row])
    assert (out[:r * per_row] == 12345).all() and (out[(r + 1) * per_row:] == 12345).all()
  assert np.array_equal(whole, dr.entropy_decode(data, info)[0])


def test_header_declares_the_jpegdec_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.jpeg_dec  # noqa: F401  (importable without a GPU)
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  L = _lib.lib()
  for name in ("vp_jpegdec_desc_size", "vp_jpegdec_workspace_bytes", "vp_jpegdec_create", "vp_jpegdec_destroy", "vp_jpegdec_decode",
               "vp_jpegdec_tensor"):
    assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.exported_symbols()
  assert L.vp_jpegdec_desc_size() == ctypes.sizeof(_lib.JpegDecDesc) == 28
  body = hdr[hdr.index("typedef struct vp_jpegdec_desc {"):hdr.index("} vp_jpegdec_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.JpegDecDesc._fields_]
  assert ctypes.sizeof(_lib.JpegDecFile) == 56
  assert "#define VP_JPEGDEC_META_BYTES %d" % _lib.JPEGDEC_META_BYTES in hdr
  src = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  assert "jpeg_dec.hip" in src.split("SRCS =")[1].split("\n")[0]
  n = ctypes.sizeof(_lib.JpegDecDesc)
  assert L.vp_jpegdec_workspace_bytes(ctypes.byref(_lib.JpegDecDesc(n, 64, 256, 768, 1 << 20, 4096, 1))) > 64 * 3 * 256 * 768
  for what, d in [("max_files", _lib.JpegDecDesc(n, 0, 64, 64, 1 << 20, 64, 1)), ("max_height", _lib.JpegDecDesc(n, 1, 0, 64, 1 << 20, 64, 1)),
                  ("max_width", _lib.JpegDecDesc(n, 1, 64, 9000, 1 << 20, 64, 1)), ("max_file_bytes", _lib.JpegDecDesc(n, 1, 64, 64, 0, 64, 1)),
                  ("max_segments_per_file", _lib.JpegDecDesc(n, 1, 64, 64, 1 << 20, 0, 1)), ("bgr", _lib.JpegDecDesc(n, 1, 64, 64, 1 << 20, 64, 2)),
                  ("struct_bytes", _lib.JpegDecDesc(n - 4, 1, 64, 64, 1 << 20, 64, 1))]:
    assert L.vp_jpegdec_workspace_bytes(ctypes.byref(d)) == 0 and what in L.vp_last_error().decode(), what
    h = ctypes.c_void_p()
    assert L.vp_jpegdec_create(ctypes.byref(d), None, 0, ctypes.byref(h)) == -1 and not h.value


def test_parse_refuses_a_restart_file_whose_markers_are_missing():
  """A file with a restart interval cut in the middle of its scan has fewer markers than intervals: no lane would own the MCUs behind the
  last marker, so the parser refuses it (the data generator then hands it to PIL, which raises as it does without the flag) and the
  restatement reports it corrupt."""
  from voicepuppet_amd.jpeg_dec import parse
  good = pil_files()["48x32_rst_rows"]
  assert parse(good).refused is None
  info = dr.parse(good)
  cut = good[:info["rst"][0] - 3]
  r = parse(cut)
  assert r.refused and "restart markers missing" in r.refused
  with pytest.raises(dr.Corrupt):
    dr.segments(dr.parse(cut))
  blocks = pil_files()["48x32_rst_blocks"]
  b = bytearray(blocks)
  at = dr.parse(blocks)["rst"][2]
  b[at + 1] = 0xc8                                   # a marker that is no RSTn ends the scan early
  assert "restart markers missing" in parse(bytes(b)).refused


def test_parse_gives_a_reason_for_an_empty_sos_segment():
  from voicepuppet_amd.jpeg_dec import parse
  good = pil_files()["16x16"]
  at = good.index(b"\xff\xda")
  r = parse(good[:at] + b"\xff\xda\x00\x02" + good[at + 4:])
  assert r.refused == "truncated header"

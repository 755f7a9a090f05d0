"""4:2:2 and table-less JPEG files, without a GPU: the restatement of the third layout (tests/jpeg_dec_422_ref.py) against libjpeg (PIL)
byte for byte, and the product's parser flags (voicepuppet_amd/jpeg_dec.py::parse accept_422, default_huffman) against it."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_422_ref as r4  # noqa: E402
import jpeg_dec_ref as dr  # noqa: E402
from test_jpeg_dec_host import _image, _pil, _pil_rgb, pil_files  # noqa: E402

# (name, H, W, PIL settings, noise): every one subsampling=1, i.e. components 2x1, 1x1, 1x1
CASES_422 = [("8x16", 8, 16, {"quality": 50}, False), ("17x33", 17, 33, {"quality": 90}, False), ("41x15", 41, 15, {"quality": 50}, False),
             ("9x1", 9, 1, {"quality": 90}, False), ("33x2", 33, 2, {"quality": 50}, False), ("64x47", 64, 47, {"quality": 90}, True),
             ("64x47_opt", 64, 47, {"quality": 50, "optimize": True}, True), ("17x33_rst", 17, 33, {"quality": 90, "restart_marker_blocks": 2}, False),
             ("48x96", 48, 96, {"quality": 90}, True)]


def files_422():
  return {name: _pil(_image(w, h, 40 + i, noise), subsampling=1, **kw) for i, (name, h, w, kw, noise) in enumerate(CASES_422)}


def strip_dht(data, keep=()):
  """the file without its DHT segments (all of them, or all but those whose first table is (class, id) in keep)"""
  data = bytes(data)
  out, p = [data[:2]], 2
  while data[p + 1] != 0xda:
    n = int.from_bytes(data[p + 2:p + 4], "big")
    if data[p + 1] != 0xc4 or (data[p + 4] >> 4, data[p + 4] & 15) in keep:
      out.append(data[p:p + 2 + n])
    p += 2 + n
  return b"".join(out) + data[p:]


def dht_bodies(data):
  """{(class, id): (BITS, HUFFVAL)} of a file's DHT segments"""
  data, p, out = bytes(data), 2, {}
  while data[p + 1] != 0xda:
    n = int.from_bytes(data[p + 2:p + 4], "big")
    if data[p + 1] == 0xc4:
      body, q = data[p + 4:p + 2 + n], 0
      while q < len(body):
        bits = body[q + 1:q + 17]
        out[(body[q] >> 4, body[q] & 15)] = (bits, body[q + 17:q + 17 + sum(bits)])
        q += 17 + sum(bits)
    p += 2 + n
  return out


@pytest.mark.parametrize("name", [c[0] for c in CASES_422])
def test_422_pixels_equal_libjpeg(name):
  data = files_422()[name]
  info = r4.parse(data)
  h, w = next((c[1], c[2]) for c in CASES_422 if c[0] == name)
  assert info["sampling"] == 3 and info["bpm"] == 4 and info["size"] == (h, w)
  assert (info["mcux"], info["mcuy"]) == (-(-w // 16), -(-h // 8))
  assert bool(info["dri"]) == name.endswith("_rst") and (not info["dri"] or len(info["rst"]) > 0)
  got, want = r4.decode(data), _pil_rgb(data)
  diff = np.abs(got.astype(int) - want.astype(int))
  print(name, "max", diff.max(), "share", (diff > 0).mean())
  assert got.shape == want.shape and np.array_equal(got, want)


def test_the_restated_segment_loop_equals_jpeg_dec_ref_on_its_own_layouts():
  """jpeg_dec_422_ref restates the header walk and the segment loop for any block sequence: on 4:2:0 and 4:4:4 files, with and without
  restart markers, it gives jpeg_dec_ref's dictionary, coefficients, entries and pixels."""
  for name in ("17x33", "40x24_444", "48x32_opt_q100", "48x32_rst_blocks"):
    data = pil_files()[name]
    a, b = r4.parse(data), dr.parse(data)
    assert sorted(a) == sorted(b)
    for k in a:
      assert np.array_equal(a[k], b[k]) if k != "quant" else all(np.array_equal(a[k][t], b[k][t]) for t in b[k]), k
    ca, ea = r4.entropy_decode(data, a)
    cb, eb, _ = dr.entropy_decode(data, b)
    assert np.array_equal(ca, cb) and ea == eb
    assert np.array_equal(r4.decode(data), dr.decode(data))


@pytest.mark.parametrize("name", [c[0] for c in CASES_422])
def test_parse_accept_422_equals_the_restatement(name):
  from voicepuppet_amd import jpeg_dec as jd
  data = files_422()[name]
  refused = jd.parse(data)
  assert refused.refused and "sampling" in refused.refused
  with pytest.raises(dr.Refused):
    dr.parse(data)
  info, ref = jd.parse(data, accept_422=True), r4.parse(data)
  assert info.refused is None
  assert (info.height, info.width) == ref["size"] and info.sampling == 3 and info.scan == ref["scan"] and info.dri == ref["dri"]
  assert (info.mcux, info.mcuy) == (ref["mcux"], ref["mcuy"]) and list(info.rst) == ref["rst"]
  assert [tuple(t) for t in zip(info.tq, info.td, info.ta)] == ref["tables"]
  want = dr.segments(ref)
  assert info.segments.tolist() == [[byte, bit, 0, 0, mcu0, count] for byte, bit, _, mcu0, count in want]
  assert sum(s[4] for s in want) == info.mcux * info.mcuy
  blob = jd.meta_blob(info)
  assert len(blob) == jd.META_BYTES + 24 * len(want) and np.frombuffer(blob, np.int32, 8).tolist()[3:6] == [3, info.mcux, info.mcuy]
  for (tc, th), (bits, vals) in ref["huff"].items():
    at = 640 + 1424 * (2 * tc + th)
    assert blob[at:at + 1424] == jd._huff_table(bytes(bits), bytes(vals))
  # a size limit still refuses, and the 4:2:0 / 4:4:4 files parse as without the flag
  assert "oversize" in jd.parse(data, info.height - 1, info.width, accept_422=True).refused
  plain = pil_files()["17x33"]
  assert jd.parse(plain, accept_422=True, default_huffman=True).__dict__.keys() == jd.parse(plain).__dict__.keys()
  assert jd.parse(plain, accept_422=True, default_huffman=True).tables == jd.parse(plain).tables


def test_k3_constants_are_the_tables_pil_writes():
  from voicepuppet_amd import jpeg_dec as jd
  for kw in ({"subsampling": 1, "quality": 50}, {"quality": 95}, {"subsampling": 0, "quality": 20}):
    bodies = dht_bodies(_pil(_image(32, 24, 7), **kw))
    assert sorted(bodies) == [(0, 0), (0, 1), (1, 0), (1, 1)] == sorted(jd.K3_HUFFMAN)
    for k, (bits, vals) in bodies.items():
      assert (bytes(bits), bytes(vals)) == jd.K3_HUFFMAN[k]
      assert len(bits) + len(vals) + 1 == {0: 29, 1: 179}[k[0]]


def test_default_huffman_fills_the_tables_a_file_leaves_out():
  from voicepuppet_amd import jpeg_dec as jd
  for name, kw in (("17x33", {"accept_422": True}), ("8x16", {"accept_422": True})):
    data = files_422()[name]
    bare = strip_dht(data)
    assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")] and len(bare) == len(data) - 4 * 4 - 2 * 29 - 2 * 179
    no = jd.parse(bare, **kw)
    assert no.refused and "table the scan uses is missing" in no.refused
    full, filled = jd.parse(data, **kw), jd.parse(bare, default_huffman=True, **kw)
    assert filled.refused is None and filled.tables == full.tables
    assert filled.scan == full.scan - (len(data) - len(bare)) and (filled.mcux, filled.mcuy, filled.sampling) == (full.mcux, full.mcuy, 3)
    assert _pil_rgb(bare).tobytes() == _pil_rgb(data).tobytes()         # libjpeg implies the same tables
  # the same for a 4:2:0 file, without the other flag
  data = pil_files()["17x33"]
  assert jd.parse(strip_dht(data), default_huffman=True).tables == jd.parse(data).tables
  assert jd.parse(strip_dht(data)).refused


def test_tables_the_file_defines_win_over_the_defaults():
  """An optimize=True file has tables of its own.  With some of them stripped, the ones left are the file's, and the rest K.3's."""
  from voicepuppet_amd import jpeg_dec as jd
  data = files_422()["64x47_opt"]
  own = dht_bodies(data)
  assert all((bytes(own[k][0]), bytes(own[k][1])) != jd.K3_HUFFMAN[k] for k in own)
  full = jd.parse(data, accept_422=True, default_huffman=True)
  assert full.tables == jd.parse(data, accept_422=True).tables
  part = jd.parse(strip_dht(data, keep=((0, 0), (1, 1))), accept_422=True, default_huffman=True)
  assert part.refused is None
  for i, k in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
    got = part.tables[512 + 1424 * i:512 + 1424 * (i + 1)]
    assert got == (jd._huff_table(bytes(own[k][0]), bytes(own[k][1])) if k in ((0, 0), (1, 1)) else jd._huff_table(*jd.K3_HUFFMAN[k]))


def test_index_segments_reproduce_the_whole_scan_decode_422():
  data = files_422()["48x96"]
  info = r4.parse(data)
  whole, entries = r4.entropy_decode(data, info)
  assert sorted(entries) == list(range(6)) and info["mcux"] == 6
  per_row = info["mcux"] * 4
  for r, seg in enumerate(dr.entry_segments(info, entries)):
    out = np.full_like(whole, 12345)
    r4.decode_segment(data, info, seg, out)
    assert np.array_equal(out[r * per_row:(r + 1) * per_row], whole[r * per_row:(r + 1) * per_row])
    assert (out[:r * per_row] == 12345).all() and (out[(r + 1) * per_row:] == 12345).all()

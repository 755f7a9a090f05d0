"""The device JPEG decoder's third layout, 4:2:2 (sampling 3), and frames without Huffman tables, against the restatement
(tests/jpeg_dec_422_ref.py, pinned against libjpeg byte for byte in tests/test_jpeg_dec_422_host.py) and against PIL: coefficients and
pixels exactly, alone and inside a mixed batch that crosses a launch group, layout, segmentation invariance, the index scan, malformed
data and the C ABI's refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_422_ref as r4  # noqa: E402
from jpeg_ref import ZIGZAG  # noqa: E402
from test_jpeg_dec_422_host import CASES_422, files_422, strip_dht  # noqa: E402
from test_jpeg_dec_host import _image, _pil, _pil_rgb, pil_files  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}
MAX_H, MAX_W = 64, 96


def reference(name, data):
  """(info, coefficients row-major inside a block, RGB pixels) of the restatement, computed once per file"""
  if name not in _REF:
    info = r4.parse(data)
    coef = r4.entropy_decode(data, info)[0]
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef
    _REF[name] = (info, nat, r4.pixels(info, r4.planes(info, coef)))
  return _REF[name]


def _decoder(key, *a, **kw):
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  if ("dec", key) not in _REF:
    _REF[("dec", key)] = JpegDecoder(*a, accept_422=True, default_huffman=True, **kw)
  return _REF[("dec", key)]


def _batch_decoders():
  return {bgr: _decoder(("batch", bgr), 34, MAX_H, MAX_W, bgr=bgr) for bgr in (False, True)}


def _mixed_batch(data):
  """34 files: `data` at 0, 31 and 32 (the launch group is 32 files), 4:4:4, 4:2:0 and other 4:2:2 files between"""
  p, q = pil_files(), files_422()
  fill = [("p17x33", p["17x33"]), ("p40x24_444", p["40x24_444"]), ("q17x33", q["17x33"]), ("p48x32_opt_q100", p["48x32_opt_q100"]),
          ("q41x15", q["41x15"]), ("p48x32_rst_rows", p["48x32_rst_rows"])]
  batch = [fill[i % len(fill)] for i in range(34)]
  for at in (0, 31, 32):
    batch[at] = (None, data)
  return batch


@pytest.mark.parametrize("name", [c[0] for c in CASES_422])
def test_422_coefficients_and_pixels_equal_the_restatement_and_pil(name):
  data = files_422()[name]
  info, coef, rgb = reference(name, data)
  H, W = info["size"]
  assert np.array_equal(rgb, _pil_rgb(data))
  batch = _mixed_batch(data)
  for bgr, dec in _batch_decoders().items():
    out, status = dec.decode([data])
    assert status.cpu().tolist() == [0]
    assert np.array_equal(dec.tensor("coefficients")[0, :len(coef)].cpu().numpy(), coef)
    px = out[0].cpu().numpy()
    assert np.array_equal(px[:H, :W], rgb[..., ::-1] if bgr else rgb)
    assert int(px[H:].max() if H < MAX_H else 0) == 0 and int(px[:, W:].max() if W < MAX_W else 0) == 0
    # chroma fills the left half of its plane: ceil(W / 2) columns of H rows hold the component
    out, status = dec.decode([b for _, b in batch])
    assert status.cpu().tolist() == [0] * 34
    host, co = out.cpu().numpy(), dec.tensor("coefficients").cpu().numpy()
    for i, (other, blob) in enumerate(batch):
      oi, oc, orgb = reference(other or name, blob)
      h, w = oi["size"]
      assert np.array_equal(host[i, :h, :w], orgb[..., ::-1] if bgr else orgb), (i, other)
      assert np.array_equal(co[i, :len(oc)], oc), (i, other)


def test_422_layout_pitch_stride_and_guard_bytes():
  import torch
  q = files_422()
  names = ["17x33", "41x15", "9x1", "64x47", "33x2"]
  dec = _batch_decoders()[True]
  out = torch.full((6, 70, 67, 3), 0xa5, dtype=torch.uint8, device="cuda")[:, :, :66]      # pitch 201: odd rows are not dword aligned
  _, status = dec.decode([q[n] for n in names], out=out)
  assert status.cpu().tolist() == [0] * 5
  host = out.cpu().numpy()
  base = out._base.cpu().numpy()
  assert (host[5] == 0xa5).all() and (base[:, :, 66:] == 0xa5).all()
  for i, n in enumerate(names):
    info, _, rgb = reference(n, q[n])
    H, W = info["size"]
    assert np.array_equal(host[i, :H, :W], rgb[..., ::-1]), n
    assert (host[i, H:] == 0xa5).all() and (host[i, :, W:] == 0xa5).all(), n


def test_422_segmentation_invariance():
  """A 48 x 96 file (6 MCU rows of 6 MCUs) as one lane, from the entries that decode recorded (one lane per MCU row), and its
  restart-marker re-saves (an interval of one MCU row, and one of 4 MCUs that rows do not divide)."""
  from voicepuppet_amd import jpeg_dec as jd
  dec = _batch_decoders()[False]
  img = _image(96, 48, 48, True)
  plain = files_422()["48x96"]
  info, coef, rgb = reference("48x96", plain)
  a, st = dec.decode([plain])
  assert st.cpu().tolist() == [0] and dec.last_segments == [1]
  a = a.cpu().numpy().copy()
  entries = dec.tensor("entries")[0, :6].cpu().numpy().copy()
  _, want = r4.entropy_decode(plain, info)
  for r in range(6):
    byte, bit, p = want[r]
    assert entries[r].tolist()[:2] == [byte, bit]
    assert int(entries[r, 2]) & 0xffffffff == (p[0] & 0xffff) | ((p[1] & 0xffff) << 16) and entries[r, 3] == (p[2] & 0xffff)
  b, st = dec.decode([plain], indexes=[entries])
  assert st.cpu().tolist() == [0] and dec.last_segments == [6]
  assert np.array_equal(b.cpu().numpy(), a) and np.array_equal(dec.tensor("coefficients")[0, :len(coef)].cpu().numpy(), coef)
  assert np.array_equal(a[0, :48, :96], rgb)
  for kw, dri, lanes in (({"restart_marker_rows": 1}, 6, 6), ({"restart_marker_blocks": 4}, 4, 9)):
    marked = _pil(img, subsampling=1, quality=90, **kw)
    assert jd.parse(marked, accept_422=True).dri == dri
    c, st = dec.decode([marked])
    assert st.cpu().tolist() == [0] and dec.last_segments == [lanes]
    assert np.array_equal(c[0, :48, :96].cpu().numpy(), reference("48x96_dri%d" % dri, marked)[2])


def test_422_index_scan_finds_the_entries_of_the_one_lane_decode():
  plain = files_422()["48x96"]
  info, coef, rgb = reference("48x96", plain)
  off = _batch_decoders()[False]
  a, st = off.decode([plain])
  assert st.cpu().tolist() == [0] and off.last_segments == [1]
  entries = off.tensor("entries")[0, :6].cpu().numpy().copy()
  on = _decoder("scan32", 2, MAX_H, MAX_W, bgr=False, scan_chunk_bytes=32)
  b, st = on.decode([plain])
  assert st.cpu().tolist() == [0]
  assert on.tensor("scan_ok")[:1].cpu().tolist() == [1] and on.last_segments == [6]
  assert np.array_equal(on.tensor("entries")[0, :6].cpu().numpy(), entries)
  assert np.array_equal(b[0, :48, :96].cpu().numpy(), rgb)
  assert np.array_equal(on.tensor("coefficients")[0, :len(coef)].cpu().numpy(), coef)


def test_422_frame_without_huffman_tables():
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  data = files_422()["17x33"]
  bare = strip_dht(data)
  want = _pil_rgb(bare)
  assert np.array_equal(want, reference("17x33", data)[2])
  out, st = _batch_decoders()[False].decode([bare, data])
  assert st.cpu().tolist() == [0, 0]
  assert np.array_equal(out[0, :17, :33].cpu().numpy(), want) and np.array_equal(out[1, :17, :33].cpu().numpy(), want)
  strict = JpegDecoder(1, MAX_H, MAX_W, bgr=False)
  with pytest.raises(ValueError, match="sampling"):
    strict.decode([data])
  with pytest.raises(ValueError, match="table the scan uses is missing"):
    JpegDecoder(1, MAX_H, MAX_W, bgr=False, accept_422=True).decode([bare])


def test_422_file_cut_in_its_entropy_data_gives_status_minus_one():
  """One call: a good file, the same file cut in the middle of its scan (every decoder runs out of data there), the good file again."""
  import torch
  good = files_422()["64x47"]
  info, _, rgb = reference("64x47", good)
  cut = good[:(info["scan"] + len(good)) // 2]
  with pytest.raises(r4.dr.Corrupt):
    r4.entropy_decode(cut, r4.parse(cut))
  dec = _batch_decoders()[False]
  guard = 4096
  buf = torch.full((3 * MAX_H * MAX_W * 3 + guard,), 0x3c, dtype=torch.uint8, device="cuda")
  out = buf[:3 * MAX_H * MAX_W * 3].view(3, MAX_H, MAX_W, 3)
  _, status = dec.decode([good, cut, good], out=out)
  assert status.cpu().tolist() == [0, -1, 0]
  host = out.cpu().numpy()
  assert np.array_equal(host[0, :64, :47], rgb) and np.array_equal(host[2, :64, :47], rgb)
  assert (buf[-guard:] == 0x3c).all()


def test_the_c_abi_refuses_a_sampling_it_does_not_know():
  import torch
  from voicepuppet_amd import jpeg_dec as jd
  dec = _batch_decoders()[False]
  data = files_422()["17x33"]
  out = torch.full((1, MAX_H, MAX_W, 3), 0x5a, dtype=torch.uint8, device="cuda")
  status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
  for sampling in (4, 0):
    info = jd.parse(data, accept_422=True)
    info.sampling = sampling
    with pytest.raises(RuntimeError, match=r"1: 4:4:4, 2: 4:2:0, 3: 4:2:2"):
      dec.enqueue(dec.pack([(data, info, None, None, "f")]), out, out.stride(1), out.stride(0), status)
  torch.cuda.synchronize()
  assert (out == 0x5a).all() and status.cpu().tolist() == [77]
  good, st = dec.decode([data])                      # the handle is as it was
  assert st.cpu().tolist() == [0] and np.array_equal(good[0, :17, :33].cpu().numpy(), reference("17x33", data)[2])

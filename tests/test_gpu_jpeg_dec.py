"""The device JPEG decoder (libvp_hip.so vp_jpegdec_*, voicepuppet_amd.jpeg_dec) against its numpy restatement (tests/jpeg_dec_ref.py, itself
pinned against libjpeg byte for byte in tests/test_jpeg_dec_host.py): coefficients and pixels exactly, layout, segmentation invariance and
malformed data."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_ref as dr  # noqa: E402
from jpeg_ref import ZIGZAG  # noqa: E402
from test_jpeg_dec_host import _image, _pil, all_files  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, data):
  """(info, coefficients row-major inside a block, RGB pixels) of the restatement, computed once per file"""
  if name not in _REF:
    info = dr.parse(data)
    coef = dr.entropy_decode(data, info)[0]
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef
    _REF[name] = (info, nat, dr.pixels(info, dr.planes(info, coef)))
  return _REF[name]


def _decoders():
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  if "dec" not in _REF:
    _REF["dec"] = {bgr: JpegDecoder(8, 64, 192, bgr=bgr) for bgr in (False, True)}
  return _REF["dec"]


@pytest.mark.parametrize("name", sorted(all_files()))
def test_coefficients_and_pixels_equal_the_restatement(name):
  data = all_files()[name]
  info, coef, rgb = reference(name, data)
  H, W = info["size"]
  for bgr, dec in _decoders().items():
    out, status = dec.decode([data])
    assert status.cpu().tolist() == [0]
    got = dec.tensor("coefficients")[0, :len(coef)].cpu().numpy()
    assert np.array_equal(got, coef)
    px = out[0, :H, :W].cpu().numpy()
    assert np.array_equal(px, rgb[..., ::-1] if bgr else rgb)
    assert int(out[0, H:].max() if H < 64 else 0) == 0 and int(out[0, :, W:].max()) == 0


def test_layout_pitch_stride_and_batch_position():
  """Five files of different sizes and table sets in one call into a pre-filled buffer with a pitch and stride larger than any image:
  nothing outside an image's W x H changes, and every file equals its own single-file decode."""
  import torch
  files = all_files()
  names = ["pil_17x33", "pil_40x24_444", "pil_48x32_opt_q100", "pil_48x32_rst_blocks", "rt_noise_q10"]
  dec = _decoders()[True]
  out = torch.full((6, 70, 67, 3), 0xa5, dtype=torch.uint8, device="cuda")[:, :, :66]      # pitch 201: odd rows are not dword aligned
  got, status = dec.decode([files[n] for n in names], out=out)
  assert status.cpu().tolist() == [0] * 5
  host = out.cpu().numpy()
  assert (host[5] == 0xa5).all()
  for i, n in enumerate(names):
    info, _, rgb = reference(n, files[n])
    H, W = info["size"]
    assert np.array_equal(host[i, :H, :W], rgb[..., ::-1]), n
    assert (host[i, H:] == 0xa5).all() and (host[i, :, W:] == 0xa5).all(), n
    single, st = dec.decode([files[n]])
    assert st.cpu().tolist() == [0] and np.array_equal(single[0, :H, :W].cpu().numpy(), host[i, :H, :W]), n


def test_segmentation_invariance():
  """A 64 x 192 file without restart markers as one segment, from the index that decode recorded (one lane per MCU row: 4 segments), and
  its restart_marker_rows=1 re-save by its markers."""
  from voicepuppet_amd import jpeg_dec as jd
  dec = _decoders()[False]
  img = _image(192, 64, 40)
  plain, marked = _pil(img, quality=90), _pil(img, quality=90, restart_marker_rows=1)
  a, st = dec.decode([plain])
  assert st.cpu().tolist() == [0] and dec.last_segments == [1]
  a = a.cpu().numpy().copy()
  coef_a = dec.tensor("coefficients")[0].cpu().numpy().copy()
  entries = dec.tensor("entries")[0, :4].cpu().numpy().copy()
  info = dr.parse(plain)
  _, want, _ = dr.entropy_decode(plain, info)
  assert [tuple(e[:2]) for e in entries.tolist()] == [want[r][:2] for r in range(4)]
  for r in range(4):
    p = want[r][2]
    assert int(entries[r, 2]) & 0xffffffff == (p[0] & 0xffff) | ((p[1] & 0xffff) << 16) and entries[r, 3] == (p[2] & 0xffff)
  b, st = dec.decode([plain], indexes=[entries])
  assert st.cpu().tolist() == [0] and dec.last_segments == [4]
  assert np.array_equal(b.cpu().numpy(), a) and np.array_equal(dec.tensor("coefficients")[0].cpu().numpy(), coef_a)
  assert np.array_equal(a[0], reference("seg_plain", plain)[2])
  c, st = dec.decode([marked])
  assert st.cpu().tolist() == [0] and dec.last_segments == [4] and jd.parse(marked).dri == 12
  assert np.array_equal(c[0].cpu().numpy(), reference("seg_marked", marked)[2])


def test_index_cache_by_path_and_npz_round_trip(tmp_path):
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  dec = _decoders()[True]
  dec.index.clear()
  paths = []
  for i in range(2):
    p = str(tmp_path / ("%d.jpg" % i))
    with open(p, "wb") as f:
      f.write(_pil(_image(96, 48, 50 + i), quality=90))
    paths.append(p)
  first, st = dec.decode(paths)
  first = first.cpu().numpy().copy()
  assert st.cpu().tolist() == [0, 0] and dec.last_segments == [1, 1]
  second, st = dec.decode(paths)                    # the first call's entries were harvested: one lane per MCU row
  assert st.cpu().tolist() == [0, 0] and dec.last_segments == [3, 3]
  assert np.array_equal(second.cpu().numpy(), first)
  dec.save_index(str(tmp_path / "index.npz"))
  other = JpegDecoder(2, 48, 96, bgr=True)
  other.load_index(str(tmp_path / "index.npz"))
  assert sorted(other.index) == sorted(dec.index) and all(np.array_equal(other.index[k], dec.index[k]) for k in dec.index)
  third, st = other.decode(paths)
  assert st.cpu().tolist() == [0, 0] and other.last_segments == [3, 3] and np.array_equal(third.cpu().numpy(), first[:, :48, :96])


def _malformed():
  """A file cut in the middle of its scan and one with a run of flipped bytes in the scan, chosen by a seeded search on the CPU for
  which the restatement reports failure."""
  good = _pil(_image(64, 48, 60, True), quality=90)
  info = dr.parse(good)
  rng = np.random.default_rng(61)
  out = []
  for kind in ("cut", "flip"):
    for _ in range(200):
      at = int(rng.integers(info["scan"] + 8, len(good) - 16))
      if kind == "cut":
        bad = good[:at]
      else:
        b = bytearray(good)
        for i in range(at, at + 6):
          b[i] ^= 0x5a if b[i] ^ 0x5a != 0xff else 0x5b
        bad = bytes(b)
      try:
        dr.entropy_decode(bad, dr.parse(bad))
      except dr.Corrupt:
        out.append(bad)
        break
    else:
      raise AssertionError("no %s point under which the restatement fails" % kind)
  return good, out


def test_malformed_data_is_survived():
  """Bounded code on malformed data: status -1 or a clean decode, the other files of the call unaffected, the guard regions behind the
  output and the workspace unchanged."""
  import torch
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  good, (cut, flip) = _malformed()
  dec = JpegDecoder(4, 48, 64, bgr=False)
  ws_used = dec.L.vp_jpegdec_workspace_bytes(__import__("ctypes").byref(dec.desc))
  guard = 4096
  # the decoder's own workspace tensor is exactly ws_used bytes: give it one with a guard behind
  big = torch.full((ws_used + guard,), 0x3c, dtype=torch.uint8, device="cuda")
  import ctypes
  h = ctypes.c_void_p()
  dec.L.vp_jpegdec_destroy(dec.h)
  dec.workspace = big
  assert dec.L.vp_jpegdec_create(ctypes.byref(dec.desc), ctypes.c_void_p(big.data_ptr()), ws_used, ctypes.byref(h)) == 0
  dec.h = h
  buf = torch.full((4 * 48 * 64 * 3 + guard,), 0x3c, dtype=torch.uint8, device="cuda")
  out = buf[:4 * 48 * 64 * 3].view(4, 48, 64, 3)
  _, status = dec.decode([good, cut, good, flip], out=out)
  st = status.cpu().tolist()
  assert st[0] == 0 and st[2] == 0 and st[1] in (0, -1) and st[3] in (0, -1)
  assert st[1] == -1                                  # a cut scan runs out of data on any decoder
  want = reference("malformed_good", good)[2]
  host = out.cpu().numpy()
  assert np.array_equal(host[0], want) and np.array_equal(host[2], want)
  assert (buf[-guard:] == 0x3c).all() and (big[-guard:] == 0x3c).all()

"""The device index scan (JpegDecoder(scan_chunk_bytes=...), vp_jpegdec_enable_scan, jpegdec_scan_kernel): a first decode that already runs
one lane per MCU row, against the scan's Python restatement (tests/jpeg_scan_ref.py: entries, verdict and rounds int for int), the decoder's
numpy restatement (tests/jpeg_dec_ref.py: coefficients and pixels byte for byte) and the same decoder without the scan."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_ref as dr  # noqa: E402
import jpeg_scan_ref as sr  # noqa: E402
from jpeg_ref import ZIGZAG  # noqa: E402
from test_jpeg_dec_host import _image, _pil  # noqa: E402
from test_jpeg_scan_host import CASES, TRIPTYCH, scan_files, scanned, serial, triptych  # noqa: E402

pytestmark = pytest.mark.gpu
_REF = {}


def reference(name, data):
  """(info, coefficients row-major inside a block, RGB pixels) of the restatement, once per file"""
  if name not in _REF:
    info = dr.parse(data)
    coef = serial(name, data)[0]
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef
    _REF[name] = (info, nat, dr.pixels(info, dr.planes(info, coef)))
  return _REF[name]


def _decoder(key, *a, **kw):
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  if key not in _REF:
    _REF[key] = JpegDecoder(*a, **kw)
  return _REF[key]


def _check_first_sight(name, data, on, off, chunk):
  """the assertions of a first decode by a scan-enabled decoder `on`; `off`: the same decoder without the scan"""
  info, coef, rgb = reference(name, data)
  H, W = info["size"]
  want = scanned(name, data, chunk)
  assert want.ok
  out, status = on.decode([data])
  assert status.cpu().tolist() == [0]
  assert on.tensor("scan_ok")[:1].cpu().tolist() == [1]
  assert on.last_segments == [info["mcuy"]]
  assert np.array_equal(on.tensor("entries")[0, :info["mcuy"]].cpu().numpy(), want.entries_int)
  assert on.tensor("scan_rounds")[:1].cpu().tolist() == [want.rounds]
  got_coef = on.tensor("coefficients")[0, :len(coef)].cpu().numpy()
  px = out[0, :H, :W].cpu().numpy()
  assert np.array_equal(got_coef, coef) and np.array_equal(px, rgb)
  ref, st = off.decode([data])
  assert st.cpu().tolist() == [0] and off.last_segments == [1]
  assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy())
  assert np.array_equal(off.tensor("coefficients")[0, :len(coef)].cpu().numpy(), got_coef)
  assert np.array_equal(off.tensor("entries")[0, :info["mcuy"]].cpu().numpy(), want.entries_int)
  assert on.harvest() == [] and on.last_scan_rounds == [want.rounds]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_first_decode_runs_by_rows_and_equals_the_restatements(name):
  on = _decoder("on32", 8, 64, 192, bgr=False, scan_chunk_bytes=32)
  off = _decoder("off", 8, 64, 192, bgr=False)
  _check_first_sight(name, scan_files()[name], on, off, 32)


@pytest.mark.parametrize("chunk", [32, 128])
def test_more_chunks_than_lanes_are_scanned_in_sweeps(chunk):
  data = triptych()
  assert scanned(TRIPTYCH[0], data, chunk).sweeps > 1
  on = _decoder("tri%d" % chunk, 1, 256, 768, bgr=False, scan_chunk_bytes=chunk)
  off = _decoder("tri_off", 1, 256, 768, bgr=False)
  _check_first_sight(TRIPTYCH[0], data, on, off, chunk)


def _mixed():
  """33 files: un-indexed multi-row files, one with restart markers (1), one given its index (2), a single-MCU-row 8 x 8 file (3), a gap (4)"""
  plain = list(scan_files().values())
  files = [plain[i % len(plain)] for i in range(33)]
  files[1] = _pil(_image(96, 48, 90), quality=90, restart_marker_rows=1)
  files[3] = _pil(_image(8, 8, 91), quality=90)
  indexes = [None] * 33
  indexes[2] = sr.entries_int(dr.entropy_decode(files[2])[1], dr.parse(files[2])["mcuy"])
  return files, indexes


def _decode_with_gap(dec, files, indexes, gap):
  import torch
  items = dec.items(files, indexes)
  items[gap] = None
  out = torch.full((len(files), 64, 192, 3), 0xa5, dtype=torch.uint8, device="cuda")
  status = torch.empty(len(files), dtype=torch.int32, device="cuda")
  dec.decode_into(items, out, out.stride(1), out.stride(0), status, raise_bad=False)
  torch.cuda.synchronize()
  return out.cpu().numpy(), status.cpu().tolist(), dec.tensor("coefficients")[:len(files)].cpu().numpy(), list(dec.last_segments)


def test_mixed_batch_across_two_launch_groups():
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  files, indexes = _mixed()
  on = JpegDecoder(33, 64, 192, bgr=True, scan_chunk_bytes=32)
  off = JpegDecoder(33, 64, 192, bgr=True)
  a = _decode_with_gap(on, files, indexes, 4)
  b = _decode_with_gap(off, files, indexes, 4)
  assert a[1] == b[1] == [0] * 33
  assert np.array_equal(a[0], b[0]) and (a[0][4] == 0xa5).all()
  rows = [0 if i == 4 else dr.parse(f)["mcuy"] for i, f in enumerate(files)]
  for i in range(33):
    if i != 4:
      n = rows[i] * dr.parse(files[i])["mcux"] * dr.parse(files[i])["bpm"]
      assert np.array_equal(a[2][i, :n], b[2][i, :n]), i
  scanned_rows = [i for i in range(33) if i not in (1, 2, 3, 4)]
  ok = on.tensor("scan_ok")[:33].cpu().tolist()
  assert ok == [1 if i in scanned_rows else 0 for i in range(33)]
  assert a[3] == [rows[i] for i in range(33)]              # by rows: scanned, by markers (1: one interval per row), from the index (2); 1 and 0
  assert b[3] == [rows[i] if i in (1, 2) else (0 if i == 4 else 1) for i in range(33)]
  rounds = on.tensor("scan_rounds")[:33].cpu().tolist()
  assert all((rounds[i] > 0) == (i in scanned_rows) for i in range(33))


def test_one_round_is_not_enough_and_the_file_is_decoded_by_one_lane():
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  dec = JpegDecoder(1, 64, 192, bgr=False, scan_chunk_bytes=32, scan_max_rounds=1)
  verdicts = []
  for name, data in scan_files().items():
    info, coef, rgb = reference(name, data)
    H, W = info["size"]
    want = sr.scan(data, 32, max_rounds=1)
    out, status = dec.decode([data])
    assert status.cpu().tolist() == [0] and np.array_equal(out[0, :H, :W].cpu().numpy(), rgb), name
    ok = dec.tensor("scan_ok")[:1].cpu().tolist()[0]
    assert ok == int(want.ok) and dec.tensor("scan_rounds")[:1].cpu().tolist() == [1], name
    assert dec.last_segments == [info["mcuy"] if ok else 1], name
    verdicts.append(ok)
  assert 0 in verdicts


def _malformed():
  """tests/test_gpu_jpeg_dec.py's recipe (a cut and a run of flipped bytes in the scan for which the restatement reports failure, by a
  seeded search on the CPU), and two more: an EOI marker written into the scan, a frame header that claims 64 rows for a 48-row scan."""
  good = _pil(_image(64, 48, 60, True), quality=90)
  info = dr.parse(good)
  rng = np.random.default_rng(61)
  out = []
  for kind in ("cut", "flip", "marker"):
    for _ in range(200):
      at = int(rng.integers(info["scan"] + 8, len(good) - 16))
      if kind == "cut":
        bad = good[:at]
      else:
        b = bytearray(good)
        if kind == "flip":
          for i in range(at, at + 6):
            b[i] ^= 0x5a if b[i] ^ 0x5a != 0xff else 0x5b
        else:
          b[at:at + 2] = b"\xff\xd9"
        bad = bytes(b)
      try:
        dr.entropy_decode(bad, dr.parse(bad))
      except dr.Corrupt:
        out.append(bad)
        break
    else:
      raise AssertionError("no %s point under which the restatement fails" % kind)
  at = good.index(b"\xff\xc0") + 5
  assert good[at:at + 2] == (48).to_bytes(2, "big")
  out.append(good[:at] + (64).to_bytes(2, "big") + good[at + 2:])
  return good, out


def test_malformed_data_takes_the_bounded_one_lane_path():
  """Statuses and every row of status 0 equal the decoder without the scan; no damaged file's scan holds; the guard behind the output
  and the scan workspace's own tail are untouched."""
  import torch
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  good, bad = _malformed()
  files = [good] + bad + [good]
  on = JpegDecoder(6, 64, 64, bgr=False, scan_chunk_bytes=32)
  off = JpegDecoder(6, 64, 64, bgr=False)
  guard = 4096
  outs = []
  for dec in (on, off):
    buf = torch.full((6 * 64 * 64 * 3 + guard,), 0x3c, dtype=torch.uint8, device="cuda")
    out, status = dec.decode(files, out=buf[:6 * 64 * 64 * 3].view(6, 64, 64, 3))
    outs.append((out.cpu().numpy(), status.cpu().tolist()))
    assert (buf[-guard:] == 0x3c).all()
  (a, sa), (b, sb) = outs
  assert sa == sb and sa[0] == 0 and sa[5] == 0 and sa[1] == -1 and sa[4] == -1
  for i in range(6):
    if sa[i] == 0:
      assert np.array_equal(a[i], b[i]), i
  assert np.array_equal(a[0, :48], reference("malformed_good", good)[2])
  ok = on.tensor("scan_ok")[:6].cpu().tolist()
  assert ok[0] == 1 and ok[5] == 1 and ok[1] == 0 and ok[3] == 0 and ok[4] == 0
  assert on.last_segments[0] == 3 and on.last_segments[1] == 1


def test_pipeline_first_epoch_runs_by_rows_and_equals_the_host_decode(tmp_path):
  """FramePrefetcher with device_jpeg_decode and device_jpeg_scan=128 on a folder of 8 small triptychs: the first-epoch batches are the
  PIL path's bit for bit under the same seed, every file runs by rows at first sight, and the index cache is full after one epoch."""
  import torch
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  S, N = 64, 2
  folder = tmp_path / "clip"
  folder.mkdir()
  for i in range(8):
    (folder / ("%d.jpg" % i)).write_bytes(_pil(_image(3 * S, S, 100 + i), quality=90))
  (tmp_path / "train.txt").write_text("%s|8\n" % folder)

  def batches(on, scan):
    g = PixReferDataGenerator(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "params.yml"))
    p = g.params
    p.dataset_path, p.batch_size, p.img_size, p.shuffle_bufsize = str(tmp_path / "train.txt"), N, S, 1
    amd = dict(p.get("amd") or {})
    amd["device_jpeg_decode"], amd["device_jpeg_scan"] = on, scan
    p.amd = amd
    g.set_params(p)
    assert g.device_jpeg_decode == on and g.device_jpeg_scan == scan
    random.seed(5)
    it = g.get_device_dataset().make_one_shot_iterator()
    out, segs = [], []
    for _ in range(4):                                  # one epoch: 8 samples
      b = it.next_batch()
      torch.cuda.synchronize()
      out.append([t.cpu().numpy().copy() for t in b])
      segs.append(list(it._pf.segments_used))
    return out, segs, it
  host, _, _ = batches(False, 0)
  dev, segs, it = batches(True, 128)
  for a, b in zip(host, dev):
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  assert it._pf.decoder.scan_chunk_bytes == 128
  assert segs[0] == [S // 16] * (2 * N), segs             # the very first batch: one lane per MCU row
  dec = it._pf.decoder
  assert dec.harvest() == []
  assert len(dec.index) == 8 and all(v.shape == (S // 16, 4) for v in dec.index.values())
  for key, v in dec.index.items():
    data = open(key[0], "rb").read()
    assert np.array_equal(v, sr.entries_int(dr.entropy_decode(data)[1], S // 16)), key[0]
  assert len(dec.last_scan_rounds) == 2 * N and max(dec.last_scan_rounds) > 0

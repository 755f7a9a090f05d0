"""The device index scan's definition, without a GPU: the plain Python restatement (tests/jpeg_scan_ref.py) of jpegdec_scan_kernel finds, chunk
by chunk, the entry points the serial decode of tests/jpeg_dec_ref.py records; how many fixed-point rounds that takes; and the C ABI."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_ref as dr  # noqa: E402
import jpeg_scan_ref as sr  # noqa: E402
from test_jpeg_dec_host import _image, _pil  # noqa: E402

# (name, width, height, seed, noise, PIL settings).  stuffed_start and long_straddle: seeds found by a search over seeds 0 .. 63 for the
# condition their test asserts (a chunk of 32 bytes that starts on the stuffed 0x00 of an 0xff 0x00 pair; a code longer than 9 bits
# across a chunk end)
CASES = [("96x48_q90", 96, 48, 70, False, {"quality": 90}),
         ("96x48_q50", 96, 48, 71, True, {"quality": 50}),
         ("96x48_444_q100", 96, 48, 72, True, {"quality": 100, "subsampling": 0}),
         ("64x48_q100", 64, 48, 73, True, {"quality": 100}),
         ("64x48_444_q50_opt", 64, 48, 74, False, {"quality": 50, "subsampling": 0, "optimize": True}),
         ("64x48_q90_opt", 64, 48, 75, True, {"quality": 90, "optimize": True}),
         ("17x19_q90", 17, 19, 76, False, {"quality": 90}),
         ("17x19_444_q100_opt", 17, 19, 77, True, {"quality": 100, "subsampling": 0, "optimize": True}),
         ("stuffed_start", 96, 48, 0, True, {"quality": 100}),
         ("long_straddle", 96, 48, 0, True, {"quality": 90})]
CHUNKS = (32, 64, 128)
TRIPTYCH = ("triptych_256x768_noise_q95", 768, 256, 78, True, {"quality": 95})
MAX_ROUNDS_DEFAULT = 512         # JpegDecoder(scan_max_rounds=...)
_CACHE = {}


def scan_files():
  if "files" not in _CACHE:
    _CACHE["files"] = {name: _pil(_image(w, h, seed, noise), **kw) for name, w, h, seed, noise, kw in CASES}
  return _CACHE["files"]


def triptych():
  if "triptych" not in _CACHE:
    name, w, h, seed, noise, kw = TRIPTYCH
    _CACHE["triptych"] = _pil(_image(w, h, seed, noise), **kw)
  return _CACHE["triptych"]


def scanned(name, data, chunk):
  """the restatement's scan of a file, once per (file, chunk size)"""
  if (name, chunk) not in _CACHE:
    _CACHE[(name, chunk)] = sr.scan(data, chunk)
  return _CACHE[(name, chunk)]


def serial(name, data):
  """(coefficients, entries) of the serial decode, once per file: entropy_decode for the small files, the same code row by row for the
  triptych (test_oracle_by_rows_is_the_serial_decode)"""
  if ("serial", name) not in _CACHE:
    _CACHE[("serial", name)] = dr.entropy_decode(data)[:2] if len(data) < 1 << 15 else sr.oracle_by_rows(data)
  return _CACHE[("serial", name)]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_scan_entries_equal_the_serial_decode(name):
  data = scan_files()[name]
  info = dr.parse(data)
  want = dr.entropy_decode(data, info)[1]
  assert sorted(want) == list(range(info["mcuy"])) and info["mcuy"] >= 2
  for chunk in CHUNKS:
    got = scanned(name, data, chunk)
    print(name, chunk, "chunks", got.chunks, "rounds", got.rounds)
    assert got.ok and got.sweeps == 1 and got.blocks == info["mcux"] * info["mcuy"] * info["bpm"]
    assert got.entries == want, chunk
    assert np.array_equal(got.entries_int, sr.entries_int(want, info["mcuy"]))


def test_oracle_by_rows_is_the_serial_decode():
  for name, data in scan_files().items():
    coef, entries, _ = dr.entropy_decode(data)
    got = sr.oracle_by_rows(data)
    assert np.array_equal(got[0], coef) and got[1] == entries, name


def test_scan_of_the_noise_triptych_in_sweeps():
  """More chunks than a workgroup has lanes: sweeps, each from the settled exit of the chunk before."""
  name, data = TRIPTYCH[0], triptych()
  want = serial(name, data)[1]
  assert sorted(want) == list(range(16))
  for chunk in CHUNKS:
    got = scanned(name, data, chunk)
    print(name, chunk, "chunks", got.chunks, "sweeps", got.sweeps, "rounds", got.rounds)
    assert got.chunks > sr.SCAN_LANES and got.sweeps > 1
    assert got.ok and got.entries == want, chunk
  name = "96x48_444_q100"                       # and a small file in sweeps of 64 chunks: nothing changes
  small = sr.scan(scan_files()[name], 32, lanes=64)
  assert small.ok and small.sweeps > 8 and small.entries == scanned(name, scan_files()[name], 32).entries


def test_a_chunk_starts_on_a_stuffed_zero():
  data = scan_files()["stuffed_start"]
  got = scanned("stuffed_start", data, 32)
  assert got.cold_on_stuffed >= 1 and got.ok and got.entries == dr.entropy_decode(data)[1]


def test_a_long_code_lies_across_a_chunk_end():
  data = scan_files()["long_straddle"]
  got = scanned("long_straddle", data, 32)
  assert got.straddles >= 1 and got.ok and got.entries == dr.entropy_decode(data)[1]


def test_bounded_rounds_and_damaged_files_are_reported_not_trusted():
  """max_rounds 1 on a file that needs more: not ok.  A flipped byte run in the scan: whatever the walk makes of it, the verdict is only
  ok when the block total is right and no settled lane met an invalid code - and then the entries are the serial decode's."""
  data = scan_files()["96x48_444_q100"]
  assert scanned("96x48_444_q100", data, 32).rounds > 1
  one = sr.scan(data, 32, max_rounds=1)
  assert not one.ok and one.rounds == 1
  info = dr.parse(data)
  rng = np.random.default_rng(5)
  verdicts = []
  for _ in range(12):
    b = bytearray(data)
    at = int(rng.integers(info["scan"] + 8, len(data) - 16))
    for i in range(at, at + 6):
      b[i] ^= 0x5a if b[i] ^ 0x5a != 0xff else 0x5b
    bad = bytes(b)
    got = sr.scan(bad, 32, max_rounds=64)
    verdicts.append(got.ok)
    try:
      want = dr.entropy_decode(bad, dr.parse(bad))[1]
    except dr.Corrupt:
      want = None
    if got.ok and want is not None:
      assert got.entries == want
  assert not all(verdicts)
  cut = sr.scan(data[:len(data) // 2], 32, max_rounds=64)
  assert not cut.ok


# rounds the restatement needs (the last, unchanged round included; the most over a file's sweeps) per file and chunk size.  Dense noise
# (quality 100, or 95 on the triptych) has almost no end-of-block symbols to fall into step on, so there the count is about the number
# of chunks of a sweep's longest unsettled run; the photographic-like files settle in a handful of rounds.
EXPECTED_ROUNDS = {"96x48_q90": {"32": 17, "64": 9, "128": 5},
                   "96x48_q50": {"32": 12, "64": 6, "128": 3},
                   "96x48_444_q100": {"32": 157, "64": 79, "128": 40},
                   "64x48_q100": {"32": 112, "64": 54, "128": 28},
                   "64x48_444_q50_opt": {"32": 2, "64": 1, "128": 1},
                   "64x48_q90_opt": {"32": 76, "64": 36, "128": 18},
                   "17x19_q90": {"32": 3, "64": 1, "128": 1},
                   "17x19_444_q100_opt": {"32": 38, "64": 20, "128": 10},
                   "stuffed_start": {"32": 204, "64": 100, "128": 51},
                   "long_straddle": {"32": 64, "64": 32, "128": 13},
                   "triptych_256x768_noise_q95": {"32": 209, "64": 105, "128": 53}}
RECORD = os.path.join(ROOT, "profiles", "jpeg_scan.json")


def rounds_needed():
  return {name: {str(chunk): scanned(name, data, chunk).rounds for chunk in CHUNKS}
          for name, data in list(scan_files().items()) + [(TRIPTYCH[0], triptych())]}


def rounds_record(rounds):
  return {"lanes_per_sweep": sr.SCAN_LANES, "rounds_by_file_and_chunk_bytes": rounds, "most": max(max(v.values()) for v in rounds.values()),
          "scan_max_rounds_default": MAX_ROUNDS_DEFAULT}


def test_rounds_needed_are_recorded_and_the_default_bound_is_twice_the_most():
  """The fixed-point rounds every file takes equal the counts held here and the record in profiles/jpeg_scan.json as committed (this
  test writes nothing; `python tests/test_jpeg_scan_host.py` rewrites the record's restatement_rounds after a deliberate change).
  JpegDecoder's default scan_max_rounds is at least twice the most."""
  rounds = rounds_needed()
  print(json.dumps(rounds))
  assert rounds == EXPECTED_ROUNDS
  most = max(max(v.values()) for v in rounds.values())
  assert 2 * most <= MAX_ROUNDS_DEFAULT
  import inspect
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  assert inspect.signature(JpegDecoder.__init__).parameters["scan_max_rounds"].default == MAX_ROUNDS_DEFAULT
  assert inspect.signature(JpegDecoder.__init__).parameters["scan_chunk_bytes"].default is None
  with open(RECORD) as f:
    assert json.load(f)["restatement_rounds"] == rounds_record(rounds)


def test_header_declares_the_scan_abi_and_refuses_bad_chunk_sizes():
  from voicepuppet_amd import _lib
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  L = _lib.lib()
  for name in ("vp_jpegdec_scan_workspace_bytes", "vp_jpegdec_enable_scan"):
    assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.exported_symbols()
  assert L.vp_jpegdec_desc_size() == ctypes.sizeof(_lib.JpegDecDesc) == 28 and ctypes.sizeof(_lib.JpegDecFile) == 56
  d = _lib.JpegDecDesc(ctypes.sizeof(_lib.JpegDecDesc), 64, 256, 768, 1 << 20, 4096, 1)
  sizes = [L.vp_jpegdec_scan_workspace_bytes(ctypes.byref(d), c) for c in (32, 128, 4096)]
  assert sizes[0] >= 32 * (1 << 20) // 32 * 8 and sizes[0] > sizes[1] > sizes[2] > 0
  for bad in (0, 48, 8192):
    assert L.vp_jpegdec_scan_workspace_bytes(ctypes.byref(d), bad) == 0
    why = L.vp_last_error().decode()
    assert "chunk_bytes %d" % bad in why and "power of two" in why, why
  d.max_files = 0
  assert L.vp_jpegdec_scan_workspace_bytes(ctypes.byref(d), 128) == 0 and "max_files" in L.vp_last_error().decode()
  # enable_scan is host only: refused values name themselves, a decoder without the call has no scan tensors
  d.max_files = 2
  h, ws = ctypes.c_void_p(), L.vp_jpegdec_workspace_bytes(ctypes.byref(d))
  fake = ctypes.c_void_p(1 << 20)                    # never dereferenced by the host entry points
  assert L.vp_jpegdec_create(ctypes.byref(d), fake, ws, ctypes.byref(h)) == 0
  p, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
  assert L.vp_jpegdec_tensor(h, b"scan_ok", ctypes.byref(p), shp) != 0 and "vp_jpegdec_enable_scan" in L.vp_last_error().decode()
  need = L.vp_jpegdec_scan_workspace_bytes(ctypes.byref(d), 128)
  assert L.vp_jpegdec_enable_scan(h, fake, need, 48, 32) != 0 and "chunk_bytes" in L.vp_last_error().decode()
  assert L.vp_jpegdec_enable_scan(h, fake, need, 128, 0) != 0 and "max_rounds" in L.vp_last_error().decode()
  assert L.vp_jpegdec_enable_scan(h, fake, need, 128, 1025) != 0 and "max_rounds" in L.vp_last_error().decode()
  assert L.vp_jpegdec_enable_scan(h, fake, need - 1, 128, 32) != 0 and "too small" in L.vp_last_error().decode()
  assert L.vp_jpegdec_enable_scan(h, fake, need, 128, 32) == 0
  for name in (b"scan_ok", b"scan_rounds"):
    assert L.vp_jpegdec_tensor(h, name, ctypes.byref(p), shp) == 0 and list(shp)[:1] == [2] and p.value
  L.vp_jpegdec_destroy(h)


def test_launcher_flag_and_config_key():
  """train_pixrefer.py --device_jpeg_scan [N]: the bare flag means 128 bytes, a following number is N; the flag overrides
  amd.device_jpeg_scan whenever it is given, a 0 (off) included."""
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  from voicepuppet_amd.pixrefer.train_pixrefer import parse_options
  base = ["--config_path", "params.yml"]
  assert parse_options(base).device_jpeg_scan is None
  assert parse_options(base + ["--device_jpeg_scan"]).device_jpeg_scan == 128
  assert parse_options(["--device_jpeg_scan"] + base).device_jpeg_scan == 128
  assert parse_options(base + ["--device_jpeg_scan", "64"]).device_jpeg_scan == 64
  assert parse_options(base + ["--device_jpeg_scan=256"]).device_jpeg_scan == 256
  assert parse_options(base + ["--device_jpeg_scan", "0"]).device_jpeg_scan == 0
  o = parse_options(["--device_jpeg_scan", "--steps", "3"] + base)
  assert (o.device_jpeg_scan, o.steps, o.config_path) == (128, 3, "params.yml")

  def configured(key, forced):
    g = PixReferDataGenerator(os.path.join(ROOT, "config", "params.yml"))
    p = g.params
    p.dataset_path, p.batch_size = os.path.join(ROOT, "config", "absent.txt"), 2
    amd = dict(p.get("amd") or {})
    amd["device_jpeg_scan"] = key
    p.amd = amd
    if forced is not None:
      g.force_device_jpeg_scan = forced
    g.set_params(p)
    return g.device_jpeg_scan
  assert [configured(0, None), configured(128, None), configured(0, 64), configured(128, 64), configured(128, 0)] == [0, 128, 64, 64, 0]


if __name__ == "__main__":                           # regenerate the record's restatement_rounds; everything else in the file is kept
  rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
  rec["restatement_rounds"] = rounds_record(rounds_needed())
  with open(RECORD, "w") as f:
    f.write(json.dumps(rec, indent=1) + "\n")

"""The AVI layout and writer without a GPU (voicepuppet_amd/avi.py host_segment, AviWriter; include/vp_hip.h vp_avimux_*): files read back
by an independent reader (tests/avi_ref.py), the sample conversion rule, splitting at max_bytes, the refusals, the C ABI's descriptor
checks and the launchers' flags."""
import ctypes
import io
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avi_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_jpeg(h, w, seed):
  from PIL import Image
  rng = np.random.default_rng(seed)
  y, x = np.mgrid[0:h, 0:w]
  img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
  buf = io.BytesIO()
  Image.fromarray(img).save(buf, "JPEG", quality=75)
  return buf.getvalue()


def signal_s16(n, seed=0):
  s = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)
  if n >= 4:
    s[:4] = (-32768, 32767, 0, -1)
  return s


def as_f32(s16):
  return s16.astype(np.float32) / np.float32(32768.0)        # how WavLoader and the stream ingest hand int16 on


def write(path, pushes, width, height, **kw):
  """pushes: [(jpegs, pcm_f32 or None)] -> the writer's paths."""
  from voicepuppet_amd.avi import AviWriter, host_segment
  w = AviWriter(str(path), width, height, **kw)
  for jpegs, pcm in pushes:
    w.append(*host_segment(jpegs, pcm))
  w.close()
  return w.paths


@pytest.mark.parametrize("h,w", [(16, 16), (16, 48), (512, 512)])
def test_file_reads_back_frames_and_audio_exactly(tmp_path, h, w):
  """PIL-encoded frames and a known int16 signal, a frame and 40 ms per push: the reader accepts the file, the frames are the input
  bytes and decode with PIL, the audio is the int16 input."""
  from PIL import Image
  n = 5
  jpegs = [pil_jpeg(h, w, i) for i in range(n)]
  s16 = signal_s16(640 * n)
  paths = write(tmp_path / "a.avi", [([jpegs[i]], as_f32(s16[640 * i:640 * (i + 1)])) for i in range(n)], w, h)
  assert paths == [str(tmp_path / "a.avi")]
  a = avi_ref.check(paths[0], w, h)
  assert a.video == jpegs
  for p in a.video:
    im = Image.open(io.BytesIO(p))
    im.load()
    assert im.size == (w, h)
  assert np.array_equal(np.frombuffer(b"".join(a.audio), "<i2"), s16)
  assert [c[0] for c in a.chunks] == [b"01wb", b"00dc"] * n                  # interleaved: a push's audio, then its frame
  assert a.avih["dwMaxBytesPerSec"] == round(sum(8 + len(p) + (len(p) & 1) for _, _, p in a.chunks) / (n * 0.04))


def test_segment_layout_odd_even_and_single_byte_lengths():
  from voicepuppet_amd.avi import FCC_00DC, FCC_01WB, host_segment
  jpegs = [b"\xff", b"ab", b"abc", bytes(range(64)), bytes(range(65))]
  seg, ent = host_segment(jpegs, np.array([0.5, -0.5, 0.25], np.float32))
  assert ent.dtype == np.uint32 and ent.shape == (6, 4)
  want = b"01wb" + struct.pack("<I3h", 6, 16384, -16384, 8192)
  for j in jpegs:
    want += b"00dc" + struct.pack("<I", len(j)) + j + (b"\0" if len(j) & 1 else b"")
  assert seg == want and len(seg) % 2 == 0
  assert ent[:, 0].tolist() == [FCC_01WB] + [FCC_00DC] * 5 and set(ent[:, 1].tolist()) == {0x10}
  assert ent[:, 3].tolist() == [6, 1, 2, 3, 64, 65]
  at = 0
  for ckid, _, off, n in ent.tolist():
    assert off == at and seg[off:off + 8] == struct.pack("<II", ckid, n)
    at += 8 + n + (n & 1)
  assert at == len(seg)


def test_audio_only_frames_only_and_empty_segments(tmp_path):
  from voicepuppet_amd.avi import host_segment
  s16 = signal_s16(1280, 3)
  j = [pil_jpeg(16, 16, 1), pil_jpeg(16, 16, 2)]
  seg, ent = host_segment([], as_f32(s16[:640]))
  assert seg[:4] == b"01wb" and ent.shape == (1, 4) and len(seg) == 8 + 1280
  seg, ent = host_segment(j, None)
  assert seg[:4] == b"00dc" and ent.shape == (2, 4)
  for empty in (None, np.zeros(0, np.float32)):
    seg, ent = host_segment([], empty)
    assert seg == b"" and ent.shape == (0, 4)
  assert host_segment(j, np.zeros(0, np.float32))[0] == host_segment(j)[0]                  # zero samples: no audio chunk
  pushes = [([], as_f32(s16[:640])), ([], None), (j[:1], None), ([], np.zeros(0, np.float32)), (j[1:], as_f32(s16[640:]))]
  a = avi_ref.check(write(tmp_path / "b.avi", pushes, 16, 16)[0], 16, 16)
  assert a.video == j and np.array_equal(np.frombuffer(b"".join(a.audio), "<i2"), s16)
  assert [c[0] for c in a.chunks] == [b"01wb", b"00dc", b"01wb", b"00dc"]
  a = avi_ref.check(write(tmp_path / "none.avi", [], 16, 16)[0], 16, 16)                     # no push at all: a valid, empty file
  assert a.video == [] and a.audio == [] and a.avih["dwMaxBytesPerSec"] == 0


def test_sample_conversion_rule():
  """clamp(rint(x * 32768), -32768, 32767), half to even, NaN 0; every int16 / 32768 comes back as it was."""
  from voicepuppet_amd.avi import pcm_s16
  x = np.array([1.0, -1.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 0.0, -0.0,
                0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 32766.5 / 32768, 32767.5 / 32768, -32767.5 / 32768,
                0.49 / 32768, 0.51 / 32768, 32767 / 32768.0, -32768 / 32768.0], np.float32)
  want = [32767, -32768, 32767, -32768, 32767, -32768, 0, 32767, -32768, 0, 0,
          0, 2, 2, 0, -2, -2, 32766, 32767, -32768,
          0, 1, 32767, -32768]
  got = pcm_s16(x)
  assert got.dtype == np.dtype("<i2") and got.tolist() == want
  every = np.arange(-32768, 32768).astype(np.int16)
  assert np.array_equal(pcm_s16(as_f32(every)), every)


@pytest.mark.parametrize("pushes", [1, 2, 7])
def test_any_push_split_gives_the_same_payloads(tmp_path, pushes):
  n = 14
  jpegs = [pil_jpeg(16, 48, i)[:len(pil_jpeg(16, 48, i)) - (i % 3)] for i in range(n)]          # lengths of both parities (payload is opaque)
  s16 = signal_s16(640 * n, 5)

  def run(k, name):
    per = n // k
    parts = [(jpegs[i * per:(i + 1) * per], as_f32(s16[640 * i * per:640 * (i + 1) * per])) for i in range(k)]
    return avi_ref.check(write(tmp_path / name, parts, 48, 16)[0], 48, 16)
  a, b = run(pushes, "k.avi"), run(14, "each.avi")
  assert a.video == b.video == jpegs
  assert b"".join(a.audio) == b"".join(b.audio) == s16.astype("<i2").tobytes()
  assert len(a.audio) == pushes


def test_max_bytes_splits_into_valid_parts(tmp_path):
  """A max_bytes that holds four pushes of about 2 KB: ten pushes make three files, each accepted by the reader and under max_bytes,
  and their payloads concatenate to those of one file."""
  n = 10
  jpegs = [pil_jpeg(16, 48, i) for i in range(n)]
  s16 = signal_s16(640 * n, 7)
  pushes = [([jpegs[i]], as_f32(s16[640 * i:640 * (i + 1)])) for i in range(n)]
  one = 8 + 1280 + 8 + max(len(j) + 1 for j in jpegs)
  limit = 324 + 8 + 4 * (one + 32)
  paths = write(tmp_path / "p.avi", pushes, 48, 16, max_bytes=limit)
  assert paths == [str(tmp_path / f) for f in ("p.avi", "p.part1.avi", "p.part2.avi")]
  video, audio = [], b""
  for p in paths:
    assert os.path.getsize(p) <= limit
    a = avi_ref.check(p, 48, 16)
    assert a.video and a.audio
    video += a.video
    audio += b"".join(a.audio)
  whole = avi_ref.check(write(tmp_path / "w.avi", pushes, 48, 16)[0], 48, 16)
  assert video == whole.video == jpegs and audio == b"".join(whole.audio) == s16.astype("<i2").tobytes()


def test_close_twice_del_and_refusals(tmp_path):
  from voicepuppet_amd.avi import AviWriter, host_segment
  seg, ent = host_segment([pil_jpeg(16, 16, 0)], np.zeros(640, np.float32))
  w = AviWriter(str(tmp_path / "c.avi"), 16, 16)
  w.append(seg, ent)
  w.close()
  before = open(tmp_path / "c.avi", "rb").read()
  w.close()
  assert open(tmp_path / "c.avi", "rb").read() == before
  avi_ref.check(before, 16, 16)
  with pytest.raises(ValueError):
    w.append(seg, ent)                                   # append after close
  w = AviWriter(str(tmp_path / "d.avi"), 16, 16)
  w.append(seg, ent)
  del w                                                  # __del__ closes
  assert avi_ref.check(str(tmp_path / "d.avi"), 16, 16).video == [pil_jpeg(16, 16, 0)]
  for bad in (dict(width=0), dict(height=-1), dict(width=70000), dict(frame_us=0), dict(sample_rate=0), dict(max_bytes=100), dict(max_bytes=1 << 32)):
    args = dict(width=16, height=16)
    args.update(bad)
    with pytest.raises(ValueError):
      AviWriter(str(tmp_path / "e.avi"), **args)
  w = AviWriter(str(tmp_path / "f.avi"), 16, 16, max_bytes=1000)
  with pytest.raises(ValueError):
    w.append(seg[:-2], ent)                              # entries that do not end where the segment ends
  with pytest.raises(ValueError):
    w.append(seg + b"\0\0", ent)
  with pytest.raises(ValueError):
    w.append(b"xx", np.zeros((0, 4), np.uint32))
  with pytest.raises(ValueError):
    w.append(seg, ent)                                   # one segment larger than max_bytes: a chunk run is not split
  w.close()
  assert avi_ref.check(str(tmp_path / "f.avi"), 16, 16).chunks == []


def test_header_declares_the_avimux_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.avi  # noqa: F401  (importable without a GPU)
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  L = _lib.lib()
  for name in ("vp_avimux_desc_size", "vp_avimux_workspace_bytes", "vp_avimux_out_capacity", "vp_avimux_table_bytes", "vp_avimux_create",
               "vp_avimux_segment", "vp_avimux_destroy"):
    assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.exported_symbols(), name
  assert L.vp_avimux_desc_size() == ctypes.sizeof(_lib.AviMuxDesc) == 20
  assert "avi_mux.hip" in open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()


def test_avimux_descriptor_sizes_and_refusals():
  """Host-only entry points: the capacity rule of include/vp_hip.h, and what is refused before anything is enqueued."""
  from voicepuppet_amd import _lib
  L = _lib.lib()

  def desc(max_frames=9, row_bytes=260, slots=8, max_samples=1921, struct_bytes=None):
    return _lib.AviMuxDesc(ctypes.sizeof(_lib.AviMuxDesc) if struct_bytes is None else struct_bytes, max_frames, row_bytes, slots, max_samples)
  d = desc()
  table = 16 + 16 * 8 + 16 * (9 + 8)
  assert L.vp_avimux_table_bytes(ctypes.byref(d), 9) == table and L.vp_avimux_table_bytes(ctypes.byref(d), 0) == 16 + 16 * 8 + 16 * 8
  assert L.vp_avimux_out_capacity(ctypes.byref(d)) == table + 9 * (8 + 260 + 1) + 8 * 8 + 2 * 1921
  assert L.vp_avimux_workspace_bytes(ctypes.byref(d)) >= 16 * (9 + 8)
  assert L.vp_avimux_table_bytes(ctypes.byref(d), 10) == 0 and b"frames" in L.vp_last_error()
  for bad, word in ((desc(struct_bytes=16), b"struct_bytes"), (desc(max_frames=0), b"max_frames"), (desc(max_frames=4097), b"max_frames"),
                    (desc(slots=0), b"slots"), (desc(slots=129), b"slots"), (desc(row_bytes=0), b"row_bytes"), (desc(max_samples=-1), b"max_samples"),
                    (desc(max_frames=4096, row_bytes=1 << 21), b"32 bits")):
    assert L.vp_avimux_workspace_bytes(ctypes.byref(bad)) == 0 and word in L.vp_last_error(), (word, L.vp_last_error())
    assert L.vp_avimux_out_capacity(ctypes.byref(bad)) == 0
    h = ctypes.c_void_p()
    assert L.vp_avimux_create(ctypes.byref(bad), None, 0, ctypes.byref(h)) == -1 and not h.value
  h = ctypes.c_void_p()
  assert L.vp_avimux_create(ctypes.byref(d), None, 0, ctypes.byref(h)) == -3 and not h.value      # VP_ERR_WORKSPACE
  assert L.vp_avimux_segment(None, None, 0, None, None, 0, None, None, None, 0, None, 0, None) == -1


def test_launcher_flags_parse_and_stay_off_by_default():
  from voicepuppet_amd.pixrefer import infer_bfmvid, infer_clips, infer_stream, infer_streams
  for mod, tail in ((infer_bfmvid, ["face.jpg", "a.wav"]), (infer_stream, ["face.jpg", "a.wav"]), (infer_streams, ["list.txt"]), (infer_clips, ["clips.txt"])):
    base = ["--config_path", "params.yml"]
    o, args = mod.parse_options(base + tail)
    assert (o.avi, o.avi_only, o.device_jpeg) == (False, False, False) and args == tail
    o, args = mod.parse_options(base + ["--avi"] + tail)
    assert (o.avi, o.avi_only) == (True, False) and args == tail
    o, args = mod.parse_options(["--avi_only"] + base + tail)
    assert (o.avi, o.avi_only) == (False, True) and args == tail
  o, _ = infer_clips.parse_options(["--config_path", "p.yml", "--gpus", "2", "--avi", "--avi_only", "clips.txt"])
  cmds = infer_clips.rank_commands(o, "clips.txt", 2)
  assert all("--avi" in argv and "--avi_only" in argv and argv[-1] == "clips.txt" for argv, _ in cmds)
  o, _ = infer_clips.parse_options(["--config_path", "p.yml", "--gpus", "2", "clips.txt"])
  assert all("--avi" not in argv and "--avi_only" not in argv for argv, _ in infer_clips.rank_commands(o, "clips.txt", 2))

"""AviReader's host half, without a GPU: the container walk, the frame table, the audio track and the index check, on every layout AviWriter
produces and on files put together in other writers' styles (tests/avi_files.py)."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avi_files as af  # noqa: E402
from test_jpeg_dec_host import _image, _pil  # noqa: E402

from voicepuppet_amd.avi import AviWriter, host_segment, pcm_s16  # noqa: E402
from voicepuppet_amd.avi_read import AviReader, is_avi  # noqa: E402

W, H = 48, 32


def _jpegs(n, seed=0, **kw):
  return [_pil(_image(W, H, seed + i), **kw) for i in range(n)]


def _signal(n, seed=0):
  return (np.random.default_rng(seed).uniform(-1, 1, n)).astype(np.float32)


def _write(path, data):
  with open(path, "wb") as f:
    f.write(data)
  return str(path)


def _check(reader, jpegs, samples=None):
  assert reader.frames == len(jpegs) and (reader.width, reader.height) == (W, H) and not reader.truncated
  assert reader.frame_table.dtype == np.int64 and reader.frame_table.shape == (len(jpegs), 2)
  for i, j in enumerate(jpegs):
    assert reader.frame_bytes(i) == j and int(reader.frame_table[i, 1]) == len(j)
  if samples is None:
    assert reader.audio_format is None and reader.audio_rate is None
    with pytest.raises(ValueError):
      reader.audio()
  else:
    rate, data, fmt = reader.audio()
    assert data.dtype == samples.dtype and data.shape == samples.shape and np.array_equal(data, samples)
    assert (rate, fmt) == (reader.audio_rate, reader.audio_format) and reader.audio_channels == samples.shape[1]


# ---- what AviWriter writes ----
@pytest.mark.parametrize("audio", [False, True])
def test_one_segment_of_avi_writer_reads_back(tmp_path, audio):
  jpegs, sig = _jpegs(3), _signal(1920)
  path = str(tmp_path / "a.avi")
  w = AviWriter(path, W, H, frame_us=40000, sample_rate=16000)
  w.append(*host_segment(jpegs, sig if audio else None))
  w.close()
  assert is_avi(path)
  r = AviReader(path)
  # (the writer declares its PCM stream whether or not a push carried samples: without any the track is there and empty)
  _check(r, jpegs, pcm_s16(sig).reshape(-1, 1) if audio else np.zeros((0, 1), np.int16))
  assert r.fps == 25.0 and r.check_index() == [] and r._idx1.shape[0] == 3 + int(audio)
  assert (r.audio_rate, r.audio_channels, r.audio_format) == (16000, 1, "s16")
  assert r.audio_refused is None
  assert [c[0] for c in r.chunks] == ([b"01wb"] if audio else []) + [b"00dc"] * 3


def test_several_appends_and_a_max_bytes_split_read_back(tmp_path):
  jpegs = _jpegs(7, seed=3)
  jpegs[2] = jpegs[2] + b"\0" if len(jpegs[2]) % 2 == 0 else jpegs[2]        # an odd-sized chunk among them
  sigs = [_signal(640 * k, k) for k in (2, 3, 2)]
  groups = [jpegs[:2], jpegs[2:5], jpegs[5:]]
  path = str(tmp_path / "b.avi")
  w = AviWriter(path, W, H, sample_rate=16000)
  for g, s in zip(groups, sigs):
    w.append(*host_segment(g, s))
  w.close()
  r = AviReader(path)
  _check(r, jpegs, pcm_s16(np.concatenate(sigs)).reshape(-1, 1))
  assert r.check_index() == []
  assert any(int(n) & 1 for n in r.frame_table[:, 1])
  # the same pushes into files that hold one segment each
  seg_bytes = [len(host_segment(g, s)[0]) for g, s in zip(groups, sigs)]
  probe = AviWriter(str(tmp_path / "probe.avi"), W, H)
  limit = len(probe._head) + max(seg_bytes) + 8 + 16 * 8
  probe.close()
  split = str(tmp_path / "c.avi")
  w = AviWriter(split, W, H, sample_rate=16000, max_bytes=limit)
  for g, s in zip(groups, sigs):
    w.append(*host_segment(g, s))
  w.close()
  assert len(w.paths) == 3 and w.paths[1].endswith("c.part1.avi")
  for p, g, s in zip(w.paths, groups, sigs):
    r = AviReader(p)
    _check(r, g, pcm_s16(s).reshape(-1, 1))
    assert r.check_index() == []


# ---- other writers' styles ----
def _foreign(tmp_path, name="f.avi", audio=("s16", 2, 44100), idx=None, avix=False, cut=None):
  """Frames 0 and 1 in one 'rec ' list with audio, JUNK, frame 2 as 00db with an odd size, a dropped frame, frame 4; optionally a second
  RIFF 'AVIX' with frames 5 and 6.  -> (path, the jpegs per frame, samples or None, movi parts, movi fourcc offset)"""
  j = _jpegs(7, seed=11)
  if len(j[2]) % 2 == 0:
    j[2] += b"\0"
  strls, samples, pcm = [af.video_strl(W, H, scale_rate=(1001, 30000))], None, [b"", b"", b""]
  if audio is not None:
    fmt, ch, rate = audio
    rng = np.random.default_rng(5)
    samples = (rng.integers(-32768, 32768, (1470 * 3, ch)).astype("<i2") if fmt == "s16" else rng.uniform(-1, 1, (1470 * 3, ch)).astype("<f4"))
    strls.append(af.audio_strl(1 if fmt == "s16" else 3, ch, rate, 16 if fmt == "s16" else 32))
    pcm = [samples[1470 * k:1470 * (k + 1)].tobytes() for k in range(3)]
  wb = (lambda k: [af.chunk(b"01wb", pcm[k])]) if audio is not None else (lambda k: [])
  parts = [af.lst(b"rec ", *(wb(0) + [af.chunk(b"00dc", j[0]), af.chunk(b"00dc", j[1])])),
           af.chunk(b"JUNK", b"x" * 7), af.chunk(b"ix00", b"\0" * 24), af.chunk(b"02tx", b"sub")] + wb(1) + \
          [af.chunk(b"00db", j[2]), af.chunk(b"00dc", b""), af.chunk(b"zzzz", b"??")] + wb(2) + [af.chunk(b"00dc", j[4])]
  more = [af.riff(b"AVIX", af.lst(b"movi", af.chunk(b"00dc", j[5]), af.chunk(b"00dc", j[6])))] if avix else []
  index = None
  if idx is not None:
    index = lambda movi_at: af.old_index(af.positions(movi_at, parts), movi_at if idx == "movi" else 0)      # noqa: E731
  data, movi_at = af.avi(W, H, strls, parts, idx1=index, more_riffs=more)
  if cut is not None:
    data = data[:len(data) - cut]
  frames = [j[0], j[1], j[2], j[2], j[4]] + ([j[5], j[6]] if avix else [])
  return _write(tmp_path / name, data), frames, samples, parts, movi_at


def test_rec_lists_junk_odd_sizes_db_ids_and_no_index(tmp_path):
  path, frames, samples, parts, movi_at = _foreign(tmp_path)
  r = AviReader(path)
  _check(r, frames, samples.astype(np.int16))
  assert (r.audio_rate, r.audio_channels, r.audio_format) == (44100, 2, "s16")
  assert abs(r.fps - 30000 / 1001.0) < 1e-12
  assert r.repeats.tolist() == [False, False, False, True, False] and r.frame_table[3].tolist() == r.frame_table[2].tolist()
  assert r.check_index() == [] and r._idx1 is None
  assert [(c, at, n) for c, at, n in r.chunks] == af.positions(movi_at, parts)
  assert int(r.frame_table[2, 1]) & 1


@pytest.mark.parametrize("base", ["movi", "file"])
def test_idx1_offsets_from_the_movi_fourcc_or_the_file_start(tmp_path, base):
  path, frames, samples, _, _ = _foreign(tmp_path, idx=base)
  r = AviReader(path)
  _check(r, frames, samples.astype(np.int16))
  assert r._idx1.shape[0] == len(r.chunks) == 9 and r.check_index() == []
  # an index that names another size, or lacks an entry, is reported
  data = bytearray(open(path, "rb").read())
  at = data.rindex(b"idx1")
  struct.pack_into("<I", data, at + 8 + 16 * 4 + 12, 5)
  bad = AviReader(_write(tmp_path / "bad.avi", bytes(data))).check_index()
  assert len(bad) == 1 and "entry 4" in bad[0]
  n = struct.unpack_from("<I", data, at + 4)[0]
  struct.pack_into("<I", data, at + 4, n - 16)
  struct.pack_into("<I", data, 4, len(data) - 8 - 16)
  short = AviReader(_write(tmp_path / "short.avi", bytes(data[:-16]))).check_index()
  assert len(short) == 2 and "not in idx1" in short[1]


def test_a_second_avix_riff_continues_the_clip(tmp_path):
  path, frames, samples, _, _ = _foreign(tmp_path, idx="movi", avix=True)
  r = AviReader(path)
  _check(r, frames, samples.astype(np.int16))
  assert r.frames == 7 and len(r._movi) == 2 and r.check_index() == []


def test_mono_float32_audio(tmp_path):
  path, frames, samples, _, _ = _foreign(tmp_path, audio=("f32", 1, 16000))
  r = AviReader(path)
  _check(r, frames, samples.astype(np.float32))
  assert (r.audio_rate, r.audio_channels, r.audio_format) == (16000, 1, "f32")


def test_an_adpcm_stream_is_refused_and_the_clip_is_silent(tmp_path):
  j = _jpegs(2)
  strls = [af.video_strl(W, H), af.audio_strl(2, 1, 22050, 4, extra=struct.pack("<HH", 2, 1012))]
  data, _ = af.avi(W, H, strls, [af.chunk(b"01wb", b"\x11" * 256), af.chunk(b"00dc", j[0]), af.chunk(b"00dc", j[1])])
  r = AviReader(_write(tmp_path / "adpcm.avi", data))
  _check(r, j, None)
  assert r.audio_refused and "tag 2" in r.audio_refused and "PCM" in r.audio_refused
  with pytest.raises(ValueError, match="tag 2"):
    r.audio()
  # a PCM stream behind the refused one is taken
  strls.append(af.audio_strl(1, 1, 8000, 16))
  s = np.arange(100, dtype="<i2")
  data, _ = af.avi(W, H, strls, [af.chunk(b"01wb", b"\x11" * 256), af.chunk(b"02wb", s.tobytes()), af.chunk(b"00dc", j[0])])
  r = AviReader(_write(tmp_path / "two.avi", data))
  assert r.audio_refused is None and np.array_equal(r.audio()[1][:, 0], s) and r.audio_rate == 8000


def test_a_file_without_a_motion_jpeg_stream_is_refused(tmp_path):
  dib, _ = af.avi(W, H, [af.video_strl(W, H, compression=b"\0\0\0\0", handler=b"DIB ")], [af.chunk(b"00db", b"\0" * (3 * W * H))])
  with pytest.raises(ValueError, match="not Motion-JPEG"):
    AviReader(_write(tmp_path / "dib.avi", dib))
  only_audio, _ = af.avi(W, H, [af.audio_strl(1, 1, 8000, 16)], [af.chunk(b"00wb", b"\0" * 32)])
  with pytest.raises(ValueError, match="no video stream"):
    AviReader(_write(tmp_path / "audio.avi", only_audio))
  with pytest.raises(ValueError, match="not an AVI file"):
    AviReader(_write(tmp_path / "wave.avi", af.riff(b"WAVE", af.chunk(b"fmt ", b"\0" * 16))))
  with pytest.raises(ValueError, match="not an AVI file"):
    AviReader(_write(tmp_path / "tiny.avi", b"RIFF"))
  # the handler alone may name the codec, and a second video stream after a DIB one is taken
  by_handler, _ = af.avi(W, H, [af.video_strl(W, H, compression=b"\0\0\0\0", handler=b"mjpg")], [af.chunk(b"00dc", _jpegs(1)[0])])
  assert AviReader(_write(tmp_path / "handler.avi", by_handler)).frames == 1
  second, _ = af.avi(W, H, [af.video_strl(W, H, compression=b"\0\0\0\0", handler=b"DIB "), af.video_strl(W, H, compression=b"JPEG", handler=b"\0\0\0\0")],
                     [af.chunk(b"00db", b"\0" * 10), af.chunk(b"01dc", _jpegs(1)[0])])
  r = AviReader(_write(tmp_path / "second.avi", second))
  assert r.frames == 1 and r.frame_bytes(0) == _jpegs(1)[0]


def test_a_first_frame_of_no_bytes_is_an_error(tmp_path):
  data, _ = af.avi(W, H, [af.video_strl(W, H)], [af.chunk(b"00dc", b""), af.chunk(b"00dc", _jpegs(1)[0])])
  with pytest.raises(ValueError, match="first video chunk is empty"):
    AviReader(_write(tmp_path / "empty.avi", data))


def test_a_truncated_last_chunk_stops_the_table_one_frame_short(tmp_path):
  path, frames, samples, _, _ = _foreign(tmp_path, cut=9)
  r = AviReader(path)
  assert r.truncated and r.frames == 4
  for i in range(4):
    assert r.frame_bytes(i) == frames[i]
  assert np.array_equal(r.audio()[1], samples.astype(np.int16))
  assert int(r.frame_table[:, 0].max() + r.frame_table[-1, 1]) <= os.path.getsize(path)


def test_a_chunk_size_past_the_end_of_the_file_ends_the_walk(tmp_path):
  path, frames, _, parts, movi_at = _foreign(tmp_path, idx="movi")
  data = bytearray(open(path, "rb").read())
  third = af.positions(movi_at, parts)[5]                         # the 00db chunk of frame 2
  assert third[0] == b"00db"
  struct.pack_into("<I", data, third[1] + 4, 0x7fffffff)
  r = AviReader(_write(tmp_path / "huge.avi", bytes(data)))
  assert r.truncated and r.frames == 2 and [r.frame_bytes(i) for i in range(2)] == frames[:2]
  assert (r.frame_table[:, 0] + r.frame_table[:, 1] <= len(data)).all()
  assert r.check_index() != []                                     # the index names chunks the walk never reached


# ---- audio to the training loader ----
def test_wav_loader_reads_the_track_of_an_avi_as_it_reads_a_wav(tmp_path):
  from scipy.io import wavfile
  from voicepuppet_amd.generator.loader import WavLoader
  from voicepuppet_amd.pcm import read_wav
  for name, audio in (("s.avi", ("s16", 2, 44100)), ("f.avi", ("f32", 1, 16000))):
    path, _, samples, _, _ = _foreign(tmp_path, name=name, audio=audio)
    r = AviReader(path)
    wav = str(tmp_path / (name + ".wav"))
    r.write_wav(wav)
    rate, data, fmt = read_wav(wav)
    assert (rate, fmt) == (audio[2], audio[0]) and np.array_equal(data, samples)
    direct = str(tmp_path / (name + ".direct.wav"))
    wavfile.write(direct, audio[2], samples.astype(samples.dtype.newbyteorder("=")) if audio[1] > 1 else samples.astype(samples.dtype.newbyteorder("="))[:, 0])
    a, b, c = WavLoader(sr=16000).get_data(path), WavLoader(sr=16000).get_data(wav), WavLoader(sr=16000).get_data(direct)
    assert a.dtype == np.float32 and a.ndim == 1 and a.size == (samples.shape[0] * 16000 + audio[2] - 1) // audio[2]
    assert np.array_equal(a, b) and np.array_equal(a, c)

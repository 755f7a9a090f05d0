"""An AVI 1.0 reader written apart from voicepuppet_amd/avi.py (struct only, no shared code): walks RIFF / LIST / chunks, returns the
headers, the video and audio payloads in file order and idx1, and checks the structure - every size field against the file length, every
chunk on an even offset, every idx1 entry on a chunk header whose fourcc and length match, dwTotalFrames and both dwLength against the
counts found."""
import struct

AVIH = ("dwMicroSecPerFrame", "dwMaxBytesPerSec", "dwPaddingGranularity", "dwFlags", "dwTotalFrames", "dwInitialFrames", "dwStreams",
        "dwSuggestedBufferSize", "dwWidth", "dwHeight")
STRH = ("fccType", "fccHandler", "dwFlags", "wPriority", "wLanguage", "dwInitialFrames", "dwScale", "dwRate", "dwStart", "dwLength",
        "dwSuggestedBufferSize", "dwQuality", "dwSampleSize")


class Avi:
  pass


def _chunks(buf, begin, end):
  """(fourcc, payload offset, payload size) of the chunks in buf[begin:end]; a LIST's payload starts with its type."""
  at = begin
  while at < end:
    assert at % 2 == 0, "chunk at odd offset %d" % at
    assert at + 8 <= end, "chunk header at %d runs past %d" % (at, end)
    fcc, size = struct.unpack_from("<4sI", buf, at)
    assert at + 8 + size <= end, "%r at %d: %d bytes run past %d" % (fcc, at, size, end)
    yield fcc, at + 8, size
    at += 8 + size + (size & 1)
  assert at == end or at == end + 1, (at, end)


def parse(data):
  """data: the file's bytes (or a path).  Returns an Avi with avih, streams [(strh dict, strf bytes)], video / audio (payloads in file
  order), chunks [(fourcc, header offset, payload)], idx1 [(ckid, flags, offset, length)], movi (offset of the 'movi' fourcc)."""
  if isinstance(data, str):
    with open(data, "rb") as f:
      data = f.read()
  buf = bytes(data)
  a = Avi()
  riff, size, form = struct.unpack_from("<4sI4s", buf, 0)
  assert riff == b"RIFF" and form == b"AVI ", (riff, form)
  assert size + 8 == len(buf), "RIFF size %d, file %d bytes" % (size, len(buf))
  a.avih, a.streams, a.video, a.audio, a.chunks, a.idx1, a.movi = None, [], [], [], [], None, None
  for fcc, at, n in _chunks(buf, 12, len(buf)):
    if fcc == b"LIST" and buf[at:at + 4] == b"hdrl":
      for f2, at2, n2 in _chunks(buf, at + 4, at + n):
        if f2 == b"avih":
          assert n2 == 56, n2
          a.avih = dict(zip(AVIH, struct.unpack_from("<10I", buf, at2)))
        elif f2 == b"LIST":
          assert buf[at2:at2 + 4] == b"strl"
          strh = strf = None
          for f3, at3, n3 in _chunks(buf, at2 + 4, at2 + n2):
            if f3 == b"strh":
              assert n3 == 56, n3
              strh = dict(zip(STRH, struct.unpack_from("<4s4sIHHIIIIIIiI", buf, at3)))
              strh["rcFrame"] = struct.unpack_from("<4h", buf, at3 + 48)
            elif f3 == b"strf":
              strf = buf[at3:at3 + n3]
          assert strh is not None and strf is not None
          a.streams.append((strh, strf))
    elif fcc == b"LIST" and buf[at:at + 4] == b"movi":
      assert a.movi is None
      a.movi = at
      for f2, at2, n2 in _chunks(buf, at + 4, at + n):
        payload = buf[at2:at2 + n2]
        a.chunks.append((f2, at2 - 8, payload))
        if f2 == b"00dc":
          a.video.append(payload)
        elif f2 == b"01wb":
          a.audio.append(payload)
        else:
          raise AssertionError("unexpected chunk %r in movi" % f2)
    elif fcc == b"idx1":
      assert n % 16 == 0
      a.idx1 = [struct.unpack_from("<4sIII", buf, at + 16 * i) for i in range(n // 16)]
    else:
      raise AssertionError("unexpected chunk %r at %d" % (fcc, at - 8))
  assert a.avih is not None and a.movi is not None and a.idx1 is not None
  return a, buf


def check(data, width=None, height=None, frame_us=40000, sample_rate=16000):
  """parse + the structural checks; returns the Avi."""
  a, buf = parse(data)
  h = a.avih
  assert h["dwFlags"] == 0x10 | 0x100, hex(h["dwFlags"])                # AVIF_HASINDEX | AVIF_ISINTERLEAVED
  assert h["dwStreams"] == 2 and len(a.streams) == 2
  assert h["dwMicroSecPerFrame"] == frame_us
  assert h["dwTotalFrames"] == len(a.video), (h["dwTotalFrames"], len(a.video))
  (vh, vf), (ah, af) = a.streams
  assert vh["fccType"] == b"vids" and vh["fccHandler"] == b"MJPG" and vh["dwScale"] == frame_us and vh["dwRate"] == 1000000
  assert vh["dwLength"] == len(a.video), (vh["dwLength"], len(a.video))
  assert len(vf) == 40
  bi = struct.unpack("<IiiHH4sIiiII", vf)
  assert bi[0] == 40 and bi[3] == 1 and bi[4] == 24 and bi[5] == b"MJPG" and bi[6] == 3 * bi[1] * bi[2], bi
  assert (bi[1], bi[2]) == (h["dwWidth"], h["dwHeight"])
  if width is not None:
    assert (bi[1], bi[2]) == (width, height), bi
  assert ah["fccType"] == b"auds" and ah["dwScale"] == 1 and ah["dwRate"] == sample_rate and ah["dwSampleSize"] == 2
  audio_bytes = sum(len(p) for p in a.audio)
  assert audio_bytes % 2 == 0 and ah["dwLength"] == audio_bytes // 2, (ah["dwLength"], audio_bytes)
  assert len(af) == 16 and struct.unpack("<HHIIHH", af) == (1, 1, sample_rate, 2 * sample_rate, 2, 16), struct.unpack("<HHIIHH", af)
  assert len(a.idx1) == len(a.chunks), (len(a.idx1), len(a.chunks))
  for (ckid, flags, off, n), (fcc, at, payload) in zip(a.idx1, a.chunks):
    assert flags == 0x10
    assert a.movi + off == at, "idx1 offset %d + movi %d is not the chunk header at %d" % (off, a.movi, at)
    assert struct.unpack_from("<4sI", buf, a.movi + off) == (ckid, n) and ckid == fcc and n == len(payload)
  assert h["dwSuggestedBufferSize"] >= max([len(p) for _, _, p in a.chunks] or [0])
  assert vh["dwSuggestedBufferSize"] >= max([len(p) for p in a.video] or [0])
  assert ah["dwSuggestedBufferSize"] >= max([len(p) for p in a.audio] or [0])
  return a

"""AVI files put together with struct, in the styles of writers other than voicepuppet_amd.avi.AviWriter: what tests/test_avi_read_host.py
and tests/test_gpu_avi_read.py feed AviReader.  Written from the AVI RIFF file reference (RIFF / LIST / chunk layout, AVIMAINHEADER,
AVISTREAMHEADER, BITMAPINFOHEADER, WAVEFORMATEX, AVIOLDINDEX) and the OpenDML extension's 'AVIX' RIFFs.

Test infrastructure only: nothing under voicepuppet_amd/ imports it.
"""
import struct


def chunk(fcc, data):
  data = bytes(data)
  return struct.pack("<4sI", fcc, len(data)) + data + b"\0" * (len(data) & 1)


def lst(kind, *parts):
  body = kind + b"".join(parts)
  return struct.pack("<4sI", b"LIST", len(body)) + body


def video_strl(width, height, fps=25, compression=b"MJPG", handler=b"MJPG", scale_rate=None):
  scale, rate = scale_rate if scale_rate is not None else (1, fps)
  strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", handler, 0, 0, 0, 0, scale, rate, 0, 0, 0, -1, 0, 0, 0, width, height)
  strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, compression, 3 * width * height, 0, 0, 0, 0)
  return lst(b"strl", chunk(b"strh", strh), chunk(b"strf", strf))


def audio_strl(tag, channels, rate, bits, extra=b""):
  block = channels * bits // 8 if bits >= 8 else 1
  strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, block, rate * block, 0, 0, 0, -1, block, 0, 0, 0, 0)
  strf = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits) + extra
  return lst(b"strl", chunk(b"strh", strh), chunk(b"strf", strf))


def avih(width, height, frames, streams, frame_us=40000, flags=0x10):
  return chunk(b"avih", struct.pack("<14I", frame_us, 0, 0, flags, frames, 0, streams, 0, width, height, 0, 0, 0, 0))


def riff(form, *parts):
  body = form + b"".join(parts)
  return struct.pack("<4sI", b"RIFF", len(body)) + body


def avi(width, height, strls, movi_parts, idx1=None, frame_us=40000, more_riffs=(), junk=True):
  """One RIFF 'AVI ' (hdrl, optional JUNK, movi, optional idx1) and the RIFFs in more_riffs behind it.  -> (bytes, offset of the 'movi'
  fourcc).  idx1: None, or a function (movi fourcc offset) -> index bytes."""
  hdrl = lst(b"hdrl", avih(width, height, 0, len(strls), frame_us), *strls)
  head = hdrl + (chunk(b"JUNK", b"\0" * 13) if junk else b"")
  movi = lst(b"movi", *movi_parts)
  movi_at = 12 + len(head) + 8
  tail = chunk(b"idx1", idx1(movi_at)) if idx1 is not None else b""
  return riff(b"AVI ", head, movi, tail) + b"".join(more_riffs), movi_at


def positions(movi_at, movi_parts):
  """(fourcc, offset of the header in the file, bytes) of the stream chunks in movi_parts (flat chunks and one level of 'rec ' lists)"""
  out, at = [], movi_at + 4

  def walk(blob, base):
    p = 0
    while p + 8 <= len(blob):
      fcc, n = struct.unpack_from("<4sI", blob, p)
      if fcc == b"LIST":
        walk(blob[p + 12:p + 8 + n], base + p + 12)
      elif fcc[:2].isdigit():
        out.append((fcc, base + p, n))
      p += 8 + n + (n & 1)
  for part in movi_parts:
    walk(part, at)
    at += len(part)
  return out


def old_index(entries, base):
  """AVIOLDINDEX entries for (fourcc, header offset in the file, bytes), offsets counted from `base`"""
  return b"".join(struct.pack("<4sIII", fcc, 0x10, at - base, n) for fcc, at, n in entries)

"""Reading AVI files (Motion-JPEG video + PCM audio): the counterpart of avi.py, and what stands in for ffmpeg where a tool takes a clip.

What the reference does with ffmpeg and cv2.VideoCapture (datasets/make_data_from_GRID.py:110-141: the audio track to a .wav; :381 and
:641: the frames one by one on the host) for the one video format that needs no codec: an AVI file is a list of chunks, a Motion-JPEG
video chunk is a JPEG file, and JpegDecoder decodes those on the device byte for byte as libjpeg does.

  AviReader(path)      host parsing, no GPU needed: RIFF 'AVI ' and the 'AVIX' RIFFs behind it, hdrl (avih; per strl the strh and strf),
                       then a walk over the movi lists chunk by chunk, which is the authority on what the file holds (idx1 is only
                       compared with it: check_index).  Every offset and size is checked against the file's length before a byte of it
                       is used; a chunk that runs past the end ends the walk (truncated).
  audio(), write_wav   the PCM track as stored: pcm.read_wav's triple
  read(first, n)       frames on the device: one readinto of the file span into JpegDecoder's pinned staging, parse() per frame (4:2:2 and
                       frames without Huffman tables accepted), one decode.  The device index scan is on: MJPEG frames have no restart
                       markers.  A frame outside the decoder's subset (progressive, grey, 4:4:0, two fields in one chunk) is decoded with
                       PIL and copied in (fallbacks); a dropped frame (a zero-length chunk) is a device copy of the frame before it.

Out of scope: compressed audio (audio_refused says which), OpenDML super-indexes (skipped: the walk does not need them), other codecs.
"""
import io
import mmap
import os
import struct

import numpy as np

MJPEG_FOURCCS = (b"MJPG", b"mjpg", b"JPEG", b"jpeg")
SAMPLING_NAMES = {1: "4:4:4", 2: "4:2:0", 3: "4:2:2"}


def is_avi(path):
  """Whether the file's first twelve bytes are RIFF....AVI ."""
  try:
    with open(path, "rb") as f:
      head = f.read(12)
  except OSError:
    return False
  return len(head) == 12 and head[:4] == b"RIFF" and head[8:12] == b"AVI "


class AviReader(object):
  """frames, width, height, fps, frame_table (int64 [frames, 2]: offset and bytes of every frame's JPEG file; a dropped frame has the row
  of the frame it repeats, and repeats[i] set), audio_rate, audio_channels, audio_format ("s16", "f32" or None), audio_refused (None, or
  why the file's audio stream is not read), truncated, fallbacks (frames read() decoded with PIL so far), chunks (every stream chunk the
  walk met: (fourcc, offset of its header, bytes)).  batch: the most frames one device decode takes (read() splits longer runs)."""

  def __init__(self, path, batch=32, scan_chunk_bytes=128):
    self.path = str(path)
    st = os.stat(self.path)
    self.size, self._mtime_ns, self._abspath = int(st.st_size), int(st.st_mtime_ns), os.path.abspath(self.path)
    self.batch, self.scan_chunk_bytes = int(batch), scan_chunk_bytes
    self.truncated, self.fallbacks, self.audio_refused = False, 0, None
    self.streams, self.chunks, self._idx1, self._movi = [], [], None, []
    self.micro_sec_per_frame = 0
    self._video = self._audio = None
    self._frames, self._repeats, self._audio_chunks = [], [], []
    self._decoders, self._file = {}, None
    if self.size < 12:
      raise ValueError("%s: not an AVI file (%d bytes)" % (self.path, self.size))
    with open(self.path, "rb") as f:
      m = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
      try:
        self._parse(m)
      finally:
        m.close()
    self.frame_table = np.array(self._frames, np.int64).reshape(-1, 2)
    self.repeats = np.array(self._repeats, bool)
    self.frames = int(self.frame_table.shape[0])

  # ---- the container ----
  def _children(self, m, pos, end):
    """(fourcc, data offset, bytes, list type or None) of the chunks in [pos, end), end <= the file's length.  A chunk whose data would
    pass `end` is not yielded: truncated is set and the walk of this list ends (a LIST that would pass it is yielded as far as it
    goes, so that the frames of a recording that was cut are still found)."""
    while pos + 8 <= end:
      fcc, n = struct.unpack_from("<4sI", m, pos)
      if pos + 8 + n > end:
        self.truncated = True
        if fcc != b"LIST" or pos + 12 > end:
          return
        n = end - pos - 8                   # a list that was cut: what is there of it is walked, and nothing behind it
      kind = None
      if fcc in (b"LIST", b"RIFF"):
        if n < 4:
          self.truncated = True
          return
        kind = bytes(m[pos + 8:pos + 12])
      yield fcc, pos + 8, n, kind
      pos += 8 + n + (n & 1)

  def _parse(self, m):
    size, pos, first = self.size, 0, True
    while pos + 12 <= size:
      fcc, n, form = struct.unpack_from("<4sI4s", m, pos)
      if first and (fcc != b"RIFF" or form != b"AVI "):
        raise ValueError("%s: not an AVI file (no RIFF 'AVI ' header)" % self.path)
      if fcc != b"RIFF":
        break
      end = pos + 8 + n
      if end > size:                      # a RIFF size past the end of the file (a recording that was cut): what is there is walked
        self.truncated, end = True, size
      if first or form == b"AVIX":
        for c, at, cn, kind in self._children(m, pos + 12, end):
          if c == b"LIST" and kind == b"hdrl" and first:
            self._hdrl(m, at + 4, at + cn)
          elif c == b"LIST" and kind == b"movi":
            if not self.streams:
              raise ValueError("%s: the movi list comes before the stream headers" % self.path)
            self._choose_streams()
            self._movi.append(at)           # the offset of the 'movi' fourcc
            self._walk(m, at + 4, at + cn)
          elif c == b"idx1" and first and self._idx1 is None:
            self._idx1 = np.frombuffer(m[at:at + cn - cn % 16], "<u4").reshape(-1, 4).copy()
      first = False
      pos = end + (n & 1)
    if self._video is None:
      self._choose_streams()
    if not self._movi:
      raise ValueError("%s: no movi list" % self.path)

  def _hdrl(self, m, pos, end):
    for c, at, n, kind in self._children(m, pos, end):
      if c == b"avih" and n >= 40:
        self.micro_sec_per_frame = struct.unpack_from("<I", m, at)[0]
      elif c == b"LIST" and kind == b"strl":
        s = {"type": None, "handler": b"", "scale": 0, "rate": 0, "strf": b""}
        for c2, at2, n2, _ in self._children(m, at + 4, at + n):
          if c2 == b"strh" and n2 >= 28:
            s["type"], s["handler"] = bytes(m[at2:at2 + 4]), bytes(m[at2 + 4:at2 + 8])
            s["scale"], s["rate"] = struct.unpack_from("<II", m, at2 + 20)
          elif c2 == b"strf":
            s["strf"] = bytes(m[at2:at2 + min(n2, 64)])
        self.streams.append(s)

  def _choose_streams(self):
    """The first Motion-JPEG video stream and the first PCM audio stream (what PcmIngest takes)."""
    if self._video is not None:
      return
    why = "no video stream"
    for i, s in enumerate(self.streams):
      if s["type"] != b"vids":
        continue
      if len(s["strf"]) < 20:
        why = "video stream %d has no BITMAPINFOHEADER" % i
        continue
      w, h = struct.unpack_from("<ii", s["strf"], 4)
      comp = s["strf"][16:20]
      if comp not in MJPEG_FOURCCS and s["handler"] not in MJPEG_FOURCCS:
        why = "video stream %d is %r / %r, not Motion-JPEG (one of MJPG, mjpg, JPEG, jpeg)" % (i, comp, s["handler"])
        continue
      if w < 1 or h == 0:
        why = "video stream %d is %d x %d" % (i, w, h)
        continue
      self._video, self.width, self.height = i, int(w), int(abs(h))
      break
    if self._video is None:
      raise ValueError("%s: %s" % (self.path, why))
    v = self.streams[self._video]
    if v["scale"] and v["rate"]:
      self.fps = v["rate"] / float(v["scale"])
    elif self.micro_sec_per_frame:
      self.fps = 1e6 / self.micro_sec_per_frame
    else:
      raise ValueError("%s: neither the video stream nor the main header gives a frame rate" % self.path)
    self.audio_rate = self.audio_channels = self.audio_format = None
    for i, s in enumerate(self.streams):
      if s["type"] != b"auds":
        continue
      if len(s["strf"]) < 16:
        self.audio_refused = self.audio_refused or "audio stream %d has no WAVEFORMAT" % i
        continue
      tag, ch, rate, _, _, bits = struct.unpack_from("<HHIIHH", s["strf"], 0)
      fmt = {(1, 16): "s16", (3, 32): "f32"}.get((tag, bits))
      if fmt is None or not 1 <= ch <= 8 or rate < 1:
        self.audio_refused = self.audio_refused or ("audio stream %d: format tag %d, %d bits, %d channels, %d Hz; only PCM is read (tag 1 "
                                                    "with 16 bits, tag 3 with 32 bits, 1 .. 8 channels)" % (i, tag, bits, ch, rate))
        continue
      self._audio, self.audio_rate, self.audio_channels, self.audio_format = i, int(rate), int(ch), fmt
      self.audio_refused = None
      break

  def _walk(self, m, pos, end):
    for c, at, n, kind in self._children(m, pos, end):
      if c == b"LIST":
        if kind == b"rec ":
          self._walk(m, at + 4, at + n)
        continue
      if not (c[:2].isdigit() and c[2:] in (b"dc", b"db", b"wb", b"pc", b"tx")):
        continue                            # JUNK, ix##, anything unknown
      stream = int(c[:2])
      self.chunks.append((c, at - 8, n))
      if stream == self._video and c[2:] in (b"dc", b"db"):
        if n == 0:
          if not self._frames:
            raise ValueError("%s: the first video chunk is empty (a dropped frame with no frame before it)" % self.path)
          self._frames.append(self._frames[-1])
          self._repeats.append(True)
        else:
          self._frames.append((at, n))
          self._repeats.append(False)
      elif stream == self._audio and c[2:] == b"wb":
        if n:
          self._audio_chunks.append((at, n))

  def check_index(self):
    """idx1 against the walk -> the list of mismatches (strings; empty: the index names exactly the chunks the walk met, or the file has
    no idx1).  Offsets may count from the 'movi' fourcc (the AVI specification, AviWriter) or from the file's start (many writers)."""
    if self._idx1 is None:
      return []
    first_movi_end = self._movi[1] if len(self._movi) > 1 else None
    walk = [c for c in self.chunks if first_movi_end is None or c[1] < first_movi_end]      # idx1 speaks of the first RIFF only
    idx = [(struct.pack("<I", int(e[0])), int(e[2]), int(e[3])) for e in self._idx1 if struct.pack("<I", int(e[0])) != b"rec "]
    best = None
    for base in (self._movi[0], 0):
      bad = []
      for i in range(max(len(idx), len(walk))):
        if i >= len(idx):
          bad.append("the walk's chunk %d (%s at %d, %d bytes) is not in idx1" % (i, walk[i][0].decode("latin-1"), walk[i][1], walk[i][2]))
        elif i >= len(walk):
          bad.append("idx1 entry %d (%s at %d, %d bytes) names no chunk of the walk" % (i, idx[i][0].decode("latin-1"), idx[i][1] + base, idx[i][2]))
        elif (idx[i][0], idx[i][1] + base, idx[i][2]) != walk[i]:
          bad.append("idx1 entry %d: %s at %d, %d bytes; the walk: %s at %d, %d bytes" % (
              i, idx[i][0].decode("latin-1"), idx[i][1] + base, idx[i][2], walk[i][0].decode("latin-1"), walk[i][1], walk[i][2]))
      if best is None or len(bad) < len(best):
        best = bad
    return best

  # ---- host access ----
  def _fh(self):
    if self._file is None:
      self._file = open(self.path, "rb", buffering=0)
    return self._file

  def close(self):
    if self._file is not None:
      self._file.close()
      self._file = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def frame_bytes(self, i):
    """The JPEG file of frame i (a dropped frame: of the frame it repeats)."""
    at, n = (int(v) for v in self.frame_table[i])
    f = self._fh()
    f.seek(at)
    return f.read(n)

  def audio(self):
    """(rate, samples [n, channels] int16 or float32, "s16" or "f32"): pcm.read_wav's triple, the samples as stored."""
    if self._audio is None:
      raise ValueError("%s: no PCM audio track%s" % (self.path, " (%s)" % self.audio_refused if self.audio_refused else ""))
    f, parts = self._fh(), []
    for at, n in self._audio_chunks:
      f.seek(at)
      parts.append(f.read(n))
    raw = b"".join(parts)
    dt = np.dtype("<i2") if self.audio_format == "s16" else np.dtype("<f4")
    frame = dt.itemsize * self.audio_channels
    data = np.frombuffer(raw[:len(raw) - len(raw) % frame], dt).reshape(-1, self.audio_channels)
    return self.audio_rate, np.ascontiguousarray(data.astype(dt.newbyteorder("="))), self.audio_format

  def write_wav(self, path):
    """A PCM .wav of the samples as stored (int16, or IEEE float32)."""
    from scipy.io import wavfile
    rate, data, _ = self.audio()
    wavfile.write(path, rate, data if data.shape[1] > 1 else data[:, 0])

  def describe(self):
    """'N frames 4:2:2' (the first frame's chroma layout; 'other' for a frame the device decoder does not take)."""
    from .jpeg_dec import parse
    what = "other"
    if self.frames:
      info = parse(self.frame_bytes(0), accept_422=True, default_huffman=True)
      what = "other" if info.refused else SAMPLING_NAMES[info.sampling]
    return "%d frames %s" % (self.frames, what)

  # ---- frames on the device ----
  def _decoder(self, bgr):
    from .jpeg_dec import JpegDecoder
    if bgr not in self._decoders:
      biggest = int(self.frame_table[:, 1].max()) if self.frames else 1
      self._decoders[bgr] = JpegDecoder(self.batch, self.height, self.width, bgr=bgr, max_file_bytes=max(biggest, 1),
                                        scan_chunk_bytes=self.scan_chunk_bytes, accept_422=True, default_huffman=True)
    return self._decoders[bgr]

  @property
  def last_segments(self):
    """JpegDecoder.last_segments of the last device decode: lanes per decoded frame (gaps 0)."""
    return self._last_decoder.last_segments

  def save_index(self, path, bgr=False):
    self._decoder(bool(bgr)).save_index(path)

  def load_index(self, path, bgr=False):
    self._decoder(bool(bgr)).load_index(path)

  def _pil(self, data, bgr):
    from PIL import Image
    img = np.array(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)
    if img.shape != (self.height, self.width, 3):
      raise ValueError("%s: a frame of %d x %d in a stream of %d x %d" % (self.path, img.shape[1], img.shape[0], self.width, self.height))
    return np.ascontiguousarray(img[..., ::-1]) if bgr else img

  def read(self, first, n, out=None, bgr=False):
    """Frames first .. first + n - 1 -> device uint8 [n, height, width, 3] (RGB, or BGR).  out: a device tensor to write into ([>= n,
    height, width, 3], the pixel and channel strides dense)."""
    import torch
    first, n, bgr = int(first), int(n), bool(bgr)
    if n < 1 or first < 0 or first + n > self.frames:
      raise IndexError("%s: frames %d .. %d of %d" % (self.path, first, first + n - 1, self.frames))
    if out is None:
      out = torch.empty(n, self.height, self.width, 3, dtype=torch.uint8, device="cuda")
    if not (out.dtype == torch.uint8 and out.is_cuda and out.dim() == 4 and out.shape[0] >= n and tuple(out.shape[1:]) == (self.height, self.width, 3)
            and out.stride(3) == 1 and out.stride(2) == 3):
      raise ValueError("read: out is device uint8 [>= %d, %d, %d, 3] with dense pixels" % (n, self.height, self.width))
    for k in range(0, n, self.batch):
      self._read_batch(first + k, min(self.batch, n - k), out[k:], bgr, out[k - 1] if k else None)
    return out[:n]

  def _read_batch(self, first, n, out, bgr, prev):
    import torch
    from .jpeg_dec import parse
    dec = self._decoder(bgr)
    self._last_decoder = dec
    rows = self.frame_table[first:first + n]
    # a frame is decoded unless it repeats the frame in front of it in this call (that one is then copied on the device; prev: the
    # row in front of this batch)
    copies = [(i > 0 or prev is not None) and bool(self.repeats[first + i]) for i in range(n)]
    if all(copies):
      for i in range(n):
        out[i].copy_(out[i - 1] if i else prev)
      return
    lo = int(min(rows[i, 0] for i in range(n) if not copies[i]))
    hi = int(max(rows[i, 0] + rows[i, 1] for i in range(n) if not copies[i]))
    dec.harvest()                           # (no wait: every earlier read ended by reading its status) the index of those reads is used
    token, span = dec.stage(hi - lo)
    f = self._fh()
    f.seek(lo)
    got = f.readinto(memoryview(span))
    if got != hi - lo:
      raise IOError("%s: read %d of %d bytes at %d (the file changed under the reader)" % (self.path, got, hi - lo, lo))
    items, host = [], {}
    for i in range(n):
      if copies[i]:
        items.append(None)
        continue
      at, nbytes = int(rows[i, 0]) - lo, int(rows[i, 1])
      data = span[at:at + nbytes].tobytes()
      info = parse(data, self.height, self.width, accept_422=True, default_huffman=True)
      if info.refused is None and (info.height, info.width) != (self.height, self.width):
        info.refused = "%d x %d in a stream of %d x %d" % (info.width, info.height, self.width, self.height)
      if info.refused:
        host[i] = data
        items.append(None)
        continue
      # the key of frame first + i: of the frame it repeats when it is a dropped frame at the head of the batch (the same bytes)
      src = first + i
      while self.repeats[src]:
        src -= 1
      items.append(((at, nbytes), info, ("%s#%d" % (self._abspath, src), self.size, self._mtime_ns), None, "%s frame %d" % (self.path, src)))
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    bad = []
    if any(it is not None for it in items):
      dec.enqueue(dec.pack(items, token), out, out.stride(1), out.stride(0), status, raise_bad=False)
      bad = np.flatnonzero(status.cpu().numpy() != 0).tolist()
    for i in bad:                           # damaged entropy data: what PIL makes of it, as for a frame outside the subset
      host[i] = span[int(rows[i, 0]) - lo:int(rows[i, 0]) - lo + int(rows[i, 1])].tobytes()
    for i in sorted(host):
      out[i].copy_(torch.from_numpy(self._pil(host[i], bgr)).cuda())
      self.fallbacks += 1
    for i in range(n):
      if copies[i]:
        out[i].copy_(out[i - 1] if i else prev)

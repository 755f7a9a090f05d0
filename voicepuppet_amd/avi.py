"""AVI files (Motion-JPEG video + 16-bit PCM audio) from the frames and the audio of a push, without ffmpeg.

What the reference does at the end of a clip (infer_bfmvid.py:245: ffmpeg over output/%d.jpg and the wav) needs a program that none of
the machines this project runs on has.  Motion-JPEG in AVI with a PCM track needs no codec beyond the JPEG encoder that exists: it is a
byte layout.  Three parts:

  AviMuxer      the device half (libvp_hip.so: vp_avimux_*, csrc/avi_mux.hip): the JPEG rows of JpegEncoder.encode and the float32 samples
                of a push become, per slot, one contiguous run of RIFF chunks (`01wb` audio, then `00dc` per frame) plus its index
                entries.  segment only enqueues; to_host waits once, for the table, and copies the used part of the blob.
  host_segment  the same layout in numpy: the fallback for a slot the device gave up on, and the entry point without a GPU.
  AviWriter     the file: RIFF 'AVI ', hdrl (avih, a vids/MJPG strl, an auds/PCM strl), movi, idx1.  append writes a segment as it is;
                close writes the index and patches the sizes and counts.  A file stays under max_bytes (RIFF sizes are 32 bits; OpenDML is
                not written): the writer closes it and continues in <stem>.part<k>.avi.

A sample x leaves as clamp(rint(x * 32768), -32768, 32767), round half to even, NaN 0 (include/vp_hip.h): a signal that arrived as int16
leaves exactly as it came.
"""
import ctypes
import os
import struct

import numpy as np

from ._handle import Handle, ptr, stream

FCC_00DC, FCC_01WB = 0x63643030, 0x62773130      # '00dc', '01wb' as little-endian uint32
AVIIF_KEYFRAME = 0x10
AVIF_HASINDEX, AVIF_ISINTERLEAVED = 0x10, 0x100
RIFF_MAX = 0xFFFFFFFF


def pcm_s16(x):
  """float32 samples -> int16 little-endian under the rule above."""
  x = np.asarray(x, dtype=np.float32).reshape(-1)
  with np.errstate(invalid="ignore", over="ignore"):
    v = np.rint(x * np.float32(32768.0))
    v = np.minimum(np.maximum(v, np.float32(-32768.0)), np.float32(32767.0))
  v = np.where(np.isnan(x), np.float32(0.0), v)
  return v.astype("<i2")


def host_segment(jpegs, pcm_f32=None):
  """One slot's segment of one push: (bytes, uint32 [n, 4] AVIOLDINDEX entries with offsets from the segment's start).  jpegs: the
  frames' .jpg files (bytes-like), in order; pcm_f32: the float32 samples that go with them (None or empty: no audio chunk)."""
  parts, entries, at = [], [], 0
  if pcm_f32 is not None and np.asarray(pcm_f32).size:
    s16 = pcm_s16(pcm_f32).tobytes()
    parts += [struct.pack("<4sI", b"01wb", len(s16)), s16]
    entries.append((FCC_01WB, AVIIF_KEYFRAME, at, len(s16)))
    at += 8 + len(s16)
  for j in jpegs:
    j = bytes(j)
    parts += [struct.pack("<4sI", b"00dc", len(j)), j, b"\0" * (len(j) & 1)]
    entries.append((FCC_00DC, AVIIF_KEYFRAME, at, len(j)))
    at += 8 + len(j) + (len(j) & 1)
  return b"".join(parts), np.array(entries, dtype=np.uint32).reshape(-1, 4)


class AviWriter:
  """append(segment, entries) for every push of one talker, close() at the end (also from __del__; a second close does nothing).
  paths: the files written so far."""

  def __init__(self, path, width, height, frame_us=40000, sample_rate=16000, max_bytes=1 << 30):
    width, height, frame_us, sample_rate, max_bytes = int(width), int(height), int(frame_us), int(sample_rate), int(max_bytes)
    if not (0 < width < 65536 and 0 < height < 65536):
      raise ValueError("AviWriter: width and height in 1 .. 65535, got %d x %d" % (width, height))
    if frame_us < 1 or sample_rate < 1:
      raise ValueError("AviWriter: frame_us and sample_rate must be positive")
    self.path, self.width, self.height, self.frame_us, self.sample_rate = str(path), width, height, frame_us, sample_rate
    self._header()                                     # (sets self._head: the bytes in front of the first chunk)
    if not len(self._head) + 8 < max_bytes <= RIFF_MAX:
      raise ValueError("AviWriter: max_bytes %d outside %d .. 2^32 - 1 (RIFF sizes are 32 bits)" % (max_bytes, len(self._head) + 9))
    self.max_bytes = max_bytes
    self.paths, self.closed, self._f = [], False, None
    self._open(self.path)

  def _header(self):
    W, H = self.width, self.height
    buf, at = bytearray(), {}

    def put(fmt, *v, name=None):
      if name:
        at[name] = len(buf)
      buf.extend(struct.pack("<" + fmt, *v))
    put("4sI4s", b"RIFF", 0, b"AVI ")
    strl_v, strl_a = 4 + (8 + 56) + (8 + 40), 4 + (8 + 56) + (8 + 16)
    put("4sI4s", b"LIST", 4 + (8 + 56) + (8 + strl_v) + (8 + strl_a), b"hdrl")
    put("4sI", b"avih", 56)
    put("I", self.frame_us)
    put("I", 0, name="max_bytes_per_sec")
    put("II", 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED)
    put("I", 0, name="total_frames")
    put("II", 0, 2)
    put("I", 0, name="buffer")
    put("II4I", W, H, 0, 0, 0, 0)
    put("4sI4s", b"LIST", strl_v, b"strl")
    put("4sI", b"strh", 56)
    put("4s4sIHHIIII", b"vids", b"MJPG", 0, 0, 0, 0, self.frame_us, 1000000, 0)
    put("I", 0, name="video_length")
    put("I", 0, name="video_buffer")
    put("iI4h", -1, 0, 0, 0, W if W < 32768 else 32767, H if H < 32768 else 32767)
    put("4sI", b"strf", 40)
    put("IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", 3 * W * H, 0, 0, 0, 0)
    put("4sI4s", b"LIST", strl_a, b"strl")
    put("4sI", b"strh", 56)
    put("4s4sIHHIIII", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, self.sample_rate, 0)
    put("I", 0, name="audio_length")
    put("I", 0, name="audio_buffer")
    put("iI4h", -1, 2, 0, 0, 0, 0)
    put("4sI", b"strf", 16)
    put("HHIIHH", 1, 1, self.sample_rate, 2 * self.sample_rate, 2, 16)
    put("4s", b"LIST")
    put("I", 0, name="movi_size")
    put("4s", b"movi", name="movi")
    self._head, self._at = bytes(buf), at

  def _open(self, path):
    self._f = open(path, "wb")
    self._f.write(self._head)
    self.paths.append(path)
    self._movi_bytes = 0            # chunk bytes behind the 'movi' fourcc
    self._entries = []
    self._n_entries = 0
    self._frames = self._audio_bytes = self._video_buffer = self._audio_buffer = 0

  def _end_file(self):
    f, at = self._f, self._at
    idx = np.concatenate(self._entries).astype("<u4") if self._entries else np.zeros((0, 4), "<u4")
    f.write(struct.pack("<4sI", b"idx1", 16 * idx.shape[0]))
    f.write(idx.tobytes())
    size = f.tell()
    samples = self._audio_bytes // 2
    seconds = max(self._frames * self.frame_us / 1e6, samples / float(self.sample_rate))
    rate = int(min(RIFF_MAX, round(self._movi_bytes / seconds))) if seconds > 0 else 0
    for name, v in (("movi_size", 4 + self._movi_bytes), ("total_frames", self._frames), ("video_length", self._frames),
                    ("audio_length", samples), ("max_bytes_per_sec", rate), ("buffer", max(self._video_buffer, self._audio_buffer)),
                    ("video_buffer", self._video_buffer), ("audio_buffer", self._audio_buffer)):
      f.seek(at[name])
      f.write(struct.pack("<I", v))
    f.seek(4)
    f.write(struct.pack("<I", size - 8))
    f.close()
    self._f = None

  def _size_with(self, seg_bytes, n):
    return len(self._head) + self._movi_bytes + seg_bytes + 8 + 16 * (self._n_entries + n)

  def append(self, segment, entries):
    """segment: the bytes of whole chunks (AviMuxer.to_host, host_segment); entries: their uint32 [n, 4] index entries, offsets from
    the segment's start."""
    if self.closed:
      raise ValueError("AviWriter.append: %s is closed" % self.path)
    entries = np.asarray(entries, dtype=np.uint32).reshape(-1, 4)
    seg = memoryview(segment).cast("B") if not isinstance(segment, np.ndarray) else memoryview(np.ascontiguousarray(segment, dtype=np.uint8))
    n, nbytes = int(entries.shape[0]), seg.nbytes
    end = int(entries[-1, 2]) + 8 + int(entries[-1, 3]) + (int(entries[-1, 3]) & 1) if n else 0
    if end != nbytes:
      raise ValueError("AviWriter.append: %d entries end at byte %d of a segment of %d bytes" % (n, end, nbytes))
    if n == 0:
      return
    if self._size_with(nbytes, n) > self.max_bytes and self._n_entries:
      self._end_file()                                 # this part is full: the segment opens the next one
      stem, ext = os.path.splitext(self.path)
      self._open("%s.part%d%s" % (stem, len(self.paths), ext or ".avi"))
    if self._size_with(nbytes, n) > self.max_bytes:
      raise ValueError("AviWriter.append: a segment of %d bytes does not fit a file of max_bytes %d" % (nbytes, self.max_bytes))
    self._f.write(seg)
    e = entries.copy()
    e[:, 2] += np.uint32(4 + self._movi_bytes)         # idx1 offsets count from the 'movi' fourcc
    self._entries.append(e)
    self._n_entries += n
    self._movi_bytes += nbytes
    video = entries[:, 0] == FCC_00DC
    self._frames += int(video.sum())
    self._audio_bytes += int(entries[~video, 3].sum())
    if video.any():
      self._video_buffer = max(self._video_buffer, int(entries[video, 3].max()))
    if (~video).any():
      self._audio_buffer = max(self._audio_buffer, int(entries[~video, 3].max()))

  @property
  def frames(self):
    """Frames in the file that is open (a new part starts at 0)."""
    return self._frames

  def close(self):
    if self.closed:
      return
    self.closed = True
    if self._f is not None:
      self._end_file()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass


class AviSegments:
  """What AviMuxer.segment enqueued: the blob and the inputs it was made from (kept for the slots the host has to rebuild)."""

  def __init__(self, blob, table_bytes, frames, data, lengths, frame_slot, pcm, offsets, counts):
    self.blob, self.table_bytes, self.frames = blob, table_bytes, frames
    self.data, self.lengths, self.frame_slot, self.pcm, self.offsets, self.counts = data, lengths, frame_slot, pcm, offsets, counts


class AviMuxer(Handle):
  """segment(data, lengths, frame_slot, pcm, offsets, counts) enqueues one vp_avimux_segment on the current stream and returns an
  AviSegments; to_host(seg[, frames]) -> {slot: (uint8 array with the slot's chunks, uint32 [n, 4] entries)} for the slots that have any.
  max_frames / max_samples: the most rows / samples (all slots together) one call may carry; row_bytes: the widest row
  (JpegEncoder.capacity).  quality: what the host encodes a frame at that the device encoder gave up on."""

  def __init__(self, max_frames, row_bytes, slots, max_samples, quality=75):
    import torch
    from . import _lib
    if not torch.cuda.is_available():
      raise RuntimeError("AviMuxer needs an MI355X (host_segment is the layout without one)")
    desc = _lib.AviMuxDesc(ctypes.sizeof(_lib.AviMuxDesc), int(max_frames), int(row_bytes), int(slots), int(max_samples))
    self._open("avimux", desc, invalid="invalid AVI muxer descriptor")
    self.max_frames, self.row_bytes, self.slots, self.max_samples, self.quality = int(max_frames), int(row_bytes), int(slots), int(max_samples), int(quality)
    self.capacity = int(self.L.vp_avimux_out_capacity(ctypes.byref(self.desc)))

  def table_bytes(self, frames):
    return int(self.L.vp_avimux_table_bytes(ctypes.byref(self.desc), int(frames)))

  def call_capacity(self, frames, row_bytes, samples):
    """Bytes that hold every segment of a call of `frames` rows of `row_bytes` and `samples` samples (vp_avimux_out_capacity's rule)."""
    return self.table_bytes(frames) + frames * (8 + row_bytes + 1) + 8 * self.slots + 2 * samples

  def _i32(self, v):
    """int32 [slots] on the device: a device tensor as it is, host values through pinned memory (no wait)."""
    import torch
    if torch.is_tensor(v) and v.is_cuda:
      assert v.dtype == torch.int32 and v.is_contiguous() and v.numel() == self.slots
      return v
    host = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(self.slots)))
    return host.pin_memory().to("cuda", non_blocking=True)

  def segment(self, data, lengths, frame_slot, pcm=None, offsets=None, counts=None, out=None):
    """data uint8 [K, row] / lengths int32 [K]: JpegEncoder.encode's pair (None, None: no frame); frame_slot int32 [K] device,
    non-decreasing; pcm: float32 device samples, slot s's at offsets[s] .. + counts[s] (int32 [slots], device tensors or host
    sequences; None: no audio).  out: a uint8 device tensor to write into (its size is the capacity); allocated when None."""
    import torch
    from . import _lib
    K = 0 if data is None else int(data.shape[0])
    row = 1
    if K:
      if not (data.is_cuda and data.dtype == torch.uint8 and data.dim() == 2 and data.stride(1) == 1 and lengths.is_cuda and
              lengths.dtype == torch.int32 and lengths.is_contiguous() and frame_slot.is_cuda and frame_slot.dtype == torch.int32 and
              frame_slot.is_contiguous() and lengths.numel() == K and frame_slot.numel() == K):
        raise ValueError("segment: device data uint8 [K, row], lengths int32 [K], frame_slot int32 [K]")
      row = int(data.stride(0))
    n = 0 if pcm is None else int(pcm.numel())
    if n:
      if not (pcm.is_cuda and pcm.dtype == torch.float32 and pcm.is_contiguous()) or offsets is None or counts is None:
        raise ValueError("segment: pcm is a contiguous float32 device tensor and comes with offsets and counts")
      offsets, counts = self._i32(offsets), self._i32(counts)
    if out is None:
      out = torch.empty(self.call_capacity(K, row, n), dtype=torch.uint8, device="cuda")
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    _lib.check(self.L.vp_avimux_segment(self.h, ptr(data) if K else None, row, ptr(lengths) if K else None, ptr(frame_slot) if K else None, K,
                                        ptr(pcm) if n else None, ptr(offsets) if n else None, ptr(counts) if n else None, n, ptr(out),
                                        int(out.numel()), stream()), "vp_avimux_segment")
    return AviSegments(out, self.table_bytes(K), K, data if K else None, lengths if K else None, frame_slot if K else None,
                       pcm if n else None, offsets if n else None, counts if n else None)

  @staticmethod
  def _pinned(src):
    import torch
    host = torch.empty(src.shape, dtype=src.dtype).pin_memory()
    host.copy_(src, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()

  def to_host(self, seg, frames=None):
    """One pinned copy of the table (the wait), then one of the used part of the blob.  frames: the raw uint8 frames of the call's rows,
    for a slot with a frame the device encoder gave up on (status 1: rebuilt with host_segment and jpeg.host_jpeg; without them it
    raises).  A segment past the blob's capacity (status 2) raises."""
    S, T = self.slots, seg.table_bytes
    table = self._pinned(seg.blob[:T]).view("<u4")
    head, slot, entries = table[:4], table[4:4 + 4 * S].reshape(S, 4), table[4 + 4 * S:].reshape(-1, 4)
    if int(head[0]) != T:
      raise RuntimeError("AVI blob: table of %d bytes, expected %d" % (int(head[0]), T))
    if int(head[3]) == 2:
      raise RuntimeError("AVI blob: the segments of slots %s do not fit its %d bytes" % (np.flatnonzero(slot[:, 3] == 2).tolist(), int(seg.blob.numel())))
    used = int(head[1])
    body = self._pinned(seg.blob[T:used]) if used > T else np.zeros(0, np.uint8)
    res, e0 = {}, 0
    for s in range(S):
      off, nbytes, n, status = (int(v) for v in slot[s])
      if status == 1:
        res[s] = self._rebuild(seg, s, frames)
      elif n:
        res[s] = (body[off - T:off - T + nbytes], entries[e0:e0 + n].astype(np.uint32))
      e0 += n
    return res

  def _rebuild(self, seg, s, frames):
    from .jpeg import host_jpeg
    rows = np.flatnonzero(seg.frame_slot.cpu().numpy() == s)
    lengths = seg.lengths.cpu().numpy()
    jpegs = []
    for r in rows:
      if lengths[r] >= 0:
        jpegs.append(seg.data[r, :int(lengths[r])].cpu().numpy().tobytes())
      elif frames is None:
        raise RuntimeError("frame %d of slot %d did not fit the device encoder's slots and no raw frame was given" % (r, s))
      else:
        jpegs.append(host_jpeg(frames[int(r)].cpu().numpy(), self.quality))
    pcm = None
    if seg.pcm is not None:
      o, c = int(seg.offsets.cpu()[s]), int(seg.counts.cpu()[s])
      pcm = seg.pcm[o:o + c].cpu().numpy()
    return host_segment(jpegs, pcm)

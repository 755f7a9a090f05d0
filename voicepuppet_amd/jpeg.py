"""JPEG encoding of uint8 RGB frames on the device (libvp_hip.so: vp_jpeg_*, csrc/jpeg_enc.hip).

What the reference does per frame on the host (infer_bfmvid.py:243-244, cv2.imwrite) and the launchers here did with PIL on a thread pool:
a baseline 4:2:0 JFIF file per frame, libjpeg's quality scale, the Annex K Huffman tables, one restart interval per MCU row.  encode only
enqueues; to_host waits once, for the lengths, and then copies the used part of the byte rows.  A frame the device could not fit
(length -1: include/vp_hip.h, capacity rule) is encoded by PIL from the raw frame.
"""
import ctypes
import io
import logging

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr, rows_to_host, stream

logger = logging.getLogger(__name__)


def jpeg_desc(height, width, max_frames, quality=75):
  return _lib.JpegDesc(ctypes.sizeof(_lib.JpegDesc), int(max_frames), int(height), int(width), int(quality))


class JpegEncoder(Handle):
  """encode(frames uint8 [K, H, W, 3] device, K <= max_frames) -> (bytes uint8 [K, cap] device, lengths int32 [K] device), enqueued on the
  current stream; to_host(bytes, lengths[, frames]) -> list of K bytes objects, each a complete .jpg file."""

  _warned = False

  def __init__(self, height, width, max_frames, quality=75):
    if not torch.cuda.is_available():
      raise RuntimeError("JpegEncoder needs an MI355X (no CPU fallback)")
    self._open("jpeg", jpeg_desc(height, width, max_frames, quality), (stream(),), invalid="invalid JPEG encoder descriptor")
    self.height, self.width, self.max_frames, self.quality = int(height), int(width), int(max_frames), int(quality)
    self.capacity = int(self.L.vp_jpeg_frame_capacity(ctypes.byref(self.desc)))

  def encode(self, frames, out=None, lengths=None):
    """out / lengths: rows of a larger [*, cap] / [*] pair to write into (a push that encodes in several launches); allocated when None."""
    K = int(frames.shape[0])
    if frames.dtype != torch.uint8 or not frames.is_cuda or not frames.is_contiguous() or tuple(frames.shape[1:]) != (self.height, self.width, 3):
      raise ValueError("encode: contiguous uint8 device frames [K, %d, %d, 3]" % (self.height, self.width))
    if not 1 <= K <= self.max_frames:
      raise ValueError("encode: %d frames, 1 .. %d" % (K, self.max_frames))
    if out is None:
      out = torch.empty(K, self.capacity, dtype=torch.uint8, device="cuda")
      lengths = torch.empty(K, dtype=torch.int32, device="cuda")
    assert out.is_contiguous() and lengths.is_contiguous() and out.shape[0] >= K and lengths.shape[0] >= K
    _lib.check(self.L.vp_jpeg_encode(self.h, ptr(frames), K, ptr(out), int(out.shape[1]), ptr(lengths), stream()), "vp_jpeg_encode")
    return out[:K], lengths[:K]

  def header(self):
    n = ctypes.c_size_t()
    _lib.check(self.L.vp_jpeg_header(self.h, None, 0, ctypes.byref(n)), "vp_jpeg_header")
    buf = (ctypes.c_ubyte * n.value)()
    _lib.check(self.L.vp_jpeg_header(self.h, buf, n.value, ctypes.byref(n)), "vp_jpeg_header")
    return bytes(buf)

  def coefficients(self):
    """int16 [max_frames, H/16, 6 * W/16, 64] view of the quantised coefficients (tests; encodes store them from this call on)."""
    return self._tensor("coefficients", torch.int16, 4)

  def to_host(self, data, lengths, frames=None):
    """One pinned copy of the lengths (the wait), then one of the used prefix of the rows (rows_to_host).  frames: the raw frames, for
    the rows the device gave up on (length -1); without them such a row raises."""
    (host, n), = rows_to_host([(data, lengths)])
    files = []
    for i in range(len(n)):
      if n[i] >= 0:
        files.append(host[i, :n[i]].tobytes())
        continue
      if frames is None:
        raise RuntimeError("frame %d did not fit the device encoder's slots and no raw frame was given" % i)
      if not JpegEncoder._warned:
        JpegEncoder._warned = True
        logger.warning("a frame did not fit the device JPEG encoder's slots: encoded on the host (logged once)")
      files.append(host_jpeg(frames[i].cpu().numpy(), self.quality))
    return files


def host_jpeg(frame_u8, quality=75):
  """The host encoder of the same format (PIL / libjpeg: 4:2:0, one restart interval per MCU row)."""
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(np.asarray(frame_u8)).save(buf, "JPEG", quality=int(quality), subsampling=2, restart_marker_rows=1)
  return buf.getvalue()

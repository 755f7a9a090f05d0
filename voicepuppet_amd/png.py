"""PNG encoding of device tensors (libvp_hip.so: vp_png_*, csrc/png_enc.hip).

What the reference's image summaries do on the host (train_pixrefer.py:105-118: tf.summary.image, a float -> uint8 conversion and a zlib
PNG per image): a PNG file per frame, straight from a uint8 or float32 device tensor, any run of 1, 3 or 4 channels of its pixels.
encode only enqueues; files waits once, for the lengths, and then copies the used part of the byte rows.  A file's size is bounded by the
descriptor alone (stored strips), so there is no frame the device cannot fit.  The byte stream is restated in tests/png_ref.py.
"""
import ctypes

import torch

from . import _lib
from ._handle import Handle, ptr, rows_to_host, stream


def png_desc(max_frames, height, width, channels=3, filter=-1):
  return _lib.PngDesc(ctypes.sizeof(_lib.PngDesc), int(max_frames), int(height), int(width), int(channels), int(filter))


class PngEncoder(Handle):
  """encode(t [K, H, W, P] device, uint8 or float32, K <= max_frames; channels [channel_offset, channel_offset + channels) of the P
  per pixel) -> (bytes uint8 [K, cap] device, lengths int32 [K] device), enqueued on the current stream; files(...) -> K bytes objects,
  each a complete .png file."""

  def __init__(self, max_frames, height, width, channels=3, filter=-1):
    if not torch.cuda.is_available():
      raise RuntimeError("PngEncoder needs an MI355X (no CPU fallback)")
    self._open("png", png_desc(max_frames, height, width, channels, filter), (stream(),), invalid="invalid PNG encoder descriptor")
    self.max_frames, self.height, self.width, self.channels, self.filter = int(max_frames), int(height), int(width), int(channels), int(filter)
    self.capacity = int(self.L.vp_png_frame_capacity(ctypes.byref(self.desc)))
    self.rows_per_strip = int(self.L.vp_png_rows_per_strip(ctypes.byref(self.desc)))
    self._frames = 0

  def encode(self, t, channel_offset=0, frames=None):
    if t.dim() == 3:
      t = t.unsqueeze(-1)
    if t.dtype not in (torch.uint8, torch.float32) or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or \
       tuple(t.shape[1:3]) != (self.height, self.width):
      raise ValueError("encode: a contiguous uint8 or float32 device tensor [K, %d, %d, P]" % (self.height, self.width))
    K = int(t.shape[0]) if frames is None else int(frames)
    if not 1 <= K <= min(self.max_frames, int(t.shape[0])):
      raise ValueError("encode: %d frames, 1 .. %d" % (K, min(self.max_frames, int(t.shape[0]))))
    out = torch.empty(K, self.capacity, dtype=torch.uint8, device="cuda")
    lengths = torch.empty(K, dtype=torch.int32, device="cuda")
    dtype = _lib.PNG_U8 if t.dtype == torch.uint8 else _lib.PNG_F32
    _lib.check(self.L.vp_png_encode(self.h, ptr(t), dtype, int(t.shape[3]), int(channel_offset), K, ptr(out), self.capacity, ptr(lengths),
                                    stream()), "vp_png_encode")
    self._frames = K
    return out, lengths

  def to_host(self, rows, lengths):
    """One pinned copy of the lengths (the wait), then one of the used prefix of the rows (rows_to_host) -> list of bytes."""
    (host, n), = rows_to_host([(rows, lengths)])
    return [host[i, :n[i]].tobytes() for i in range(len(n))]

  def files(self, t, channel_offset=0, frames=None):
    return self.to_host(*self.encode(t, channel_offset, frames))

  def header(self):
    n = ctypes.c_size_t()
    _lib.check(self.L.vp_png_header(self.h, None, 0, ctypes.byref(n)), "vp_png_header")
    buf = (ctypes.c_ubyte * n.value)()
    _lib.check(self.L.vp_png_header(self.h, buf, n.value, ctypes.byref(n)), "vp_png_header")
    return bytes(buf)

  def last_strips(self):
    """int32 [K, strips, 2] on the host: per strip of the last encode its IDAT chunk's bytes and 1 when it was stored (tests)."""
    m = self._tensor("strips", torch.int32, 3)            # [max_frames, strips, 4]
    return m[:self._frames, :, [0, 3]].cpu().numpy()

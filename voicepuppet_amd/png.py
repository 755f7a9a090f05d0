"""PNG encoding of device tensors (libvp_hip.so: vp_png_*, csrc/png_enc.hip).

What the reference's image summaries do on the host (train_pixrefer.py:105-118: tf.summary.image, a float -> uint8 conversion and a zlib
PNG per image): a PNG file per frame, straight from a uint8 or float32 device tensor, any run of 1, 3 or 4 channels of its pixels.
encode only enqueues; files waits once, for the lengths, and then copies the used part of the byte rows.  A file's size is bounded by the
descriptor alone (stored strips), so there is no frame the device cannot fit.  The byte stream is restated in tests/png_ref.py.
"""
import ctypes

import torch

from . import _lib


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def png_desc(max_frames, height, width, channels=3, filter=-1):
  return _lib.PngDesc(ctypes.sizeof(_lib.PngDesc), int(max_frames), int(height), int(width), int(channels), int(filter))


class PngEncoder:
  """encode(t [K, H, W, P] device, uint8 or float32, K <= max_frames; channels [channel_offset, channel_offset + channels) of the P
  per pixel) -> (bytes uint8 [K, cap] device, lengths int32 [K] device), enqueued on the current stream; files(...) -> K bytes objects,
  each a complete .png file."""

  def __init__(self, max_frames, height, width, channels=3, filter=-1):
    if not torch.cuda.is_available():
      raise RuntimeError("PngEncoder needs an MI355X (no CPU fallback)")
    self.L = _lib.lib()
    self.desc = png_desc(max_frames, height, width, channels, filter)
    ws = self.L.vp_png_workspace_bytes(ctypes.byref(self.desc))
    if ws == 0:
      raise ValueError("invalid PNG encoder descriptor: " + self.L.vp_last_error().decode())
    self.max_frames, self.height, self.width, self.channels, self.filter = int(max_frames), int(height), int(width), int(channels), int(filter)
    self.capacity = int(self.L.vp_png_frame_capacity(ctypes.byref(self.desc)))
    self.rows_per_strip = int(self.L.vp_png_rows_per_strip(ctypes.byref(self.desc)))
    self.workspace = torch.empty(ws, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    _lib.check(self.L.vp_png_create(ctypes.byref(self.desc), _ptr(self.workspace), ws, _stream(), ctypes.byref(h)), "vp_png_create")
    self.h = h
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
    _lib.check(self.L.vp_png_encode(self.h, _ptr(t), dtype, int(t.shape[3]), int(channel_offset), K, _ptr(out), self.capacity, _ptr(lengths),
                                    _stream()), "vp_png_encode")
    self._frames = K
    return out, lengths

  def to_host(self, rows, lengths):
    """One pinned copy of the lengths (the wait), then one of the used prefix of the rows -> list of bytes."""
    K = int(lengths.shape[0])
    pinned = torch.empty(K, dtype=torch.int32).pin_memory()
    pinned.copy_(lengths, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    n = pinned.numpy().copy()
    host = torch.empty(K, int(n.max()), dtype=torch.uint8).pin_memory()
    host.copy_(rows[:K, :int(n.max())], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    host = host.numpy()
    return [host[i, :n[i]].tobytes() for i in range(K)]

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
    p = ctypes.c_void_p()
    shp = (ctypes.c_int64 * 4)()
    _lib.check(self.L.vp_png_tensor(self.h, b"strips", ctypes.byref(p), shp), "vp_png_tensor")
    n = 4 * int(shp[0]) * int(shp[1]) * int(shp[2])
    off = p.value - self.workspace.data_ptr()
    m = self.workspace[off:off + n].view(torch.int32).view(int(shp[0]), int(shp[1]), 4)
    return m[:self._frames, :, [0, 3]].cpu().numpy()

  def __del__(self):
    try:
      if getattr(self, "h", None):
        self.L.vp_png_destroy(self.h)
        self.h = None
    except Exception:
      pass

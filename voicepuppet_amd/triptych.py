"""PixReferNet training triptychs on the device (libvp_hip.so: vp_triptych_*, csrc/triptych.hip).

A triptych is one S x 3S file per frame, [frame | 3-D face on the frame | mask]: what train_pixrefer.py learns from (generator.py:924-1040)
and what only step 5 / step 6 of the reference's datasets/make_data_from_GRID.py could write (:408-471, :690-695), with TensorFlow 1, MXNet
and OpenCV.  TriptychBuilder.build takes what this package already has on the device - decoded frames, ClipRenderer.render_view's render and
face_mask, the paste geometry of infer_bfmvid.paste_geometry per frame - and enqueues the hole fill, mask resize, erosion, blur, paste and
panels (include/vp_hip.h has each stage's definition); write encodes the rows with JpegEncoder and writes <i>.jpg.  No CPU fallback for build.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr, stream

logger = logging.getLogger(__name__)

STATUS = {0: "built", 1: "side < 11 (the 21-tap blur's REFLECT_101 border)", 2: "side > max_side",
          3: "the paste rectangle is not wholly inside the canvas"}
JPEG_MAX_WIDTH = 832                # include/vp_hip.h vp_jpeg_desc: the device encoder's widest row


def triptych_desc(size, max_frames, face_size=224, max_side=None):
  return _lib.TriptychDesc(ctypes.sizeof(_lib.TriptychDesc), int(max_frames), int(size), int(face_size), int(size if max_side is None else max_side))


def fill_holes(masks):
  """scipy.ndimage.binary_fill_holes(mask > 0) for uint8 device masks [n, h, w] (h, w <= 256) -> uint8 [n, h, w] of 0 / 1; enqueues only."""
  if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3):
    raise ValueError("fill_holes: uint8 device masks [n, h, w]")
  masks = masks.contiguous()
  out = torch.empty_like(masks)
  n, h, w = masks.shape
  _lib.check(_lib.lib().vp_triptych_fill_holes(ptr(masks), n, h, w, ptr(out), stream()), "vp_triptych_fill_holes")
  return out


class TriptychBuilder(Handle):
  """build(frames uint8 [T,S,S,3] RGB, render uint8 [T,face,face,3] in the rasteriser's order, face_mask uint8 [T,face,face], geometry int
  [T,3] = (side, y0, x0)[, alpha uint8 [T,S,S]]) -> (triptych uint8 [T,S,3S,3], status int32 [T]), device tensors, T <= max_frames; the call
  only enqueues.  A frame whose status is not 0 (STATUS) leaves its triptych row as it was (zeros, or the rows of `out`)."""

  def __init__(self, size, max_frames, face_size=224, max_side=None):
    if not torch.cuda.is_available():
      raise RuntimeError("TriptychBuilder needs an MI355X (no CPU fallback)")
    self._open("triptych", triptych_desc(size, max_frames, face_size, max_side), (stream(),), invalid="invalid triptych descriptor")
    self.size, self.max_frames, self.face_size = int(size), int(max_frames), int(face_size)
    self.max_side = int(self.desc.max_side)
    self._encoder = None

  def _check(self, t, shape, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
      raise ValueError("%s must be a contiguous uint8 device tensor %s" % (what, list(shape)))
    return t

  def _geometry(self, geometry, T):
    g = torch.as_tensor(np.asarray(geometry) if not torch.is_tensor(geometry) else geometry)
    if tuple(g.shape) != (T, 3) or g.dtype.is_floating_point:
      raise ValueError("geometry must be integers [%d, 3] = (side, y0, x0)" % T)
    return g.to(device="cuda", dtype=torch.int32).contiguous()

  def _frames(self, T):
    if not 1 <= T <= self.max_frames:
      raise ValueError("%d frames, 1 .. %d" % (T, self.max_frames))

  def build(self, frames, render, face_mask, geometry, alpha=None, out=None):
    T, S, F = int(frames.shape[0]), self.size, self.face_size
    self._frames(T)
    self._check(frames, (T, S, S, 3), "frames")
    self._check(render, (T, F, F, 3), "render")
    if alpha is None or face_mask is not None:
      self._check(face_mask, (T, F, F), "face_mask")
    if alpha is not None:
      self._check(alpha, (T, S, S), "alpha")
    geom = self._geometry(geometry, T)
    trip = torch.zeros(T, S, 3 * S, 3, dtype=torch.uint8, device="cuda") if out is None else self._check(out, (T, S, 3 * S, 3), "out")
    status = torch.empty(T, dtype=torch.int32, device="cuda")
    _lib.check(self.L.vp_triptych_build(self.h, ptr(frames), ptr(render), ptr(face_mask), ptr(geom), ptr(alpha), T, ptr(trip), ptr(status),
                                        stream()), "vp_triptych_build")
    return trip, status

  def mask(self, face_mask, geometry, fill=True):
    """Stages a-d alone (b-d with fill=False, on face_mask > 0 as it is) -> the uint8 view [T, max_side, max_side] of the workspace whose
    top-left side x side corner is frame t's blurred mask (a later call overwrites it)."""
    T = int(face_mask.shape[0])
    self._frames(T)
    self._check(face_mask, (T, self.face_size, self.face_size), "face_mask")
    geom = self._geometry(geometry, T)
    _lib.check(self.L.vp_triptych_mask(self.h, ptr(face_mask), ptr(geom), T, 1 if fill else 0, stream()), "vp_triptych_mask")
    return self.tensor("mask")[:T]

  def tensor(self, name):
    """'mask' uint8 [max_frames, max_side, max_side], 'filled' uint8 [max_frames, face, face]: views of the workspace."""
    return self._tensor(name, torch.uint8, 3)

  def encode(self, triptych, quality=95):
    """The rows as complete .jpg files (list of bytes): JpegEncoder on the device where it takes the S x 3S frame (3S <= 832, S a multiple
    of 16), else the host encoder of the same format, logged once."""
    from .jpeg import JpegEncoder, host_jpeg
    T, S = int(triptych.shape[0]), self.size
    self._check(triptych, (T, S, 3 * S, 3), "triptych")
    if 3 * S > JPEG_MAX_WIDTH or S % 16:
      if self._encoder != "host":
        self._encoder = "host"
        logger.warning("triptychs of %d x %d are outside the device JPEG encoder's sizes: encoded on the host (logged once)", S, 3 * S)
      return [host_jpeg(f, quality) for f in triptych.cpu().numpy()]
    if self._encoder is None or self._encoder.quality != int(quality):
      self._encoder = JpegEncoder(S, 3 * S, self.max_frames, quality)
    data, lengths = self._encoder.encode(triptych)
    return self._encoder.to_host(data, lengths, triptych)

  def write(self, triptych, status, out_dir, first_index, quality=95):
    """Writes <first_index + t>.jpg for every row (cv2.imwrite's default quality, make_data_from_GRID.py:471).  A row whose status is not 0
    repeats the file before it, as step 6 does for a frame without landmarks (:679-683), so the numbering stays dense; when there is no
    file before it (the clip's first frame) the clip is refused with the reason.  Waits for the rows.  Returns the indices repeated."""
    st = status.cpu().numpy()
    first_index = int(first_index)
    if st[0] != 0 and not (first_index > 0 and os.path.exists(os.path.join(out_dir, "%d.jpg" % (first_index - 1)))):
      raise ValueError("frame %d cannot be built and there is no frame before it to repeat: %s" % (first_index, STATUS.get(int(st[0]), int(st[0]))))
    files = self.encode(triptych, quality)
    repeated, last = [], None
    for t in range(len(st)):
      if st[t] != 0:
        if last is None:
          with open(os.path.join(out_dir, "%d.jpg" % (first_index - 1)), "rb") as f:
            last = f.read()
        repeated.append(first_index + t)
      else:
        last = files[t]
      with open(os.path.join(out_dir, "%d.jpg" % (first_index + t)), "wb") as f:
        f.write(last)
    return repeated

"""PixReferNet input pipeline on the device (reference: generator/generator.py:956-1019).

The reference prepares every training sample on the host: two cv2.imread's, BGR->RGB, a random square crop of the S x 3S
triptych, cv2.resize back to S x S and the 6-channel packing - float32, 18 * S * S values per sample, then a host-to-device
copy of all of it.  At thousands of frames per second that thread is the bottleneck.  Here the host only hands over the decoded
uint8 frames (2 * 9 * S * S bytes per sample: 8x fewer bytes over PCIe) and three integers per crop; libvp_hip.so's
vp_pixrefer_pack_frames does the rest in one kernel, and `FramePrefetcher` overlaps the copies of batch k+1 with step k on a
second HIP stream (pinned staging buffers, event hand-off).
"""
import random

import numpy as np
import torch

from .. import _lib
from .._handle import ptr, stream


def draw_crop(img_size, crop_ratio, rng=random):
  """(rx, ry, rsize) exactly as generator.py:975-977 / 994-996 draws them."""
  rsize = rng.randint(int(img_size * crop_ratio), img_size)
  rx = rng.randint(0, img_size - rsize)
  ry = rng.randint(0, img_size - rsize)
  return rx, ry, rsize


class DeviceFramePacker:
  """uint8 triptych frames + crops -> (inputs, fg_inputs, targets, masks) float32 device tensors."""

  def __init__(self, batch, img_size, device=None):
    if not torch.cuda.is_available():
      raise RuntimeError("DeviceFramePacker needs an MI355X (no CPU fallback)")
    self.L = _lib.lib()
    self.batch, self.S = batch, img_size
    self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    f = lambda c: torch.empty(batch, img_size, img_size, c, dtype=torch.float32, device=self.device)
    self.out = (f(6), f(6), f(3), f(3))

  def __call__(self, ex_u8, cur_u8, crops):
    """ex_u8 / cur_u8: [N, S, 3S, 3] uint8 device tensors (BGR, as cv2.imread); crops: [N, 2, 3] int32 device tensor."""
    N, S = self.batch, self.S
    assert ex_u8.shape == (N, S, 3 * S, 3) and cur_u8.shape == ex_u8.shape and ex_u8.dtype == torch.uint8 and cur_u8.dtype == torch.uint8
    assert crops.shape == (N, 2, 3) and crops.dtype == torch.int32
    ex_u8, cur_u8, crops = ex_u8.contiguous(), cur_u8.contiguous(), crops.contiguous()
    _lib.check(self.L.vp_pixrefer_pack_frames(ptr(ex_u8), ptr(cur_u8), ptr(crops), N, S, ptr(self.out[0]), ptr(self.out[1]), ptr(self.out[2]),
                                              ptr(self.out[3]), stream()), "vp_pixrefer_pack_frames")
    return self.out


class CompressedBatch:
  """A batch whose frames are still .jpg files: ex / cur are lists of N entries, each an item of JpegDecoder.decode_into, (bytes,
  JpegInfo, key, None, path), or - for a file the parser refused - the decoded [S, 3S, 3] uint8 BGR frame; crops as in the raw form."""

  def __init__(self, ex, cur, crops):
    self.ex, self.cur, self.crops = ex, cur, crops


class FramePrefetcher:
  """Double-buffered host -> device hand-over of uint8 frame batches on a side stream.

  `source` yields (ex [N,S,3S,3] uint8, cur [N,S,3S,3] uint8, crops [N,2,3] int32) as numpy arrays or torch tensors; pinned
  torch tensors cross PCIe straight from where they are (they must stay unchanged until two batches later).  next() returns the four packed
  float32 tensors of the oldest batch in flight (valid until the next call) and starts the copies of a following one; the
  copies and the pack kernel of batch k+1 overlap the training step of batch k.

  A source may also yield CompressedBatch objects (the data generator with device_jpeg_decode): the files of the batch cross PCIe in
  one pinned blob, vp_jpegdec_decode writes the frames straight into the slot's device tensors on the side stream, and the same packer
  follows.  The decoder's status and entry points are copied to pinned memory behind it and looked at three batches later (when the
  decoder's staging buffer is reused, long after they arrived): a file that did not decode raises RuntimeError naming it; no host wait
  is added.  segments_used: the segment count per file of the last compressed batch filled (0: a frame that came decoded).
  device_jpeg_scan: None, or the chunk bytes of the decoder's index scan (JpegDecoder(scan_chunk_bytes=...)): a file then runs one
  lane per MCU row in the batch that first sees it.  segments_used is then a lazy read-only property: it is resolved from the decoder's
  last call when it is read (a host wait for that call), not a snapshot taken when the batch was filled.
  """

  def __init__(self, source, batch, img_size, depth=2, device=None, device_jpeg_scan=None):
    self.source = iter(source)
    self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    # the process's fourth executor stream (include/vp_hip.h vp_host_stream): the training engine beside this prefetcher keeps to three
    # (vp_pixrefer_use_streams), a stream created here would be a fifth one on a shared hardware queue
    sp = _lib.lib().vp_host_stream()
    if not sp:
      _lib.check(-1, "vp_host_stream")
    self.stream = torch.cuda.ExternalStream(sp, device=self.device)
    S = img_size
    self.slots = []
    for _ in range(depth):
      host = (torch.empty(batch, S, 3 * S, 3, dtype=torch.uint8).pin_memory(), torch.empty(batch, S, 3 * S, 3, dtype=torch.uint8).pin_memory(),
              torch.empty(batch, 2, 3, dtype=torch.int32).pin_memory())
      dev = tuple(torch.empty_like(h, device=self.device) for h in host)
      self.slots.append({"host": host, "dev": dev, "packer": DeviceFramePacker(batch, img_size, self.device),
                         "ready": torch.cuda.Event(), "free": torch.cuda.Event(), "busy": False})
    self.head = self.tail = 0
    self.batch, self.img_size = batch, img_size
    self.decoder = None                               # JpegDecoder of 2 * batch files, made by the first CompressedBatch
    self.device_jpeg_scan = device_jpeg_scan
    self._segments_used = []
    self._copied = []                                 # copy-done events of the last batches whose sources were read in place
    for _ in range(depth):
      self._fill()

  def _fill(self):
    slot = self.slots[self.head % len(self.slots)]
    # The contract for pinned sources read in place: a buffer stays unchanged "until two batches later".  Enqueuing is not
    # executing: nothing else throttles a host that runs ahead of the device (a launcher that reads no loss per step), so before the
    # source may produce batch k - possibly into the buffer batch k-3 or older was read from - the H2D copies of batch k-2 (and, in
    # stream order, of everything before it) must have EXECUTED.  They normally have; the wait is then a query.
    if len(self._copied) >= 2:
      self._copied[-2].synchronize()
    try:
      got = next(self.source)
    except StopIteration:
      return False
    if isinstance(got, CompressedBatch):
      self._fill_compressed(slot, got)
      slot["busy"] = True
      self.head += 1
      return True
    ex, cur, crops = got
    # a source that already decodes into PINNED torch tensors (what a decoder thread should do) is copied from directly; anything
    # else is staged through this slot's pinned buffers first (a host memcpy of 18 * S * S bytes per sample on the calling thread)
    srcs = []
    staged = False
    for h, a in zip(slot["host"], (ex, cur, crops)):
      if isinstance(a, torch.Tensor) and a.is_pinned() and a.dtype == h.dtype and a.shape == h.shape and a.is_contiguous():
        srcs.append(a)
        continue
      if not staged and slot["busy"]:
        slot["ready"].synchronize()                   # the previous copies out of this slot's pinned buffers have completed
      staged = True
      h.copy_(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)))
      srcs.append(h)
    slot["src"] = srcs                                # keeps a caller's pinned tensors alive until the slot is refilled
    with torch.cuda.stream(self.stream):
      if slot["busy"]:
        self.stream.wait_event(slot["free"])          # the consumer of this slot's previous batch has been enqueued past it
      for d, h in zip(slot["dev"], srcs):
        d.copy_(h, non_blocking=True)
      if not staged:
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self._copied = self._copied[-2:] + [ev]
      slot["packer"](*slot["dev"])
      slot["ready"].record(self.stream)
    slot["busy"] = True
    self.head += 1
    return True

  def _fill_compressed(self, slot, b):
    N, S = self.batch, self.img_size
    if self.decoder is None:
      from ..jpeg_dec import JpegDecoder
      self.decoder = JpegDecoder(2 * N, S, 3 * S, bgr=True, scan_chunk_bytes=self.device_jpeg_scan)
      self._status = torch.empty(2 * N, dtype=torch.int32, device=self.device)
    if "frames" not in slot:                          # ex and cur as the two halves of one tensor: one decode call fills both
      slot["frames"] = torch.empty(2, N, S, 3 * S, 3, dtype=torch.uint8, device=self.device)
    frames = slot["frames"]
    items = list(b.ex) + list(b.cur)
    assert len(items) == 2 * N
    raw = [i for i, it in enumerate(items) if not isinstance(it, tuple)]
    if raw and slot["busy"]:
      slot["ready"].synchronize()                     # the staging rows below were last read by this slot's previous batch
    with torch.cuda.stream(self.stream):
      if slot["busy"]:
        self.stream.wait_event(slot["free"])
      for i in raw:                                   # frames that came decoded (refused files): staged through the slot's pinned rows
        h = slot["host"][i // N][i % N]
        h.copy_(torch.from_numpy(np.ascontiguousarray(items[i])))
        frames[i // N][i % N].copy_(h, non_blocking=True)
        items[i] = None
      crops = b.crops if isinstance(b.crops, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b.crops))
      if not crops.is_pinned():
        slot["host"][2].copy_(crops)
        crops = slot["host"][2]
      slot["dev"][2].copy_(crops, non_blocking=True)
      if any(it is not None for it in items):
        flat = frames.view(2 * N, S, 3 * S, 3)
        self.decoder.decode_into(items, flat, flat.stride(1), flat.stride(0), self._status)
        self._segments_used = None                    # the decoder's last call: resolved when asked for
      else:
        self._segments_used = [0] * (2 * N)
      ev = torch.cuda.Event()
      ev.record(self.stream)
      self._copied = self._copied[-2:] + [ev]
      slot["src"] = [crops]
      slot["packer"](frames[0], frames[1], slot["dev"][2])
      slot["ready"].record(self.stream)

  @property
  def segments_used(self):
    return list(self.decoder.last_segments) if self._segments_used is None else self._segments_used

  def next(self):
    if self.tail == self.head:
      raise StopIteration
    # the slot handed out by the previous call is free once everything enqueued so far on the compute stream has run
    if self.tail > 0:
      prev = self.slots[(self.tail - 1) % len(self.slots)]
      prev["free"].record(torch.cuda.current_stream())
      self._fill()
    slot = self.slots[self.tail % len(self.slots)]
    torch.cuda.current_stream().wait_event(slot["ready"])
    self.tail += 1
    return slot["packer"].out

  __next__ = next

  def __iter__(self):
    return self


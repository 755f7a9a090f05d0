"""Clean-up of alpha mattes on the device (libvp_hip.so: vp_matteclean_*, csrc/matte_clean.hip): the components of the matte's support
that are neither large enough nor the subject (they do not leave through the bottom edge and hold no anchor) are removed with the haze
below the support, and enclosed holes of the core are filled.  include/vp_hip.h defines every number; tests/matte_clean_ref.py restates
it in numpy.

The stage a keyer puts behind its key: KeyMatte marks a prop, noise speckle and the frame's edge as subject and a patch of backdrop
colour on the subject as a hole.  It works on any uint8 matte, one read from a file as well.  It is component bookkeeping, not a matting
solve: it moves no edge.  The defaults below are untuned on real footage.

clean only enqueues on the current stream; report() is the one host read.
"""
import ctypes

import torch

from . import _lib
from ._handle import Handle, ptr, stream, u8_plane

REPORT_FIELDS = ("components", "kept", "pixels_removed", "pixels_zeroed", "holes_filled", "pixels_filled", "status")
STATUS_ALL_KEPT, STATUS_CAP = 1, 2
KEEP = {"all": _lib.MATTECLEAN_KEEP_ALL, "anchored": _lib.MATTECLEAN_KEEP_ANCHORED}


def matteclean_desc(max_frames, max_height, max_width):
  return _lib.MatteCleanDesc(ctypes.sizeof(_lib.MatteCleanDesc), int(max_frames), int(max_height), int(max_width))


def default_min_area(height, width):
  return int(height) * int(width) // 1024


def default_max_hole(height, width):
  return int(height) * int(width) // 256


class MatteCleaner(Handle):
  """clean(matte) for device uint8 mattes [n, H, W], n <= max_frames, 16 <= H <= max_height, 16 <= W <= max_width.  The workspace is at
  most 12 bytes per pixel of max_frames x max_height x max_width."""

  def __init__(self, max_frames, max_height, max_width):
    if not torch.cuda.is_available():
      raise RuntimeError("MatteCleaner needs an MI355X (no CPU fallback)")
    self._open("matteclean", matteclean_desc(max_frames, max_height, max_width), invalid="invalid matte cleaner descriptor")
    self.max_frames, self.max_height, self.max_width = int(max_frames), int(max_height), int(max_width)
    self._n = 0

  def clean(self, matte, support=32, core=224, min_area=None, max_hole=None, grow=4, keep="anchored", anchors=None, out=None):
    """-> device uint8 [n, H, W].  Components of {matte >= support} (8-connected) are kept when they have min_area pixels and, with
    keep="anchored", touch the bottom row or hold one of the frame's anchors (int32 [n, k, 2] of (x, y), k <= 256; the 68 landmarks);
    when nothing is kept that way, everything is, and report() says so.  Below the support a pixel survives within `grow` (0 .. 16,
    Chebyshev) of a kept component.  Then the 4-connected components of {result < core} that touch no frame edge and have at most
    max_hole pixels become 255; max_hole=0 skips that.  Defaults: min_area H * W // 1024, max_hole H * W // 256; all defaults are
    untuned on real footage.  out: a contiguous device uint8 [>= n, H, W]."""
    u8_plane(matte, "clean", "matte")
    n, H, W = (int(v) for v in matte.shape)
    if keep not in KEEP:
      raise ValueError("clean: keep must be 'all' or 'anchored'")
    k = 0
    if anchors is not None:
      if anchors.dim() != 3 or anchors.dtype != torch.int32 or not anchors.is_cuda or tuple(anchors.shape[::2]) != (n, 2):
        raise ValueError("clean: anchors must be a device int32 tensor [%d, k, 2] of (x, y)" % n)
      anchors = anchors.contiguous()
      k = int(anchors.shape[1])
    if out is None:
      out = torch.empty(max(n, 1), H, W, dtype=torch.uint8, device="cuda")
    else:
      u8_plane(out, "clean", "out", n, H, W)
    rc = self.L.vp_matteclean_clean(self.h, ptr(matte), n, H, W, int(support), int(core), -1 if min_area is None else int(min_area),
                                    -1 if max_hole is None else int(max_hole), int(grow), KEEP[keep], ptr(anchors if k else None), k, ptr(out),
                                    stream())
    _lib.check(rc, "vp_matteclean_clean")
    self._n = n
    return out[:n]

  def report(self):
    """int32 [n, 8] of the last clean, on the host (the one host read): components, kept, pixels of removed components, pixels below the
    support that became 0, holes filled, pixels filled, status (1: nothing passed the rule and everything was kept; 2: a step cap of
    the labelling was reached - a bug, the result is not to be used), 0."""
    return self.tensor("report")[:self._n].cpu().numpy()

  def tensor(self, name):
    """'labels': int32 [max_frames, H, W] of the last call, -1 outside the support, else the smallest y * W + x of the pixel's component;
    'report': int32 [max_frames, 8].  Views of the workspace."""
    return self._tensor(name, torch.int32, 3 if name == "labels" else 2)


def summary(report):
  """The dataset tool's words for a report (any number of frames)."""
  r = report.reshape(-1, _lib.MATTECLEAN_REPORT_INTS).sum(0)
  removed = int(r[0] - r[1])
  return "removed %d component%s / %d px, filled %d hole%s / %d px" % (removed, "" if removed == 1 else "s", int(r[2]), int(r[4]),
                                                                      "" if r[4] == 1 else "s", int(r[5]))

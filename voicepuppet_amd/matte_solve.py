"""Trimap and closed-form matting solve on the device (libvp_hip.so: vp_mattesolve_*, csrc/matte_solve.hip): the trimap from an erosion
and a dilation of a matte, and alpha inside its unknown band from the matting Laplacian of Levin, Lischinski and Weiss, solved by
preconditioned conjugate gradients in float64.  include/vp_hip.h defines every number; tests/matte_solve_ref.py restates it in numpy.

Stages two and three of the matte that step 6 of the reference's datasets/make_data_from_GRID.py makes (:654-672), with a linear solve in
place of its matting network: no weights, no backdrop model.  Behind KeyMatte and MatteCleaner it moves the matte's edge to where the
colours put it; behind any binary mask (a segmentation read from files) it is the path for footage with a cluttered background, where
the key is the wrong tool.  The defaults below come from synthetic scenes and are untuned on real footage.

trimap and solve only enqueue on the current stream; report() is the one host read.
"""
import ctypes

import torch

from . import _lib
from ._handle import Handle, ptr, rgb_frames, stream, u8_plane

REPORT_FIELDS = ("unknown", "iterations", "status", "residual")
STATUS_NO_CONSTRAINT, STATUS_BREAKDOWN = 1, 2
DEFAULT_EPS, DEFAULT_ITERS, DEFAULT_TOL = 1.0, 512, 1e-6


def mattesolve_desc(max_frames, max_height, max_width, max_radius=2):
  return _lib.MatteSolveDesc(ctypes.sizeof(_lib.MatteSolveDesc), int(max_frames), int(max_height), int(max_width), int(max_radius))


def default_erode(height, width):
  """The reference's 30 x 30 is for 720 x 576 video: 1 / 19 of the shorter side, at least 5, at most 64."""
  return max(5, min(_lib.MATTESOLVE_MAX_SQUARE, min(int(height), int(width)) // 19))


def default_dilate(height, width):
  """The reference's 20 x 20: 1 / 29 of the shorter side, at least 5, at most 64."""
  return max(5, min(_lib.MATTESOLVE_MAX_SQUARE, min(int(height), int(width)) // 29))


class MatteSolver(Handle):
  """trimap(matte) then solve(frames, trimap) for n <= max_frames frames of 16 <= H <= max_height, 16 <= W <= max_width.  Frames are device
  uint8 RGB [n, H, W, 3]; strided views are taken as they are when a pixel's three values and a row's pixels are adjacent (a padded
  JpegDecoder output).  The workspace is 48 bytes per pixel of max_frames x max_height x max_width: six float64 planes."""

  def __init__(self, max_frames, max_height, max_width, max_radius=2):
    if not torch.cuda.is_available():
      raise RuntimeError("MatteSolver needs an MI355X (no CPU fallback)")
    self._open("mattesolve", mattesolve_desc(max_frames, max_height, max_width, max_radius), invalid="invalid matte solver descriptor")
    self.max_frames, self.max_height, self.max_width, self.max_radius = int(max_frames), int(max_height), int(max_width), int(max_radius)
    self._n = 0

  def trimap(self, matte, support=32, core=224, erode=None, dilate=None, out=None):
    """-> device uint8 [n, H, W]: 255 where the erode x erode square around the pixel lies in {matte >= core}, else 127 where the
    dilate x dilate square meets {matte >= support}, else 0; a k x k square covers the offsets -(k // 2) .. k - 1 - (k // 2), clipped to
    the image.  erode, dilate: 1 .. 64; defaults max(5, min(H, W) // 19) and max(5, min(H, W) // 29), the reference's 30 and 20 for
    720 x 576 scaled to the frame; untuned on real footage.  out: a contiguous device uint8 [>= n, H, W], not the matte itself."""
    u8_plane(matte, "trimap", "matte")
    n, H, W = (int(v) for v in matte.shape)
    if out is None:
      out = torch.empty(max(n, 1), H, W, dtype=torch.uint8, device="cuda")
    else:
      u8_plane(out, "trimap", "out")
      u8_plane(out, "trimap", "out", n, H, W)
    rc = self.L.vp_mattesolve_trimap(self.h, ptr(matte), n, H, W, int(support), int(core), 0 if erode is None else int(erode),
                                     0 if dilate is None else int(dilate), ptr(out), stream())
    _lib.check(rc, "vp_mattesolve_trimap")
    return out[:n]

  def solve(self, frames, trimap, radius=1, eps=DEFAULT_EPS, iters=DEFAULT_ITERS, tol=DEFAULT_TOL, out=None):
    """-> device uint8 [n, H, W]: 0 and 255 where the trimap is 0 and 255, elsewhere the solution of the matting Laplacian's system for
    the frame's colours: windows of (2 radius + 1)^2 pixels, eps the regulariser in grey levels squared, conjugate gradients until the
    relative residual is at most tol or `iters` iterations have run (the launches of all `iters` are enqueued; a frame that has
    stopped costs nothing more).  tensor('alpha') holds the unclamped float64 solution.  The defaults (radius 1, eps 1, iters 512)
    are untuned on real footage.  out: a contiguous device uint8 [>= n, H, W]; it may be the trimap."""
    pitch, stride, n, H, W = rgb_frames(frames, "solve")
    u8_plane(trimap, "solve", "trimap")
    u8_plane(trimap, "solve", "trimap", n, H, W, exact=True)
    if out is None:
      out = torch.empty(max(n, 1), H, W, dtype=torch.uint8, device="cuda")
    else:
      u8_plane(out, "solve", "out")
      u8_plane(out, "solve", "out", n, H, W)
    rc = self.L.vp_mattesolve_solve(self.h, ptr(frames), pitch, stride, n, H, W, ptr(trimap), int(radius), float(eps), int(iters), float(tol),
                                    ptr(out), stream())
    _lib.check(rc, "vp_mattesolve_solve")
    self._n = n
    return out[:n]

  def laplacian(self, frames, p, radius=1, eps=DEFAULT_EPS):
    """The single op behind the solve (vp_mattesolve_laplacian): L p for a contiguous device float64 [n, H, W], no masking."""
    pitch, stride, n, H, W = rgb_frames(frames, "laplacian")
    if p.dtype != torch.float64 or not p.is_cuda or not p.is_contiguous() or tuple(p.shape) != (n, H, W):
      raise ValueError("laplacian: p must be a contiguous device float64 [%d, %d, %d]" % (n, H, W))
    out = torch.empty_like(p)
    rc = self.L.vp_mattesolve_laplacian(self.h, ptr(frames), pitch, stride, n, H, W, int(radius), float(eps), ptr(p), ptr(out), stream())
    _lib.check(rc, "vp_mattesolve_laplacian")
    return out

  def report(self):
    """Of the last solve, on the host (the one host read): {'unknown': int32 [n], 'iterations': int32 [n], 'status': int32 [n] (bit 1:
    no constraint reaches the band or the trimap has no unknown pixel, x = 0; bit 2: the iteration broke down and stopped where it
    was), 'residual': float64 [n], the recurrence's final sqrt(r.r / b.b)}."""
    rep = self.tensor("report")[:self._n].cpu()
    ints = rep.numpy()
    return {"unknown": ints[:, 0].copy(), "iterations": ints[:, 1].copy(), "status": ints[:, 2].copy(),
            "residual": rep[:, 4:6].contiguous().view(torch.float64)[:, 0].numpy().copy()}

  def tensor(self, name):
    """'alpha': float64 [max_frames, H, W] of the last call, the unclamped solution with 0 and 1 on the known pixels; 'report': int32
    [max_frames, 8] (a float64 at byte 16 of each row); 'tiles': int32 [max_frames, ceil(H / 32), ceil(W / 32)], 1 where the tile holds
    an unknown pixel.  Views of the workspace."""
    if name == "alpha":
      return self._tensor(name, torch.float64, 3)
    return self._tensor(name, torch.int32, 2 if name == "report" else 3)


def summary(report, iters=None, tol=None):
  """The dataset tool's words for a report (means over the frames), and whether any frame needs a warning: a status bit, or, given
  iters and tol, a frame that ran all its iterations without reaching tol."""
  n = len(report["unknown"])
  text = "solve: %d px unknown, %d iterations, residual %.0e" % (round(float(report["unknown"].mean())) if n else 0,
                                                                round(float(report["iterations"].mean())) if n else 0,
                                                                float(report["residual"].mean()) if n else 0.0)
  flagged = int((report["status"] != 0).sum())
  capped = int(((report["status"] == 0) & (report["iterations"] >= iters) & (report["residual"] > tol)).sum()) if iters is not None else 0
  return text, flagged, capped

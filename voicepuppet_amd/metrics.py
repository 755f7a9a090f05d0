"""Frame quality metrics on the device (libvp_hip.so: vp_frame_metrics_*, csrc/frame_metrics.hip): per frame pair L1, MSE, PSNR and SSIM of
two batches of three-channel NHWC frames that are already on the device.  include/vp_hip.h defines the numbers (SSIM: Wang et al. 2004,
skimage's structural_similarity with gaussian_weights=True, use_sample_covariance=False, data_range=255, channel_axis=-1).

compare only enqueues on the current stream and returns a device float64 [n, 4] tensor; compare(...).cpu() is the host read.
"""
import ctypes

import torch

from . import _lib
from ._handle import Handle, frame_layout, ptr, stream

L1, MSE, PSNR, SSIM = 0, 1, 2, 3
COLUMNS = ("L1", "MSE", "PSNR", "SSIM")
# value_range -> (scale, offset) of v = x * scale + offset; (0, 1) is the deprocessed generator output (bench.py --dump-outputs)
VALUE_RANGES = {(-1, 1): (127.5, 127.5), (0, 255): (1.0, 0.0), (0, 1): (255.0, 0.0)}


def frame_metrics_desc(max_frames, max_height, max_width):
  return _lib.FrameMetricsDesc(ctypes.sizeof(_lib.FrameMetricsDesc), int(max_frames), int(max_height), int(max_width))


class FrameMetrics(Handle):
  """compare(a, b) for device tensors [n, H, W, 3], both uint8 or both float32, n <= max_frames, 11 <= H <= max_height, 11 <= W <= max_width
  -> device float64 [n, 4], columns L1, MSE, PSNR, SSIM (the module's constants).  Strided views are taken as they are when a pixel's three
  values and a row's pixels are adjacent (stride 1 and 3 on the last two axes): a padded decoder output against a dense tensor."""

  def __init__(self, max_frames, max_height, max_width):
    if not torch.cuda.is_available():
      raise RuntimeError("FrameMetrics needs an MI355X (no CPU fallback)")
    self._open("frame_metrics", frame_metrics_desc(max_frames, max_height, max_width), invalid="invalid frame metrics descriptor")
    self.max_frames, self.max_height, self.max_width = int(max_frames), int(max_height), int(max_width)

  def compare(self, a, b, value_range=(-1, 1), out=None):
    """value_range: of float32 operands, (-1, 1) (the generator's output), (0, 255) or (0, 1); values outside are clamped.  uint8 ignores it.
    out: a contiguous device float64 [>= n, 4] to write into; allocated when None."""
    if a.dim() != 4 or a.shape[3] != 3 or a.shape != b.shape or a.dtype != b.dtype or not (a.is_cuda and b.is_cuda) \
       or a.dtype not in (torch.uint8, torch.float32):
      raise ValueError("compare: two device tensors [n, H, W, 3] of the same shape, both uint8 or both float32")
    n, H, W = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    ap, as_ = frame_layout(a, "compare", "a")
    bp, bs = frame_layout(b, "compare", "b")
    if out is None:
      out = torch.empty(max(n, 1), 4, dtype=torch.float64, device="cuda")
    if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != 4 or out.shape[0] < n:
      raise ValueError("compare: out must be a contiguous device float64 [>= %d, 4]" % n)
    if a.dtype == torch.uint8:
      rc = self.L.vp_frame_metrics_u8(self.h, ptr(a), ap, as_, ptr(b), bp, bs, n, H, W, ptr(out), stream())
      _lib.check(rc, "vp_frame_metrics_u8")
    else:
      try:
        scale, offset = VALUE_RANGES[tuple(value_range)]
      except (KeyError, TypeError):
        raise ValueError("compare: value_range %r, (-1, 1), (0, 255) or (0, 1)" % (value_range,))
      rc = self.L.vp_frame_metrics_f32(self.h, ptr(a), ap, as_, ptr(b), bp, bs, n, H, W, scale, offset, ptr(out), stream())
      _lib.check(rc, "vp_frame_metrics_f32")
    return out[:n]

  def tensor(self, name):
    """'abs_sum', 'sq_sum': int64 [max_frames] views of the workspace, the integer sums of the frames of the last uint8 compare."""
    return self._tensor(name, torch.int64, 1)

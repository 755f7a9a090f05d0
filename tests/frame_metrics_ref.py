"""Float64 numpy restatement of the frame metrics of include/vp_hip.h (vp_frame_metrics_*), written apart from the kernel: every SSIM window
is an explicit weighted sum over its 11 x 11 values with the two-dimensional window, not two one-dimensional passes.

metrics(a, b) takes two [H, W, 3] arrays of values in [0, 255] (uint8, or float64 already mapped by map_f32) and returns
(L1, MSE, PSNR, SSIM); sums(a, b) the exact integer sums of a uint8 pair."""
import numpy as np

SIGMA, TAPS = 1.5, 11
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def window():
  """the 11 x 11 Gaussian window: the outer product of the normalised 11-tap vector"""
  g = np.exp(-((np.arange(TAPS, dtype=np.float64) - 5.0) ** 2) / (2.0 * SIGMA * SIGMA))
  g /= g.sum()
  return np.outer(g, g)


def map_f32(x, scale=127.5, offset=127.5):
  """float32 values -> the doubles the device compares: min(max(x * scale + offset, 0), 255), no rounding; a NaN maps to 0"""
  v = np.asarray(x, np.float32).astype(np.float64) * np.float64(scale) + np.float64(offset)
  return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0))


def _weighted(x, w):
  """sum over every interior 11 x 11 window of w * x: [H - 10, W - 10]"""
  win = np.lib.stride_tricks.sliding_window_view(x, (TAPS, TAPS))
  return np.einsum("ijkl,kl->ij", win, w)


def ssim_map(a, b):
  """S per window and channel, [H - 10, W - 10, 3]"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3 and a.shape[0] >= TAPS and a.shape[1] >= TAPS
  w = window()
  out = np.empty((a.shape[0] - TAPS + 1, a.shape[1] - TAPS + 1, 3), np.float64)
  for c in range(3):
    x, y = a[..., c], b[..., c]
    mx, my = _weighted(x, w), _weighted(y, w)
    vx = _weighted(x * x, w) - mx * mx
    vy = _weighted(y * y, w) - my * my
    cov = _weighted(x * y, w) - mx * my
    out[..., c] = ((2.0 * mx * my + C1) * (2.0 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
  return out


def sums(a, b):
  """(sum |a - b|, sum (a - b)^2) of a uint8 pair as Python integers"""
  assert a.dtype == np.uint8 and b.dtype == np.uint8
  d = a.astype(np.int64) - b.astype(np.int64)
  return int(np.abs(d).sum()), int((d * d).sum())


def psnr(mse):
  return np.inf if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def metrics(a, b):
  """(L1, MSE, PSNR, SSIM) of one frame pair"""
  if a.dtype == np.uint8 and b.dtype == np.uint8:
    s1, s2 = sums(a, b)
    l1, mse = s1 / float(a.size), s2 / float(a.size)
  else:
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    l1, mse = float(np.abs(d).mean()), float((d * d).mean())
  return np.array([l1, mse, psnr(mse), ssim_map(a, b).mean()], np.float64)


def batch(a, b):
  """[n, H, W, 3] pairs -> [n, 4]"""
  return np.stack([metrics(x, y) for x, y in zip(a, b)])

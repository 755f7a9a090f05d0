"""The stream ingest's definition (include/vp_hip.h vp_pcmin_*, csrc/pcm_in.hip) restated in numpy: WavLoader's conversion and channel mean,
scipy's default resample_poly design, the sum y[m] = sum_k h[m down - k up + half] x[k] in float64, and the emission rule.  The device is
compared with this in tests/test_gpu_pcm.py; tests/test_pcm_host.py pins this against scipy.signal.resample_poly itself."""
import math

import numpy as np

COMMON_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def ratio(rate, out_rate=16000):
  """(up, down, half, taps per phase)"""
  g = math.gcd(int(rate), int(out_rate))
  up, down = out_rate // g, rate // g
  if up == down:
    return 1, 1, 0, 1
  half = 10 * max(up, down)
  return up, down, half, -(-(2 * half + 1) // up)


def design(rate, out_rate=16000):
  """resample_poly's filter for float32 input: float32(firwin(...)) * up, in float32"""
  from scipy.signal import firwin
  up, down, half, _ = ratio(rate, out_rate)
  if up == down:
    return np.ones(1, np.float32)
  h = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)).astype(np.float32)
  h *= up
  return h


def mono(raw, channels):
  """WavLoader.get_data's expressions: interleaved int16 / float32 [n * channels] -> float32 [n]"""
  raw = np.asarray(raw).reshape(-1, channels)
  if raw.dtype.kind == "i":
    data = raw.astype(np.float32) / float(np.iinfo(raw.dtype).max + 1)
  else:
    data = raw.astype(np.float32)
  return data[:, 0] if channels == 1 else data.mean(axis=1)


def samples_after(rate, n, finished=False, out_rate=16000):
  up, down, half, _ = ratio(rate, out_rate)
  total = -(-n * up // down)
  if finished:
    return total
  return min(max((n * up - 1 - half) // down + 1, 0), total)


def last_input_needed(rate, m, out_rate=16000):
  """Index of the newest input frame output m reads (its last tap to arrive)"""
  up, down, half, _ = ratio(rate, out_rate)
  return (m * down + half) // up


def resample(x, rate, out_rate=16000, h=None):
  """float64 y[m], m = 0 .. ceil(N up / down) - 1, from float x [N] and the filter h (default: design(rate), the float32 bank)"""
  up, down, half, T = ratio(rate, out_rate)
  x = np.asarray(x, np.float64)
  if up == down:
    return x.copy()
  h = np.asarray(design(rate, out_rate) if h is None else h, np.float64)
  N = x.shape[0]
  m = np.arange(-(-N * up // down), dtype=np.int64)
  q = m * down + half
  t = np.arange(T, dtype=np.int64)
  j = (q % up)[:, None] + t[None, :] * up
  k = (q // up)[:, None] - t[None, :]
  ok = (j < h.shape[0]) & (k >= 0) & (k < N)
  hv = np.where(ok, h[np.minimum(j, h.shape[0] - 1)], 0.0)
  xv = np.where(ok, x[np.clip(k, 0, N - 1)], 0.0)
  return (hv * xv).sum(axis=1)


def bound(rate, xmax, out_rate=16000, h=None):
  """B = (taps per phase + 1) * 2^-24 * max over the phases of sum |h| * max |x|: the forward error bound of a float32 dot product of
  that length (gamma_n <= n u) plus the rounding of the bank to float32"""
  up, down, half, T = ratio(rate, out_rate)
  if up == down:
    return 0.0
  h = np.abs(np.asarray(design(rate, out_rate) if h is None else h, np.float64))
  worst = max(float(h[p::up].sum()) for p in range(up))
  return (T + 1) * 2.0 ** -24 * worst * float(xmax)


def clip(rate, channels=1, fmt="s16", seconds=0.25, seed=0):
  """A seeded noise + chirp clip of about `seconds` with a ragged length: interleaved [n, channels] int16 or float32"""
  rng = np.random.default_rng(seed * 1000003 + rate + 17 * channels)
  n = int(rate * seconds) + int(rng.integers(1, 97))
  tt = np.arange(n) / float(rate)
  chans = []
  for c in range(channels):
    f0, f1 = 100.0 + 50.0 * c, 0.45 * rate
    chirp = np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / tt[-1] * tt * tt))
    chans.append(0.45 * chirp + 0.25 * rng.uniform(-1, 1, n))
  x = np.stack(chans, axis=1)
  if fmt == "s16":
    return np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
  return x.astype(np.float32)

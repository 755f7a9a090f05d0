"""Float64 reference, derived per-element bound, input families and case table of tests/test_gpu_logmel_ops.py (CPU only: no torch,
no device).  The constants and their derivations are stated in that file's docstring."""
import collections
import functools

import numpy as np

from oracle import audio_ref as ar

U = 2.0 ** -24
EPS = 1e-6
EPS_F32 = float(np.float32(1e-6))        # the kernels' 1e-6f
K_LOG = 4.0                              # 2 ulp of the result = 4 u |result| (twice the 1 ulp commonly stated for logf; no accuracy table is installed)
C_IN, C_STAGE, C_UNTANGLE, C_MAG = 2, 6, 8, 3
C_FUSED = C_IN + 2 * 4 * C_STAGE + C_UNTANGLE + C_MAG       # 61
C_UNFUSED = 3 + 8 + C_MAG                                    # win_length + 14
VACUOUS, VACUOUS_SHARE = 1e-3, 0.02
CLIP_SCALES = (1.0, 0.6, 1.6)
TONE_BINS_512 = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256)
IMPULSE_POS_512 = (0, 1, 255, 256, 257, 511, 100, 101)       # the last two: the even / odd pair of z[n] = x[2n] + i x[2n+1]
NOISE_FLOOR, TONE_AMP = 1e-2, 3e-2

Case = collections.namedtuple("Case", "name sr nmel win hop lo hi b frames tail fams")


def _c(name, nmel, win, hop, b, frames, tail, fams, sr=16000, lo=80.0, hi=7600.0):
  return Case(name, sr, nmel, win, hop, lo, hi, b, frames, tail, tuple(fams.split()))


# tail: samples after the last frame that no frame covers (0 < tail < hop; hop = 1 leaves none)
FUSED_CASES = [
    _c("f1", 80, 512, 128, 1, 1, 77, "sweep tones clicks silence"),
    _c("f5", 79, 512, 160, 1, 5, 33, "sweep tones clicks silence"),
    _c("f31", 40, 512, 128, 1, 31, 127, "sweep tones clicks"),
    _c("f32hop1", 1, 512, 1, 2, 16, 0, "sweep tones clicks silence"),
    _c("f33straddle", 80, 512, 128, 3, 11, 5, "sweep tones clicks silence"),        # block 0 ends inside clip 2, frame 32 is its last
    _c("f65hop512", 80, 512, 512, 5, 13, 100, "sweep tones clicks impulse silence"),
    _c("f33hop640", 80, 512, 640, 3, 11, 130, "sweep tones clicks impulse silence"),  # gaps of 128 samples between frames
    _c("f32edges", 40, 512, 160, 1, 32, 1, "sweep tones clicks", lo=300.0, hi=3400.0),
    _c("f33sr8000", 80, 512, 128, 3, 11, 64, "sweep tones clicks", sr=8000),         # Nyquist = 4000 Hz < upper_hz: bin 256 carries weight
    _c("f65", 80, 512, 128, 1, 65, 3, "sweep tones clicks"),
]
# igemm pixel tile of plan_fwd for P = B F rows (igemm_pixel_tile below): 16 up to P = 16 (32 at win 16), 32 for 17 .. 95, 128 from 96
UNFUSED_CASES = [
    _c("u512x81_p15", 81, 512, 128, 3, 5, 9, "clicks silence"),                     # below the 16-pixel tile
    _c("u512x81_p16", 81, 512, 512, 1, 16, 16, "clicks impulse"),                   # exactly one 16-pixel tile
    _c("u512x81_p17", 81, 512, 528, 1, 17, 3, "clicks impulse"),                    # 17: the first P of the 32-pixel tile; hop = win + 16
    _c("u512x128_p33", 128, 512, 1, 3, 11, 0, "clicks silence"),                    # 32-pixel tile + 1; one all-zero mel column
    _c("u256x80_p32", 80, 256, 64, 1, 32, 13, "clicks"),                            # exactly one 32-pixel tile; one all-zero mel column
    _c("u256x80_p33", 80, 256, 1, 3, 11, 0, "clicks silence"),
    _c("u256x80_p31", 80, 256, 256, 1, 31, 100, "clicks impulse"),
    _c("u256x80_p96", 80, 256, 272, 3, 32, 7, "clicks impulse"),                    # 96: the first P of the 128-pixel tile (below one tile)
    _c("u16x8_p128", 8, 16, 4, 1, 128, 2, "sweep tones clicks silence"),             # exactly one 128-pixel tile
    _c("u16x8_p129", 8, 16, 16, 3, 43, 5, "sweep tones clicks impulse silence"),     # 128 + 1
    _c("u16x1_p127", 1, 16, 32, 1, 127, 9, "sweep tones clicks impulse"),
    _c("u16x1_p1", 1, 16, 1, 1, 1, 0, "sweep clicks"),
    _c("u1024x80_p5", 80, 1024, 256, 1, 5, 100, "clicks"),
    _c("u1024x80_p33", 80, 1024, 1040, 3, 11, 50, "clicks impulse"),
    _c("u4096x128_p2", 128, 4096, 4096, 1, 2, 17, "clicks impulse"),
    _c("u4096x128_p6", 128, 4096, 1024, 3, 2, 500, "clicks silence"),
]
ALL_CASES = FUSED_CASES + UNFUSED_CASES
BOTH_PATHS = (_c("both80", 80, 512, 128, 3, 11, 5, "clicks"), _c("both81", 81, 512, 128, 3, 11, 5, "clicks"))


def is_fused(c):
  return c.win == 512 and c.nmel <= 80


def samples(c):
  return c.win + (c.frames - 1) * c.hop + c.tail


def igemm_pixel_tile(win, p):
  """Pixel tile of the DFT product's plan (pick_igemm_cfg, conv_ops.h) for rows = ncol = round_up(win + 2, 8) and P = B F pixels."""
  rows = -(-(win + 2) // 8) * 8
  return 128 if p >= 96 else (32 if rows <= 64 or p > 16 else 16)


def f32(a):
  return np.asarray(a, np.float32).astype(np.float64)


def case_seed(c):
  return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 100000


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: [B, L] float64 holding float32 values
# ---------------------------------------------------------------------------------------------------------------------------------
def covered(c):
  """[L] bool: samples that some frame reads."""
  m = np.zeros(samples(c), bool)
  for f in range(c.frames):
    m[f * c.hop:f * c.hop + c.win] = True
  return m


def tone_bins(c):
  return sorted({k * c.win // 512 for k in TONE_BINS_512} | {0, 1, c.win // 2 - 1, c.win // 2})


def impulse_positions(c):
  return sorted({min(p * c.win // 512, c.win - 1) for p in IMPULSE_POS_512} | {1, c.win // 2 + 1, c.win - 1, 4 * c.win // 16, 4 * c.win // 16 + 1})


def tone_of(c, clip, region):
  bins = tone_bins(c)
  return bins[(region + 5 * clip + case_seed(c)) % len(bins)]


def impulse_of(c, clip, frame):
  """(position inside the frame, amplitude): every (clip, frame) has its own amplitude."""
  pos = impulse_positions(c)
  n0 = pos[(frame + 3 * clip + 2) % len(pos)]
  return n0, CLIP_SCALES[clip % 3] * (0.25 + 0.5 * ((7 * frame + 3 * clip) % 23) / 23.0) * (-1.0 if (frame + clip) % 2 else 1.0)


def make_pcm(c, fam):
  """family `fam` for case c.  silence: clip 0 (B = 1: the only clip) silent, the others the case's first loud family."""
  n, seed = samples(c), case_seed(c)
  out = np.zeros((c.b, n))
  for b in range(c.b):
    rng = np.random.default_rng(1000 * seed + b)
    scale = CLIP_SCALES[b % 3]
    t = np.arange(n)
    if fam == "silence":
      if b > 0:
        out[b] = make_pcm(c, c.fams[0])[b]
    elif fam == "sweep":            # test_gpu_audio.synth_pcm, per clip its own noise and scale
      ts = t / 16000.0
      sweep = 0.3 * np.sin(2 * np.pi * (100 + (4000 - 100) * ts / max(ts[-1], 1e-9) / 2) * ts)
      out[b] = scale * np.clip(0.1 * rng.normal(size=n) + sweep, -1, 1)
    elif fam == "tones":            # region r = samples [r win, (r + 1) win): a tone at the centre of one bin, over the noise floor
      k = np.array([tone_of(c, b, r) for r in range(n // c.win + 1)])[t // c.win]
      out[b] = scale * (NOISE_FLOOR * rng.normal(size=n) + TONE_AMP * np.cos(2 * np.pi * k * t / c.win + 0.3 * b))
    elif fam == "clicks":           # sparse clicks anywhere, about four per window (two where the window is longer than 512)
      hit = rng.random(n) < (4.0 if c.win <= 512 else 2.0) / c.win
      hit[rng.integers(0, n)] = True
      out[b] = scale * hit * rng.uniform(0.2, 0.9, size=n) * rng.choice([-1.0, 1.0], size=n)
    elif fam == "impulse":          # hop >= win: frames are disjoint, frame f owns samples [f hop, f hop + win) and gets ONE sample there
      assert c.hop >= c.win
      for f in range(c.frames):
        n0, a = impulse_of(c, b, f)
        out[b, f * c.hop + n0] = a
    else:
      raise ValueError(fam)
  return f32(out)


def device_pcm(c, pcm):
  """What the device is given: the samples no frame covers (the tail, the gaps of hop > win) are NaN - a read of one shows."""
  return np.where(covered(c)[None, :], pcm, np.nan).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mel_matrix(c):
  """[nb, nmel] float64 of the float32 matrix (TF keeps it in float32)."""
  m = f32(ar.linear_to_mel_weight_matrix(c.nmel, c.win // 2 + 1, c.sr, c.lo, c.hi))
  m.setflags(write=False)
  return m


def mel_matrix_as_created(c):
  """vp_logmel_create's loops (plan_bfmnet.hip) restated: float64 arithmetic in ITS order, cast to float32."""
  nb = c.win // 2 + 1
  hz2mel = lambda f: 1127.0 * np.log1p(f / 700.0)
  lo, hi = hz2mel(float(np.float32(c.lo))), hz2mel(float(np.float32(c.hi)))
  k = np.arange(nb, dtype=np.float64)[:, None]
  j = np.arange(c.nmel, dtype=np.float64)[None, :]
  m = hz2mel(k * (c.sr / 2.0) / (nb - 1))
  e0, e1, e2 = lo + (hi - lo) * j / (c.nmel + 1), lo + (hi - lo) * (j + 1) / (c.nmel + 1), lo + (hi - lo) * (j + 2) / (c.nmel + 1)
  v = np.minimum((m - e0) / (e1 - e0), (e2 - m) / (e2 - e1))
  v = np.where(v > 0, v, 0.0)
  v[0] = 0.0
  return v.astype(np.float32)


def zero_columns(c):
  return np.flatnonzero(~mel_matrix(c).any(axis=0))


def frame_sums(c, pcm):
  """s_f = sum_n |x_n w_n|, [B, F]."""
  idx = np.arange(c.win)[None, :] + c.hop * np.arange(c.frames)[:, None]
  return (np.abs(pcm[:, idx]) * ar.hann_periodic(c.win)).sum(-1)


def mag_constant(c):
  return C_FUSED if is_fused(c) else c.win + C_UNFUSED


Ref = collections.namedtuple("Ref", "mag acc log bound zero dacc")


def from_mag(c, mag, s):
  """Reference and bound from float64 magnitudes [B, F, nb] and frame sums [B, F]."""
  mel = mel_matrix(c)
  nk = 257 if is_fused(c) else c.win // 2 + 1
  acc = mag @ mel
  dmag = mag_constant(c) * U * s
  dacc = dmag[..., None] * mel.sum(0) + (nk + 2) * U * acc
  darg = dacc + U * EPS + U * (acc + dacc + EPS) * (1 + U)          # + the rounding of 1e-6f and of the float32 sum acc + 1e-6f
  arg = acc + EPS
  log = np.log(arg)
  with np.errstate(divide="ignore", invalid="ignore"):
    dlog = np.where(darg < arg, np.log1p(darg / np.where(darg < arg, arg - darg, 1.0)), np.inf)
  bound = dlog + K_LOG * U * (np.abs(log) + np.where(np.isfinite(dlog), dlog, 0.0))
  zero = np.zeros(acc.shape, bool)
  zero[..., zero_columns(c)] = True
  zero |= (s == 0)[..., None]                                       # a silent frame: acc = 0 exactly as well
  return Ref(mag, acc, log, bound, zero, dacc)


def reference(c, pcm):
  return from_mag(c, ar.stft_mag(pcm, c.win, c.hop, c.win), frame_sums(c, pcm))


def impulse_closed_form(c, pcm=None):
  """log(a w[n0] colsum(mel)[m] + 1e-6): |X_k| of one sample a at n0 is a w[n0] at every bin."""
  w, cs = ar.hann_periodic(c.win), mel_matrix(c).sum(0)
  out = np.zeros((c.b, c.frames, c.nmel))
  for b in range(c.b):
    for f in range(c.frames):
      n0, a = impulse_of(c, b, f)
      out[b, f] = np.log(abs(float(np.float32(a))) * w[n0] * cs + EPS)
  return out


LOG_EPS_F32 = float(np.log(EPS_F32))


def vacuous_share(ref):
  live = ~ref.zero
  return float((ref.bound[live] > VACUOUS).mean()) if live.any() else 0.0


def reference_conditions(c, ref):
  """Asserted on the reference alone, before any device call."""
  share = vacuous_share(ref)
  assert share <= VACUOUS_SHARE, "%s: %.1f %% of the elements have a log-domain bound above %g" % (c.name, 100 * share, VACUOUS)
  assert (ref.acc[ref.zero] == 0).all(), "%s: a zero mel column or silent frame with a non-zero reference energy" % c.name
  assert ref.zero[..., zero_columns(c)].all()


def compare(c, got, ref):
  """(ratio [B, F, nmel], ok): |got - ref| / bound per element; the acc = 0 elements against log(1e-6f) under the K_LOG term alone."""
  got = np.asarray(got, np.float64)
  assert got.shape == ref.log.shape, (got.shape, ref.log.shape)
  with np.errstate(invalid="ignore"):
    ratio = np.abs(got - ref.log) / ref.bound
    ratio = np.where(ref.zero, np.abs(got - LOG_EPS_F32) / (K_LOG * U * abs(LOG_EPS_F32)), ratio)
  ratio = np.where(np.isfinite(got), ratio, np.inf)
  return ratio, bool((ratio <= 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# two independent float32 restatements of the front end
# ---------------------------------------------------------------------------------------------------------------------------------
def _frames32(c, pcm):
  idx = np.arange(c.win)[None, :] + c.hop * np.arange(c.frames)[:, None]
  return pcm.astype(np.float32)[:, idx] * ar.hann_periodic(c.win).astype(np.float32)


def _fft_r2(x):
  n = x.shape[-1]
  if n == 1:
    return x
  e, o = _fft_r2(x[..., ::2]), _fft_r2(x[..., 1::2])
  t = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64) * o
  return np.concatenate([e + t, e - t], axis=-1)


def _tail32(c, mag32):
  acc = mag32.astype(np.float32) @ mel_matrix(c).astype(np.float32)
  return np.log(acc + np.float32(1e-6)).astype(np.float64)


def logmel_f32_fft(c, pcm):
  """radix-2 decimation-in-time FFT in complex64."""
  z = _fft_r2(_frames32(c, pcm).astype(np.complex64))
  assert z.dtype == np.complex64
  return _tail32(c, np.abs(z[..., :c.win // 2 + 1]))


def logmel_f32_dft(c, pcm):
  """float32 DFT matrix product."""
  nb = c.win // 2 + 1
  ang = 2 * np.pi * ((np.arange(c.win)[:, None] * np.arange(nb)[None, :]) % c.win) / c.win
  fr = _frames32(c, pcm)
  re, im = fr @ np.cos(ang).astype(np.float32), fr @ (-np.sin(ang)).astype(np.float32)
  assert re.dtype == np.float32
  return _tail32(c, np.sqrt(re * re + im * im))

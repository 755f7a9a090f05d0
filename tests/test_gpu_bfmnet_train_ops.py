"""Op-level float64 parity of the BFMNet TRAINING kernels (csrc/bfm_train.hip and the training half of csrc/gru_device.h), the
counterpart of test_gpu_bfmnet_ops.py for everything of the training step that is not a matrix product.

Rules common to every GPU case (as test_gpu_bfmnet_ops.py, whose helpers are reused)
  * the device sees float32 values; the reference is float64 arithmetic on exactly those values.  What an entry point takes as an input
    (mean / rstd / shift of the batch-norm backward, the saved gates of the GRU backward) is TEST-MADE, rounded to float32 and exact for
    the reference: no backward test depends on a forward kernel;
  * outputs are prefilled with NaN between two guard bands of a sentinel that must come back untouched; in-place entry points get the
    guard bands only;
  * the clips / row groups of a batch differ in seed and scale (CLIP_SCALES);
  * the comparison is PER ELEMENT, |got - ref| <= bound, u = 2^-24, v = 2^-53; where a bound is 0 the element must be bit-equal;
  * every case recomputes the launcher's formula (bn_shape, dw_wgrad_shape, tblk) and asserts the class it was written for.

Bounds (first order in u; the integer factors count the roundings on the longest path, an addition of an exact 0 rounds nothing)
  chan_sums / finalize (float64 sums of P float32 terms in at most P + nchunk inexact additions: gamma = (P + nchunk) v)
    mean   u |m| + gamma E|x|
    var    u (|var| + e) + e,  e = 5 gamma E[x^2]   (c = 5: Sum x^2 once, m^2 = (Sum x / P)^2 twice as |m| E|x| <= E[x^2], and the four
           local roundings s1 / P, m * m, the difference, s0 / P, each <= v E[x^2]; 3 (P + nchunk) + 4 <= 5 (P + nchunk))
    rstd   u |rstd| + (e / 2) (var + eps)^-3/2 + 3 v |rstd|        scale == rstd bit for bit
    shift  u |shift| + |m| bound(rstd) + rstd bound_f64(m)          (the device multiplies by the ROUNDED rstd: u |m| rstd is in bound(rstd))
  batch-norm backward (dz = da act'(y), y = fl(rstd x + shift) decided exactly; leaky: dz carries one rounding, lk = 1, else lk = 0)
    dbeta  u |dbeta| + (gamma + lk u) Sum |dz|
    c1     u |c1| + (gamma + 2 v + lk u) E|dz|
    c2     u |c2| + (gamma + 2 v + (2 + lk) u) E|dz xhat|          (xhat = fl(fl(x - mean) rstd): two roundings)
    dx     u |dx| + rstd (6 u S + bound(c1) + |xhat| bound(c2)),  S = |dz| + |c1| + |xhat c2|
           (6: dz's own, x - mean, * rstd, * c2, the two subtractions; then the product with rstd)
  element-wise   one rounding per element (fmaf + activation; a product; a copy; out + ears * (-2 | -4), a product with a power of two):
                 BIT-EXACT against numpy float32.  Two roundings where the compiler may contract (act(.) * mask + add; decay * moving +
                 factor * batch): u (|a| + |b|) + u |ref| over the two products / terms a, b - covers every contraction.
  colsum         (rows + 1) u Sum |x|  (one chain in row order)
  dw weight grad (items_per_wave * HS + 3 + ceil(G / 16) + 5) u Sum |x dy|   per (tap, channel), from dw_wgrad_shape
  max-pool bwd   3 u Sum |dy| where more than one window holds the element, 0 (exact) elsewhere
  GRU forward, one step from the device's own h_prev (n roundings of a chain are bounded by (n + 3) u Sum |terms|)
    a_gate  (128 + 3) u (|xg| + Sum |h||whg|)                      r, u: bound(a) / 4 + K_SIG u |r|
    a_cand  (64 + 3) u (|xc| + Sum |r h||whc|) + Sum |h| bound(r) |whc|        c: bound(a) + K_TANH u |c|
    h'      |h - c| bound(u) + (1 - u) bound(c) + 3 u (|u h| + |(1 - u) c|)
    K_SIG / K_TANH: twice the worst error of 1 / (1 + expf(-a)) and tanhf(a) measured on the MI355X over [-20, 20] through this kernel
    with whg = whc = 0 (no copy of the HIP math accuracy table is installed): measured 2.670 / 2.389 u |ref| (2.558 / 1.365 ulp),
    rounded up to 2.68 / 2.39, allowed 5.36 / 4.78; test_gru_gate_functions_as_measured repeats the measurement and asserts the figures.
  GRU backward: a running bound next to the reference (gru_bwd_ref); e = bound of the carried dh, eg = e + u |g|
    d_ac  (1 - u)|1 - c^2| eg + 4 u |d_ac| + 2 u |d_c|             d_u  |h - c| eg + 3 u |d_u|
    d_rh  (64 + 3) u |whc| |d_ac| + |whc| bound(d_ac)              d_ar |h| r (1 - r) bound(d_rh) + 4 u |d_ar|
    d_au  u (1 - u) bound(d_u) + 4 u |d_au|                        each of d_ac, d_ar, d_au + 8 eta, eta = 2^-149: the gradients of saturated
                                                                   gates reach the float32 subnormals, where a rounding loses up to eta, not u |x|
    dh'   u_gate eg + u |g u| + r bound(d_rh) + u |dhp| + (128 + 3) u |whg| |d_ag| + |whg| bound(d_ag) + u |dh'|
    (valid for any T; it grows with the products of the absolute-value matrices, so at T = 125 it is loose for the early steps)
  vertex loss   gD: 4 u Sum |terms| of the element;  loss: (u Sum |D| vm + 2 u Sum |D' - D| vm) / B + (2 T + 20 + nblk / 256) v loss
  float64 sums  (n / blocks + 10) v Sum x^2;  vp_sum_f64: (n / 256 + 10) v (|add| + |scale| Sum |p|)
  clip / Adam   g' = g scale: 2 u |g'|  (scale == 1 below the clip: bit-identical)
    m   (1 - b1) 2 u |g'| + u (|b1 m| + |(1 - b1) g'|) + u |m'|          (1 - b1, 1 - b2 are exact in float32 for 0.9, 0.999)
    v   2 (1 - b2) |g'| 2 u |g'| + u (|b2 v| + 2 (1 - b2) g'^2) + u |v'|
    p   u |p'| + |q| (5 u + (bound(v) / (2 sqrt v) + 2 u sqrt v) / (sqrt v + eps)) + lr bound(m) / (sqrt v + eps),  q = lr m / (sqrt v + eps)

Case tables: BN_CASES, ACT_SIZES, DW_CASES, POOL axes, GRU_CASES, VLOSS_CASES, FLAT_SIZES below.  The batch-norm backward runs every
(P, C) class with act 0 (vp_bn_train_bwd, no shift), ReLU and ReLU6, and the leaky branch once; the 32-clip vertex-loss case of the
issue runs at B = 8: its float64 reference at B = 32 (82 M elements) costs four times the 16-core seconds and 3 GB for no new launch
class (B J is no multiple of 256 either way, and the clips still differ in length).  DW_CASES states the class dw_wgrad_shape really
gives each shape: H = 20 at 40 columns is two segments of one unroll each (segments longer than one unroll need more than 2048 / (H / 20)
columns: (32, 120, 40, 32) runs six unrolls per segment, three items per wave); (2, 12, 3, 6) is there for a channel count that is no
multiple of 4, which vp_dwconv7x3_wgrad accepts.

Measured on an MI355X (worst |got - ref| / bound per kernel over all cases; 296 cases, 23 s):
  bn_train_fwd 0.983   bn_train_bwd 1.000   affine_act 1.000   moving_update 0.975   l2_regulariser 1.000   adam_tf_clipped 0.999
  (these bounds are dominated by the rounding of the output itself: half an ulp IS u |ref| just above a power of two)
  colsum 0.388   dwconv7x3_wgrad 0.054   maxpool_hw_bwd 0.333   gru_train_fwd 0.302   gru_train_bwd 0.420   vertex_loss 0.200
  clip_scale 0.626   sum_f64 0.008   sumsq 0.005   step_report, act_bwd, mul, add_ears, gru_split, stem_im2col: bit-equal
  GRU forward end to end against oracle.audio_ref.gru_seq: rel-L2 4.3e-08 ... 7.4e-08 (T = 1 ... 125)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import audio_ref as ar
from oracle import bfmnet_train_torch as bt
from voicepuppet_amd import _lib

import gpu_util as gu
from test_gpu_bfmnet_ops import CLIP_SCALES, SENTINEL, VP_ERR_ARG, assert_guards, f32, guarded

gpu = pytest.mark.gpu
U = 2.0 ** -24
V = 2.0 ** -53
ETA = 2.0 ** -149                       # spacing of the float32 subnormals: what one rounding can lose below 2^-126
BN_EPS = 1e-3
SIG_MEASURED, TANH_MEASURED = 2.68, 2.39      # worst |err| / (u |ref|) on the MI355X, rounded up (test_gru_gate_functions_as_measured)
K_SIG, K_TANH = 2 * SIG_MEASURED, 2 * TANH_MEASURED
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_RELU6 = 0, 1, 2, 5


# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' formulas, restated (csrc/bfm_train.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def tblk(work, cap=4096):
  return max(1, min((work + 255) // 256, cap))


def bn_shape(pixels, c):
  cq, ql = c // 4, 3
  while ql < 6 and (1 << ql) < cq:
    ql += 1
  rl = 256 >> ql
  return ql, max(1, min(pixels // (rl * 8), 256))


def dw_wgrad_shape(b, h, w):
  """(HS, nseg, G, items per wave, rows of the last segment)"""
  cols = b * w
  nseg = min((2048 + cols - 1) // cols, max(h // 10, 1))
  hs = (h + nseg - 1) // nseg
  hs = (hs + 9) // 10 * 10
  nseg = (h + hs - 1) // hs
  g = min((cols * nseg + 3) // 4, 256)
  return hs, nseg, g, -(-(cols * nseg) // (4 * g)), h - (nseg - 1) * hs


# (P, C) -> (ql, nchunk, blocks in y)
BN_CASES = {(1, 4): (3, 1, 1), (7, 8): (3, 1, 1), (31, 32): (3, 1, 1), (1600, 32): (3, 6, 1), (19200, 32): (3, 75, 1), (19200, 384): (6, 256, 2),
            (153600, 32): (3, 256, 1), (153600, 192): (6, 256, 1), (9600, 1536): (6, 256, 6), (257, 768): (6, 8, 3)}
# (B, H, W, C) -> (HS, nseg, G, items per wave, rows of the last segment)
DW_CASES = {(2, 9, 5, 8): (10, 1, 3, 1, 9), (1, 10, 40, 32): (10, 1, 10, 1, 10), (1, 20, 40, 32): (10, 2, 20, 1, 10), (1, 125, 40, 32): (20, 7, 70, 1, 5),
            (1, 125, 3, 1536): (20, 7, 6, 1, 5), (3, 17, 1, 64): (20, 1, 1, 1, 17), (4, 120, 40, 384): (10, 12, 256, 2, 10),
            (32, 120, 40, 32): (60, 2, 256, 3, 60), (3, 60, 20, 192): (10, 6, 90, 1, 10), (2, 30, 10, 100): (10, 3, 15, 1, 10), (2, 12, 3, 6): (20, 1, 2, 1, 12)}
# (pixels, c): quads below 256, no multiple of 256, above the 4096 x 256 grid cap of tblk
ACT_SIZES = [(7, 8), (257, 12), (8200, 516)]
STEM_CASES = [(1, 5, 80), (3, 125, 80), (2, 8, 7), (8, 125, 80)]      # the last: im2col_9x5_kernel's stride loop runs twice
POOL_ABOVE_CAP = (4, 120, 40, 256)                                    # the first pool at batch 4 x 24 frames: 1 228 800 quads
POOLS = [((2, 2), (1, 2)), ((5, 3), (5, 3))]                          # (window, stride) of the net's two SAME max-pools
GRU_CASES = [(1, 1, [1]), (4, 7, [7, 4, 1, 0]), (3, 24, [24, 23, 12]), (32, 24, None), (2, 125, [125, 60])]
VLOSS_CASES = [(2, 4, 360, [4, 3]), (1, 1, 360, [1]), (3, 5, 257, [5, 0, 1]), (4, 24, 107127, [24, 24, 13, 2]), (8, 24, 107127, [24, 1, 17, 0, 24, 9, 2, 23])]
FLAT_SIZES = [4, 1020, 262144, 1000000, 4200000]      # the last: more quads than the 4096 x 256 of adam_clip_kernel's capped grid


def gru_seq_len(b, t, seq):
  if seq is not None:
    return np.asarray(seq, np.int32)
  s = np.random.default_rng(b * 100 + t).integers(1, t + 1, size=b)
  s[[3, 17]] = 0
  s[0] = t
  return s.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references with their bounds (CPU only)
# ---------------------------------------------------------------------------------------------------------------------------------
def rows(p, c, seed, sigma=1.0, offset=0.0):
  """[p, c] float32 values as float64: three row groups (the 'clips') with their own seed and scale, a per-channel offset."""
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((p, c), dtype=np.float32)
  cut = [0, p // 3, 2 * p // 3, p]
  for i in range(3):
    x[cut[i]:cut[i + 1]] *= np.float32(CLIP_SCALES[i] * sigma)
  if p < 3:
    x *= np.float32(sigma)
  return (x + np.float32(offset)).astype(np.float64)


def bn_fwd_inputs(p, c, seed):
  rng = np.random.default_rng(seed + 1)
  x = rows(p, c, seed, 1.0, rng.normal(0, 2.0, c).astype(np.float32))
  if c >= 32:
    x[:, 1] = 3.25                                                                 # variance exactly 0
    x[:, 2] = f32(100.0 + 0.01 * np.random.default_rng(seed + 2).standard_normal(p))      # mean 100, deviation 0.01
  beta = f32(rng.uniform(-3.0, 9.0, c))
  return x, beta


def bn_fwd_ref(x, beta, nchunk, eps=BN_EPS):
  """{name: (reference, bound)} of vp_bn_train_fwd: two-pass float64."""
  p = x.shape[0]
  eps = float(np.float32(eps))
  m = x.mean(0)
  var = ((x - m) ** 2).mean(0)
  gam = (p + nchunk) * V
  em = gam * np.abs(x).mean(0)
  e = 5 * gam * (x * x).mean(0)
  rstd = 1.0 / np.sqrt(var + eps)
  b_rstd = U * rstd + 0.5 * e * (var + eps) ** -1.5 + 3 * V * rstd
  shift = beta - m * rstd
  return {"mean": (m, U * np.abs(m) + em), "var": (var, U * (var + e) + e), "rstd": (rstd, b_rstd),
          "shift": (shift, U * np.abs(shift) + np.abs(m) * b_rstd + rstd * em)}


def act_deriv(act, y):
  if act == ACT_LRELU:
    return np.where(y >= 0, 1.0, float(np.float32(0.2)))
  if act == ACT_RELU:
    return (y > 0).astype(np.float64)
  if act == ACT_RELU6:
    return ((y > 0) & (y < 6)).astype(np.float64)
  return np.ones_like(y, np.float64)


def act_fwd32(act, v):
  """act_f on float32 values in float32 arithmetic (one IEEE product for the leaky branch)."""
  v = v.astype(np.float32)
  if act == ACT_LRELU:
    return np.where(v >= 0, v, np.float32(0.2) * v)
  if act == ACT_RELU:
    return np.maximum(v, np.float32(0))
  if act == ACT_RELU6:
    return np.minimum(np.maximum(v, np.float32(0)), np.float32(6))
  return v


def fma32(a, x, b):
  """fl32(a * x + b) of float32 values held in float64.  The product is exact in float64.  Where the float64 sum is exact too (TwoSum
  residual 0) float32(sum) is the fused result, ties included (both round to even).  Where it is not, the float64 value must not sit on
  a float32 rounding tie (the lost bits would decide the direction) - asserted; then float32(float64 value) IS the fused result."""
  p = a * x
  y = p + b
  bb = y - p
  inexact = ((p - (y - bb)) + (b - bb)) != 0
  y32 = y.astype(np.float32)
  lo = y32.astype(np.float64)
  other = np.nextafter(y32, np.where(y > lo, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
  assert not (inexact & (y != lo) & (y == 0.5 * (lo + other))).any(), "an inexact float64 pre-activation sits on a float32 rounding tie"
  return y32


def bn_bwd_inputs(p, c, seed):
  """x, da, and TEST-MADE mean / rstd / shift (float32 values): near the statistics of x, beta spread so that y hits every regime."""
  rng = np.random.default_rng(seed + 3)
  off = rng.normal(0, 2.0, c).astype(np.float32)
  x = rows(p, c, seed, 1.3, off)
  da = rows(p, c, seed + 50, 1.0)
  mean = f32(off + rng.normal(0, 0.05, c))
  rstd = f32(1.0 / 1.3 * rng.uniform(0.8, 1.25, c))
  beta = np.linspace(-2.0, 8.0, c)[rng.permutation(c)] if c <= 8 else rng.uniform(-3.0, 9.0, c)
  shift = f32(beta - mean * rstd)
  return x, da, mean, rstd, shift


def bn_bwd_ref(x, da, mean, rstd, shift, act, nchunk):
  """{name: (reference, bound)} of vp_bn_act_train_bwd for dx, dbeta and the workspace's c1, c2; and the pre-activation y."""
  p = x.shape[0]
  y = fma32(rstd, x, shift).astype(np.float64) if act else None
  dz = da * act_deriv(act, y) if act else da
  lk = 1.0 if act == ACT_LRELU else 0.0
  xhat = (x - mean) * rstd
  gam = (p + nchunk) * V
  adz, adzx = np.abs(dz), np.abs(dz * xhat)
  dbeta, c1, c2 = dz.sum(0), dz.mean(0), (dz * xhat).mean(0)
  b_dbeta = U * np.abs(dbeta) + (gam + lk * U) * adz.sum(0)
  b_c1 = U * np.abs(c1) + (gam + 2 * V + lk * U) * adz.mean(0)
  b_c2 = U * np.abs(c2) + (gam + 2 * V + (2 + lk) * U) * adzx.mean(0)
  dx = rstd * (dz - c1 - xhat * c2)
  s = adz + np.abs(c1) + np.abs(xhat * c2)
  b_dx = U * np.abs(dx) + rstd * (6 * U * s + b_c1 + np.abs(xhat) * b_c2)
  return {"dx": (dx, b_dx), "dbeta": (dbeta, b_dbeta), "c1": (c1, b_c1), "c2": (c2, b_c2)}, y


def assert_regimes6(y):
  lo, hi, mid = float((y < 0).mean()), float((y > 6).mean()), float(((y >= 0) & (y <= 6)).mean())
  assert lo >= 0.10 and hi >= 0.10 and mid >= 0.30, (lo, hi, mid)


def dw_wgrad_ref(x, dy, shape):
  """(dW [21, C], bound): the float64 sum of test_gpu_bfmnet_train.py and the chain-length bound of the launch shape."""
  b, h, w, c = x.shape
  hs, nseg, g, ipw, _ = shape
  xp = np.pad(x, ((0, 0), (3, 3), (1, 1), (0, 0)))
  ref = np.stack([(xp[:, kh:kh + h, kw:kw + w, :] * dy).sum((0, 1, 2)) for kh in range(7) for kw in range(3)])
  ax, ady = np.abs(xp), np.abs(dy)
  mag = np.stack([(ax[:, kh:kh + h, kw:kw + w, :] * ady).sum((0, 1, 2)) for kh in range(7) for kw in range(3)])
  return ref, (ipw * hs + 3 + -(-g // 16) + 5) * U * mag


def pool_geometry(h, w, k, s):
  pt, _, ho = ar.same_pads(h, k[0], s[0])
  pl, _, wo = ar.same_pads(w, k[1], s[1])
  return pt, pl, ho, wo


def maxpool_bwd_ref(x, dy, k, s):
  """(dx, bound): TF MaxPoolGrad - the FIRST maximum of a row-major scan of the (clipped) window takes the window's gradient."""
  b, h, w, c = x.shape
  pt, pl, ho, wo = pool_geometry(h, w, k, s)
  dx, mag, cnt = np.zeros_like(x), np.zeros_like(x), np.zeros((h, w), int)
  for oh in range(ho):
    h0, h1 = max(oh * s[0] - pt, 0), min(oh * s[0] - pt + k[0], h)
    for ow in range(wo):
      w0, w1 = max(ow * s[1] - pl, 0), min(ow * s[1] - pl + k[1], w)
      win = x[:, h0:h1, w0:w1, :].reshape(b, -1, c)
      first = np.argmax(win, axis=1)                     # numpy returns the first of equal maxima; the reshape is row-major
      g = np.zeros_like(win)
      np.put_along_axis(g, first[:, None, :], dy[:, oh, ow][:, None, :], axis=1)
      dx[:, h0:h1, w0:w1, :] += g.reshape(b, h1 - h0, w1 - w0, c)
      mag[:, h0:h1, w0:w1, :] += np.abs(g).reshape(b, h1 - h0, w1 - w0, c)
      cnt[h0:h1, w0:w1] += 1
  return dx, np.where(cnt[None, :, :, None] > 1, 3 * U * mag, 0.0)


def sigmoid(a):
  return 1.0 / (1.0 + np.exp(-a))


def gru_inputs(b, t, seed, hdim=256, wsig=0.05):
  """xg [b,t,2h], xc [b,t,h], whg [h,2h], whc [h,h]: two fifths of the units get inputs 25 times as wide (saturated gates)."""
  rng = np.random.default_rng(seed)
  wide = np.where(rng.uniform(size=2 * hdim) < 0.4, 25.0, 1.0)
  xg = f32(np.stack([CLIP_SCALES[i % 3] * np.random.default_rng(seed * 1000 + i).normal(size=(t, 2 * hdim)) for i in range(b)]) * wide)
  xc = f32(np.stack([CLIP_SCALES[i % 3] * np.random.default_rng(seed * 1000 + 500 + i).normal(size=(t, hdim)) for i in range(b)]) * wide[:hdim] * 0.3)
  return xg, xc, f32(rng.normal(0, wsig, (hdim, 2 * hdim))), f32(rng.normal(0, wsig, (hdim, hdim)))


def gru_step_ref(xg, xc, whg, whc, h):
  """One step from h (exact): {r, u, c, hn: (reference, bound)} and the gate pre-activation."""
  hd = h.shape[-1]
  ag = xg + h @ whg
  b_ag = 131 * U * (np.abs(xg) + np.abs(h) @ np.abs(whg))
  g = sigmoid(ag)
  b_g = b_ag / 4 + K_SIG * U * g
  r, u = g[..., :hd], g[..., hd:]
  b_r, b_u = b_g[..., :hd], b_g[..., hd:]
  rh = r * h
  ac = xc + rh @ whc
  b_ac = 67 * U * (np.abs(xc) + np.abs(rh) @ np.abs(whc)) + (np.abs(h) * b_r + U * np.abs(rh)) @ np.abs(whc)
  c = np.tanh(ac)
  b_c = b_ac + K_TANH * U * np.abs(c)
  hn = u * h + (1 - u) * c
  b_h = np.abs(h - c) * b_u + (1 - u) * b_c + 3 * U * (np.abs(u * h) + np.abs((1 - u) * c))
  return {"r": (r, b_r), "u": (u, b_u), "c": (c, b_c), "hn": (hn, b_h)}, ag


def gru_fwd_ref(xg, xc, whg, whc, seq):
  """float64 forward with what the training kernel saves: out, r, u, c, hprev (past the end: 0, 0, 0, 0, the frozen state)."""
  b, t, hd = xc.shape
  h = np.zeros((b, hd))
  out, r, u, c, hp = [np.zeros((b, t, hd)) for _ in range(5)]
  for i in range(t):
    live = (i < np.asarray(seq))[:, None]
    g = sigmoid(xg[:, i] + h @ whg)
    ri, ui = g[:, :hd], g[:, hd:]
    ci = np.tanh(xc[:, i] + (ri * h) @ whc)
    hn = ui * h + (1 - ui) * ci
    hp[:, i] = h
    r[:, i], u[:, i], c[:, i], out[:, i] = [np.where(live, a, 0.0) for a in (ri, ui, ci, hn)]
    h = np.where(live, hn, h)
  return out, r, u, c, hp


def gru_bwd_ref(dout, whg, whc, seq, r, u, c, hp):
  """(dag, dac, bound(dag), bound(dac)): float64 backward through time to the gate / candidate pre-activations from the SAVED r, u, c,
  h_prev (exact inputs), and the running bound of the module docstring carried next to it."""
  b, t, hd = dout.shape
  dag, dac = np.zeros((b, t, 2 * hd)), np.zeros((b, t, hd))
  b_dag, b_dac = np.zeros_like(dag), np.zeros_like(dac)
  dh, e = np.zeros((b, hd)), np.zeros((b, hd))
  awg, awc = np.abs(whg), np.abs(whc)
  seq = np.asarray(seq)
  for i in range(t - 1, -1, -1):
    live = (i < seq)[:, None]
    ri, ui, ci, hi = r[:, i], u[:, i], c[:, i], hp[:, i]
    g = dout[:, i] + dh
    eg = e + U * np.abs(g)
    d_u, d_c = g * (hi - ci), g * (1 - ui)
    d_ac = d_c * (1 - ci * ci)
    e_ac = (1 - ui) * np.abs(1 - ci * ci) * eg + 4 * U * np.abs(d_ac) + 2 * U * np.abs(d_c) + 8 * ETA
    e_du = np.abs(hi - ci) * eg + 3 * U * np.abs(d_u)
    d_rh = d_ac @ whc.T
    e_rh = 67 * U * (np.abs(d_ac) @ awc.T) + e_ac @ awc.T
    dhp = g * ui + d_rh * ri
    e_hp = ui * eg + U * np.abs(g * ui) + ri * e_rh + U * np.abs(dhp)
    d_ar = d_rh * hi * ri * (1 - ri)
    e_ar = np.abs(hi) * ri * (1 - ri) * e_rh + 4 * U * np.abs(d_ar) + 8 * ETA
    d_au = d_u * ui * (1 - ui)
    e_au = ui * (1 - ui) * e_du + 4 * U * np.abs(d_au) + 8 * ETA
    d_ag, e_ag = np.concatenate([d_ar, d_au], 1), np.concatenate([e_ar, e_au], 1)
    new = dhp + d_ag @ whg.T
    e_new = e_hp + 131 * U * (np.abs(d_ag) @ awg.T) + e_ag @ awg.T + U * np.abs(new)
    dag[:, i], dac[:, i] = np.where(live, d_ag, 0.0), np.where(live, d_ac, 0.0)
    b_dag[:, i], b_dac[:, i] = np.where(live, e_ag, 0.0), np.where(live, e_ac, 0.0)
    dh, e = np.where(live, new, dh), np.where(live, e_new, e)
  return dag, dac, b_dag, b_dac


def vloss_inputs(b, t, j, seed):
  """D [b,t,j] with exact zeros and equal neighbours D[t + 1] == D[t] planted (a twentieth each); vmask of 1 and 10."""
  d = np.stack([np.float32(CLIP_SCALES[i % 3]) * np.random.default_rng(seed * 1000 + i).standard_normal((t, j), dtype=np.float32) for i in range(b)])
  rng = np.random.default_rng(seed)
  d[rng.uniform(size=d.shape) < 0.05] = 0.0
  if t > 1:
    same = rng.uniform(size=(b, t - 1, j)) < 0.05
    d[:, 1:][same] = d[:, :-1][same]
  vm = np.where(rng.uniform(size=j) < 0.1, 10.0, 1.0)
  return d.astype(np.float64), vm


def vloss_ref(d, vm, seq):
  """(loss, bound(loss), gD, bound(gD)) of vp_bfm_vertex_loss, clip by clip."""
  b, t, j = d.shape
  gd, bg = np.zeros_like(d), np.zeros_like(d)
  frame = video = 0.0
  for i in range(b):
    n = int(seq[i])
    fm = (np.arange(t) < n).astype(np.float64)[:, None]
    frame += float((np.abs(d[i]) * fm * vm).sum())
    g = np.sign(d[i]) * fm * vm / b
    mag = np.abs(g)
    if t > 1:
      w = d[i, 1:] - d[i, :-1]
      pm = (np.arange(t - 1) < n - 1).astype(np.float64)[:, None]
      video += float((np.abs(w) * pm * vm).sum())
      s = np.sign(w) * pm * vm / b
      g[1:] += s
      g[:-1] -= s
      mag[1:] += np.abs(s)
      mag[:-1] += np.abs(s)
    gd[i], bg[i] = g, 4 * U * mag
  loss = (frame + video) / b
  nblk = -(-b * j // 256)
  return loss, (U * frame + 2 * U * video) / b + (2 * t + 20 + nblk / 256.0) * V * loss, gd, bg


def two_term_bound(a, b, round_a=True, round_b=True):
  """a + b where a and / or b are themselves rounded products and the compiler may contract one of them into the sum: u |a| and / or
  u |b| for the products, u |a + b| for the sum (a contraction only removes one of the terms)."""
  return (U * np.abs(a) if round_a else 0.0) + (U * np.abs(b) if round_b else 0.0) + U * np.abs(a + b)


def f64_sum_bound(n, blocks, total):
  """(n / blocks + 10) v total: a float64 sum of n terms of magnitude sum `total` whose longest chain is at most n / blocks additions
  (a thread of one of `blocks` blocks; vp_sum_f64 is one block: n / 256), then an 8-level tree and the final sum / scale"""
  return (n / blocks + 10) * V * total


def adam_ref(p, g, m, v, lr, sumsq, clip, b1, b2, eps):
  """{name: (reference, bound)} of one vp_adam_tf_clipped call from float32 state (exact): tf.clip_by_global_norm + AdamOptimizer."""
  scale = clip / max(math.sqrt(sumsq), clip)
  gc = g * scale
  e_g = 2 * U * np.abs(gc) if scale != 1.0 else np.zeros_like(gc)
  m1 = b1 * m + (1 - b1) * gc
  e_m = (1 - b1) * e_g + U * (np.abs(b1 * m) + np.abs((1 - b1) * gc)) + U * np.abs(m1)
  v1 = b2 * v + (1 - b2) * gc * gc
  e_v = 2 * (1 - b2) * np.abs(gc) * e_g + U * (np.abs(b2 * v) + 2 * (1 - b2) * gc * gc) + U * v1
  sq = np.sqrt(v1)
  den = sq + eps
  q = lr * m1 / den
  with np.errstate(divide="ignore", invalid="ignore"):
    e_sq = np.where(v1 > 0, e_v / (2 * sq), 0.0)
  p1 = p - q
  e_p = U * np.abs(p1) + np.abs(q) * (5 * U + (e_sq + 2 * U * sq) / den) + lr * e_m / den
  return {"g": (gc, e_g), "m": (m1, e_m), "v": (v1, e_v), "p": (p1, e_p)}


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests: the references against torch.autograd in float64 (tie-free inputs, 1e-12 relative), the bounds against a float32
# restatement of the kernel's own order of operations
# ---------------------------------------------------------------------------------------------------------------------------------
def t64(a, grad=False):
  return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def rel_max(a, b):
  return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_launch_shape_tables():
  for (p, c), (ql, nch, by) in BN_CASES.items():
    assert bn_shape(p, c) == (ql, nch) and (c // 4 + (1 << ql) - 1) >> ql == by, (p, c, bn_shape(p, c))
  per = -(-257 // 8)
  assert 257 - 7 * per == 26 < per                                    # (257, 768): a ragged last chunk
  assert bn_shape(31, 32)[1] == 1 and 31 < 32                          # fewer rows than the 32 row lanes of one block
  for k, want in DW_CASES.items():
    assert dw_wgrad_shape(*k[:3]) == want, (k, dw_wgrad_shape(*k[:3]))
  assert [tblk(p * c // 4) for p, c in ACT_SIZES] == [1, 4, 4096] and ACT_SIZES[2][0] * ACT_SIZES[2][1] // 4 > 4096 * 256
  L = _lib.lib()
  for n in FLAT_SIZES:
    assert L.vp_sumsq_partials(n) == tblk(n, 1024)
  assert tblk(FLAT_SIZES[3], 1024) == 1024 and FLAT_SIZES[3] > 3 * 1024 * 256      # the stride loop of the reductions runs 3 to 4 times
  assert tblk(FLAT_SIZES[4] // 4) == 4096 and FLAT_SIZES[4] // 4 > 4096 * 256       # and adam_clip_kernel's (tblk(n / 4)) a second time
  assert tblk(POOL_ABOVE_CAP[0] * POOL_ABOVE_CAP[1] * POOL_ABOVE_CAP[2] * POOL_ABOVE_CAP[3] // 4) == 4096
  assert POOL_ABOVE_CAP[0] * POOL_ABOVE_CAP[1] * POOL_ABOVE_CAP[2] * POOL_ABOVE_CAP[3] // 4 > 4096 * 256
  b, h, w = STEM_CASES[-1]
  assert b * h * ((w + 1) // 2) * 48 > 4096 * 256 and all(bb * hh * ((ww + 1) // 2) * 48 <= 4096 * 256 for bb, hh, ww in STEM_CASES[:-1])
  for b, _, j, _ in VLOSS_CASES:
    assert L.vp_vertex_loss_partials(b, j) == -(-b * j // 256)
  assert all((b * 107127) % 256 for b in (4, 8)) and 107127 % 256


@pytest.mark.parametrize("act", [ACT_NONE, ACT_LRELU, ACT_RELU, ACT_RELU6])
def test_bn_bwd_reference_against_autograd(act):
  """The test-made statistics are those of x itself here (rounded to float32 they would not be a batch-norm: float64 throughout)."""
  rng = np.random.default_rng(act)
  p, c = 60, 8
  x, da = rng.normal(1.0, 1.5, (p, c)), rng.normal(size=(p, c))
  beta = np.linspace(-2.0, 8.0, c)
  mean, var = x.mean(0), x.var(0)
  rstd = 1.0 / np.sqrt(var + BN_EPS)
  shift = beta - mean * rstd
  y = rstd * x + shift
  dz = da * act_deriv(act, y)
  if act == ACT_LRELU:
    dz = da * np.where(y >= 0, 1.0, 0.2)
  xhat = (x - mean) * rstd
  dx = rstd * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))
  xt, bt_ = t64(x.T.reshape(1, c, p, 1), True), t64(beta, True)
  z = bt._bn(xt, bt_, "s", bt.Stats())
  a = {ACT_NONE: lambda v: v, ACT_LRELU: bt._lrelu, ACT_RELU: torch.relu, ACT_RELU6: torch.nn.functional.relu6}[act](z)
  a.backward(t64(da.T.reshape(1, c, p, 1)))
  assert rel_max(dx, xt.grad.numpy().reshape(c, p).T) < 1e-12
  assert rel_max(dz.sum(0), bt_.grad.numpy()) < 1e-12
  # the function under test, from the same (float64) statistics, act 0: identical formula
  got, _ = bn_bwd_ref(x, dz, mean, rstd, shift, 0, 1)
  assert rel_max(got["dx"][0], dx) < 1e-12 and rel_max(got["dbeta"][0], dz.sum(0)) < 1e-12


def test_dw_wgrad_reference_against_autograd():
  rng = np.random.default_rng(1)
  b, h, w, c = 2, 12, 5, 6
  x, dy, wt = rng.normal(size=(b, h, w, c)), rng.normal(size=(b, h, w, c)), t64(rng.normal(size=(7, 3, c, 1)), True)
  bt._dw(t64(x).permute(0, 3, 1, 2), wt).backward(t64(dy).permute(0, 3, 1, 2))
  ref, bound = dw_wgrad_ref(x, dy, dw_wgrad_shape(b, h, w))
  assert rel_max(ref, wt.grad.numpy().reshape(21, c)) < 1e-12 and (bound > 0).all()


@pytest.mark.parametrize("k,s,h,w", [((2, 2), (1, 2), 7, 5), ((5, 3), (5, 3), 10, 3), ((2, 2), (1, 2), 1, 1), ((5, 3), (5, 3), 7, 5)])
def test_maxpool_bwd_reference_against_autograd(k, s, h, w):
  rng = np.random.default_rng(h + w)
  x = rng.normal(size=(2, h, w, 4))
  xt = t64(x, True)
  y = bt._pool(xt.permute(0, 3, 1, 2), k, s)
  dy = rng.normal(size=tuple(y.shape))
  y.backward(t64(dy))
  ref, _ = maxpool_bwd_ref(x, dy.transpose(0, 2, 3, 1), k, s)
  assert rel_max(ref, xt.grad.numpy()) < 1e-12
  assert tuple(y.shape[2:]) == pool_geometry(h, w, k, s)[2:]


def test_maxpool_bwd_reference_takes_the_first_maximum():
  """2 x 3 by hand, (2,2) / (1,2) SAME (one row and one column of padding at the far edges): windows (oh, ow) cover rows oh..oh+1,
  columns 2 ow..2 ow + 1.  Row-major first maximum of each window:
    x = 1 1 5     (0,0): 1 1 / 1 1 -> (0,0)    (0,1): 5 / 5 -> (0,2)
        1 1 5     (1,0): 1 1       -> (1,0)    (1,1): 5     -> (1,2)"""
  x = np.array([[1, 1, 5], [1, 1, 5]], np.float64).reshape(1, 2, 3, 1)
  dy = np.array([[10, 20], [30, 40]], np.float64).reshape(1, 2, 2, 1)
  dx, bound = maxpool_bwd_ref(x, dy, (2, 2), (1, 2))
  assert (dx.reshape(2, 3) == np.array([[10, 0, 20], [30, 0, 40]])).all()
  assert (bound.reshape(2, 3)[0] == 0).all() and (bound.reshape(2, 3)[1, ::2] > 0).all()      # row 1 sits in two windows


def gru_as_oracle_inputs(xg, xc, whg, whc):
  """The (x, wg, bg, wc, bc) of gru_seq whose gate / candidate pre-activations are xg + h whg and xc + (r h) whc: x = [xg | xc] through
  identity blocks (products with 1 and 0 are exact)."""
  hd = xc.shape[-1]
  x = np.concatenate([xg, xc], -1)
  wg, wc = np.zeros((4 * hd, 2 * hd)), np.zeros((4 * hd, hd))
  wg[:2 * hd], wg[3 * hd:] = np.eye(2 * hd), whg
  wc[2 * hd:3 * hd], wc[3 * hd:] = np.eye(hd), whc
  return x, wg, np.zeros(2 * hd), wc, np.zeros(hd)


def test_gru_references_against_autograd():
  b, t, hd, seq = 3, 6, 8, [6, 3, 0]
  xg, xc, whg, whc = gru_inputs(b, t, 4, hd, 0.4)
  out, r, u, c, hp = gru_fwd_ref(xg, xc, whg, whc, seq)
  x, wg, bg, wc, bc = gru_as_oracle_inputs(xg, xc, whg, whc)
  assert rel_max(out, ar.gru_seq(x, seq, wg, bg, wc, bc)) < 1e-12
  xt = t64(x, True)
  dout = np.random.default_rng(0).normal(size=out.shape)
  o = bt.gru_seq(xt, seq, t64(wg), t64(bg), t64(wc), t64(bc))
  assert rel_max(out, o.detach().numpy()) < 1e-12
  o.backward(t64(dout))
  dag, dac, b_dag, b_dac = gru_bwd_ref(dout, whg, whc, seq, r, u, c, hp)
  assert rel_max(dag, xt.grad.numpy()[..., :2 * hd]) < 1e-12 and rel_max(dac, xt.grad.numpy()[..., 2 * hd:]) < 1e-12
  assert (dag[1, 3:] == 0).all() and (dac[2] == 0).all() and (b_dag >= 0).all()
  # one step of gru_step_ref from the saved h_prev is the forward's step
  st, _ = gru_step_ref(xg[:, 2], xc[:, 2], whg, whc, hp[:, 2])
  assert rel_max(st["hn"][0][0], out[0, 2]) < 1e-12 and rel_max(st["r"][0][:2], r[:2, 2]) < 1e-12


def test_vertex_loss_reference_against_autograd():
  """oracle vertex_loss takes the decoder output: with exBase = [I_64; 0] D[..., :64] = expression(true) - out, so d loss / d out = -gD."""
  b, t, j, seq = 3, 5, 66, [5, 1, 3]
  rng = np.random.default_rng(2)
  coeff, out = rng.normal(size=(b, t, 144)), rng.normal(size=(b, t, 64))
  ex = np.zeros((j, 64))
  ex[:64] = np.eye(64)
  vm = np.where(rng.uniform(size=j) < 0.3, 10.0, 1.0)
  ot = t64(out, True)
  loss = bt.vertex_loss(ot, t64(coeff), seq, t64(np.zeros((j, 80))), t64(ex), t64(np.zeros(j)), t64(vm))
  loss.backward()
  d = np.zeros((b, t, j))
  d[..., :64] = coeff[..., 80:144] - out
  ref, bl, gd, bg = vloss_ref(d, vm, seq)
  assert abs(ref - float(loss.detach())) <= 1e-12 * abs(ref) and rel_max(-gd[..., :64], ot.grad.numpy()) < 1e-12
  assert (gd[..., 64:] == 0).all() and (gd[1, 1:] == 0).all()


def test_simple_bounds_hold_a_float32_restatement():
  """The max-pool, two-term and float64-sum bounds, as test_bounds_hold_a_float32_restatement does for the others."""
  f = np.float32
  # max-pool backward: the same scatter in float32, windows in the kernel's order (oh, then ow); ties and overlapping windows
  x = np.clip(np.round(rows(2 * 7 * 5, 8, 3, 2.0, 3.0).reshape(2, 7, 5, 8) * 2) / 2, 0.0, 6.0)
  for k, s in POOLS:
    _, _, ho, wo = pool_geometry(7, 5, k, s)
    dy = rows(2 * ho * wo, 8, 4).reshape(2, ho, wo, 8)
    ref, bound = maxpool_bwd_ref(x, dy, k, s)
    got, _ = maxpool_bwd_ref(f(x), f(dy), k, s)
    assert got.dtype == np.float32 and inside(got, ref, bound)
    moved = np.roll(got, 1, axis=2)                                    # the gradient handed to the neighbour of the first maximum
    assert not inside(moved, ref, bound)
    assert (bound > 0).any() == (s[0] < k[0])
  # act(.) * mask + add and decay * moving + factor * batch: both products rounded, one fused into the sum, the other fused
  a, m, r, d = [rows(500, 4, 30 + i) for i in range(4)]
  fused = lambda p, q, c: (p * q + c).astype(f)                        # p * q exact in float64 (float32 factors)
  for got in (f(a) * f(m) + f(r), fused(a, m, r)):
    assert inside(got, a * m + r, two_term_bound(a * m, r, True, False))
  for got in (f(a) * f(m) + f(r) * f(d), fused(a, m, (f(r) * f(d)).astype(np.float64)), fused(r, d, (f(a) * f(m)).astype(np.float64))):
    assert inside(got, a * m + r * d, two_term_bound(a * m, r * d))
  assert not inside((a * m + r * d) * (1 + 4e-7) + 1e-7, a * m + r * d, two_term_bound(a * m, r * d))
  # sumsq_kernel's order in float64: grid-stride chains, the 8-level tree of a block, the partials in order
  n = 700001
  x = rows(n, 1, 40)[:, 0]
  nb = tblk(n, 1024)
  sq = np.zeros(-(-n // (nb * 256)) * nb * 256)
  sq[:n] = x * x
  acc = np.zeros(nb * 256)
  for trip in sq.reshape(-1, nb * 256):
    acc = acc + trip
  part = acc.reshape(nb, 256)
  while part.shape[1] > 1:
    part = part[:, :part.shape[1] // 2] + part[:, part.shape[1] // 2:]
  total = 0.0
  for v in part[:, 0]:
    total += v
  ss = math.fsum(x * x)
  assert abs(total - ss) <= f64_sum_bound(n, nb, ss) and abs(total - sq[5] - ss) > f64_sum_bound(n, nb, ss)


def chain32(terms):
  """float32 sum of the rows of `terms` in order (one chain)."""
  s = np.zeros(terms.shape[1:], np.float32)
  for row in terms.astype(np.float32):
    s = s + row
  return s


def inside(got, ref, bound):
  return bool((np.abs(np.asarray(got, np.float64) - ref) <= bound).all())


def test_bounds_hold_a_float32_restatement():
  """Each bound function on one small case: the kernel's order of operations restated in float32 numpy lies inside it, and an error
  of 1e-4 relative (or a dropped row) does not."""
  f = np.float32
  # batch-norm forward: float64 sums of float32 values, E[x^2] - m^2, rounded once
  x, beta = bn_fwd_inputs(1600, 32, 3)
  ref = bn_fwd_ref(x, beta, 6)
  m = x.sum(0) / 1600
  v = np.maximum((x * x).sum(0) / 1600 - m * m, 0)
  r = f(1.0 / np.sqrt(v + float(f(BN_EPS))))
  for name, got in (("mean", f(m)), ("var", f(v)), ("rstd", r), ("shift", f(beta - m * r.astype(np.float64)))):
    assert inside(got, *ref[name]), name
  assert not inside(f(m) * f(1.0001), *ref["mean"]) and not inside(r * f(1.0001), ref["rstd"][0][:1], ref["rstd"][1][:1])
  # batch-norm backward, ReLU6
  x, da, mean, rstd, shift = bn_bwd_inputs(300, 8, 5)
  ref, y = bn_bwd_ref(x, da, mean, rstd, shift, ACT_RELU6, 1)
  x3, m3, r3 = f(x), f(mean), f(rstd)
  dz = f(da) * f(act_deriv(ACT_RELU6, y))
  xh = (x3 - m3) * r3
  c1, c2 = f(dz.astype(np.float64).sum(0) / 300), f((dz.astype(np.float64) * xh).sum(0) / 300)
  dx = r3 * (dz - c1 - xh * c2)
  assert inside(dx, *ref["dx"]) and inside(c1, *ref["c1"]) and inside(c2, *ref["c2"]) and inside(f(dz.astype(np.float64).sum(0)), *ref["dbeta"])
  assert not inside(dx * f(1.0001), *ref["dx"])
  drop = f((dz.astype(np.float64) * xh)[:-1].sum(0) / 300)
  assert not inside(drop, *ref["c2"])
  # depthwise weight gradient: one float32 chain over all rows per (tap, channel)
  b, h, w, c = 2, 9, 5, 8
  xx, dy = rows(b * h * w, c, 7).reshape(b, h, w, c), rows(b * h * w, c, 8).reshape(b, h, w, c)
  ref, bound = dw_wgrad_ref(xx, dy, dw_wgrad_shape(b, h, w))
  xp = np.pad(xx, ((0, 0), (3, 3), (1, 1), (0, 0)))
  got = np.stack([chain32((xp[:, kh:kh + h, kw:kw + w, :] * dy).reshape(-1, c)) for kh in range(7) for kw in range(3)])
  assert inside(got, ref, bound) and not inside(got * f(1.0001), ref, bound)
  # column sums
  xx = rows(96, 65, 9)
  assert inside(chain32(xx), xx.sum(0), 97 * U * np.abs(xx).sum(0))
  # GRU: one step and the backward through time, float32 throughout
  bb, t, seq = 2, 5, [5, 3]
  xg, xc, whg, whc = gru_inputs(bb, t, 6)
  out, r, u, c, hp = [f32(a) for a in gru_fwd_ref(xg, xc, whg, whc, seq)]
  st, _ = gru_step_ref(xg[:, 2], xc[:, 2], whg, whc, hp[:, 2])
  h3 = f(hp[:, 2])
  g3 = f(1) / (f(1) + np.exp(-(f(xg[:, 2]) + h3 @ f(whg))))
  c3 = np.tanh(f(xc[:, 2]) + (g3[:, :256] * h3) @ f(whc))
  hn = g3[:, 256:] * h3 + (f(1) - g3[:, 256:]) * c3
  assert inside(g3[:, :256], *st["r"]) and inside(g3[:, 256:], *st["u"]) and inside(c3, *st["c"]) and inside(hn, *st["hn"])
  assert not inside(hn * f(1.0001), *st["hn"])
  dout = rows(bb * t, 256, 12).reshape(bb, t, 256)
  dag, dac, b_dag, b_dac = gru_bwd_ref(dout, whg, whc, seq, r, u, c, hp)
  dh = np.zeros((bb, 256), f)
  for i in range(t - 1, -1, -1):
    live = (i < np.asarray(seq))[:, None]
    ri, ui, ci, hi = f(r[:, i]), f(u[:, i]), f(c[:, i]), f(hp[:, i])
    g = f(dout[:, i]) + dh
    d_ac = g * (f(1) - ui) * (f(1) - ci * ci)
    d_rh = d_ac @ f(whc).T
    d_ag = np.concatenate([d_rh * hi * ri * (f(1) - ri), g * (hi - ci) * ui * (f(1) - ui)], 1)
    new = g * ui + d_rh * ri + d_ag @ f(whg).T
    if i < 3:
      assert inside(d_ag[:1], dag[:1, i], b_dag[:1, i]) and inside(d_ac, dac[:, i] * live, b_dac[:, i] + (1 - live) * 1e30)
      assert inside(d_ag[1], dag[1, i], b_dag[1, i])
    dh = np.where(live, new, dh)
  assert not inside(dag[:, 0] * 1.0001, dag[:, 0], b_dag[:, 0])
  # vertex loss: float32 terms, float64 sum
  d, vm = vloss_inputs(2, 4, 360, 1)
  loss, bl, gd, bg = vloss_ref(d, vm, [4, 3])
  assert (d == 0).mean() > 0.03 and (d[:, 1:] == d[:, :-1]).mean() > 0.03 and set(np.unique(vm)) == {1.0, 10.0}
  inv, acc, got = f(1) / f(2), 0.0, np.zeros(d.shape, f)
  for i, n in enumerate([4, 3]):
    for k in range(4):
      if k < n:
        acc += float((np.abs(f(d[i, k])) * f(vm)).astype(np.float64).sum())
        got[i, k] += np.sign(f(d[i, k])) * f(vm) * inv
      if k + 1 < 4 and k < n - 1:
        w = f(d[i, k + 1]) - f(d[i, k])
        acc += float((np.abs(w) * f(vm)).astype(np.float64).sum())
        got[i, k] -= np.sign(w) * f(vm) * inv
        got[i, k + 1] += np.sign(w) * f(vm) * inv
  assert abs(acc / 2 - loss) <= bl and inside(got, gd, bg) and abs(acc / 2 * (1 + 1e-6) - loss) > bl
  # Adam with a clip above and below the norm, from non-zero slots
  n = 1020
  p, g, m, v = rows(n, 1, 20)[:, 0], rows(n, 1, 21)[:, 0], f32(rows(n, 1, 22)[:, 0] * 0.1), f32(np.abs(rows(n, 1, 23)[:, 0]) * 0.01)
  b1, b2, eps, lr = float(f(0.9)), float(f(0.999)), float(f(1e-8)), float(f(3e-4))
  assert float(f(1) - f(0.9)) == 1 - b1 and float(f(1) - f(0.999)) == 1 - b2          # exact in float32, as the bound assumes
  for clip in (1.0, 1e6):
    ss = float((g * g).sum())
    ref = adam_ref(p, g, m, v, lr, ss, clip, b1, b2, eps)
    sc = f(clip / max(math.sqrt(ss), clip))
    gg = f(g) * sc
    m1 = f(b1) * f(m) + (f(1) - f(b1)) * gg
    v1 = f(b2) * f(v) + (f(1) - f(b2)) * gg * gg
    p1 = f(p) - f(lr) * m1 / (np.sqrt(v1) + f(eps))
    for name, got in (("g", gg), ("m", m1), ("v", v1), ("p", p1)):
      assert inside(got, *ref[name]), (clip, name)
    assert not inside(p1 + f(lr) * f(1e-3), *ref["p"])
  z = np.zeros(4)
  ref = adam_ref(p[:4], z, z, z, lr, 0.0, 1.0, b1, b2, eps)
  assert (ref["p"][0] == p[:4]).all() and (ref["p"][1] == U * np.abs(p[:4])).all() and np.isfinite(ref["p"][1]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------------------
def dev(a):
  return gu.dev_f32(a)


def nan_out(shape, row=64):
  return guarded(tuple(shape), row)


def in_place(values, row=64):
  return guarded(tuple(np.shape(values)), row, fill=np.asarray(values))


def host(t):
  torch.cuda.synchronize()
  return t.cpu().numpy().astype(np.float64)


def chk(kernel, name, got, ref, bound):
  """Per-element bound (bit-equal where the bound is 0); prints `RATIO kernel worst` first, names the worst elements on failure."""
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  assert np.isfinite(got).all(), "%s: %d elements not written / not finite, first at %s" % (name, int((~np.isfinite(got)).sum()), np.argwhere(~np.isfinite(got))[0])
  err = np.abs(got - ref)
  with np.errstate(divide="ignore", invalid="ignore"):
    ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
  worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
  print("\nRATIO %s %.4f   (%s, at %s)" % (kernel, ratio[worst] if ratio.size else 0.0, name, worst))
  bad = np.argwhere(ratio > 1)
  assert len(bad) == 0, "%s: %d of %d elements outside the bound, e.g. %s: got %r want %r bound %.3e" % (
      name, len(bad), ratio.size, bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])], bound[tuple(bad[0])])


def exact(kernel, name, got, want32):
  chk(kernel, name, got, np.asarray(want32, np.float32).astype(np.float64), 0.0)


def workspace(nbytes):
  return torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device="cuda")


def f64_out(n):
  """(whole, view): n float64 NaN between two bands of 8 sentinels."""
  whole = torch.full((n + 16,), SENTINEL, dtype=torch.float64, device="cuda")
  whole[8:8 + n] = float("nan")
  return whole, whole[8:8 + n]


def assert_f64_guards(whole):
  assert bool((whole[:8] == SENTINEL).all()) and bool((whole[-8:] == SENTINEL).all()), "guard band written"


@gpu
@pytest.mark.parametrize("p,c", list(BN_CASES))
def test_bn_train_fwd(p, c):
  L = _lib.lib()
  assert bn_shape(p, c) == BN_CASES[(p, c)][:2]
  nch = bn_shape(p, c)[1]
  x, beta = bn_fwd_inputs(p, c, seed=p + c)
  ref = bn_fwd_ref(x, beta, nch)
  if p == 1:
    assert (ref["var"][0] == 0).all() and np.allclose(ref["rstd"][0], 1 / math.sqrt(float(np.float32(BN_EPS))), rtol=1e-15)
  if c >= 32:
    assert ref["var"][0][1] == 0 and abs(ref["mean"][0][2] - 100) < 0.01 and (p < 3 or 0.003 < math.sqrt(ref["var"][0][2]) < 0.03)
  assert L.vp_bn_train_workspace_bytes(p, c) == nch * 2 * c * 8 + 2 * c * 4 + 256
  ws, xd, bd = workspace(L.vp_bn_train_workspace_bytes(p, c)), dev(x), dev(beta)
  outs = {k: nan_out((c,)) for k in ("mean", "var", "rstd", "scale", "shift")}
  o = lambda k: gu.ptr(outs[k][1])
  _lib.check(L.vp_bn_train_fwd(gu.ptr(xd), p, c, gu.ptr(bd), BN_EPS, o("mean"), o("var"), o("rstd"), o("scale"), o("shift"), gu.ptr(ws), gu.stream()), "vp_bn_train_fwd")
  got = {k: host(v[1]) for k, v in outs.items()}
  for k, (whole, _, g) in outs.items():
    assert_guards(whole, g)
  for k in ("mean", "var", "rstd", "shift"):
    chk("bn_train_fwd", "%s (%d, %d)" % (k, p, c), got[k], *ref[k])
  assert (got["scale"] == got["rstd"]).all() and (got["var"] >= 0).all()


def run_bn_bwd(x, da, mean, rstd, shift, act, alias=False):
  """(got dict, float64): dx, dbeta and the c1 / c2 the launcher leaves in its workspace."""
  L = _lib.lib()
  p, c = x.shape
  nch = bn_shape(p, c)[1]
  ws = workspace(L.vp_bn_train_workspace_bytes(p, c))
  xd, md, rd, sd = dev(x), dev(mean), dev(rstd), dev(shift)
  if alias:
    wdx, dxv, gdx = in_place(da, c)
    dad = dxv
  else:
    wdx, dxv, gdx = nan_out((p, c), c)
    dad = dev(da)
  wdb, dbv, gdb = nan_out((c,))
  if act:
    rc = L.vp_bn_act_train_bwd(gu.ptr(xd), gu.ptr(dad), p, c, gu.ptr(md), gu.ptr(rd), gu.ptr(sd), act, gu.ptr(dxv), gu.ptr(dbv), gu.ptr(ws), gu.stream())
  else:
    rc = L.vp_bn_train_bwd(gu.ptr(xd), gu.ptr(dad), p, c, gu.ptr(md), gu.ptr(rd), gu.ptr(dxv), gu.ptr(dbv), gu.ptr(ws), gu.stream())
  _lib.check(rc, "vp_bn_act_train_bwd")
  torch.cuda.synchronize()
  assert_guards(wdx, gdx)
  assert_guards(wdb, gdb)
  # c1, c2 are not outputs: the launcher keeps them in its workspace behind the float64 partials [nchunk][2][c] (vp_bn_act_train_bwd in
  # csrc/bfm_train.hip: c1 = workspace + nchunk * 2 * c doubles, c2 = c1 + c).  The size ties this test to that layout: if the size
  # changes, re-read the launcher before trusting the two slices below.
  assert L.vp_bn_train_workspace_bytes(p, c) == nch * 2 * c * 8 + 2 * c * 4 + 256
  cc = ws[nch * 2 * c * 8:nch * 2 * c * 8 + 2 * c * 4].view(torch.float32)
  return {"dx": host(dxv), "dbeta": host(dbv), "c1": host(cc[:c]), "c2": host(cc[c:])}


@gpu
@pytest.mark.parametrize("p,c,act", [(p, c, a) for p, c in BN_CASES for a in (ACT_NONE, ACT_RELU, ACT_RELU6)] + [(1600, 32, ACT_LRELU)])
def test_bn_train_bwd(p, c, act):
  assert bn_shape(p, c) == BN_CASES[(p, c)][:2]
  x, da, mean, rstd, shift = bn_bwd_inputs(p, c, seed=p + c + act)
  ref, y = bn_bwd_ref(x, da, mean, rstd, shift, act, bn_shape(p, c)[1])
  if act == ACT_RELU6 and p * c >= 56:
    assert_regimes6(y)
  got = run_bn_bwd(x, da, mean, rstd, shift, act)
  for k in ("c1", "c2", "dbeta", "dx"):
    chk("bn_train_bwd", "%s (%d, %d) act %d" % (k, p, c, act), got[k], *ref[k])


@gpu
def test_bn_train_bwd_in_place():
  """dx may alias da (include/vp_hip.h)."""
  p, c, act = 1600, 32, ACT_RELU6
  x, da, mean, rstd, shift = bn_bwd_inputs(p, c, seed=77)
  ref, y = bn_bwd_ref(x, da, mean, rstd, shift, act, bn_shape(p, c)[1])
  assert_regimes6(y)
  got = run_bn_bwd(x, da, mean, rstd, shift, act, alias=True)
  for k in ("c1", "c2", "dbeta", "dx"):
    chk("bn_train_bwd", "%s in place" % k, got[k], *ref[k])


@gpu
@pytest.mark.parametrize("act", [ACT_RELU, ACT_RELU6])
def test_bn_train_bwd_at_the_kinks(act):
  """rstd = 1, shift = 0: y == x.  x exactly 0, exactly 6 and their float32 neighbours, with |da| = 2 there: the derivative is 0 at 0 and
  at 6 (act_d), 1 just inside, and a wrong decision moves dx by rstd |da| = 2."""
  p, c = 64, 8
  f = np.float32
  x = rows(p, c, 5, 3.0, 3.0)
  plant = [f(0), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1)), f(6), np.nextafter(f(6), f(7)), np.nextafter(f(6), f(0))]
  da = rows(p, c, 6)
  for i, v in enumerate(plant):
    x[5 + i, i % c], da[5 + i, i % c] = float(v), 2.0
  mean, rstd, shift = np.full(c, 0.5), np.ones(c), np.zeros(c)
  want = {ACT_RELU: [0, 1, 0, 1, 1, 1], ACT_RELU6: [0, 1, 0, 0, 0, 1]}[act]
  assert [float(act_deriv(act, np.float64(v))) for v in plant] == want
  ref, y = bn_bwd_ref(x, da, mean, rstd, shift, act, 1)
  assert (y == x).all()
  got = run_bn_bwd(x, da, mean, rstd, shift, act)
  for k in ("c1", "c2", "dbeta", "dx"):
    chk("bn_train_bwd", "%s at the kinks, act %d" % (k, act), got[k], *ref[k])


def affine_cases():
  out = []
  for si, (p, c) in enumerate(ACT_SIZES):
    k = 0
    for sc in (1, 0):
      for mk in (0, 1):
        for ad in (0, 1):
          acts = (ACT_NONE, ACT_LRELU, ACT_RELU, ACT_RELU6)
          for act in (acts if si < 2 else acts[k % 4:k % 4 + 1]):       # the 4 M element size: every pointer combination, act walking
            out.append((p, c, sc, mk, ad, act))
          k += 1
  return out


@gpu
@pytest.mark.parametrize("p,c,sc,mk,ad,act", affine_cases())
def test_affine_act_fwd(p, c, sc, mk, ad, act):
  L = _lib.lib()
  rng = np.random.default_rng(p + c)
  x = rows(p, c, 3 * p + act, 2.5, rng.normal(0, 1.0, c).astype(np.float32))
  scale, shift = f32(rng.uniform(0.5, 1.5, c)), f32(rng.uniform(-3.0, 9.0, c))
  mask = f32((rng.uniform(size=(p, c)) < 0.75) / 0.75) if mk else None
  add = rows(p, c, 7 * p + 1) if ad else None
  a32 = act_fwd32(act, fma32(scale, x, shift) if sc else x.astype(np.float32))
  whole, yv, g = nan_out((p, c), c)
  xd, sd, hd, md, rd = dev(x), dev(scale) if sc else None, dev(shift) if sc else None, dev(mask), dev(add)
  if ad:
    rc = L.vp_affine_act_add_fwd(gu.ptr(xd), gu.ptr(sd), gu.ptr(hd), gu.ptr(md), gu.ptr(rd), p, c, act, gu.ptr(yv), gu.stream())
  else:
    rc = L.vp_affine_act_fwd(gu.ptr(xd), gu.ptr(sd), gu.ptr(hd), gu.ptr(md), p, c, act, gu.ptr(yv), gu.stream())
  _lib.check(rc, "vp_affine_act_fwd")
  got = host(yv)
  assert_guards(whole, g)
  name = "affine (%d, %d) scale %d mask %d add %d act %d" % (p, c, sc, mk, ad, act)
  if not mk and not ad:
    if act == ACT_RELU6 and sc:
      assert_regimes6(fma32(scale, x, shift))
    exact("affine_act", name, got, a32)
    return
  t = a32.astype(np.float64) * (mask if mk else 1.0)
  ref = t + (add if ad else 0.0)
  chk("affine_act", name, got, ref, two_term_bound(t, add, bool(mk), False) if ad else U * np.abs(t))


@gpu
@pytest.mark.parametrize("p,c", ACT_SIZES)
@pytest.mark.parametrize("act,mk", [(ACT_NONE, 1), (ACT_LRELU, 0), (ACT_LRELU, 1), (ACT_RELU, 0), (ACT_RELU, 1), (ACT_RELU6, 0), (ACT_RELU6, 1)])
def test_act_bwd(p, c, act, mk):
  L = _lib.lib()
  n = p * c
  rng = np.random.default_rng(n + act)
  ya = act_fwd32(act, rows(n, 1, n + 1, 4.0, 3.0)[:, 0])
  ya[:8] = np.array([0, 6, np.nextafter(np.float32(6), np.float32(0)), np.nextafter(np.float32(0), np.float32(1)), 0, 6, 1, 7], np.float32)
  dy = rows(n, 1, n + 2)[:, 0].astype(np.float32)
  d = dy.copy()
  mask = None
  if mk:
    mask = ((rng.uniform(size=n) < 0.75) / 0.75).astype(np.float32)
    d = d * mask
  d = d * act_deriv(act, ya.astype(np.float64)).astype(np.float32)
  whole, dxv, g = nan_out((n,))
  dyd, yd, md = dev(dy), dev(ya), dev(mask)
  _lib.check(L.vp_act_bwd(gu.ptr(dyd), gu.ptr(yd), gu.ptr(md), n, act, gu.ptr(dxv), gu.stream()), "vp_act_bwd")
  got = host(dxv)
  assert_guards(whole, g)
  exact("act_bwd", "act_bwd n %d act %d mask %d" % (n, act, mk), got, d)


@gpu
@pytest.mark.parametrize("n", [5, 771, 4100 * 256 + 3])
def test_mul_and_moving_update(n):
  L = _lib.lib()
  a, b, m = [rows(n, 1, n + i)[:, 0] for i in range(3)]
  assert tblk(n) == {5: 1, 771: 4}.get(n, 4096) and (n < 1000 or n > 4096 * 256)      # the last size: more elements than 4096 blocks hold
  whole, ov, g = nan_out((n,))
  ad, bd = dev(a), dev(b)
  _lib.check(L.vp_mul_f32(gu.ptr(ad), gu.ptr(bd), gu.ptr(ov), n, gu.stream()), "vp_mul_f32")
  got = host(ov)
  assert_guards(whole, g)
  exact("mul", "mul n %d" % n, got, a.astype(np.float32) * b.astype(np.float32))
  decay = float(np.float32(0.999))
  whole, mv, g = in_place(m)
  _lib.check(L.vp_moving_update(gu.ptr(mv), gu.ptr(ad), gu.ptr(bd), n, decay, gu.stream()), "vp_moving_update")
  got = host(mv)
  assert_guards(whole, g)
  t0, t1 = decay * m, b * a
  chk("moving_update", "moving_update n %d" % n, got, t0 + t1, two_term_bound(t0, t1))


@gpu
@pytest.mark.parametrize("nrows", [1, 96, 768, 1000])
def test_add_ears(nrows):
  L = _lib.lib()
  out, ears = rows(nrows, 64, nrows), f32(np.abs(rows(nrows, 1, nrows + 1)[:, 0]) * 0.3)
  whole, ov, g = in_place(out)
  ed = dev(ears)
  _lib.check(L.vp_add_ears_f32(gu.ptr(ov), gu.ptr(ed), nrows, gu.stream()), "vp_add_ears_f32")
  got = host(ov)
  assert_guards(whole, g)
  ref = out.copy()
  ref[:, 16:20] += ears[:, None] * np.array([-2.0, -2.0, -2.0, -4.0])
  exact("add_ears", "add_ears rows %d" % nrows, got, ref.astype(np.float32))


@gpu
@pytest.mark.parametrize("nrows", [1, 3, 4, 5, 96, 768])
@pytest.mark.parametrize("cols", [64, 256, 512, 65])
def test_colsum(nrows, cols):
  L = _lib.lib()
  x = rows(nrows, cols, nrows + cols, 1.0, 0.5)
  whole, ov, g = nan_out((cols,))
  xd = dev(x)
  _lib.check(L.vp_colsum_f32(gu.ptr(xd), nrows, cols, gu.ptr(ov), gu.stream()), "vp_colsum_f32")
  got = host(ov)
  assert_guards(whole, g)
  chk("colsum", "colsum (%d, %d)" % (nrows, cols), got, x.sum(0), (nrows + 1) * U * np.abs(x).sum(0))


@gpu
def test_gru_split_recurrent():
  L = _lib.lib()
  gk, ck = rows(512, 512, 1), rows(512, 256, 2)
  outs = [nan_out(s, 256) for s in ((256, 512), (256, 256), (512, 256), (256, 256))]
  gd, cd = dev(gk), dev(ck)
  _lib.check(L.vp_gru_split_recurrent(gu.ptr(gd), gu.ptr(cd), *[gu.ptr(o[1]) for o in outs], gu.stream()), "vp_gru_split_recurrent")
  want = (gk[256:], ck[256:], gk[256:].T, ck[256:].T)
  for (whole, v, g), w, name in zip(outs, want, ("whg", "whc", "whg_t", "whc_t")):
    got = host(v)
    assert_guards(whole, g)
    exact("gru_split", name, got, w.astype(np.float32))


@gpu
@pytest.mark.parametrize("b,h,w", STEM_CASES)
def test_stem_im2col(b, h, w):
  L = _lib.lib()
  x = rows(b * h, w, h + w).reshape(b, h, w)
  pl, _, wo = ar.same_pads(w, 5, 2)
  assert ar.same_pads(h, 9, 1)[0] == 4
  xp = np.pad(x, ((0, 0), (4, 4), (pl, 6)))
  ref = np.zeros((b, h, wo, 48))
  for kh in range(9):
    for kw in range(5):
      ref[..., kh * 5 + kw] = xp[:, kh:kh + h, kw:kw + 2 * wo:2]
  whole, cv, g = nan_out((b * h * wo, 48), 48 * wo)
  xd = dev(x)
  _lib.check(L.vp_stem_im2col(gu.ptr(xd), gu.ptr(cv), b, h, w, gu.stream()), "vp_stem_im2col")
  got = host(cv).reshape(b, h, wo, 48)
  assert_guards(whole, g)
  assert (ref[..., 45:] == 0).all() and (got[..., 45:] == 0).all()
  exact("stem_im2col", "im2col (%d, %d, %d)" % (b, h, w), got, ref.astype(np.float32))


@gpu
@pytest.mark.parametrize("b,h,w,c", list(DW_CASES))
def test_dwconv7x3_wgrad(b, h, w, c):
  L = _lib.lib()
  shape = dw_wgrad_shape(b, h, w)
  assert shape == DW_CASES[(b, h, w, c)]
  x, dy = rows(b * h * w, c, h + w + c).reshape(b, h, w, c), rows(b * h * w, c, h + w + c + 1).reshape(b, h, w, c)
  ref, bound = dw_wgrad_ref(x, dy, shape)
  assert L.vp_dwconv7x3_wgrad_workspace_bytes(b, h, w, c) == shape[2] * 21 * c * 4
  ws = workspace(shape[2] * 21 * c * 4)
  whole, dv, g = nan_out((21, c), c)
  xd, dyd = dev(x), dev(dy)
  _lib.check(L.vp_dwconv7x3_wgrad(gu.ptr(xd), gu.ptr(dyd), gu.ptr(dv), b, h, w, c, gu.ptr(ws), gu.stream()), "vp_dwconv7x3_wgrad")
  got = host(dv)
  assert_guards(whole, g)
  chk("dwconv7x3_wgrad", "wgrad (%d, %d, %d, %d) HS %d nseg %d G %d items/wave %d last %d" % ((b, h, w, c) + shape), got, ref, bound)


@gpu
@pytest.mark.parametrize("c", [4, 256])
@pytest.mark.parametrize("w", [1, 3, 5, 40])
@pytest.mark.parametrize("h", [1, 5, 7, 10, 120])
@pytest.mark.parametrize("geo", [0, 1])
def test_maxpool_hw_bwd(geo, h, w, c, ties=True, b=2):
  L = _lib.lib()
  k, s = POOLS[geo]
  x = rows(b * h * w, c, h + w + c, 2.0, 3.0).reshape(b, h, w, c)
  if ties:
    x = np.clip(np.round(x * 2) / 2, 0.0, 6.0)
  _, _, ho, wo = pool_geometry(h, w, k, s)
  dy = rows(b * ho * wo, c, h + w + c + 9).reshape(b, ho, wo, c)
  ref, bound = maxpool_bwd_ref(x, dy, k, s)
  if ties and h >= 5 and w >= 3 and c == 256:
    win = x[:, :k[0], :k[1], :].reshape(b, -1, c)
    assert ((win == win.max(1, keepdims=True)).sum(1) > 1).mean() > 0.05           # windows with equal maxima
  assert (bound > 0).any() == (geo == 0 and h > 1)
  whole, dv, g = nan_out((b, h, w, c), w * c)
  xd, dyd = dev(x), dev(dy)
  _lib.check(L.vp_maxpool_hw_bwd(gu.ptr(xd), gu.ptr(dyd), gu.ptr(dv), b, h, w, c, k[0], k[1], s[0], s[1], gu.stream()), "vp_maxpool_hw_bwd")
  got = host(dv)
  assert_guards(whole, g)
  chk("maxpool_hw_bwd", "pool %s/%s (%d, %d, %d) ties %d" % (k, s, h, w, c, ties), got, ref, bound)


@gpu
@pytest.mark.parametrize("geo", [0, 1])
def test_maxpool_hw_bwd_without_ties(geo):
  test_maxpool_hw_bwd(geo, 10, 5, 8, ties=False)


@gpu
def test_maxpool_hw_bwd_above_the_grid_cap():
  """More quads than 4096 blocks hold: the stride loop of maxpool_same_bwd_kernel runs a second time (a 32-clip batch does this)."""
  b, h, w, c = POOL_ABOVE_CAP
  assert b * h * w * c // 4 > 4096 * 256 and tblk(b * h * w * c // 4) == 4096
  test_maxpool_hw_bwd(0, h, w, c, b=b)


def run_gru_fwd(xg, xc, whg, whc, seq):
  L = _lib.lib()
  b, t, _ = xc.shape
  outs = [nan_out((b, t, 256), 256) for _ in range(5)]
  ins = [dev(a) for a in (xg, xc, whg, whc)]
  sq = torch.tensor(np.asarray(seq, np.int32), device="cuda")
  _lib.check(L.vp_gru_train_fwd(*[gu.ptr(a) for a in ins], gu.ptr(sq), *[gu.ptr(o[1]) for o in outs], b, t, gu.stream()), "vp_gru_train_fwd")
  got = [host(o[1]) for o in outs]
  for whole, _, g in outs:
    assert_guards(whole, g)
  return got


@gpu
def test_gru_gate_functions_as_measured():
  """The measurement behind K_SIG / K_TANH, repeated: with whg = whc = 0 the gates are 1 / (1 + expf(-xg)) and tanhf(xc) of the inputs
  alone (xg + 0 is exact).  Inputs over [-20, 20], half of the candidate's and a quarter of the gates' over [-2, 2]; the worst error in
  units of u |ref| must not exceed the figure the allowance is twice of."""
  b, t = 4096, 1
  rng = np.random.default_rng(0)
  xg, xc = f32(rng.uniform(-20, 20, (b, t, 512))), f32(rng.uniform(-20, 20, (b, t, 256)))
  xc[:b // 2] = f32(rng.uniform(-2, 2, (b // 2, t, 256)))
  xg[:b // 4] = f32(rng.uniform(-2, 2, (b // 4, t, 512)))
  out, r, u, c, hp = run_gru_fwd(xg, xc, np.zeros((256, 512)), np.zeros((256, 256)), np.ones(b, np.int32))
  g, gref, cref = np.concatenate([r, u], -1), sigmoid(xg), np.tanh(xc)
  ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
  es, et = np.abs(g - gref), np.abs(c - cref)
  ws, wt = float((es / (U * gref)).max()), float((et / (U * np.abs(cref))).max())
  print("\nsigmoid: worst %.3f u |ref| (%.3f ulp); tanh: worst %.3f u |ref| (%.3f ulp)" % (ws, (es / ulp(gref)).max(), wt, (et / ulp(cref)).max()))
  assert ws <= SIG_MEASURED and wt <= TANH_MEASURED
  assert (hp == 0).all() and inside(out, (1 - gref[..., 256:]) * cref, 3 * U * np.abs(cref) + K_SIG * U * np.abs(cref) + K_TANH * U * np.abs(cref))


@gpu
@pytest.mark.parametrize("b,t,seq", GRU_CASES, ids=lambda v: str(v)[:24])
def test_gru_train_fwd(b, t, seq):
  seq = gru_seq_len(b, t, seq)
  if b == 32:
    assert (seq == 0).sum() == 2 and len(set(seq.tolist())) > 8
  xg, xc, whg, whc = gru_inputs(b, t, seed=b + t)
  out, r, u, c, hp = run_gru_fwd(xg, xc, whg, whc, seq)
  live = np.arange(t)[None, :] < seq[:, None]
  # (a) the chain
  assert (hp[:, 0] == 0).all()
  nxt = live[:, 1:]
  assert (hp[:, 1:][nxt] == out[:, :-1][nxt]).all()
  for i in range(b):
    n = int(seq[i])
    frozen = out[i, n - 1] if n > 0 else np.zeros(256)
    assert (out[i, n:] == 0).all() and (r[i, n:] == 0).all() and (u[i, n:] == 0).all() and (c[i, n:] == 0).all() and (hp[i, n:] == frozen).all()
  # (b) every live step from the device's own h_prev
  st, ag = gru_step_ref(xg[live], xc[live], whg, whc, hp[live])
  if live.sum() >= 3:
    assert (np.abs(ag) > 15).mean() >= 0.05 and (np.abs(ag) < 2).mean() >= 0.2, ((np.abs(ag) > 15).mean(), (np.abs(ag) < 2).mean())
  for name, got in (("r", r), ("u", u), ("c", c), ("hn", out)):
    chk("gru_train_fwd", "%s (%d, %d)" % (name, b, t), got[live], *st[name])
  # (c) end to end
  x, wg, bg, wc, bc = gru_as_oracle_inputs(xg, xc, whg, whc)
  want = ar.gru_seq(x, seq, wg, bg, wc, bc)
  e = gu.rel_l2(out, want)
  print("gru_train_fwd (%d, %d): end to end rel_l2 %.2e" % (b, t, e))
  assert e < 1e-5


@gpu
@pytest.mark.parametrize("b,t,seq", GRU_CASES, ids=lambda v: str(v)[:24])
def test_gru_train_bwd(b, t, seq):
  L = _lib.lib()
  seq = gru_seq_len(b, t, seq)
  xg, xc, whg, whc = gru_inputs(b, t, seed=b + t)
  saved = [f32(a) for a in gru_fwd_ref(xg, xc, whg, whc, seq)[1:]]              # r, u, c, h_prev: the float64 forward, rounded
  dout = rows(b * t, 256, b + t + 3).reshape(b, t, 256)                          # non-zero in the dead rows too: they are ignored
  dag, dac, b_dag, b_dac = gru_bwd_ref(dout, whg, whc, seq, *saved)
  dead = ~(np.arange(t)[None, :] < seq[:, None])
  assert (dag[dead] == 0).all() and (b_dag[dead] == 0).all() and (b_dac[dead] == 0).all() and (dead.sum() == 0 or (dout[dead] != 0).any())
  wg, gv, gg = nan_out((b, t, 512), 512)
  wc, cv, gc = nan_out((b, t, 256), 256)
  ins = [dev(dout), dev(np.ascontiguousarray(whg.T)), dev(np.ascontiguousarray(whc.T))]
  sq = torch.tensor(seq, device="cuda")
  sv = [dev(a) for a in saved]
  _lib.check(L.vp_gru_train_bwd(*[gu.ptr(a) for a in ins], gu.ptr(sq), *[gu.ptr(a) for a in sv], gu.ptr(gv), gu.ptr(cv), b, t, gu.stream()), "vp_gru_train_bwd")
  got_g, got_c = host(gv), host(cv)
  assert_guards(wg, gg)
  assert_guards(wc, gc)
  chk("gru_train_bwd", "dag (%d, %d)" % (b, t), got_g, dag, b_dag)
  chk("gru_train_bwd", "dac (%d, %d)" % (b, t), got_c, dac, b_dac)
  last = np.maximum(seq - 1, 0)                                                  # the first step computed: no carried error yet
  tight = b_dac[np.arange(b), last]
  assert (tight <= 8 * U * (np.abs(dac[np.arange(b), last]) + np.abs(dout[np.arange(b), last])) + 8 * ETA).all()


def sum_f64(part, scale=1.0, add=None):
  L = _lib.lib()
  whole, ov = f64_out(1)
  _lib.check(L.vp_sum_f64(gu.ptr(part), part.numel(), float(scale), gu.ptr(add), gu.ptr(ov), gu.stream()), "vp_sum_f64")
  torch.cuda.synchronize()
  assert_f64_guards(whole)
  return float(ov.cpu()[0])


@gpu
@pytest.mark.parametrize("b,t,j,seq", VLOSS_CASES, ids=lambda v: str(v)[:20])
def test_bfm_vertex_loss(b, t, j, seq):
  L = _lib.lib()
  d, vm = vloss_inputs(b, t, j, seed=b + t)
  loss, bl, gd, bg = vloss_ref(d, vm, seq)
  nblk = L.vp_vertex_loss_partials(b, j)
  assert nblk == -(-b * j // 256)
  assert j % 256 != 0                                             # (b, j) over B x J: with B > 1 a block straddles two clips
  wp, pv = f64_out(nblk)
  whole, gv, g = nan_out((b, t, j), j)
  dd, vd, sq = dev(d), dev(vm), torch.tensor(np.asarray(seq, np.int32), device="cuda")
  _lib.check(L.vp_bfm_vertex_loss(gu.ptr(dd), gu.ptr(vd), gu.ptr(sq), b, t, j, gu.ptr(gv), gu.ptr(pv), gu.stream()), "vp_bfm_vertex_loss")
  got = host(gv)
  assert_guards(whole, g)
  assert_f64_guards(wp)
  chk("vertex_loss", "gD (%d, %d, %d)" % (b, t, j), got, gd, bg)
  parts = pv.cpu().numpy()
  chk("vertex_loss", "loss, partials summed on the host", np.array([math.fsum(parts)]), np.array([loss]), np.array([bl]))
  chk("vertex_loss", "loss through vp_sum_f64", np.array([sum_f64(pv)]), np.array([loss]), np.array([bl]))
  dead = ~(np.arange(t)[None, :] < np.asarray(seq)[:, None])
  assert (got[dead] == 0).all()


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 1024])
@pytest.mark.parametrize("with_add", [0, 1])
def test_sum_f64(n, with_add):
  p = np.random.default_rng(n).normal(size=n)
  pd = torch.tensor(p, dtype=torch.float64, device="cuda")
  add = torch.tensor([3.25], dtype=torch.float64, device="cuda") if with_add else None
  got = sum_f64(pd, -0.7, add)
  ref = (3.25 if with_add else 0.0) + -0.7 * math.fsum(p)
  chk("sum_f64", "sum_f64 n %d add %d" % (n, with_add), np.array([got]), np.array([ref]), np.array([f64_sum_bound(n, 256, (3.25 if with_add else 0) + 0.7 * np.abs(p).sum())]))      # one block: chains of n / 256


def flat_n(n):
  if n != "ntrain":
    return n
  from voicepuppet_amd.bfmnet import train_engine as te
  return sum(int(np.prod(s)) for name, _, s in te.bfmnet_manifest() if te.trainable(name))


@gpu
@pytest.mark.parametrize("n", FLAT_SIZES + ["ntrain"])
def test_sumsq_and_l2_regulariser(n):
  L = _lib.lib()
  if n == "ntrain":
    n = flat_n(n)
    from voicepuppet_amd.bfmnet.train_engine import BFMNetTrainEngine
    model = bt.synthetic_model(60, 3)
    assert BFMNetTrainEngine(1, 4, {"exBase": model["exBase"], "vmask": model["vmask"]}).ntrain == n
    assert n > 1024 * 256 and n % 4 == 0                       # the arena exceeds the 1024-block cap: every block strides
    print("ntrain = %d: %.1f trips of the 1024 x 256 stride loop" % (n, n / (1024.0 * 256)))
  nb = L.vp_sumsq_partials(n)
  assert nb == tblk(n, 1024)
  x = rows(n, 1, n % 1000 + 1)[:, 0]
  xd = dev(x)
  wp, pv = f64_out(nb)
  _lib.check(L.vp_sumsq(gu.ptr(xd), n, gu.ptr(pv), gu.stream()), "vp_sumsq")
  torch.cuda.synchronize()
  assert_f64_guards(wp)
  ss = math.fsum(x * x)
  bound = np.array([f64_sum_bound(n, nb, ss)])
  chk("sumsq", "sumsq n %d" % n, np.array([math.fsum(pv.cpu().numpy())]), np.array([ss]), bound)
  chk("sumsq", "sumsq n %d through vp_sum_f64" % n, np.array([sum_f64(pv)]), np.array([ss]), bound + f64_sum_bound(nb, 256, ss))
  # the regulariser: grads += scale * mask * params in place, partials of mask * params^2
  mask = (np.random.default_rng(n % 1000).uniform(size=n) < 0.6).astype(np.float64)
  g0 = rows(n, 1, n % 1000 + 2)[:, 0]
  scale = float(np.float32(1e-4))
  whole, gv, g = in_place(g0)
  md = dev(mask)
  wp, pv = f64_out(nb)
  _lib.check(L.vp_l2_regulariser(gu.ptr(xd), gu.ptr(md), gu.ptr(gv), n, scale, gu.ptr(pv), gu.stream()), "vp_l2_regulariser")
  got = host(gv)
  assert_guards(whole, g)
  assert_f64_guards(wp)
  ref = scale * (x * mask) + g0
  chk("l2_regulariser", "grads n %d" % n, got, ref, U * np.abs(ref))
  sm = math.fsum(x * x * mask)
  chk("l2_regulariser", "value n %d" % n, np.array([math.fsum(pv.cpu().numpy())]), np.array([sm]), np.array([f64_sum_bound(n, nb, sm)]))


@gpu
def test_bfm_step_report():
  L = _lib.lib()
  d64 = lambda v: torch.tensor([v], dtype=torch.float64, device="cuda")
  ld, reg, ss = d64(12.345678901234), d64(987.654321), d64(2501.25)
  whole, ov = f64_out(3)
  _lib.check(L.vp_bfm_step_report(gu.ptr(ld), gu.ptr(reg), 0.5e-4, gu.ptr(ss), gu.ptr(ov), gu.stream()), "vp_bfm_step_report")
  torch.cuda.synchronize()
  assert_f64_guards(whole)
  ref = np.array([12.345678901234 + 0.5e-4 * 987.654321, 12.345678901234, math.sqrt(2501.25)])
  chk("step_report", "step_report", ov.cpu().numpy(), ref, np.array([2 * V * (12.345678901234 + 0.5e-4 * 987.654321), 0.0, 2 * V * ref[2]]))


def clip_regimes(g):
  """(name, gradients, clip): the global norm below the clip, above it, and all-zero gradients."""
  norm = math.sqrt(math.fsum(g * g))
  return [("below", g, float(np.float32(2.0 * norm + 1.0))), ("above", g, float(np.float32(0.37 * norm))), ("zero", np.zeros_like(g), 50.0)]


@gpu
@pytest.mark.parametrize("n", FLAT_SIZES + ["ntrain"])
def test_clip_scale_and_adam(n):
  L = _lib.lib()
  n = flat_n(n)
  assert n % 4 == 0
  # (FLAT_SIZES[4] is the size that certainly exceeds adam_clip_kernel's capped grid, asserted in test_launch_shape_tables; the arena's
  # own size is reported)
  print("n = %d: adam %d blocks (cap 4096 %s), clip_scale %d blocks" % (n, tblk(n // 4), "hit" if n // 4 > 4096 * 256 else "not hit", tblk(n, 1024)))
  b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
  g0 = rows(n, 1, n % 1000 + 5, 0.3)[:, 0]
  p0 = rows(n, 1, n % 1000 + 6)[:, 0]
  for name, g, clip in clip_regimes(g0):
    ss = math.fsum(g * g)
    ssd = torch.tensor([ss], dtype=torch.float64, device="cuda")
    scale = clip / max(math.sqrt(ss), clip)
    assert (scale == 1.0) == (name != "above")
    # vp_clip_scale_f32
    whole, gv, gg = in_place(g)
    _lib.check(L.vp_clip_scale_f32(gu.ptr(gv), n, gu.ptr(ssd), clip, gu.stream()), "vp_clip_scale_f32")
    got = host(gv)
    assert_guards(whole, gg)
    chk("clip_scale", "clip_scale n %d %s" % (n, name), got, g * scale, 0.0 if scale == 1.0 else 2 * U * np.abs(g * scale) + 4 * V * np.abs(g * scale))
    # two Adam steps: the second reads the non-zero slots the first left (taken from the device, exact for the reference)
    bufs = [in_place(a) for a in (p0, g, np.zeros(n), np.zeros(n))]
    state = [p0, g, np.zeros(n), np.zeros(n)]
    for step in (1, 2):
      lr_t = float(np.float32(1e-4 * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)))
      lrd = torch.tensor([lr_t], dtype=torch.float32, device="cuda")
      ref = adam_ref(state[0], state[1], state[2], state[3], lr_t, ss, clip, b1, b2, eps)
      _lib.check(L.vp_adam_tf_clipped(*[gu.ptr(v[1]) for v in bufs], n, gu.ptr(lrd), gu.ptr(ssd), clip, b1, b2, eps, gu.stream()), "vp_adam_tf_clipped")
      new = [host(v[1]) for v in bufs]
      for whole, _, gg in bufs:
        assert_guards(whole, gg)
      for k, got in zip(("p", "g", "m", "v"), new):
        chk("adam_tf_clipped", "%s n %d %s step %d" % (k, n, name, step), got, *ref[k])
      if scale == 1.0:
        assert (new[1] == state[1]).all()                      # the gradients come back bit-identical
      if name == "zero":
        assert (new[0] == p0).all() and (new[2] == 0).all() and (new[3] == 0).all()
      state = new
      if step == 1 and name != "zero":                          # a new gradient for the second step; *sumsq stays (a test-made scalar)
        g2 = rows(n, 1, n % 1000 + 7, 0.3)[:, 0]
        g2 = g2 * (math.sqrt(ss) / math.sqrt(math.fsum(g2 * g2)))          # of the same norm: the regime holds
        bufs[1][1].copy_(torch.tensor(g2, dtype=torch.float32))
        state[1] = host(bufs[1][1])


@gpu
def test_entry_points_refuse_bad_arguments():
  """Each entry point once with a bad shape or a null required pointer: VP_ERR_ARG with a message, before any launch (the output a good
  call would write is still NaN)."""
  L = _lib.lib()
  buf = torch.ones(4096, device="cuda")
  out = torch.full((4096,), float("nan"), device="cuda")
  i32 = torch.ones(8, dtype=torch.int32, device="cuda")
  d64 = torch.ones(64, dtype=torch.float64, device="cuda")
  o64 = torch.full((64,), float("nan"), dtype=torch.float64, device="cuda")
  B, O, I, D, Q, N, S = gu.ptr(buf), gu.ptr(out), gu.ptr(i32), gu.ptr(d64), gu.ptr(o64), None, gu.stream()
  calls = {
      "vp_bn_train_fwd c=6": lambda: L.vp_bn_train_fwd(B, 8, 6, B, 1e-3, O, O, O, O, O, Q, S),
      "vp_bn_train_fwd pixels=0": lambda: L.vp_bn_train_fwd(B, 0, 8, B, 1e-3, O, O, O, O, O, Q, S),
      "vp_bn_act_train_bwd c=6": lambda: L.vp_bn_act_train_bwd(B, B, 8, 6, B, B, B, 5, O, O, Q, S),
      "vp_bn_act_train_bwd no shift": lambda: L.vp_bn_act_train_bwd(B, B, 8, 8, B, B, N, 5, O, O, Q, S),
      "vp_bn_train_bwd pixels=0": lambda: L.vp_bn_train_bwd(B, B, 0, 8, B, B, O, O, Q, S),
      "vp_bn_train_bwd no mean": lambda: L.vp_bn_train_bwd(B, B, 8, 8, N, B, O, O, Q, S),
      "vp_affine_act_fwd c=6": lambda: L.vp_affine_act_fwd(B, B, B, N, 8, 6, 2, O, S),
      "vp_affine_act_fwd scale without shift": lambda: L.vp_affine_act_fwd(B, B, N, N, 8, 8, 2, O, S),
      "vp_affine_act_add_fwd no add": lambda: L.vp_affine_act_add_fwd(B, B, B, N, N, 8, 8, 2, O, S),
      "vp_affine_act_add_fwd pixels=0": lambda: L.vp_affine_act_add_fwd(B, B, B, N, B, 0, 8, 2, O, S),
      "vp_act_bwd n=6": lambda: L.vp_act_bwd(B, B, N, 6, 2, O, S),
      "vp_mul_f32 n=0": lambda: L.vp_mul_f32(B, B, O, 0, S),
      "vp_add_ears_f32 rows=0": lambda: L.vp_add_ears_f32(O, B, 0, S),
      "vp_add_ears_f32 no ears": lambda: L.vp_add_ears_f32(O, N, 4, S),
      "vp_moving_update n=0": lambda: L.vp_moving_update(O, B, B, 0, 0.999, S),
      "vp_moving_update no factor": lambda: L.vp_moving_update(O, B, N, 8, 0.999, S),
      "vp_colsum_f32 rows=0": lambda: L.vp_colsum_f32(B, 0, 8, O, S),
      "vp_gru_split_recurrent null": lambda: L.vp_gru_split_recurrent(B, N, O, O, O, O, S),
      "vp_stem_im2col w=1": lambda: L.vp_stem_im2col(B, O, 1, 5, 1, S),
      "vp_dwconv7x3_wgrad c=2": lambda: L.vp_dwconv7x3_wgrad(B, B, O, 1, 4, 4, 2, Q, S),
      "vp_dwconv7x3_wgrad no workspace": lambda: L.vp_dwconv7x3_wgrad(B, B, O, 1, 4, 4, 8, N, S),
      "vp_maxpool_hw_bwd c=6": lambda: L.vp_maxpool_hw_bwd(B, B, O, 1, 4, 4, 6, 2, 2, 1, 2, S),
      "vp_maxpool_hw_bwd h=0": lambda: L.vp_maxpool_hw_bwd(B, B, O, 1, 0, 4, 8, 2, 2, 1, 2, S),
      "vp_maxpool_hw_bwd w=-1": lambda: L.vp_maxpool_hw_bwd(B, B, O, 1, 4, -1, 8, 2, 2, 1, 2, S),
      "vp_gru_train_fwd t=0": lambda: L.vp_gru_train_fwd(B, B, B, B, I, O, O, O, O, O, 1, 0, S),
      "vp_gru_train_fwd no seq_len": lambda: L.vp_gru_train_fwd(B, B, B, B, N, O, O, O, O, O, 1, 1, S),
      "vp_gru_train_bwd b=0": lambda: L.vp_gru_train_bwd(B, B, B, I, B, B, B, B, O, O, 0, 1, S),
      "vp_bfm_vertex_loss j=0": lambda: L.vp_bfm_vertex_loss(B, B, I, 1, 1, 0, O, Q, S),
      "vp_bfm_vertex_loss no partial": lambda: L.vp_bfm_vertex_loss(B, B, I, 1, 1, 8, O, N, S),
      "vp_sumsq n=0": lambda: L.vp_sumsq(B, 0, Q, S),
      "vp_l2_regulariser no mask": lambda: L.vp_l2_regulariser(B, N, O, 8, 1e-4, Q, S),
      "vp_sum_f64 n=0": lambda: L.vp_sum_f64(D, 0, 1.0, N, Q, S),
      "vp_bfm_step_report null": lambda: L.vp_bfm_step_report(D, N, 0.5, D, Q, S),
      "vp_clip_scale_f32 clip=0": lambda: L.vp_clip_scale_f32(O, 8, D, 0.0, S),
      "vp_adam_tf_clipped n=6": lambda: L.vp_adam_tf_clipped(O, O, O, O, 6, B, D, 50.0, 0.9, 0.999, 1e-8, S),
      "vp_adam_tf_clipped clip=0": lambda: L.vp_adam_tf_clipped(O, O, O, O, 8, B, D, 0.0, 0.9, 0.999, 1e-8, S),
  }
  for name, call in calls.items():
    assert call() == VP_ERR_ARG, name
    assert len(L.vp_last_error()) > 0 and L.vp_last_error().startswith(name.split()[0].encode() + b":"), (name, L.vp_last_error())
  torch.cuda.synchronize()
  assert bool(torch.isnan(out).all()) and bool(torch.isnan(o64).all()) and bool((buf == 1).all())

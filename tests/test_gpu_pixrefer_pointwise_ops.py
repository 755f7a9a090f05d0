"""Op-level float64 parity of the PixReferNet training step's pointwise kernels (csrc/pointwise.hip): batch norm in groups (both
launch paths, backward, the tail form, column sums), act_apply, relu_bwd, the tap gather / spread pair, pack_inputs, the training
composite forward and its backward, the perceptual loss, loss_final, gan_loss, vp_adam_tf and the bf16 gradient transport.

Rules (as test_gpu_bfmnet_train_ops.py, whose helpers are reused)
  * the device sees float32 or bf16 values; the reference is float64 numpy on exactly those values, written here;
  * whatever an entry point takes as an input (mean / rstd, o4 / outputs, partial rows, Adam slots) is TEST-MADE and exact for the
    reference: no backward case depends on a forward kernel.  (The activations vp_bn_groups_fwd writes next to its statistics are the one
    place where a kernel's own float32 output, scale / shift of the same call, enters a restatement; scale / shift themselves are checked
    against float64.)
  * outputs are prefilled with NaN between guard bands of a sentinel that must come back untouched; in-place entry points: bands only;
  * the comparison is PER ELEMENT, |got - ref| <= bound, first order in u = 2^-24, v = 2^-53 and, for a bf16 store, ub = 2^-8; a bound
    of 0 means bit-equal to a numpy float32 restatement.  (ub: bf16 keeps 8 significant bits, so a correctly rounded store is off by up
    to half a unit of the eighth, 2^-8 |x| / (1 + 2^-8): 1 + 2^-8 itself is a tie and goes to 1.  The 2^-9 this file was first written
    with is what truncating float32 to NINE bits would give; every bf16 bound then measured 1.99 on the MI355X, on kernels whose store
    is bit-equal to nearest-even in the pack cases.  test_bf16_rounding_restatement asserts both halves on the CPU.) where the compiler may contract (act_apply's 0.6 z + 0.4 |z|) exactly the
    contracted and uncontracted forms are allowed (test_gpu_ops_exact.py::test_leaky_relu_forms);
  * every case restates the launcher's formula (bn_nchunk, the Pg <= 2048 rule, nblocks(work, cap), composite_nblocks,
    perceptual_nblocks) and asserts the class it was written for.

Bounds
  batch norm forward, per (group, channel), gamma_s = (Pg + nchunk) v (one launch: nchunk = 1), eps inside the square root
    mean   u |m| + gamma_s E|x|                                    e = 5 gamma_s E[x^2] (the sibling's var line)
    rstd   u |rstd| + (e / 2) (var + eps)^-3/2 + 3 v |rstd|
    scale  u |scale| + |gamma| bound(rstd)                          (fl(gamma * rstd); zero variance: scale == 0, shift == beta, bit for bit)
    shift  u |shift| + |m| bound(scale) + |scale| gamma_s E|x| + 2 v (|beta| + |m scale|)
    lrelu / relu outputs: bit-equal to act(fma(scale, y, shift)) of the call's own float32 scale / shift, then the store's rounding
  batch norm backward, zhat = fl(fl(y - mean) rstd), gamma_s = (Pg + nchunk + G) v (the sums over groups)
    dbeta  u |dbeta| + gamma_s Sum |dz|                            dgamma  u |dgamma| + (gamma_s + 2 u) Sum |dz zhat|
    c1     u |c1| + (gamma_s + 2 v) E|dz|                          c2      u |c2| + (gamma_s + 2 v + 2 u) E|dz zhat|
    dy     2 u |dy| + |gamma rstd| (6 u S + bound(c1) + |zhat| bound(c2)),  S = |dz| + |c1| + |zhat c2|   (the sibling's dx line, one more
           rounding for fl(gamma * rstd)); + ub |dy| for a bf16 store; accumulate: + u |old + new|
    tail, raw = 1: c2 = rstd (Sum dz y - mean Sum dz) / Pg in float64: u |c2| + (gamma_s + 4 v) rstd (E|dz y| + |mean| E|dz|), and
           dgamma likewise; raw = 0 as above (the test's own float64 chunk sums are within the same gamma_s)
  colsum   u |s| + (Pg + nchunk + G) v Sum |x|  (+ u |old + s| with accumulate)
  relu_bwd, tap_gather (the float32 chain in kh, kw order, then + bias), tap_spread, pack_inputs (2 x - 1: the product is exact, one
           rounding either way), grad pack / unpack: BIT-EQUAL
  composite forward, d = K_TANH u |o| the error of tanhf (measured, below)
    alpha  d_3 / 2 + u |alpha|                 tg = fl(2 t - 1): u |tg|
    out    |alpha| d_c + |o_c - tg| b(alpha) + |1 - alpha| b(tg) + u |1 - alpha| |tg| + u (|o alpha| + |tg (1 - alpha)|) + u |out|
    ofg    |alpha| d_c + |o_c + 1| b(alpha) + u |o alpha| + u |o alpha + alpha| + u |ofg|
    sums   (n / nblocks + 10) v Sum |terms| + Sum over the terms of (b(tg) + b(out) + u |tg - out|), resp. (b(alpha) + u |m - alpha|)
  composite backward (s, tg, alpha restated in float32; the signs are exact), t = 1 - o^2: e_t = u o^2 + u |t|
    c < 3  |alpha t| (u |d_fg| + u |d_out + d_fg|) + |(d_out + d_fg) alpha| e_t + 2 u |v|   (+ ub |v|)
    alpha  dal = Sum_c (d_out (o - tg) + d_fg (o + 1) + d_al): 12 u Sum |terms| (at most 3 roundings inside a term, 9 additions);
           v = dal t / 2: |t / 2| b(dal) + |dal / 2| e_t + u |v|
  perceptual  df3: 2 u |ref| (+ ub |ref|), bit-equal where difference and product are exact; partial: 2 u Sum x^2 + the float64-sum bound
  loss_final  2 u |ref| + (n / 256 + 10) v Sum |terms|
  gan_loss, dp = K_SIG u p the error of 1 / (1 + expf(-a)); q = x + eps with eps = fl32(1e-12): b(q) = b(x) + u q;
    err(log q) = b(q) / q + K_LOG u |log q|;  the loss terms sum these, + u per float32 operation, + the float64-sum bound
    seeds: |ref| times the sum of the relative errors of the factors (b(q) / q + 2 u for a division, dp / p + u, (dp + u (1 - p)) /
    (1 - p) + u, u for each further product) + 4 eta (+ ub |ref|)
    saturated plants |a| = 50, 100: 1 + expf(-a) == 1 (a >= 40) or expf overflows (a <= -87), so the device's p is exactly 1 resp. 0 and
    its error is e^-|a| itself: dp += e^-|a| there.  With it the eps = 1e-12 inside every logarithm and quotient turns that error into
    at most e^-50 / 1e-12 = 2e-10 relative: the absolute term.  NOT covered: 17 < |a| < 40, where 1 - p is within a few u of 0 and
    fl32(1 - p) jumps between 0 and neighbouring multiples of u, i.e. the float32 formula itself has no small error.
  vp_adam_tf (the sibling's m, v, p lines without the clip), eta = 2^-149 for the subnormal g^2
    m   u (|b1 m| + |(1 - b1) g|) + u |m'| + 2 eta          v   u (|b2 v| + 2 (1 - b2) g^2) + u |v'| + 3 eta
    p   u |p'| + |q| (5 u + (bound(v) / (2 sqrt v) + 2 u sqrt v) / (sqrt v + eps)) + lr_t bound(m) / (sqrt v + eps)

Function errors measured on the MI355X through the kernels that use them (no copy of the HIP math accuracy table is installed):
see TANH_MEASURED, SIG_MEASURED, LOG_MEASURED below; test_function_errors_as_measured repeats the measurement and asserts them.

Measured on an MI355X: tanhf 2.253 u |ref| over [-8, 8], 1 / (1 + expf(-a)) 1.506 u |ref| over [-8, 8], logf 2.826 u |ref| over the
arguments the sigmoid of [-8, 8] gives (3.4e-4 .. 1 - 3.4e-4, |log| > 1e-3); rounded up to 2.26 / 1.51 / 2.83, allowed 4.52 / 3.02 / 5.66.
Worst |got - ref| / bound per kernel over all cases (185 cases, 9 s):
  bn_fwd 0.970   bn_bwd 0.996   bn_bwd_tail 0.986   adam_tf 0.999   perceptual 0.995   composite_bwd 0.996
  (dominated by the rounding of the output itself: half an ulp IS u |ref|, resp. ub |ref|, just above a power of two)
  colsum 0.426   composite_fwd 0.720   loss_final 0.337   gan_loss 1.000 (the fake logit -100: the device's p is 0, the bound is the
  true p = e^-100 times 1 + K_SIG u; the largest other ratio is 0.996)
  act_apply (one of the three forms), relu_bwd, tap_gather, tap_spread, pack_inputs, grad_pack_bf16, grad_unpack_bf16: bit-equal
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from voicepuppet_amd import _lib
from voicepuppet_amd._lib import BN_PATH_ONE_LAUNCH, BN_PATH_PLANNER, BN_PATH_TWO_PASS, VP_BF16, VP_F32

import gpu_util as gu
from test_gpu_bfmnet_train_ops import (SENTINEL, U, V, ETA, VP_ERR_ARG, assert_f64_guards, assert_guards, chk, exact, f32, f64_out, f64_sum_bound,
                                       fma32, guarded)
from test_gpu_ops_exact import lrelu_forms

gpu = pytest.mark.gpu
UB = 2.0 ** -8                          # unit roundoff of a bf16 store: 8 significant bits (module docstring)
E = {"f32": 4, "bf16": 8}
DT = {"f32": VP_F32, "bf16": VP_BF16}
DTYPES = ["f32", "bf16"]
BN_EPS = 1e-5
GROUP_SCALES = (1.0, 0.45, 2.2)         # the BN groups of a case differ clearly in scale (and in offset, gamma, rstd)
# worst |err| / (u |ref|) on the MI355X, rounded up (test_function_errors_as_measured); twice that is allowed
TANH_MEASURED, SIG_MEASURED, LOG_MEASURED = 2.26, 1.51, 2.83
K_TANH, K_SIG, K_LOG = 2 * TANH_MEASURED, 2 * SIG_MEASURED, 2 * LOG_MEASURED


# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' formulas, restated (csrc/pointwise.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def nblocks(work, cap=2048):
  return max(1, min((work + 255) // 256, cap))


def bn_nchunk(pg, c, g, dtype):
  nprow = 256 // (c // E[dtype])
  return max(1, min((pg + nprow * 8 - 1) // (nprow * 8), 1024 // g))


def bn_small(pg):
  return pg <= 2048


def composite_nblocks(n, hw):
  return nblocks(n * hw, 1024)


def perceptual_nblocks(half, dtype):
  return nblocks(half // E[dtype], 1024)


def bn_class(g, pg, c, dtype, path):
  """(one launch?, nchunk, channel groups, trips of chunk_sum, apply blocks)"""
  one = path == BN_PATH_ONE_LAUNCH or (path == BN_PATH_PLANNER and bn_small(pg))
  nch = 1 if one else bn_nchunk(pg, c, g, dtype)
  return one, nch, c // E[dtype], -(-nch // 512), nblocks(g * pg * (c // E[dtype]))


# ---------------------------------------------------------------------------------------------------------------------------------
# values, buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
  """float32 -> nearest-even bf16, as float32 (NaN stays NaN)."""
  x = np.ascontiguousarray(x, np.float32)
  b = x.view(np.uint32).astype(np.uint64)
  r = ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32)
  return np.where(np.isnan(x), x, r.view(np.float32))


def bf16_truncate(x):
  x = np.ascontiguousarray(x, np.float32)
  return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def stored(x32, dtype):
  """What a store of the float32 value leaves, as float64."""
  x32 = np.asarray(x32, np.float32)
  return (bf16_round(x32) if dtype == "bf16" else x32).astype(np.float64)


def st(bound, ref, dtype):
  return bound + (UB * np.abs(ref) if dtype == "bf16" else 0.0)


def host(t):
  torch.cuda.synchronize()
  return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy().astype(np.float64)


def seen(a, dtype):
  return gu.rounded(a, dtype)


def operand(a, dtype="f32"):
  return gu.nan_banded(a, dtype)


def out(shape, dtype="f32", fill=None):
  return guarded(tuple(shape), 64, dtype, fill=fill)


def done(*bufs):
  torch.cuda.synchronize()
  for whole, _, g in bufs:
    assert_guards(whole, g)


def one_of(kernel, name, got, forms32, dtype):
  """Every element equals one of the allowed float32 evaluations (after the store's rounding)."""
  ok = np.zeros(got.shape, bool)
  for fm in forms32:
    ok |= got == stored(fm, dtype)
  print("\nRATIO %s %.4f   (%s: one of %d forms)" % (kernel, 0.0 if ok.all() else np.inf, name, len(forms32)))
  assert ok.all(), "%s: %d elements match no allowed form, first at %s" % (name, int((~ok).sum()), np.argwhere(~ok)[0])


def ws_bytes(L, g, pg, c, dtype):
  n = L.vp_bn_groups_workspace_bytes(g, pg, c, DT[dtype])
  assert n == g * bn_nchunk(pg, c, g, dtype) * 2 * c * 8 + 1024
  return n


def workspace(nbytes):
  whole, view, g = guarded((int(nbytes),), 0, "u8", min_bytes=4096)
  return whole, view, g


# ---------------------------------------------------------------------------------------------------------------------------------
# batch norm: inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_x(g, pg, c, dtype, seed, sigma=1.3):
  """[g, pg, c] device values as float64: every group its own scale and per-channel offset."""
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((g, pg, c), dtype=np.float32)
  for i in range(g):
    x[i] *= np.float32(GROUP_SCALES[i % 3] * sigma)
  off = rng.normal(0, 2.0, (g, 1, c)).astype(np.float32)
  return seen(x + off, dtype), off[:, 0].astype(np.float64)


def bn_params(c, seed):
  rng = np.random.default_rng(seed + 11)
  return f32(rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)), f32(rng.uniform(-1.0, 1.0, c))


def bn_fwd_ref(x, gamma, beta, eps, nchunk):
  """{name: (reference [G, C], bound)} of vp_bn_groups_fwd."""
  p = x.shape[1]
  eps = float(np.float32(eps))
  m = x.mean(1)
  var = ((x - m[:, None]) ** 2).mean(1)
  gam = (p + nchunk) * V
  em = gam * np.abs(x).mean(1)
  e = 5 * gam * (x * x).mean(1)
  rstd = 1.0 / np.sqrt(var + eps)
  b_rstd = U * rstd + 0.5 * e * (var + eps) ** -1.5 + 3 * V * rstd
  zero = var == 0
  scale = np.where(zero, 0.0, gamma * rstd)
  b_scale = np.where(zero, 0.0, U * np.abs(scale) + np.abs(gamma) * b_rstd)
  shift = np.where(zero, beta, beta - m * scale)
  b_shift = np.where(zero, 0.0, U * np.abs(shift) + np.abs(m) * b_scale + np.abs(scale) * em + 2 * V * (np.abs(beta) + np.abs(m * scale)))
  return {"mean": (m, U * np.abs(m) + em), "rstd": (rstd, b_rstd), "scale": (scale, b_scale), "shift": (shift, b_shift),
          "var": (var, U * (var + e) + e)}


def bn_stats_float32_accumulators(x):
  """bn_reduce_kernel + bn_finalize_kernel with the two sums held in FLOAT32 (the regression the op tests must reject): (mean, var)."""
  s0 = np.zeros(x.shape[2], np.float32)
  s1 = np.zeros(x.shape[2], np.float32)
  x32 = x[0].astype(np.float32)
  for row in x32:
    s0 = s0 + row
    s1 = s1 + row * row
  m = s0.astype(np.float64) / x.shape[1]
  return m, np.maximum(s1.astype(np.float64) / x.shape[1] - m * m, 0.0)


def offset_case():
  """f32, Pg = 4100: per-channel mean 100 (1 + c / C), deviation 0.05."""
  c, pg = 16, 4100
  rng = np.random.default_rng(77)
  x = f32(100.0 * (1 + np.arange(c) / c) + 0.05 * rng.standard_normal((1, pg, c)))
  return x, c, pg


def bn_bwd_inputs(g, pg, c, dtype, seed):
  """y, dz (device values) and TEST-MADE mean / rstd / gamma: near the statistics of y, clearly different between the groups."""
  y, off = bn_x(g, pg, c, dtype, seed)
  rng = np.random.default_rng(seed + 5)
  dz = seen(rng.standard_normal((g, pg, c)) * np.float32(0.7) * np.asarray(GROUP_SCALES)[np.arange(g) % 3][:, None, None] + rng.normal(0, 0.3, (g, 1, c)), dtype)
  mean = f32(off + rng.normal(0, 0.05, (g, c)))
  rstd = f32(1.0 / (1.3 * np.asarray(GROUP_SCALES)[np.arange(g) % 3][:, None]) * rng.uniform(0.8, 1.25, (g, c)))
  gamma, _ = bn_params(c, seed)
  return y, dz, mean, rstd, gamma


def bn_bwd_ref(y, dz, mean, rstd, gamma, nchunk, dtype, old=None, raw=False):
  """{name: (reference, bound)} of vp_bn_groups_bwd / _tail: dy [G, Pg, C], c1, c2 [G, C], dgamma, dbeta [C] (old: (dgamma, dbeta) added)."""
  g, p, _ = y.shape
  zh = (y - mean[:, None]) * rstd[:, None]
  gam = (p + nchunk + g) * V
  adz, adzx = np.abs(dz), np.abs(dz * zh)
  c1, c2 = dz.mean(1), (dz * zh).mean(1)
  b_c1 = U * np.abs(c1) + (gam + 2 * V) * adz.mean(1)
  if raw:
    mag = rstd * (np.abs(dz * y).mean(1) + np.abs(mean) * adz.mean(1))
    b_c2 = U * np.abs(c2) + (gam + 4 * V) * mag
    b_dg = (gam + 4 * V) * (mag * p).sum(0)
  else:
    b_c2 = U * np.abs(c2) + (gam + 2 * V + 2 * U) * adzx.mean(1)
    b_dg = (gam + 2 * U) * adzx.sum((0, 1))
  dbeta, dgamma = dz.sum((0, 1)), (dz * zh).sum((0, 1))
  b_db = gam * adz.sum((0, 1))
  if old is not None:
    b_dg, b_db = b_dg + U * np.abs(dgamma), b_db + U * np.abs(dbeta)
    dgamma, dbeta = dgamma + old[0], dbeta + old[1]
  coef = gamma * rstd
  dy = coef[:, None] * (dz - c1[:, None] - zh * c2[:, None])
  s = adz + np.abs(c1)[:, None] + np.abs(zh * c2[:, None])
  b_dy = 2 * U * np.abs(dy) + np.abs(coef)[:, None] * (6 * U * s + b_c1[:, None] + np.abs(zh) * b_c2[:, None])
  return {"dy": (dy, st(b_dy, dy, dtype)), "c1": (c1, b_c1), "c2": (c2, b_c2), "dgamma": (dgamma, b_dg + U * np.abs(dgamma)),
          "dbeta": (dbeta, b_db + U * np.abs(dbeta))}


def bn_partial_rows(y, dz, mean, rstd, nchunk, raw):
  """[G][nchunk][2][C] float64: (sum dz, sum dz zhat) of each pixel chunk, or the raw moments (sum dz, sum dz y)."""
  g, p, c = y.shape
  per = -(-p // nchunk)
  w = dz * y if raw else dz * ((y - mean[:, None]) * rstd[:, None])
  rows = np.zeros((g, nchunk, 2, c))
  for k in range(nchunk):
    rows[:, k, 0] = dz[:, k * per:(k + 1) * per].sum(1)
    rows[:, k, 1] = w[:, k * per:(k + 1) * per].sum(1)
  return rows


def act_forms(y, sc, sh):
  """(relu, [the three leaky forms]) of act_apply_kernel in float32: z = fma(sc, y, sh) per group (sc None: z = y)."""
  z = fma32(sc[:, None, :], y, sh[:, None, :]) if sc is not None else y.astype(np.float32)
  return np.maximum(z, np.float32(0)), [fm.astype(np.float32) for fm in lrelu_forms(z.astype(np.float64))]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests: the teeth of the offset case, the restated formulas, the rounding helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_float32_accumulation_violates_the_offset_case():
  """The offset case rejects a reduce pass whose accumulators are float32: its variance (and with it rstd) lies outside the bound."""
  x, c, pg = offset_case()
  nch = bn_nchunk(pg, c, 1, "f32")
  ref = bn_fwd_ref(x, np.ones(c), np.zeros(c), BN_EPS, nch)
  assert np.all(np.abs(ref["mean"][0] - 100.0 * (1 + np.arange(c) / c)) < 0.01) and np.all(np.abs(np.sqrt(ref["var"][0]) - 0.05) < 0.005)
  m32, var32 = bn_stats_float32_accumulators(x)
  assert (np.abs(var32 - ref["var"][0]) > ref["var"][1]).all()
  rstd32 = 1.0 / np.sqrt(var32 + float(np.float32(BN_EPS)))
  assert (np.abs(rstd32 - ref["rstd"][0]) > ref["rstd"][1]).all()
  # ... while the same restatement with float64 accumulators stays inside (the bound is no artefact of the reference)
  m64 = x[0].sum(0) / pg
  var64 = (x[0] * x[0]).sum(0) / pg - m64 * m64
  assert (np.abs(var64 - ref["var"][0]) <= ref["var"][1]).all() and (np.abs(m64 - ref["mean"][0]) <= ref["mean"][1]).all()


def test_bf16_rounding_restatement():
  """Nearest-even against torch, and the teeth of the pack test: truncation differs on its planted values."""
  x = np.concatenate([pack_plants(), f32(np.random.default_rng(3).standard_normal(4096) * 37.0)]).astype(np.float32)
  want = torch.tensor(x).to(torch.bfloat16).float().numpy()
  assert (bf16_round(x).view(np.uint32) == want.view(np.uint32)).all()
  assert (bf16_truncate(pack_plants()).view(np.uint32) != bf16_round(pack_plants()).view(np.uint32)).sum() >= 3
  # the unit roundoff of the store: nearest-even stays within UB |x| and does NOT stay within UB / 2
  fin = x[np.isfinite(x) & (np.abs(x) > 1e-30) & (np.abs(x) < 1e38)].astype(np.float64)
  err = np.abs(bf16_round(fin.astype(np.float32)).astype(np.float64) - fin)
  assert (err <= UB * np.abs(fin)).all() and (err > UB / 2 * np.abs(fin)).any()
  tie = np.float32(1 + 2.0 ** -8)
  assert bf16_round(np.array([tie]))[0] == 1.0 and (float(tie) - 1.0) > 2.0 ** -9 * float(tie)


def test_launch_classes_of_the_case_tables():
  for (g, pg, c, dtype, path), want in BN_CLASSES.items():
    assert bn_class(g, pg, c, dtype, path)[:4] == want, (g, pg, c, dtype, path, bn_class(g, pg, c, dtype, path))
  for g, pg, c, dtype in OVER_CAP:
    work = g * pg * (c // E[dtype])
    assert work > 2048 * 256 and nblocks(work) == 2048 and not bn_small(pg)
    # thread i of the capped grid goes on to item i + 2048 * 256: another group
    assert (2048 * 256 // (c // E[dtype])) // pg != 0
  assert composite_nblocks(1, COMPOSITE_SIZES[2]) == 1024 and COMPOSITE_SIZES[2] > 1024 * 256 and composite_nblocks(1, 512) == 2
  for dtype in DTYPES:
    halves = perceptual_halves(dtype)
    assert [perceptual_nblocks(h, dtype) for h in halves] == [1, 2, 1024] and halves[2] // E[dtype] == 1024 * 256 + 1


def within(name, got, ref, bound):
  bad = np.abs(np.asarray(got, np.float64) - ref) > bound
  assert not bad.any(), "%s: %d elements of the float32 restatement outside the bound, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


def test_bounds_hold_for_float32_restatements_of_the_kernels():
  """adam_tf_kernel and composite_bwd_kernel restated in numpy float32 (uncontracted, the kernel's order of operations) stay inside the
  bounds the GPU cases use: the bounds are no artefact of how the references are written."""
  f = np.float32
  n = 4096
  rng = np.random.default_rng(0)
  p, g, m, v = (rng.standard_normal(n).astype(f), rng.normal(0, 0.02, n).astype(f), rng.normal(0, 0.01, n).astype(f), (rng.normal(0, 0.01, n) ** 2).astype(f))
  g[:6] = (0.0, 0.0, 1e-20, -3e-21, 1e15, -4e14)
  m[1], v[1] = 0.0, 0.0
  lr_t, b1, b2, eps = f(1.3e-4), f(0.5), f(0.999), f(1e-8)
  m1 = b1 * m + (f(1) - b1) * g
  v1 = b2 * v + (f(1) - b2) * g * g
  p1 = p - lr_t * m1 / (np.sqrt(v1) + eps)
  assert m1.dtype == v1.dtype == p1.dtype == np.float32 and p1[1] == p[1]
  ref = adam_ref(*[a.astype(np.float64) for a in (p, g, m, v)], float(lr_t), float(b1), float(b2), float(eps))
  for k, got in (("m", m1), ("v", v1), ("p", p1)):
    within("adam " + k, got, *ref[k])
  total, l1w = 2000, 500.0
  o4, tgt, msk, outp, dd, dv, tg32, al32, ties = composite_bwd_case(total, "f32", l1w)
  ref, bound = composite_bwd_ref(o4, msk, outp, dd, dv, tg32, al32, l1w, "f32")
  o, t32, a32 = o4.astype(f), tg32.astype(f), al32.astype(f)[:, None]
  sc = f(l1w) / f(float(total) * 3.0)
  d_out = -sc * np.sign(t32 - outp.astype(f))
  d_al = -sc * np.sign(msk.astype(f) - a32)
  d_fg = dd[:, 3:6].astype(f) + dv[:, 0:3].astype(f)
  dout = (d_out + d_fg) * a32
  dal = np.zeros(total, f)
  for c in range(3):
    dal = dal + (d_out[:, c] * (o[:, c] - t32[:, c]) + d_fg[:, c] * (o[:, c] + f(1)) + d_al[:, c])
  got = np.concatenate([dout, (dal * f(0.5))[:, None]], 1) * (f(1) - o * o)
  assert got.dtype == np.float32
  within("composite_bwd", got, ref[:, :4], bound[:, :4])


# (G, Pg, C, dtype, path) -> (one launch, nchunk, channel groups, trips of chunk_sum)
P0, P2, P1 = BN_PATH_PLANNER, BN_PATH_TWO_PASS, BN_PATH_ONE_LAUNCH
BN_CLASSES = {
    (1, 1, 8, "f32", P0): (True, 1, 2, 1), (1, 1, 8, "bf16", P0): (True, 1, 1, 1),                       # zero variance, one launch
    (1, 1, 8, "f32", P2): (False, 1, 2, 1), (1, 1, 8, "bf16", P2): (False, 1, 1, 1),                     # ... and two passes
    (3, 5, 8, "f32", P0): (True, 1, 2, 1), (3, 5, 8, "bf16", P0): (True, 1, 1, 1),
    (2, 257, 64, "f32", P0): (True, 1, 16, 1), (2, 257, 64, "bf16", P0): (True, 1, 8, 1),                # the pixel loop runs twice
    (1, 2048, 16, "f32", P0): (True, 1, 4, 1), (1, 2048, 16, "bf16", P0): (True, 1, 2, 1),               # the boundary
    (1, 2049, 16, "f32", P0): (False, 5, 4, 1), (1, 2049, 16, "bf16", P0): (False, 3, 2, 1),
    (1, 2100, 8, "bf16", P0): (False, 2, 1, 1),                                                           # ncg 1: every shuffle step
    (1, 300, 256, "bf16", P2): (False, 5, 32, 1),                                                         # ncg 32: the last shuffle width
    (1, 300, 512, "bf16", P2): (False, 10, 64, 1),                                                        # ncg 64: the LDS walk
    (1, 8209, 512, "f32", P0): (False, 514, 128, 2),                                                      # f32 ncg 128; chunk_sum's second trip
    (3, 5500, 512, "f32", P0): (False, 341, 128, 1),                                                      # the 1024 / G cap
}
OVER_CAP = [(3, 180000, 8, "bf16"), (3, 90000, 8, "f32")]
COMPOSITE_SIZES = [7, 512, 262144 + 513]


def perceptual_halves(dtype):
  return [E[dtype] * 3, E[dtype] * 257, E[dtype] * (1024 * 256 + 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: batch norm
# ---------------------------------------------------------------------------------------------------------------------------------
def run_bn_fwd(x, gamma, beta, dtype, path, lrelu=True, relu=True):
  L = _lib.lib()
  g, pg, c = x.shape
  stats = {k: out((g, c)) for k in ("scale", "shift", "mean", "rstd")}
  acts = {k: out((g, pg, c), dtype) for k, on in (("lrelu", lrelu), ("relu", relu)) if on}
  ws = workspace(ws_bytes(L, g, pg, c, dtype))
  xd, gd, bd = operand(x, dtype), operand(gamma), operand(beta)
  o = lambda k: gu.ptr(stats[k][1])
  a = lambda k: gu.ptr(acts[k][1]) if k in acts else None
  _lib.check(L.vp_bn_groups_fwd(gu.ptr(xd), g, pg, c, DT[dtype], gu.ptr(gd), gu.ptr(bd), BN_EPS, o("scale"), o("shift"), o("mean"), o("rstd"),
                                a("lrelu"), a("relu"), path, gu.ptr(ws[1]), gu.stream()), "vp_bn_groups_fwd")
  done(ws, *stats.values(), *acts.values())
  return {k: host(v[1]) for k, v in list(stats.items()) + list(acts.items())}


def check_bn_fwd(name, x, gamma, beta, dtype, path, nch):
  got = run_bn_fwd(x, gamma, beta, dtype, path)
  ref = bn_fwd_ref(x, gamma, beta, BN_EPS, nch)
  for k in ("mean", "rstd", "scale", "shift"):
    chk("bn_fwd", "%s %s" % (k, name), got[k], *ref[k])
  relu, forms = act_forms(x, f32(got["scale"]), f32(got["shift"]))
  exact("bn_fwd", "relu %s" % name, got["relu"], stored(relu, dtype))
  one_of("bn_fwd", "lrelu %s" % name, got["lrelu"], forms, dtype)
  return got, ref


@gpu
@pytest.mark.parametrize("g,pg,c,dtype,path", list(BN_CLASSES))
def test_bn_groups_fwd(g, pg, c, dtype, path):
  one, nch, ncg, trips = bn_class(g, pg, c, dtype, path)[:4]
  assert (one, nch, ncg, trips) == BN_CLASSES[(g, pg, c, dtype, path)]
  x, _ = bn_x(g, pg, c, dtype, seed=g * 1000 + pg + c)
  gamma, beta = bn_params(c, pg)
  got, ref = check_bn_fwd("%s" % ((g, pg, c, dtype, path),), x, gamma, beta, dtype, path, nch)
  if pg == 1:                                                   # zero variance: scale == 0 and shift == beta bit for bit
    assert (ref["var"][0] == 0).all()
    assert (got["scale"] == 0).all() and (got["shift"] == np.broadcast_to(beta, (g, c))).all()
    assert (got["mean"] == x[:, 0]).all() and (got["rstd"] == float(np.float32(1.0 / math.sqrt(float(np.float32(BN_EPS)))))).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_groups_fwd_forced_paths_agree(dtype):
  """One shared input through both kernels: each within its bound of the reference, and of each other within the sum of the two."""
  g, pg, c = 2, 257, 64
  assert bn_class(g, pg, c, dtype, P1)[0] and not bn_class(g, pg, c, dtype, P2)[0]
  x, _ = bn_x(g, pg, c, dtype, seed=9)
  gamma, beta = bn_params(c, 9)
  a, ra = check_bn_fwd("one launch %s" % dtype, x, gamma, beta, dtype, P1, 1)
  b, rb = check_bn_fwd("two passes %s" % dtype, x, gamma, beta, dtype, P2, bn_nchunk(pg, c, g, dtype))
  for k in ("mean", "rstd", "scale", "shift"):
    chk("bn_fwd", "paths %s %s" % (k, dtype), a[k], b[k], ra[k][1] + rb[k][1])
  bare = run_bn_fwd(x, gamma, beta, dtype, P1, lrelu=False, relu=False)              # both activation outputs null: the statistics alone
  assert all((bare[k] == a[k]).all() for k in bare) and set(bare) == {"mean", "rstd", "scale", "shift"}


@gpu
def test_bn_groups_fwd_offset_case():
  """Mean 100 .. 200, deviation 0.05: the case a float32 accumulator fails (test_float32_accumulation_violates_the_offset_case)."""
  x, c, pg = offset_case()
  one, nch = bn_class(1, pg, c, "f32", P0)[:2]
  assert not one and nch == 9
  gamma, beta = bn_params(c, 1)
  check_bn_fwd("offset", x, gamma, beta, "f32", P0, nch)


def run_bn_bwd(y, dz, mean, rstd, gamma, dtype, path, alias, accumulate, old, tail=None):
  """tail: (partial rows, raw) -> vp_bn_groups_bwd_tail."""
  L = _lib.lib()
  g, pg, c = y.shape
  yd, gd, md, rd = operand(y, dtype), operand(gamma), operand(mean), operand(rstd)
  if alias:
    dyb = out((g, pg, c), dtype, fill=dz)
    dzp = gu.ptr(dyb[1])
  else:
    dyb = out((g, pg, c), dtype)
    dzd = operand(dz, dtype)
    dzp = gu.ptr(dzd)
  c1, c2 = out((g, c)), out((g, c))
  dg, db = out((c,), fill=old[0] if accumulate else None), out((c,), fill=old[1] if accumulate else None)
  dbz = out((c,))
  if tail is None:
    ws = workspace(ws_bytes(L, g, pg, c, dtype))
    _lib.check(L.vp_bn_groups_bwd(gu.ptr(yd), dzp, gu.ptr(dyb[1]), g, pg, c, DT[dtype], gu.ptr(gd), gu.ptr(md), gu.ptr(rd), gu.ptr(c1[1]),
                                  gu.ptr(c2[1]), gu.ptr(dg[1]), gu.ptr(db[1]), gu.ptr(dbz[1]), int(accumulate), path, gu.ptr(ws[1]), gu.stream()),
               "vp_bn_groups_bwd")
    done(ws)
  else:
    rows, raw = tail
    pr = torch.tensor(rows, dtype=torch.float64, device="cuda")
    _lib.check(L.vp_bn_groups_bwd_tail(gu.ptr(yd), dzp, gu.ptr(dyb[1]), g, pg, c, DT[dtype], gu.ptr(gd), gu.ptr(md), gu.ptr(rd), gu.ptr(pr),
                                       rows.shape[1], int(raw), gu.ptr(c1[1]), gu.ptr(c2[1]), gu.ptr(dg[1]), gu.ptr(db[1]), gu.ptr(dbz[1]),
                                       int(accumulate), gu.stream()), "vp_bn_groups_bwd_tail")
    torch.cuda.synchronize()
    assert (pr.cpu().numpy() == rows).all()
  done(dyb, c1, c2, dg, db, dbz)
  assert (host(dbz[1]) == 0).all()                              # prefilled with NaN
  return {"dy": host(dyb[1]), "c1": host(c1[1]), "c2": host(c2[1]), "dgamma": host(dg[1]), "dbeta": host(db[1])}


def check_bn_bwd(name, g, pg, c, dtype, path, nch, alias, accumulate, tail_nchunk=None, raw=False):
  y, dz, mean, rstd, gamma = bn_bwd_inputs(g, pg, c, dtype, seed=g * 100 + pg + c)
  rng = np.random.default_rng(pg)
  old = (f32(rng.normal(0, 50.0, c)), f32(rng.normal(0, 50.0, c)))
  tail = None if tail_nchunk is None else (bn_partial_rows(y, dz, mean, rstd, tail_nchunk, raw), raw)
  got = run_bn_bwd(y, dz, mean, rstd, gamma, dtype, path, alias, accumulate, old, tail)
  ref = bn_bwd_ref(y, dz, mean, rstd, gamma, nch if tail is None else tail_nchunk, dtype, old if accumulate else None, raw)
  for k in ("c1", "c2", "dgamma", "dbeta", "dy"):
    chk("bn_bwd_tail" if tail else "bn_bwd", "%s %s" % (k, name), got[k], *ref[k])
  return y, dz, mean, rstd, gamma, got, ref


@gpu
@pytest.mark.parametrize("g,pg,c,dtype,path", list(BN_CLASSES))
def test_bn_groups_bwd(g, pg, c, dtype, path):
  """The forward classes again; in place (how run_bn_bwd always calls it) and with accumulate alternating over the table."""
  one, nch, ncg, trips = bn_class(g, pg, c, dtype, path)[:4]
  assert (one, nch, ncg, trips) == BN_CLASSES[(g, pg, c, dtype, path)]
  accumulate = (pg + c // 8) % 2 == 1
  check_bn_bwd("%s" % ((g, pg, c, dtype, path),), g, pg, c, dtype, path, nch, alias=True, accumulate=accumulate)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", [P1, P2])
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_bn_groups_bwd_alias_and_accumulate(dtype, path, alias, accumulate):
  g, pg, c = 2, 257, 64
  one, nch = bn_class(g, pg, c, dtype, path)[:2]
  assert one == (path == P1)
  check_bn_bwd("alias %d acc %d path %d %s" % (alias, accumulate, path, dtype), g, pg, c, dtype, path, nch, alias, accumulate)


@gpu
@pytest.mark.parametrize("g,pg,c,dtype", OVER_CAP)
def test_bn_groups_bwd_threads_cross_group_borders(g, pg, c, dtype):
  """More work than 2048 blocks: every thread of bn_bwd_apply_kernel goes on to an item of ANOTHER group and must reload its
  coefficients (`grp != cur`); the groups differ by factors of two, a stale coefficient is far outside the bound."""
  one, nch = bn_class(g, pg, c, dtype, P0)[:2]
  assert not one and bn_class(g, pg, c, dtype, P0)[4] == 2048 and g * pg * (c // E[dtype]) > 2048 * 256
  y, dz, mean, rstd, gamma, got, ref = check_bn_bwd("over cap %s" % dtype, g, pg, c, dtype, P0, nch, alias=True, accumulate=False)
  # teeth: the answer with group 0's coefficients everywhere is outside the bound on most of the other groups
  stale = (gamma * rstd[0])[None, None] * (dz - ref["c1"][0][0][None, None] - ((y - mean[0]) * rstd[0]) * ref["c2"][0][0][None, None])
  assert (np.abs(stale[1:] - ref["dy"][0][1:]) > ref["dy"][1][1:]).mean() > 0.9


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("nchunk", [1, 7, 600])
def test_bn_groups_bwd_tail(dtype, raw, nchunk):
  """Finalize + apply from caller-made partial rows (a convolution epilogue's), against the reference of the full backward."""
  g, pg, c = 2, 700, 8
  assert -(-nchunk // 512) == (2 if nchunk == 600 else 1)
  check_bn_bwd("tail nchunk %d raw %d %s" % (nchunk, raw, dtype), g, pg, c, dtype, P0, None, alias=bool(raw), accumulate=nchunk == 7,
               tail_nchunk=nchunk, raw=bool(raw))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_groups(dtype, accumulate):
  L = _lib.lib()
  g, pg, c, creal = 3, 1000, 8, 4
  nch = bn_nchunk(pg, c, g, dtype)
  assert nch == 1 and c // E[dtype] == {"f32": 2, "bf16": 1}[dtype]
  x, _ = bn_x(g, pg, c, dtype, seed=31)
  old = f32(np.random.default_rng(4).normal(0, 500.0, c))
  fill = np.where(np.arange(c) < creal, old if accumulate else np.nan, 7.25 + np.arange(c))
  ob = out((c,), fill=fill)
  ws = workspace(ws_bytes(L, g, pg, c, dtype))
  xd = operand(x, dtype)
  _lib.check(L.vp_colsum_groups(gu.ptr(xd), g, pg, c, creal, DT[dtype], gu.ptr(ob[1]), accumulate, gu.ptr(ws[1]), gu.stream()), "vp_colsum_groups")
  done(ob, ws)
  got = host(ob[1])
  assert (got[creal:] == fill[creal:]).all()                    # columns creal: of out stay untouched
  s = x.sum((0, 1))[:creal]
  bound = U * np.abs(s) + (pg + nch + g) * V * np.abs(x).sum((0, 1))[:creal]
  ref = s + old[:creal] if accumulate else s
  chk("colsum", "colsum %s acc %d" % (dtype, accumulate), got[:creal], ref, bound + (U * np.abs(ref) if accumulate else 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: act_apply, relu_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def run_act_apply(y, sc, sh, dtype, lrelu, relu):
  L = _lib.lib()
  g, pg, c = y.shape
  outs = {k: out((g, pg, c), dtype) for k, on in (("lrelu", lrelu), ("relu", relu)) if on}
  yd, scd, shd = operand(y, dtype), operand(sc), operand(sh)
  a = lambda k: gu.ptr(outs[k][1]) if k in outs else None
  _lib.check(L.vp_act_apply(gu.ptr(yd), gu.ptr(scd), gu.ptr(shd), g, pg, c, DT[dtype], a("lrelu"), a("relu"), gu.stream()), "vp_act_apply")
  done(*outs.values())
  got = {k: host(v[1]) for k, v in outs.items()}
  want_relu, forms = act_forms(y, sc, sh)
  if relu:
    exact("act_apply", "relu", got["relu"], stored(want_relu, dtype))
  if lrelu:
    one_of("act_apply", "lrelu", got["lrelu"], forms, dtype)
  return got


def act_inputs(g, pg, c, dtype, seed):
  y, _ = bn_x(g, pg, c, dtype, seed)
  rng = np.random.default_rng(seed + 1)
  sc = f32(rng.uniform(0.5, 1.5, (g, c)) * np.asarray([1.0, -3.0, 0.25])[np.arange(g) % 3][:, None])
  sh = f32(rng.normal(0, 1.0, (g, c)) + np.asarray([0.0, 4.0, -2.0])[np.arange(g) % 3][:, None])
  return y, sc, sh


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("lrelu,relu", [(True, False), (False, True), (True, True)])
def test_act_apply(dtype, affine, lrelu, relu):
  g, pg, c = 3, 301, 24                                         # 24 channels: 256 % ncg != 0 in both types, the per-item reload
  assert all(256 % (c // E[d]) != 0 for d in DTYPES) and nblocks(g * pg * (c // E[dtype])) > 1
  y, sc, sh = act_inputs(g, pg, c, dtype, seed=5)
  # planted: fma(sc, y, sh) == 0 exactly, and a negative zero
  y[0, 0, 0], y[1, 7, 3] = 1.5, -0.0
  if affine:
    sc[0, 0], sh[0, 0] = 2.0, -3.0
    sc[1, 3], sh[1, 3] = 1.0, 0.0
  got = run_act_apply(y, sc if affine else None, sh if affine else None, dtype, lrelu, relu)
  for k, v in got.items():
    assert v[1, 7, 3] == 0 and (not affine or v[0, 0, 0] == 0), k


@gpu
@pytest.mark.parametrize("g,pg,c,dtype", OVER_CAP)
def test_act_apply_threads_cross_group_borders(g, pg, c, dtype):
  assert nblocks(g * pg * (c // E[dtype])) == 2048 and g * pg * (c // E[dtype]) > 2048 * 256 and 256 % (c // E[dtype]) == 0
  y, sc, sh = act_inputs(g, pg, c, dtype, seed=6)
  got = run_act_apply(y, sc, sh, dtype, True, True)
  stale = np.maximum(fma32(sc[0][None, None], y, sh[0][None, None]), 0)
  assert (stored(stale, dtype)[1:] != got["relu"][1:]).mean() > 0.3       # teeth: group 0's coefficients everywhere is another answer


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [1, 300, 2048 * 256 + 3])
def test_relu_bwd(dtype, nvec):
  L = _lib.lib()
  n = nvec * E[dtype]
  assert nvec % 256 != 0 and (nblocks(nvec) == 2048) == (nvec > 2048 * 256)
  rng = np.random.default_rng(nvec)
  y = seen(np.maximum(rng.standard_normal(n), 0) * rng.choice([0.0, 1.0, 1e-30], n), dtype)
  y[:3] = (0.0, -0.0, 1.0)
  y[-2:] = (-0.0, 0.0)
  d = seen(rng.standard_normal(n) + 3.0, dtype)                # no zero among the gradients: a wrongly kept one shows
  db = out((n,), dtype, fill=d)
  yd = operand(y, dtype)
  _lib.check(L.vp_relu_bwd(gu.ptr(yd), gu.ptr(db[1]), n, DT[dtype], gu.stream()), "vp_relu_bwd")
  done(db)
  assert (d != 0).all() and (y[[0, 1, -2, -1]] == 0).all()
  exact("relu_bwd", "relu_bwd %s %d" % (dtype, nvec), host(db[1]), np.where(y > 0, d, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: tap gather / spread, pack_inputs
# ---------------------------------------------------------------------------------------------------------------------------------
TAP_SHAPES = [(2, 5, 7, 1), (1, 30, 30, 1)]


@gpu
@pytest.mark.parametrize("n,hin,win,pad", TAP_SHAPES)
def test_tap_gather(n, hin, win, pad):
  L = _lib.lib()
  ks, hout, wout = 4, hin + 2 * pad - 3, win + 2 * pad - 3
  assert (n * hout * wout > 256) == (hin == 30)                  # one block / more than one
  rng = np.random.default_rng(hin)
  s = f32(rng.standard_normal((n, hin, win, 16)) * 10.0 ** rng.integers(-3, 4, (n, hin, win, 16)))
  bias = f32([0.37])
  acc = np.zeros((n, hout, wout), np.float32)
  sp = np.pad(s.astype(np.float32), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
  inside = np.pad(np.ones((hin, win), bool), pad)
  for kh in range(ks):
    for kw in range(ks):
      ok = inside[kh:kh + hout, kw:kw + wout]                    # a border tap is skipped, not read
      acc = np.where(ok, acc + sp[:, kh:kh + hout, kw:kw + wout, kh * ks + kw], acc)
  want = acc + np.float32(bias[0])
  yb = out((n, hout, wout))
  sd, bd = operand(s), operand(bias)
  _lib.check(L.vp_tap_gather(gu.ptr(sd), gu.ptr(bd), gu.ptr(yb[1]), n, hin, win, ks, pad, gu.stream()), "vp_tap_gather")
  done(yb)
  exact("tap_gather", "tap_gather %s" % ((n, hin, win),), host(yb[1]), want)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,hin,win,pad", TAP_SHAPES)
def test_tap_spread(n, hin, win, pad, dtype):
  L = _lib.lib()
  ld, hout, wout = 8, hin + 2 * pad - 3, win + 2 * pad - 3
  assert ((n * hin * win + 255) // 256 > 1) == (hin == 30)         # one thread per input pixel: one block / more than one
  rng = np.random.default_rng(win)
  dy = np.full((n, hout, wout, ld), 768.0)                       # channels 1:8: a sentinel that must never show up
  dy[..., 0] = seen(rng.standard_normal((n, hout, wout)) + 5.0, dtype)
  want = np.zeros((n, hin, win, 16))
  for t in range(16):
    for qi in range(hin):
      i = qi - t // 4 + pad
      if 0 <= i < hout:
        j = np.arange(win) - t % 4 + pad
        ok = (j >= 0) & (j < wout)
        want[:, qi, ok, t] = dy[:, i, j[ok], 0]
  ob = out((n, hin, win, 16), dtype)
  dyd = operand(dy, dtype)
  _lib.check(L.vp_tap_spread(gu.ptr(dyd), ld, gu.ptr(ob[1]), n, hin, win, pad, DT[dtype], gu.stream()), "vp_tap_spread")
  done(ob)
  got = host(ob[1])
  assert (got != 768.0).all() and (want == 0).any() and (dy[..., 0] != 0).all()
  exact("tap_spread", "tap_spread %s %s" % ((n, hin, win), dtype), got, want)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fg_c", [6, 3])
@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("n,hw", [(1, 7), (3, 174763)])
def test_pack_inputs(dtype, fg_c, train, n, hw):
  L = _lib.lib()
  total = n * hw
  assert (nblocks(total) == 2048 and total == 2048 * 256 + 1) if hw > 7 else total == 7
  rng = np.random.default_rng(total + fg_c)
  inp, fg = rng.random((total, 6), dtype=np.float32), rng.random((total, fg_c), dtype=np.float32)
  inp[0], fg[0, :3] = (0.0, 1.0, 0.5, 0.25, 0.75, 1.0), (0.5, 0.0, 1.0)
  i2 = inp * np.float32(2) - np.float32(1)                       # 2 x is exact: one rounding, contracted or not
  f2 = np.concatenate([fg * np.float32(2) - np.float32(1), np.full((total, 6 - fg_c), -1.0, np.float32)], 1)
  z = np.zeros((total, 1), np.float32)
  cat = lambda *cols: np.concatenate(cols + (z,) * (8 - sum(a.shape[1] for a in cols)), 1)
  want = {"gin": cat(i2), "gfg": cat(f2[:, :3]),
          "din": np.stack([cat(i2[:, 3:], f2[:, 3:]), cat(i2[:, :3], f2[:, :3]), cat(i2[:, 3:])]), "vin": cat(f2[:, 3:])}
  bufs = {"gin": out((total, 8), dtype), "gfg": out((total, 8), dtype), "din": out((3, total, 8), dtype), "vin": out((2, total, 8), dtype)}
  a, b = operand(inp), operand(fg)
  _lib.check(L.vp_pack_inputs(gu.ptr(a), gu.ptr(b), fg_c, *[gu.ptr(bufs[k][1]) for k in ("gin", "gfg", "din", "vin")], n, hw, train, DT[dtype],
                              gu.stream()), "vp_pack_inputs")
  done(*bufs.values())
  name = "pack_inputs %s fg_c %d train %d n %d" % (dtype, fg_c, train, total)
  exact("pack_inputs", "gin " + name, host(bufs["gin"][1]), stored(want["gin"], dtype))
  exact("pack_inputs", "gfg " + name, host(bufs["gfg"][1]), stored(want["gfg"], dtype))
  assert bool(torch.isnan(bufs["vin"][1][1]).all())              # the fake half is the composite's to write
  if train:
    exact("pack_inputs", "din " + name, host(bufs["din"][1]), stored(want["din"], dtype))
    exact("pack_inputs", "vin " + name, host(bufs["vin"][1][0]), stored(want["vin"], dtype))
    if fg_c == 3:
      assert (host(bufs["din"][1])[0, :, 3:6] == -1).all()
  else:
    assert bool(torch.isnan(bufs["din"][1]).all()) and bool(torch.isnan(bufs["vin"][1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: composite forward (train) and backward
# ---------------------------------------------------------------------------------------------------------------------------------
def composite_inputs(total, seed):
  rng = np.random.default_rng(seed)
  y4 = f32(np.clip(rng.normal(0, 1.5, (total, 4)), -8, 8))
  return y4, f32(rng.random((total, 3))), f32(rng.random((total, 3)))


def composite_fwd_ref(y4, tgt, msk):
  o = np.tanh(y4)
  d = K_TANH * U * np.abs(o)
  al = (o[:, 3:] + 1) / 2
  b_al = d[:, 3:] / 2 + U * np.abs(al)
  tg = 2 * tgt - 1
  b_tg = U * np.abs(tg)
  oc, dc = o[:, :3], d[:, :3]
  outv = oc * al + tg * (1 - al)
  b_out = al * dc + np.abs(oc - tg) * b_al + np.abs(1 - al) * b_tg + U * np.abs(1 - al) * np.abs(tg) + U * (np.abs(oc * al) + np.abs(tg * (1 - al))) + U * np.abs(outv)
  ofg = oc * al + al - 1
  b_ofg = al * dc + np.abs(oc + 1) * b_al + U * np.abs(oc * al) + U * np.abs(oc * al + al) + U * np.abs(ofg)
  t0, t1 = np.abs(tg - outv), np.abs(msk - al)
  e0, e1 = b_tg + b_out + U * t0, b_al + U * t1
  return {"o4": (o, d), "outputs": (outv, b_out), "outputs_fg": (ofg, b_ofg)}, (t0.sum(), e0.sum()), (t1.sum(), e1.sum())


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("total", COMPOSITE_SIZES)
def test_composite_fwd_train(dtype, total):
  L = _lib.lib()
  nb = composite_nblocks(1, total)
  assert L.vp_composite_nblocks(1, total) == nb and nb == {7: 1, 512: 2}.get(total, 1024) and (total <= 512 or total > 1024 * 256)
  y4, tgt, msk = composite_inputs(total, total)
  ref, s0, s1 = composite_fwd_ref(y4.astype(np.float64), tgt.astype(np.float64), msk.astype(np.float64))
  rng = np.random.default_rng(1)
  din0 = seen(rng.standard_normal((3, total, 8)), dtype)          # the pattern pack_inputs would have left: channels 0:3 of the fake group stay
  vin0 = seen(rng.standard_normal((2, total, 8)), dtype)
  bufs = {"o4": out((total, 4)), "outputs": out((total, 3)), "outputs_fg": out((total, 3)), "din": out((3, total, 8), dtype, fill=din0),
          "vin": out((2, total, 8), dtype, fill=vin0)}
  pw, pv = f64_out(2 * nb + 6)
  a, b, c = operand(y4), operand(tgt), operand(msk)
  _lib.check(L.vp_composite_fwd_train(gu.ptr(a), gu.ptr(b), gu.ptr(c), *[gu.ptr(bufs[k][1]) for k in ("o4", "outputs", "outputs_fg", "din", "vin")],
                                      gu.ptr(pv), 1, total, DT[dtype], gu.stream()), "vp_composite_fwd_train")
  done(*bufs.values())
  assert_f64_guards(pw)
  got = {k: host(v[1]) for k, v in bufs.items()}
  name = "%s n %d" % (dtype, total)
  for k in ("o4", "outputs", "outputs_fg"):
    chk("composite_fwd", "%s %s" % (k, name), got[k], *ref[k])
  # hand-over rows: bit-equal to the kernel's own outputs_fg, rounded by the store
  fg = stored(got["outputs_fg"], dtype)
  assert (got["din"][:2] == din0[:2]).all() and (got["vin"][0] == vin0[0]).all()
  exact("composite_fwd", "din head " + name, got["din"][2][:, :3], din0[2][:, :3])
  exact("composite_fwd", "din fg " + name, got["din"][2][:, 3:6], fg)
  exact("composite_fwd", "vin fg " + name, got["vin"][1][:, :3], fg)
  assert (got["din"][2][:, 6:] == 0).all() and (got["vin"][1][:, 3:] == 0).all()
  part = pv.cpu().numpy()
  assert np.isnan(part[2 * nb:]).all() and np.isfinite(part[:2 * nb]).all()          # partial beyond nblocks stays untouched
  part = part[:2 * nb].reshape(nb, 2)
  for j, (s, e) in enumerate((s0, s1)):
    chk("composite_fwd", "partial %d %s" % (j, name), np.array([math.fsum(part[:, j])]), np.array([s]), np.array([f64_sum_bound(3 * total, nb, s) + e]))


def composite_bwd_case(total, dtype, l1w):
  rng = np.random.default_rng(total + 3)
  o4 = f32(np.tanh(rng.normal(0, 1.5, (total, 4))))
  tgt, msk = f32(rng.random((total, 3))), f32(rng.random((total, 3)))
  outp = f32(rng.uniform(-1, 1, (total, 3)))
  dd = seen(rng.normal(0, 1e-5, (total, 8)), dtype)
  dv = seen(rng.normal(0, 1e-5, (total, 8)), dtype)
  tg32 = (tgt.astype(np.float32) * np.float32(2) - np.float32(1)).astype(np.float64)
  # planted: |o| == 1 (saturated tanh), the ties out == tg and mask == alpha
  o4[0] = (1.0, -1.0, 0.5, 1.0)
  o4[total // 2] = (0.25, 1.0, -1.0, -1.0)
  al32 = ((o4[:, 3].astype(np.float32) + np.float32(1)) * np.float32(0.5)).astype(np.float64)
  ties = np.arange(0, total, 5)
  outp[ties, 1] = tg32[ties, 1]
  msk[ties, 2] = al32[ties]
  dd[ties[::2], 4], dv[ties[::2], 1] = 0.0, 0.0
  return o4, tgt, msk, outp, dd, dv, tg32, al32, ties


def composite_bwd_ref(o4, msk, outp, dd, dv, tg, al, l1w, dtype):
  total = o4.shape[0]
  s = float(np.float32(l1w) / np.float32(float(total) * 3.0))
  d_out = -s * np.sign(tg - outp)
  d_al = -s * np.sign(msk - al[:, None])
  d_fg = dd[:, 3:6] + dv[:, 0:3]
  t = 1 - o4 * o4
  e_t = U * o4 * o4 + U * np.abs(t)
  sm = d_out + d_fg
  v = sm * al[:, None] * t[:, :3]
  b = np.abs(al[:, None] * t[:, :3]) * (U * np.abs(d_fg) + U * np.abs(sm)) + np.abs(sm * al[:, None]) * e_t[:, :3] + 2 * U * np.abs(v)
  oc = o4[:, :3]
  t1, t2 = d_out * (oc - tg), d_fg * (oc + 1)
  dal = (t1 + t2 + d_al).sum(1)
  b_dal = 12 * U * (np.abs(t1) + np.abs(t2) + np.abs(d_al)).sum(1)
  v3 = dal * 0.5 * t[:, 3]
  b3 = np.abs(0.5 * t[:, 3]) * b_dal + np.abs(0.5 * dal) * e_t[:, 3] + U * np.abs(v3)
  ref = np.concatenate([v, v3[:, None], np.zeros((total, 4))], 1)
  bound = np.concatenate([b, b3[:, None], np.zeros((total, 4))], 1)
  return ref, st(bound, ref, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("total", COMPOSITE_SIZES)
def test_composite_bwd(dtype, total):
  from voicepuppet_amd.pixrefer.pixrefer import PixReferNet
  L = _lib.lib()
  l1w = float(PixReferNet(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "params.yml")).params.l1_weight)
  assert l1w == 500.0 and (nblocks(total) > 1) == (total > 256)
  o4, tgt, msk, outp, dd, dv, tg32, al32, ties = composite_bwd_case(total, dtype, l1w)
  ref, bound = composite_bwd_ref(o4.astype(np.float64), msk.astype(np.float64), outp.astype(np.float64), dd, dv, tg32, al32, l1w, dtype)
  ob = out((total, 8), dtype)
  ops = [operand(o4), operand(tgt), operand(msk), operand(outp), operand(dd, dtype), operand(dv, dtype)]
  _lib.check(L.vp_composite_bwd(*[gu.ptr(x) for x in ops], gu.ptr(ob[1]), 1, total, l1w, DT[dtype], gu.stream()), "vp_composite_bwd")
  done(ob)
  got = host(ob[1])
  chk("composite_bwd", "dy4 %s n %d" % (dtype, total), got, ref, bound)
  assert (got[:, 4:] == 0).all()
  assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, 3] == 0 and got[total // 2, 1] == 0 and got[total // 2, 2] == 0       # |o| == 1
  # a tie with a zero incoming gradient contributes exactly 0
  z = ties[::2]
  assert (got[z, 1] == 0).all() and (np.sign(tg32 - outp)[ties, 1] == 0).all() and (np.sign(msk - al32[:, None])[ties, 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: perceptual, loss_final, gan_loss
# ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_perceptual(dtype, which):
  L = _lib.lib()
  half = perceptual_halves(dtype)[which]
  nb = perceptual_nblocks(half, dtype)
  assert L.vp_perceptual_nblocks(half, DT[dtype]) == nb == [1, 2, 1024][which]
  rng = np.random.default_rng(half)
  f = seen(np.maximum(rng.normal(0.3, 1.0, (2, half)), 0), dtype)          # post-relu: about a third zeros
  f[1, 0], f[0, 1], f[1, 1] = 0.0, 0.75, 0.75                              # planted fb == 0 (with fa != 0), fa == fb
  f[0, 0] = 1.5
  l1w = 500.0
  s = float(np.float32(l1w) / np.float32(half))
  x = f[0] - f[1]
  ref = np.where(f[1] > 0, -s * x, 0.0)
  x32 = x.astype(np.float32).astype(np.float64)
  p = -s * x32
  exact_here = (x32 == x) & (p.astype(np.float32).astype(np.float64) == p)
  bound = np.where(exact_here & (dtype == "f32"), 0.0, st(2 * U * np.abs(ref), ref, dtype))
  ob = out((half,), dtype)
  pw, pv = f64_out(nb + 4)
  fd = operand(f, dtype)
  _lib.check(L.vp_perceptual(gu.ptr(fd), gu.ptr(ob[1]), gu.ptr(pv), half, l1w, DT[dtype], gu.stream()), "vp_perceptual")
  done(ob)
  assert_f64_guards(pw)
  got = host(ob[1])
  name = "%s half %d" % (dtype, half)
  assert got[0] == 0 and got[1] == 0 and (f[1] == 0).mean() > 0.2 and exact_here.mean() > 0.05
  chk("perceptual", "df3 " + name, got, ref, bound)
  if dtype == "bf16":                                                       # where the float32 product is exact the store's rounding is all
    exact("perceptual", "df3 exact " + name, got[exact_here], stored(np.where(f[1] > 0, p, 0.0)[exact_here], dtype))
  part = pv.cpu().numpy()
  assert np.isnan(part[nb:]).all()
  tot = float((x * x).sum())
  chk("perceptual", "partial " + name, np.array([math.fsum(part[:nb])]), np.array([tot]), np.array([2 * U * tot + f64_sum_bound(half, nb, tot)]))


@gpu
@pytest.mark.parametrize("n_comp,n_perc", [(1, 1), (255, 1030), (1030, 255)])
def test_loss_final(n_comp, n_perc):
  L = _lib.lib()
  assert sorted({-(-n_comp // 256), -(-n_perc // 256)}) in ([1], [1, 5])      # trips of the one block's two loops
  rng = np.random.default_rng(n_comp)
  comp, perc = rng.uniform(0, 900.0, (n_comp, 2)), rng.uniform(0, 4e4, n_perc)
  n_out, n_feat, l1w, gw = 3.0 * 65536, 64.0 * 64 * 256, 500.0, 1.0
  prefill = np.full(8, SENTINEL)
  prefill[:2] = (1.386, 0.693)
  prefill[2:5] = np.nan
  lb = out((8,), fill=prefill)
  cd, pd = torch.tensor(comp, device="cuda"), torch.tensor(perc, device="cuda")
  _lib.check(L.vp_loss_final(gu.ptr(cd), n_comp, gu.ptr(pd), n_perc, n_out, n_feat, l1w, gw, gu.ptr(lb[1]), gu.stream()), "vp_loss_final")
  done(lb)
  got = host(lb[1])
  l1 = float(np.float32(prefill[1]))
  assert (got[:2] == f32(prefill[:2])).all() and (got[5:] == SENTINEL).all()
  content = math.fsum(perc) / 2 / n_feat
  gl1 = math.fsum(comp[:, 0]) / n_out + math.fsum(comp[:, 1]) / n_out + content
  sb = (max(n_comp, n_perc) / 256 + 10) * V
  ref = np.array([gl1, l1 * gw + gl1 * l1w, content])
  mag = np.array([gl1, l1 * gw + gl1 * l1w, content])
  chk("loss_final", "losses n %d %d" % (n_comp, n_perc), got[2:5], ref, 2 * U * np.abs(ref) + sb * mag)


def sigmoid(a):
  return 1.0 / (1.0 + np.exp(-a))


def gan_ref(a, gw, dtype):
  """{name: (reference, bound)} of vp_gan_loss for logits a [3, M] (float64 of float32 values)."""
  m = a.shape[1]
  eps = float(np.float32(1e-12))
  inv_m = float(np.float32(1) / np.float32(m))
  p, om = sigmoid(a), sigmoid(-a)                                # om = 1 - p without the cancellation
  dp = K_SIG * U * p + np.where(a >= 40, np.exp(-np.abs(a)), 0.0) + np.where(a <= -87, np.exp(-np.abs(a)), 0.0)
  pr, b_pr = (p[0] + p[1]) / 2, (dp[0] + dp[1]) / 2 + U * (p[0] + p[1]) / 2
  pf, dpf, omf = p[2], dp[2], om[2]
  q_pr, q_om, q_pf = pr + eps, omf + eps, pf + eps
  b_qpr, b_om = b_pr + U * q_pr, dpf + U * omf
  b_qom, b_qpf = b_om + U * q_om, dpf + U * q_pf
  lerr = lambda q, bq: bq / q + K_LOG * U * np.abs(np.log(q))
  t0 = -(2 * np.log(q_pr) + np.log(q_om))
  e0 = 2 * lerr(q_pr, b_qpr) + lerr(q_om, b_qom) + U * np.abs(t0)
  t1 = -np.log(q_pf)
  e1 = lerr(q_pf, b_qpf)
  loss = np.array([t0.mean(), t1.mean()])
  b_loss = U * np.abs(loss) + np.array([e0.mean(), e1.mean()]) + (m / 1024 + 10) * V * np.array([np.abs(t0).mean(), np.abs(t1).mean()])
  rel_p = lambda i: dp[i] / p[i] + U
  rel_om = lambda i: (dp[i] + U * om[i]) / om[i] + U
  dpr = -2 / q_pr * inv_m * 0.5
  seed_d = np.stack([dpr * p[0] * om[0], dpr * p[1] * om[1], 1 / q_om * inv_m * pf * omf])
  rel_d = np.stack([b_qpr / q_pr + 4 * U + rel_p(0) + rel_om(0), b_qpr / q_pr + 4 * U + rel_p(1) + rel_om(1), b_qom / q_om + 3 * U + rel_p(2) + rel_om(2)])
  seed_g = gw * (-1 / q_pf) * inv_m * pf * omf
  rel_g = b_qpf / q_pf + 4 * U + rel_p(2) + rel_om(2)
  return {"predict": (np.stack([pr, pf]), np.stack([b_pr, dpf])), "losses": (loss, b_loss),
          "seed_d": (seed_d, st(np.abs(seed_d) * rel_d + 4 * ETA, seed_d, dtype)), "seed_g": (seed_g, st(np.abs(seed_g) * rel_g + 4 * ETA, seed_g, dtype))}


def run_gan_loss(a, gw, dtype):
  L = _lib.lib()
  m = a.shape[1]
  bufs = {"seed_d": out((3, m, 8), dtype), "seed_g": out((m, 8), dtype), "predict": out((2, m)), "losses": out((2,))}
  ad = operand(a)
  _lib.check(L.vp_gan_loss(gu.ptr(ad), *[gu.ptr(bufs[k][1]) for k in ("seed_d", "seed_g", "predict", "losses")], m, gw, DT[dtype], gu.stream()), "vp_gan_loss")
  done(*bufs.values())
  return {k: host(v[1]) for k, v in bufs.items()}


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 900, 1025, 28800])
def test_gan_loss(dtype, m):
  """Random logits in [-8, 8] and, from M = 900 on, saturated plants at +-50 and +-100 in every row.  Not covered: 17 < |a| < 40 (module
  docstring: fl32(1 - p) jumps between neighbouring multiples of u there, the float32 formula has no small error to hold it to)."""
  assert (-(-m // 1024) > 1) == (m > 1024)                      # the one block's loop runs a second time
  a = f32(np.random.default_rng(m).uniform(-8, 8, (3, m)))
  if m >= 900:
    for row in range(3):
      a[row, 10 * row + np.arange(4)] = (50.0, -50.0, 100.0, -100.0)
  gw = 1.0
  got = run_gan_loss(a, gw, dtype)
  ref = gan_ref(a.astype(np.float64), gw, dtype)
  assert all(np.isfinite(v).all() for v in got.values())
  for k in ("predict", "losses"):
    chk("gan_loss", "%s %s m %d" % (k, dtype, m), got[k], *ref[k])
  for k in ("seed_d", "seed_g"):
    chk("gan_loss", "%s %s m %d" % (k, dtype, m), got[k][..., 0], *ref[k])
    assert (got[k][..., 1:] == 0).all()


@gpu
def test_function_errors_as_measured():
  """tanhf through composite_fwd's o4, 1 / (1 + expf(-a)) through gan_loss's predict, logf through the loss of one-element calls
  (against the call's own predict): worst |err| / (u |ref|) over the input range of the cases, at most the figures of the module
  docstring.  Twice each figure is what the bounds allow."""
  L = _lib.lib()
  n = 1 << 17
  grid = f32(np.linspace(-8, 8, n * 4).reshape(n, 4))
  bufs = [out((n, 4)), out((n, 3)), out((n, 3))]
  z = operand(np.zeros((n, 3)))
  gd = operand(grid)
  _lib.check(L.vp_composite_fwd(gu.ptr(gd), gu.ptr(z), *[gu.ptr(b[1]) for b in bufs], 1, n, gu.stream()), "vp_composite_fwd")
  done(*bufs)
  r = np.tanh(grid.astype(np.float64))
  with np.errstate(divide="ignore", invalid="ignore"):
    e_tanh = np.nanmax(np.where(r != 0, np.abs(host(bufs[0][1]) - r) / (U * np.abs(r)), 0.0))
  m = 28800
  a = f32(np.linspace(-8, 8, 3 * m).reshape(3, m))
  got = run_gan_loss(a, 1.0, "f32")
  pf = sigmoid(a[2].astype(np.float64))
  e_sig = np.max(np.abs(got["predict"][1] - pf) / (U * pf))
  # logf: M = 1, real logits 0; losses[1] = fl32(-logf(pf + eps)) with pf the call's own predict
  k = 512
  al = f32(np.stack([np.zeros(k), np.zeros(k), np.linspace(-8, 8, k)], 1))
  ad = torch.tensor(al, device="cuda")
  sd, sg = torch.zeros(3 * 8, device="cuda"), torch.zeros(8, device="cuda")
  pred, loss = torch.zeros(k, 2, device="cuda"), torch.zeros(k, 2, device="cuda")
  for i in range(k):
    _lib.check(L.vp_gan_loss(ctypes.c_void_p(ad.data_ptr() + 12 * i), gu.ptr(sd), gu.ptr(sg), ctypes.c_void_p(pred.data_ptr() + 8 * i),
                             ctypes.c_void_p(loss.data_ptr() + 8 * i), 1, 1.0, VP_F32, gu.stream()), "vp_gan_loss")
  pred, loss = host(pred), host(loss)
  q = (pred[:, 1].astype(np.float32) + np.float32(1e-12)).astype(np.float64)
  r = -np.log(q)
  ok = np.abs(r) > 1e-3                                          # (next to log 1 = 0 the measure |err| / |ref| has no meaning)
  e_log = np.max(np.abs(loss[ok, 1] - r[ok]) / (U * np.abs(r[ok])))
  print("\nMEASURED tanhf %.3f   sigmoid %.3f   logf %.3f   (u |ref|)" % (e_tanh, e_sig, e_log))
  assert e_tanh <= TANH_MEASURED and e_sig <= SIG_MEASURED and e_log <= LOG_MEASURED, (e_tanh, e_sig, e_log)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: vp_adam_tf, the bf16 gradient transport
# ---------------------------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, lr_t, b1, b2, eps):
  m1 = b1 * m + (1 - b1) * g
  e_m = U * (np.abs(b1 * m) + np.abs((1 - b1) * g)) + U * np.abs(m1) + 2 * ETA
  v1 = b2 * v + (1 - b2) * g * g
  e_v = U * (np.abs(b2 * v) + 2 * (1 - b2) * g * g) + U * v1 + 3 * ETA
  sq = np.sqrt(v1)
  den = sq + eps
  q = lr_t * m1 / den
  with np.errstate(divide="ignore", invalid="ignore"):
    e_sq = np.where(v1 > 0, e_v / (2 * sq), 0.0)
  p1 = p - q
  e_p = U * np.abs(p1) + np.abs(q) * (5 * U + (e_sq + 2 * U * sq) / den) + lr_t * e_m / den
  return {"p": (p1, e_p), "m": (m1, e_m), "v": (v1, e_v)}


@gpu
@pytest.mark.parametrize("n", [1, 7, 1020, 4096 * 256 + 5])
@pytest.mark.parametrize("t0", [1, 1000])
def test_adam_tf(n, t0):
  """Three consecutive steps (t0, t0 + 1, t0 + 2) from the device's own state, each against the reference started from that state."""
  L = _lib.lib()
  assert (nblocks(n, 4096) == 4096) == (n > 4096 * 256)
  lr, b1, b2, eps = (float(np.float32(x)) for x in (2e-4, 0.5, 0.999, 1e-8))
  assert float(np.float32(1) - np.float32(b2)) == 1 - b2 and 1 - b1 == 0.5            # 1 - beta is exact in float32
  rng = np.random.default_rng(n + t0)
  p0 = f32(rng.standard_normal(n))
  m0 = f32(rng.normal(0, 0.01, n)) if t0 > 1 else np.zeros(n)
  v0 = f32(rng.normal(0, 0.01, n) ** 2) if t0 > 1 else np.zeros(n)
  bufs = [out((n,), fill=a) for a in (p0, np.zeros(n), m0, v0)]
  state = [p0, None, m0, v0]
  for step in range(3):
    g = f32(np.random.default_rng(n + 10 * step).normal(0, 0.02, n))
    for i, val in enumerate((0.0, 0.0, 1e-20, -3e-21, 1e15, -4e14)):          # g == 0 (twice), g^2 subnormal, large |g|
      if i < n:
        g[i] = np.float32(val)
    bufs[1][1].copy_(torch.tensor(g, dtype=torch.float32))
    t = t0 + step
    lr_t = float(np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))
    ref = adam_ref(state[0], g, state[2], state[3], lr_t, b1, b2, eps)
    _lib.check(L.vp_adam_tf(*[gu.ptr(b[1]) for b in bufs], n, t, lr, b1, b2, eps, gu.stream()), "vp_adam_tf")
    done(*bufs)
    new = [host(b[1]) for b in bufs]
    assert (new[1] == g).all()
    for k, i in (("m", 2), ("v", 3), ("p", 0)):
      chk("adam_tf", "%s n %d t %d" % (k, n, t), new[i], *ref[k])
    zero = (g == 0) & (state[2] == 0) & (state[3] == 0)
    assert (new[0][zero] == state[0][zero]).all() and (new[2][zero] == 0).all() and (new[3][zero] == 0).all()
    assert zero.any() or t0 > 1
    state = new


def pack_plants():
  """float32 values whose bf16 rounding is decided by the rule: halfway cases of both parities, just off them, the largest finite
  value (rounds to inf), signed zeros, infinities, subnormals (halfway too)."""
  bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F817FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000,
          0x7F800000, 0xFF800000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x3F80FFFF, 0x00008001]
  return np.array(bits, np.uint32).view(np.float32)


def pack_values(n):
  x = f32(np.random.default_rng(n).standard_normal(n) * 3.0).astype(np.float32)
  pl = np.roll(pack_plants(), n)
  k = min(n, len(pl))
  x[:k] = pl[:k]
  x[n - k:] = pl[len(pl) - k:]                                   # the tail (n % 8 elements) holds plants too
  return x


PACK_SIZES = list(range(1, 10)) + [15, (1 << 20) + 5]


@gpu
@pytest.mark.parametrize("n", PACK_SIZES)
def test_grad_pack_bf16(n):
  L = _lib.lib()
  assert (n // 8 == 0) == (n < 8) and (n % 8 > 0 or n == 8) and (n < 16 or n % 8 == 5)          # vectors and a tail (n = 8: no tail)
  x = pack_values(n)
  src = torch.tensor(x, device="cuda")
  db = out((n,), "bf16")                                         # the guard band starts at element n: the tail writes n % 8 elements, not 8
  _lib.check(L.vp_grad_pack_bf16(gu.ptr(src), gu.ptr(db[1]), n, gu.stream()), "vp_grad_pack_bf16")
  done(db)
  got = db[1].view(torch.int16).cpu().numpy().view(np.uint16)
  want = (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)
  print("\nRATIO grad_pack_bf16 %.4f   (n %d)" % (0.0 if (got == want).all() else np.inf, n))
  assert (got == want).all(), (n, np.argwhere(got != want)[:8].tolist())


@gpu
@pytest.mark.parametrize("n", PACK_SIZES)
@pytest.mark.parametrize("scale", [0.125, 1.0 / 3.0])
def test_grad_unpack_bf16(n, scale):
  L = _lib.lib()
  scale = float(np.float32(scale))
  assert (n // 8 == 0) == (n < 8) and (n % 8 > 0 or n == 8) and nblocks(n // 8 + 1, 4096) == (513 if n > 15 else 1)
  x = bf16_round(pack_values(n))
  src = torch.tensor((x.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16).to("cuda").contiguous()
  ob = out((n,))
  _lib.check(L.vp_grad_unpack_bf16(gu.ptr(src), gu.ptr(ob[1]), n, scale, gu.stream()), "vp_grad_unpack_bf16")
  done(ob)
  got = ob[1].cpu().numpy().view(np.uint32)
  want = (x * np.float32(scale)).view(np.uint32)                # one IEEE product (exact for 0.125 above the subnormals)
  print("\nRATIO grad_unpack_bf16 %.4f   (n %d)" % (0.0 if (got == want).all() else np.inf, n))
  assert (got == want).all(), (n, scale, np.argwhere(got != want)[:8].tolist())


@gpu
def test_grad_transport_refuses_misaligned_pointers():
  L = _lib.lib()
  f = torch.ones(64, device="cuda")
  h = torch.full((64,), float("nan"), dtype=torch.bfloat16, device="cuda")
  o = torch.full((64,), float("nan"), device="cuda")
  S = gu.stream()
  off = lambda t, nbytes: ctypes.c_void_p(t.data_ptr() + nbytes)
  assert L.vp_grad_pack_bf16(off(f, 4), gu.ptr(h), 8, S) == VP_ERR_ARG and L.vp_grad_pack_bf16(off(f, 16), gu.ptr(h), 8, S) == VP_ERR_ARG
  assert L.vp_grad_pack_bf16(gu.ptr(f), off(h, 2), 8, S) == VP_ERR_ARG and L.vp_grad_pack_bf16(gu.ptr(f), off(h, 8), 8, S) == VP_ERR_ARG
  assert L.vp_grad_unpack_bf16(off(h, 2), gu.ptr(o), 8, 1.0, S) == VP_ERR_ARG and L.vp_grad_unpack_bf16(gu.ptr(h), off(o, 16), 8, 1.0, S) == VP_ERR_ARG
  assert L.vp_grad_pack_bf16(gu.ptr(f), gu.ptr(h), 0, S) == VP_ERR_ARG and L.vp_last_error().startswith(b"vp_grad_pack_bf16:")
  torch.cuda.synchronize()
  assert bool(torch.isnan(h.float()).all()) and bool(torch.isnan(o).all())

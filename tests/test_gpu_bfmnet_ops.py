"""Op-level float64 parity of the hand-written kernels of the BFMNet trunk (the audio counterpart of test_gpu_ops.py +
test_gpu_coverage.py): dwproj_kernel (csrc/bfm_dwproj.hip, all nine instantiations), dwconv7x3_f32_kernel / dwconv7x3_kernel<bf16>
(forward with bias + ReLU6 in both storage types, raw forward, backward-data) and conv_first_kernel, each against oracle/audio_ref.py.

Rules common to every GPU case
  * the device sees float32 values (bf16 storage: bf16-rounded values, gpu_util.rounded); the reference is float64 of those values;
  * outputs are prefilled with NaN (add = 1: with a random residual that is part of the reference) and sit between two guard bands of a
    sentinel, each at least one image row long, that must come back untouched;
  * the clips of a batch differ in seed and scale (CLIP_SCALES), so a row read from the neighbouring clip cannot cancel;
  * the comparison is PER ELEMENT against a forward-error bound computed in float64 next to the reference, u = 2^-24:
      depthwise / stem   a sum of n products, bias first, f32 FMAs:     |got - ref| <= (n + 2) u (|b| + sum |w||x|), n = 21 / 45
                         (n roundings: gamma_n = n u / (1 - n u) < (n + 2) u; the raw forward and backward-data have b = 0)
      dwproj             |got - ref| <= (ce + 21 + 4) u (|b_proj| + |y0| + sum_k |W_kj| D_ik), D_ik = the float64 depthwise + ReLU6 value
                         plus its own bound from the line above (ce products + bias + residual, and the operand's own 21 + 2)
      ReLU / ReLU6       1-Lipschitz: the bound passes through them, no element near a kink is excluded
      bf16 storage       + 2^-8 |ref| for the final rounding
    The bounds are derived, not fitted to the kernels.  (The dwproj line carries the error of D only through the factor D + bound(D); a
    strict worst case would add sum_k |W_kj| bound(D_ik) once more.  The stated line is the tighter of the two and is the one asserted.)
  * the depthwise pre-activation lands in all three ReLU6 regimes - at least 10 % below 0, 10 % above 6, 30 % between, asserted on the
    float64 reference of every dwproj and bias + ReLU6 case: the folded bias is spread over [-3, 9] per channel and the taps give the
    sum a standard deviation of about 2.5 at clip scale 1, so the shares hold even where SAME padding leaves one tap (H = W = 1).

Reduced case tables (the full cross products need not run; every value of every axis meets every kernel)
  dwproj   DWPROJ_TRIPLES = the ten (W, ce, cout) the net runs + (20, 16, 64) and (20, 32, 64): the one- and two-chunk edges of the
           double-buffered K loop on the <20, 4, 1> instantiation.  Each triple runs EVERY H class of its instantiation - 5, TR - 1, TR,
           TR + 1, 125, 5 T_win (TR = rows per tile: 2 / 4 / 8 / 16 for W = 40 / 20 / 10 / 5 and 3; T_win from
           stream_context(stream_desc(1)); duplicates dropped) - and (B, add) walks (1, 0), (3, 1), (1, 1), (3, 0) down the H classes, so
           each triple meets B = 1 and 3 and add = 0 and 1.  One more case sits just under the 0xF0000000-byte limit of the kernel's 32-bit
           lane offsets ((64, 1023, 40, 384, 64): 4 022 599 680 bytes), and B = 65 of it must be refused before any launch.
  unfused  UNFUSED_CASES, ten (B, H, W, C), run by all four entry points (vp_dwconv7x3_bn_act_t f32 and bf16, vp_dwconv7x3_raw,
           vp_dwconv7x3_bwd_data): W 1 2 3 5 10 20 40, C 4 32 384 768 1152 1536, H 1 5 8 15 16 17 125, B 1 3, every (W, cexp) of the net;
           five of them split the rows into several segments with a shorter last one (the launcher's formula is recomputed and asserted).
  stem     (B, H, W) = (1, 5, 80) (3, 125, 80) (2, 8, 80) (1, 9, 7), cout = 32.
  in place one f32 BFMNetEngine forward with vp_tune("bfm_dwproj", 1) and 0: both `pooled` tensors against the float64 MfccNet + pool.
Not here: conv_first_kernel<bf16> and the bf16 instantiations of maxpool_same_kernel - no plan launches them (dead code is not tested).
The training kernels of bfm_train.hip and gru_device.h have their own file, test_gpu_bfmnet_train_ops.py.

Measured on an MI355X (worst |got - ref| / bound per kernel, over all cases of the kernel):
  dwproj_kernel 0.149 (ce = 16 and 32; 0.012 or less from ce = 384 up, 0.014 just under the address limit)    conv_first_kernel 0.099
  dwconv7x3_f32_kernel: bias + ReLU6 0.252, raw 0.197, backward-data 0.247       dwconv7x3_kernel<bf16> 0.995 (the bf16 rounding term:
  half an ulp of an 8-bit significand IS 2^-8 |ref| just above a power of two)
  fused against unfused in place: pooled rel-L2 2.29e-06 fused, 2.17e-06 unfused, 1.43e-06 between the two
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import audio_ref as ar
from voicepuppet_amd import _lib

import gpu_util as gu
from gpu_util import SENTINEL, assert_guards, guarded      # (re-exported: test_gpu_bfmnet_train_ops.py imports them from here)

gpu = pytest.mark.gpu
U = 2.0 ** -24
VP_ERR_ARG = -1                         # enum vp_status of include/vp_hip.h
CLIP_SCALES = (1.0, 0.6, 1.6)

# (W, ce, cout) of every dwproj launch of the net, then the short-K edges; rows per tile of the instantiation of each mel width
DWPROJ_TRIPLES = [(40, 32, 64), (40, 384, 64), (20, 384, 64), (20, 384, 128), (10, 768, 128), (10, 768, 192), (5, 1152, 192), (5, 1152, 256),
                  (5, 1536, 256), (3, 1536, 256), (20, 16, 64), (20, 32, 64)]
DWPROJ_TR = {40: 2, 20: 4, 10: 8, 5: 16, 3: 16}
B_ADD = [(1, 0), (3, 1), (1, 1), (3, 0)]


def dwproj_h_classes(w):
  tr = DWPROJ_TR[w]
  out = []
  for name, h in (("5", 5), ("TR-1", tr - 1), ("TR", tr), ("TR+1", tr + 1), ("125", 125), ("5Twin", None)):
    if h is None or (h >= 1 and h not in [v for _, v in out]):
      out.append((name, h))
  return out


def dwproj_cases():
  """[(W, ce, cout, H class name, H or None for 5 T_win, B, add)]: every H class of every triple, (B, add) walking B_ADD."""
  cases = []
  for w, ce, cout in DWPROJ_TRIPLES:
    for i, (name, h) in enumerate(dwproj_h_classes(w)):
      b, add = B_ADD[i % 4]
      cases.append((w, ce, cout, name, h, b, add))
  return cases


# (B, H, W, C, rows split into >= 2 segments with a shorter last one)
UNFUSED_CASES = [(1, 125, 3, 1536, True), (3, 125, 5, 1536, True), (1, 17, 5, 1152, True), (3, 16, 10, 768, False), (1, 125, 20, 384, True),
                 (3, 15, 40, 384, False), (1, 8, 40, 32, False), (3, 5, 1, 4, False), (1, 1, 2, 32, False), (1, 125, 40, 32, True)]
UNFUSED_KERNELS = ["bn_act_f32", "bn_act_bf16", "raw", "bwd_data"]
STEM_CASES = [(1, 5, 80), (3, 125, 80), (2, 8, 80), (1, 9, 7)]


def dwconv_segments(b, h, w, c):
  """launch_dwconv7x3's row split (audio_kernels.hip): (segments, rows per segment, rows of the last segment)."""
  cols = b * w * (c // 4)
  nseg = min((131072 + cols - 1) // cols, max(h // 8, 1))
  nseg = max(nseg, 1)
  hs = (h + nseg - 1) // nseg
  nseg = (h + hs - 1) // hs
  return nseg, hs, h - (nseg - 1) * hs


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references (CPU only)
# ---------------------------------------------------------------------------------------------------------------------------------
def f32(a):
  return np.float32(a).astype(np.float64)


def clips(b, shape, seed, sigma=1.0):
  """[b, *shape]: clip i from its own seed, scaled by CLIP_SCALES[i]."""
  return f32(np.stack([CLIP_SCALES[i % 3] * sigma * np.random.default_rng(1000 * seed + i).normal(size=shape) for i in range(b)]))


def dw_inputs(b, h, w, c, seed, dtype="f32"):
  rng = np.random.default_rng(seed)
  x = gu.rounded(clips(b, (h, w, c), seed), dtype)
  wt = f32(rng.normal(0, 2.5 / np.sqrt(21.0), size=(7, 3, c, 1)))
  bias = f32(rng.uniform(-3.0, 9.0, size=c))
  return x, wt, bias


def dw_ref(x, wt, bias=None, flip=False):
  """(pre-activation, bound): depthwise 7x3 SAME (+ bias) in float64 and (21 + 2) u (|b| + sum |w||x|)."""
  if flip:
    wt = wt[::-1, ::-1]
  z = ar.depthwise_same(x, wt)
  mag = ar.depthwise_same(np.abs(x), np.abs(wt))
  if bias is not None:
    z, mag = z + bias, mag + np.abs(bias)
  return z, 23 * U * mag


def regime_shares(z):
  return float((z < 0).mean()), float((z > 6).mean()), float(((z >= 0) & (z <= 6)).mean())


def assert_regimes(z):
  lo, hi, mid = regime_shares(z)
  assert lo >= 0.10 and hi >= 0.10 and mid >= 0.30, (lo, hi, mid)


def dwproj_inputs(b, h, w, ce, cout, add, seed):
  x, wt, bias = dw_inputs(b, h, w, ce, seed)
  rng = np.random.default_rng(seed + 77)
  wp = f32(rng.normal(0, 1.0 / np.sqrt(ce), size=(ce, cout)))
  bp = f32(rng.normal(0, 0.5, size=cout))
  y0 = clips(b, (h, w, cout), seed + 5) if add else None
  return x, wt, bias, wp, bp, y0


def dwproj_ref(x, wt, bias, wp, bp, y0):
  """(reference, bound, depthwise pre-activation)"""
  z, zb = dw_ref(x, wt, bias)
  d = ar.relu6(z)
  ref = d @ wp + bp
  mag = (d + zb) @ np.abs(wp) + np.abs(bp)
  if y0 is not None:
    ref, mag = ref + y0, mag + np.abs(y0)
  return ref, (wp.shape[0] + 25) * U * mag, z


def stem_inputs(b, h, w, cout, seed):
  rng = np.random.default_rng(seed)
  x = clips(b, (h, w), seed, 3.0) - 4.0        # log-mel-like: wide, mostly negative
  wt = f32(rng.normal(0, 0.2, size=(9, 5, 1, cout)))
  bias = f32(rng.normal(0, 0.5, size=cout))
  return x, wt, bias


def stem_ref(x, wt, bias):
  z = ar.conv2d_same(x[..., None], wt, (1, 2)) + bias
  mag = ar.conv2d_same(np.abs(x)[..., None], np.abs(wt), (1, 2)) + np.abs(bias)
  return np.maximum(z, 0), 47 * U * mag


def trunk_shapes():
  """(W, cexp, cout) of every inverted-residual block, from the oracle's layer table and the mel widths 40 -> 20 -> 10 -> 5 -> 3."""
  out, cin, w = [], 32, 40
  for _, cout, exp, pool in ar.MFCCNET_BLOCKS:
    out.append((w, cin * exp, cout))
    cin = cout
    if pool:
      w = (w + 1) // 2
  return out


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests: the case tables cover what the trunk runs, and the input recipe reaches the three regimes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_the_trunk():
  shapes = trunk_shapes()
  assert len(shapes) == 17 and shapes[0] == (40, 32, 64) and shapes[-1] == (3, 1536, 256)
  assert set(shapes) == set(DWPROJ_TRIPLES[:10])               # the short-K edges are the table's only extras
  for s in shapes:
    assert s in DWPROJ_TRIPLES, s
    assert (s[0], s[1]) in {(w, c) for _, _, w, c, _ in UNFUSED_CASES}, s      # every kernel of UNFUSED_KERNELS runs the whole table
  assert {"bn_act_f32", "bn_act_bf16"} <= set(UNFUSED_KERNELS)
  # every triple meets every H class of its instantiation, both batch sizes and both add modes
  cases = dwproj_cases()
  for t in DWPROJ_TRIPLES:
    mine = [c for c in cases if c[:3] == t]
    tr = DWPROJ_TR[t[0]]
    want = {h for h in (5, tr - 1, tr, tr + 1, 125) if h >= 1} | {None}
    assert {c[4] for c in mine} == want, (t, mine)
    assert {c[5] for c in mine} == {1, 3} and {c[6] for c in mine} == {0, 1}, (t, mine)
  # the unfused axes
  assert {c[2] for c in UNFUSED_CASES} == {1, 2, 3, 5, 10, 20, 40}
  assert {c[3] for c in UNFUSED_CASES} >= {4, 32, 384, 1536}
  assert {c[1] for c in UNFUSED_CASES} == {1, 5, 8, 15, 16, 17, 125}
  assert {c[0] for c in UNFUSED_CASES} == {1, 3}


def test_unfused_cases_split_rows_as_stated():
  multi = 0
  for b, h, w, c, want in UNFUSED_CASES:
    nseg, hs, last = dwconv_segments(b, h, w, c)
    assert (nseg >= 2 and last < hs) == want, (b, h, w, c, nseg, hs, last)
    multi += want
  assert multi >= 3
  assert dwconv_segments(1, 125, 3, 1536) == (14, 9, 8)
  assert dwconv_segments(2, 9, 6, 32)[0] == 1          # the one shape of test_gpu_single_ops.py::test_dwconv7x3_bn_act


@pytest.mark.parametrize("b,h,w,c", [(3, 5, 1, 4), (1, 1, 2, 32), (3, 16, 10, 768)])
def test_input_recipe_reaches_three_regimes(b, h, w, c):
  for dtype in ("f32", "bf16"):
    x, wt, bias = dw_inputs(b, h, w, c, 11, dtype)
    z, bound = dw_ref(x, wt, bias)
    assert_regimes(z)
    assert bound.min() > 0 and (bound < 1e-3).all()


def test_dwproj_reference_on_cpu():
  """The reference and its bound for a small fused case: the regimes, and a float32 evaluation of the same sums stays inside the bound."""
  x, wt, bias, wp, bp, y0 = dwproj_inputs(3, 5, 20, 32, 64, 1, 7)
  ref, bound, z = dwproj_ref(x, wt, bias, wp, bp, y0)
  assert_regimes(z)
  d32 = np.minimum(np.maximum(ar.depthwise_same(x.astype(np.float32), wt.astype(np.float32)) + bias.astype(np.float32), 0), 6)
  got = (d32 @ wp.astype(np.float32) + bp.astype(np.float32) + y0.astype(np.float32)).astype(np.float64)
  assert (np.abs(got - ref) <= bound).all()
  assert not (np.abs(ref * (1 + 1e-4) - ref) <= bound).all()      # and a 1e-4 relative error does not


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------------------
def check(name, got, ref, bound):
  """Per-element bound; prints the worst ratio and the rel-L2 first, names the worst elements on failure."""
  got = np.asarray(got, np.float64)
  assert got.shape == ref.shape
  assert np.isfinite(got).all(), "%s: %d elements not written / not finite, first at %s" % (
      name, int((~np.isfinite(got)).sum()), np.argwhere(~np.isfinite(got))[0])
  ratio = np.abs(got - ref) / bound
  worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  print("\n%s: worst err/bound %.3f at %s, rel_l2 %.2e" % (name, ratio[worst], worst, gu.rel_l2(got, ref)))
  bad = np.argwhere(ratio > 1)
  assert len(bad) == 0, "%s: %d of %d elements outside the bound, e.g. (b, h, w, c) %s: got %r want %r bound %.2e" % (
      name, len(bad), ratio.size, bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])], bound[tuple(bad[0])])
  return float(ratio[worst])


def run_dwproj(xd, wt, bias, wp, bp, yv, add, b, h, w, ce, cout):
  L = _lib.lib()
  n = L.vp_dwproj_workspace_bytes(ce, cout)
  assert n > 0
  ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
  args = [gu.dev_f32(wt.reshape(21, ce)), gu.dev_f32(bias), gu.dev_f32(wp), gu.dev_f32(bp)]
  rc = L.vp_dwproj_fwd(gu.ptr(xd), *[gu.ptr(a) for a in args], gu.ptr(yv), add, b, h, w, ce, cout, gu.ptr(ws), gu.stream())
  torch.cuda.synchronize()
  return rc


@gpu
@pytest.mark.parametrize("w,ce,cout,hname,h,b,add", dwproj_cases(), ids=lambda v: str(v))
def test_dwproj(w, ce, cout, hname, h, b, add):
  if h is None:
    from voicepuppet_amd.stream import stream_context, stream_desc
    h = 5 * stream_context(stream_desc(1))[4]
    assert h > 17
  x, wt, bias, wp, bp, y0 = dwproj_inputs(b, h, w, ce, cout, add, seed=3 * w + ce + cout + h)
  ref, bound, z = dwproj_ref(x, wt, bias, wp, bp, y0)
  assert_regimes(z)
  whole, yv, g = guarded((b, h, w, cout), w * cout, fill=y0)
  _lib.check(run_dwproj(gu.dev_f32(x), wt, bias, wp, bp, yv, add, b, h, w, ce, cout), "vp_dwproj_fwd")
  assert_guards(whole, g)
  check("dwproj W%d ce%d cout%d H%d B%d add%d" % (w, ce, cout, h, b, add), yv.cpu().numpy(), ref, bound)


def test_dwproj_refuses_what_it_cannot_address():
  """Host logic only (no launch): a (W, ce, cout) without an instantiation and an expanded tensor past the 32-bit lane offsets."""
  L = _lib.lib()
  one = ctypes.c_void_p(256)          # never dereferenced: both refusals come before any launch or copy
  assert L.vp_dwproj_fwd(one, one, one, one, one, one, 0, 1, 5, 40, 384, 128, one, None) == VP_ERR_ARG
  assert b"dwproj_eligible" in L.vp_last_error()
  assert L.vp_dwproj_fwd(one, one, one, one, one, one, 0, 1, 5, 20, 24, 64, one, None) == VP_ERR_ARG
  assert L.vp_dwproj_fwd(one, one, one, one, one, one, 0, 65, 1023, 40, 384, 64, one, None) == VP_ERR_ARG
  assert b"0xF0000000" in L.vp_last_error()
  assert L.vp_dwproj_workspace_bytes(24, 64) == 0 and L.vp_dwproj_workspace_bytes(384, 64) > 22 * 384 * 4 + 384 * 64 * 4


@gpu
def test_dwproj_near_the_address_limit():
  """(64, 1023, 40, 384, 64): the expanded tensor is 4 022 599 680 bytes, the bound 4 026 531 840 - the last clip's lane offsets use
  the top of the 32-bit range.  Input made on the device; clips 0 and 63 are checked element by element, the rest for being written."""
  b, h, w, ce, cout = 64, 1023, 40, 384, 64
  assert b * h * w * ce * 4 == 4022599680 < 0xF0000000 <= (b + 1) * h * w * ce * 4
  free = torch.cuda.mem_get_info()[0]
  if free < 12e9:
    pytest.skip("needs 12 GB of free device memory, %d bytes are free" % free)
  L = _lib.lib()
  _, wt, bias, wp, bp, _ = dwproj_inputs(1, 1, w, ce, cout, 0, seed=9)
  gen = torch.Generator(device="cuda")
  xd = torch.empty((b, h, w, ce), dtype=torch.float32, device="cuda")
  for i in range(b):
    gen.manual_seed(500 + i)
    xd[i].normal_(0.0, CLIP_SCALES[i % 3], generator=gen)
  whole, yv, g = guarded((b, h, w, cout), w * cout)
  # one clip more: refused before anything is launched (the output stays NaN)
  assert run_dwproj(xd, wt, bias, wp, bp, yv, 0, b + 1, h, w, ce, cout) == VP_ERR_ARG
  assert b"0xF0000000" in L.vp_last_error()
  assert bool(torch.isnan(yv).all())
  _lib.check(run_dwproj(xd, wt, bias, wp, bp, yv, 0, b, h, w, ce, cout), "vp_dwproj_fwd")
  assert_guards(whole, g)
  assert not bool(torch.isnan(yv).any())
  for i in (0, b - 1):
    x = xd[i:i + 1].cpu().numpy().astype(np.float64)
    ref, bound, z = dwproj_ref(x, wt, bias, wp, bp, None)
    assert_regimes(z)
    check("dwproj near the limit, clip %d" % i, yv[i:i + 1].cpu().numpy(), ref, bound)


@gpu
@pytest.mark.parametrize("kernel", UNFUSED_KERNELS)
@pytest.mark.parametrize("b,h,w,c,multi", UNFUSED_CASES)
def test_dwconv7x3(kernel, b, h, w, c, multi):
  L = _lib.lib()
  nseg, hs, last = dwconv_segments(b, h, w, c)
  assert (nseg >= 2 and last < hs) == multi, (nseg, hs, last)
  dtype = "bf16" if kernel == "bn_act_bf16" else "f32"
  x, wt, bias = dw_inputs(b, h, w, c, seed=h + 7 * w + c, dtype=dtype)
  xd, wd, bd = gu.to_dev(x, dtype), gu.dev_f32(wt.reshape(21, c)), gu.dev_f32(bias)
  whole, yv, g = guarded((b, h, w, c), w * c, dtype)
  if kernel.startswith("bn_act"):
    z, bound = dw_ref(x, wt, bias)
    assert_regimes(z)
    ref = ar.relu6(z)
    if dtype == "bf16":
      bound = bound + 2.0 ** -8 * np.abs(ref)
    rc = L.vp_dwconv7x3_bn_act_t(gu.ptr(xd), gu.ptr(wd), gu.ptr(bd), gu.ptr(yv), _lib.VP_BF16 if dtype == "bf16" else _lib.VP_F32, b, h, w, c, gu.stream())
  elif kernel == "raw":
    ref, bound = dw_ref(x, wt)
    rc = L.vp_dwconv7x3_raw(gu.ptr(xd), gu.ptr(wd), gu.ptr(yv), b, h, w, c, gu.stream())
  else:
    ref, bound = dw_ref(x, wt, flip=True)
    rc = L.vp_dwconv7x3_bwd_data(gu.ptr(xd), gu.ptr(wd), gu.ptr(yv), b, h, w, c, gu.stream())
  _lib.check(rc, kernel)
  torch.cuda.synchronize()
  assert_guards(whole, g)
  check("dwconv7x3 %s (%d, %d, %d, %d) nseg %d x %d rows, last %d" % (kernel, b, h, w, c, nseg, hs, last), yv.float().cpu().numpy(), ref, bound)


@gpu
@pytest.mark.parametrize("b,h,w", STEM_CASES)
def test_conv_first(b, h, w):
  L = _lib.lib()
  cout = 32
  x, wt, bias = stem_inputs(b, h, w, cout, seed=h + w)
  ref, bound = stem_ref(x, wt, bias)
  assert 0.2 < (ref > 0).mean() < 0.8
  wo = (w + 1) // 2
  whole, yv, g = guarded((b, h, wo, cout), wo * cout)
  xd, wd, bd = gu.dev_f32(x), gu.dev_f32(wt.reshape(45, cout)), gu.dev_f32(bias)
  _lib.check(L.vp_conv_first_fwd(gu.ptr(xd), gu.ptr(wd), gu.ptr(bd), gu.ptr(yv), b, h, w, cout, gu.stream()), "vp_conv_first_fwd")
  torch.cuda.synchronize()
  assert_guards(whole, g)
  check("conv_first (%d, %d, %d)" % (b, h, w), yv.cpu().numpy(), ref, bound)


@gpu
def test_fused_against_unfused_in_place():
  """The plan hands dwproj_kernel the operands the op test assumes: one engine, the fused and the unfused trunk, both against float64."""
  from voicepuppet_amd.audio import BFMNetEngine
  from test_gpu_audio import synth_pcm
  L = _lib.lib()
  b, t, lens = 2, 25, [25, 11]
  p = ar.init_bfmnet_params(3, dtype=np.float32)
  mfcc = ar.extract_mfcc(synth_pcm(b, ar.pcm_length_for(t), seed=5).astype(np.float64)).astype(np.float32)
  ears = np.zeros((b, t, 1), np.float32)
  eng = BFMNetEngine(b, t)
  eng.load_params(p)
  got = {}
  try:
    for knob in (1, 0):
      assert L.vp_tune(b"bfm_dwproj", knob) == 0
      eng.forward(torch.tensor(ears, device="cuda"), torch.tensor(mfcc, device="cuda"), lens)
      torch.cuda.synchronize()
      got[knob] = eng.tensor("pooled").cpu().numpy().astype(np.float64).reshape(b, t, 256)
  finally:
    L.vp_tune(b"bfm_dwproj", 1)
  feat = ar.mfccnet_fwd({k: v.astype(np.float64) for k, v in p.items()}, mfcc.astype(np.float64)[..., None])
  ref = ar.maxpool_same(feat, (5, 3), (5, 3)).reshape(b, t, 256)
  e1, e0, d = gu.rel_l2(got[1], ref), gu.rel_l2(got[0], ref), gu.rel_l2(got[1], got[0])
  print("\npooled rel_l2: fused %.2e, unfused %.2e, fused against unfused %.2e" % (e1, e0, d))
  assert e1 < 1e-3 and e0 < 1e-3

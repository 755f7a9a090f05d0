"""Bit-exact parity of the PixReferNet convolution kernels on integer operands, and the CPU tests of the per-element bound of
test_gpu_ops.py.  The two instruments complement each other: the exact test sees any indexing error at any element (a dropped tap, a
wrong last tile, a lost K slab, a store one element off) with no tolerance to argue about; the bound sees precision errors (a partial
sum kept in bf16), which small integers pass through unharmed.

The idea: operands are small integers for which every product and every partial sum, IN ANY ORDER, is exact in float32.  Split-K,
atomics and the MFMA's internal order then cannot change the result: the device output must have the bits of the integer reference at
every element.  bf16 outputs must have the bits of the reference rounded to nearest even, and integers up to 256 are exact in bf16.

Operands (exact_operands)
  x, dy, w in {-1, 0, 1}; P(0) = 1/3 up to K = 1200, 1/2 up to 4096, 3/4 above (K: test_gpu_ops.contraction).  The second operand of
  the sum (w; dy for the weight gradient) is made sparser where the first one is large or K is long, so that the variance of an output
  K P(w != 0) E[xa^2] stays at or below VAR_CAP = 4096 (64^2: 256 is four standard deviations) - the starting recipe alone would put
  the 131072-pixel weight gradients and the affine cases above the 1 % cap below.  bias: integers in [-3, 3].
  K < 8 (the weight gradients of the two 2-pixel bottleneck cases, K = 2, where 12 of the 16 taps only ever meet padding): w / dy
  without zeros and the non-negative inputs of the float32 recipe below, or fewer than 20 % of the outputs would be non-zero.
  affine / in_act cases: x in {-15, -10, -5, 0, 1, 2}, scale in {1, 2}, shift in {0, 5, 10}: scale x + shift is an integer of at most
  five bits, fused or not, and every negative one is a multiple of 5.  The loaders (prologue_piece, plane_device.h) compute
  fmaf(scale, x, shift), then act_apply, then on the bf16 path round to bf16 (Elem<bf16>::pack).  act_apply's leaky ReLU is
  0.6f v + 0.4f |v|, which the compiler is free to contract into either product: for v = -5 m the plain form gives -m, the form
  fma(0.6f, v, 0.4f |v|) gives -m (1 + 2^-23).  Rounded to bf16 both are -m, so on the bf16 path - the benchmark's - the activated
  operand is the integer lrelu(v) = v / 5 whichever form the loader has.  On the FLOAT32 path no negative integer has that property
  (test_leaky_relu_forms lists them), so a float32 case with a leaky ReLU draws x from {0, 1, 2} and shift from {0, 4, 8}: the
  pre-activations 0 1 2 4 5 6 8 9 10 12 are reproduced by all three forms.  Its negative branch is left to the per-element bound.
  tanh (the decoder_1-like case): w and bias are scaled by 2^-6 and the variance cap is 40^2, so the exact pre-activation is a multiple
  of 1/64 inside [-4, 4] (asserted); |got - tanh(ref)| <= K_TANH u |tanh(ref)| (test_gpu_bfmnet_train_ops.py), on the bf16 path plus
  half a bf16 ulp of the device's float32 value.
Reference: torch float64 convolutions of the integers (exact), once per (case, op, recipe) for both dtypes and every knob (lru_cache;
the runs of one (case, op) are adjacent).  test_exact_reference_against_the_oracle compares it with oracle/nn_ops.py.
Asserted on the reference before the device is looked at (reference_conditions)
  * K max|a| max|b| + max|bias| < 2^24, which bounds sum |a||b| + |bias| at every element: float32 is exact in any order;
  * at most 1 % of a bf16 output above 256 in magnitude (forward, backward-data), at least 20 % of the outputs non-zero.
Runs (RUNS): every case of FWD_CASES and CLASS_CASES, forward / backward-data / backward-weight as test_gpu_ops.py runs them, f32 and
bf16, under the knobs of the rel-L2 tests: patch_min_blocks 1 (the CLASS_CASES entry's for those), patch_small_tiles 0 and 1 for the
cases of test_patch_kernel_tile_variants, s2c64 = 1 for its three cases, wgrad_slab_tile_x1000 = 0 for every weight gradient, the
lowered thin_blocks_* caps (the last three groups in bf16, as there).  Outputs, workspace and operands are guarded (gpu_util.Guarded).
test_exact_runs_use_the_classes_of_the_rel_l2_cases compares the profile's class names of every run with those of the rel-L2 test's call.

Measured on an MI355X
  347 exact runs over 130 references (43 cases; 80 kernel classes, the same run by run as the rel-L2 calls): every run bit-equal, the
  tanh case at 0.344 (f32) / 0.948 (bf16) of its bound, every guard band intact.  No kernel bug was found.
  Wall time: this file 21 s, test_gpu_ops.py 79 s with the per-element bounds and guarded buffers (54 s at the parent commit).
  Reference computation is most of this file's time: the first run of a (case, op) computes it and the next ones reuse it - 1.45 s
  against 0.35 s for the forward of the K = 4096 case, the largest.  On a 16-thread CPU without a GPU the 130 references (operands,
  torch float64 convolutions, conditions) take 35 s, at most 3.2 s each, and the CPU tests of this file 6 s.
  Worst |got - ref| / bound of test_gpu_ops.py per (op, dtype), over all its cases and knobs:
    forward         f32 0.072   bf16 0.992      backward-data   f32 0.022   bf16 0.979      backward-weight f32 0.951   bf16 0.979
  (bf16 outputs: the rounding term - half an ulp of an 8-bit significand IS 2^-8 |ref| just above a power of two.  Weight gradient:
  0.951 is the K = 2 bottleneck case, two products and one rounding, again half an ulp; 0.979 in bf16 is an affine + leaky-ReLU case
  where one operand's bf16 rounding falls on the other side than the midpoint's - the term D, tight by construction.  Where K is long
  the float32 figures are far below 1: the bound is a worst case over K roundings.)
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from voicepuppet_amd import _lib

import gpu_util as gu
import test_gpu_ops as T
from test_gpu_bfmnet_train_ops import K_TANH

gpu = pytest.mark.gpu
U = T.U
VAR_CAP, VAR_CAP_TANH = 64.0 ** 2, 40.0 ** 2
KNOB_DEFAULTS = {b"patch_min_blocks": -1, b"patch_small_tiles": 3, b"s2c64": 512, b"wgrad_slab_tile_x1000": -1,
                 b"thin_blocks_cout8": 1024, b"thin_blocks_dcout8": 512, b"thin_blocks_cin8": 512}


# ---------------------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------------------
def p_zero(k):
  return 1.0 / 3 if k <= 1200 else (0.5 if k <= 4096 else 0.75)


def ternary(rng, shape, p0):
  r = rng.random(shape, dtype=np.float32)
  nz = np.float32(1 - p0)
  return np.where(r < nz / 2, 1.0, np.where(r < nz, -1.0, 0.0))


def lrelu_forms(v):
  """The three float32 evaluations of act_apply's 0.6f v + 0.4f |v| (plain, either product contracted), as float64."""
  f = np.float32
  v = np.asarray(v, np.float64)
  p6, p4 = (f(0.6) * v.astype(f)).astype(np.float64), (f(0.4) * np.abs(v).astype(f)).astype(np.float64)
  a, b = float(f(0.6)), float(f(0.4))
  return [(p6.astype(f) + p4.astype(f)).astype(np.float64), (a * v + p4).astype(f).astype(np.float64), (b * np.abs(v) + p6).astype(f).astype(np.float64)]


def recipe_of(case, op, dtype):
  """'neg': leaky ReLU input on the bf16 path (negative pre-activations, multiples of 5); 'pos': on the float32 path; '' otherwise."""
  in_act = case[9] if op != "bwd_data" else 0
  return ("neg" if dtype == "bf16" else "pos") if in_act == 1 else ""


@functools.lru_cache(maxsize=1)
def exact_operands(case, op, recipe):
  """dict of float64 integer arrays: a (first operand as the device gets it: x or dy), xa (a after affine + activation), b (second
  operand: w, or dy for the weight gradient), bias / scale / shift or None, wscale (1, or 2^-6 under a tanh)."""
  kind, n, h, w, cin, cout, k, s, p, in_act, out_act, affine = case
  rng = np.random.default_rng([("fwd", "bwd_data", "bwd_weight").index(op)] + [int(v) for v in case])
  ho, wo = gu.out_hw(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, "f32"))
  kk = T.contraction(case, op)
  p0 = p_zero(kk)
  wshape = (k, k, cin, cout) if kind == 0 else (4, 4, cout, cin)
  o = {"bias": None, "scale": None, "shift": None, "wscale": 1.0}
  if op == "bwd_data":
    in_act, affine = 0, False
    o["a"] = o["xa"] = ternary(rng, (n, ho, wo, cout), p0)
  elif affine or in_act:
    xs, shifts = ([0, 1, 2], [0, 4, 8]) if recipe == "pos" or kk < 8 else ([-15, -10, -5, 0, 1, 2], [0, 5, 10])
    o["a"] = rng.choice(np.float64(xs), size=(n, h, w, cin))
    pre = o["a"]
    if affine:
      o["scale"], o["shift"] = rng.choice(np.float64([1, 2]), size=cin), rng.choice(np.float64(shifts), size=cin)
      pre = o["scale"] * o["a"] + o["shift"]
    assert in_act in (0, 1, 2)
    o["xa"] = np.where(pre < 0, pre / 5, pre) if in_act == 1 else (np.maximum(pre, 0) if in_act == 2 else pre)
    assert (pre[pre < 0] % 5 == 0).all() and (o["xa"] == np.round(o["xa"])).all()
    if in_act == 1 and recipe == "pos":
      assert all((fm == pre).all() for fm in lrelu_forms(pre))
  else:
    o["a"] = o["xa"] = ternary(rng, (n, h, w, cin), p0)
  cap = VAR_CAP_TANH if (op == "fwd" and out_act == 3) else VAR_CAP
  pnz = min(1 - p0 if kk >= 8 else 1.0, cap / (kk * float(np.mean(o["xa"] ** 2))))
  o["b"] = ternary(rng, wshape if op != "bwd_weight" else (n, ho, wo, cout), 1 - pnz)
  if op == "fwd":
    o["bias"] = rng.integers(-3, 4, size=cout).astype(np.float64)
    if out_act == 3:
      o["wscale"] = 2.0 ** -6
  return o


def t_nchw(a):
  return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def exact_conv(case, op, a, b, bias=None):
  """conv_op of test_gpu_ops.py restated with torch float64 convolutions (NHWC numpy in and out)."""
  kind, n, h, w, cin, cout, k, s, p = case[:9]
  if op == "bwd_weight":
    # dw[i, j, ci, co] = sum_pix g[n, s oh + i, s ow + j, ci] d[n, oh, ow, co]: a convolution of g (channels as batch) with d as the kernel, dilated by s
    g, d, st = (a, b, s) if kind == 0 else (b, a, 2)      # transposed: the gathered operand is dY, the kernel the input
    pad = p if kind == 0 else 1
    dw = F.conv2d(t_nchw(g).permute(1, 0, 2, 3), t_nchw(d).permute(1, 0, 2, 3), padding=pad, dilation=st)[:, :, :k, :k]
    return dw.permute(2, 3, 0, 1).numpy()                 # [k, k, C(g), C(d)]: HWIO for a convolution, [4, 4, cout, cin] for a transposed one
  wt = torch.from_numpy(np.ascontiguousarray(b, np.float64)).permute(3, 2, 0, 1)
  bt = None if bias is None else torch.from_numpy(np.asarray(bias, np.float64))
  st, pad = (s, p) if kind == 0 else (2, 1)
  # HWIO -> (cout, cin, kh, kw), [4, 4, cout, cin] -> (cin, cout, kh, kw): what conv2d wants for the strided direction (forward of a
  # convolution, backward-data of a transposed one) and conv_transpose2d for the other
  if (op == "fwd") == (kind == 0):
    y = F.conv2d(t_nchw(a), wt, bt, stride=st, padding=pad)
  else:
    y = F.conv_transpose2d(t_nchw(a), wt, bt, stride=st, padding=pad)
  return y.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=1)
def exact_reference(case, op, recipe):
  """float64: the exact result before the output activation's tanh (ReLU applied), and the operands' dict."""
  o = exact_operands(case, op, recipe)
  bias = None if o["bias"] is None else o["bias"] * o["wscale"]
  ref = exact_conv(case, op, o["xa"], o["b"] * o["wscale"], bias)
  if op == "fwd" and case[10] == 2:
    ref = np.maximum(ref, 0)
  return ref, o


def reference_conditions(case, op, ref, o):
  """The three conditions of the module docstring, on the reference alone."""
  kk = T.contraction(case, op)
  top = kk * np.abs(o["xa"]).max() * np.abs(o["b"]).max() + (0 if o["bias"] is None else np.abs(o["bias"]).max())
  assert top < 2 ** 24, top
  ints = ref / o["wscale"]
  assert (ints == np.round(ints)).all()
  nonzero, big = float((ints != 0).mean()), float((np.abs(ints) > 256).mean())
  assert nonzero >= 0.20, "vacuous: %.3f of the outputs are non-zero" % nonzero
  if op != "bwd_weight":
    assert big <= 0.01, "%.4f of the outputs are above 256, where bf16 rounds" % big
  if o["wscale"] != 1.0:
    assert np.abs(ref).max() <= 4.0


def f32_bits(a):
  return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)          # (+ 0: -0 becomes +0)


def bf16_bits(t):
  return ((t.float() + 0.0).to(torch.bfloat16) if t.dtype == torch.bfloat16 else (t + 0.0).to(torch.bfloat16)).view(torch.int16).numpy()


def exact_mismatch(got, ref, dtype):
  """None, or a message with the number of differing elements and the coordinates of the first few.  got: a float32 / bfloat16 torch
  tensor (the device's bits) or an array of float32 values; ref: the exact float64 values."""
  if dtype == "bf16":
    g = bf16_bits(got if torch.is_tensor(got) else torch.from_numpy(np.asarray(got, np.float32)))
    w = bf16_bits(torch.from_numpy(np.asarray(ref, np.float32)))
  else:
    g, w = f32_bits(got.numpy() if torch.is_tensor(got) else got), f32_bits(ref)
  if g.shape == w.shape and np.array_equal(g, w):
    return None
  assert g.shape == w.shape, (g.shape, w.shape)
  bad = np.argwhere(g != w)
  gv = got.float().numpy() if torch.is_tensor(got) else np.asarray(got)
  return "%d of %d elements differ; first at %s: got %s want %s" % (
      len(bad), g.size, bad[:8].tolist(), [float(gv[tuple(i)]) for i in bad[:4]], [float(ref[tuple(i)]) for i in bad[:4]])


def tanh_bound(ref_pre, dtype):
  t = np.tanh(ref_pre)
  b = K_TANH * U * np.abs(t)
  return t, (b + 2.0 ** -8 * (np.abs(t) + b) if dtype == "bf16" else b) + 1e-300


# ---------------------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------------------
def bwd_able(case):
  return case[5] >= 8 and (case[5] & (case[5] - 1)) == 0


def is_tile_variant_case(c):
  return c[6] in (3, 4) and c[7] == 1 and c[4] >= 32 and c[5] >= 64 and not c[11] and c[9] == 0


S2C64_CASES = [(0, 2, 128, 128, 64, 128, 4, 2, 1, 0, 0, False), (0, 3, 32, 64, 64, 128, 4, 2, 1, 0, 0, False), (0, 5, 64, 160, 64, 128, 4, 2, 1, 0, 0, False)]
THIN_RUNS = [("bwd_data", T.CONV1_1, b"thin_blocks_cout8", 5), ("bwd_data", T.LAYER_1, b"thin_blocks_dcout8", 5), ("fwd", T.CONV1_1, b"thin_blocks_cin8", 3)]


def make_runs():
  """[(op, case, dtype, ((knob, value), ..))], the runs of one (case, op) adjacent."""
  runs = []
  table = [(1, c) for c in T.FWD_CASES] + list(T.CLASS_CASES)
  for minblk, case in table:
    for op in ("fwd", "bwd_data", "bwd_weight"):
      if op != "fwd" and not bwd_able(case):
        continue
      base = ((b"patch_min_blocks", minblk),)
      for dtype in ("f32", "bf16"):
        runs.append((op, case, dtype, base))
      if op == "fwd" and minblk == 1 and case in T.FWD_CASES and is_tile_variant_case(case):
        runs += [(op, case, dtype, ((b"patch_min_blocks", 1), (b"patch_small_tiles", small))) for small in (0, 1) for dtype in ("f32", "bf16")]
      if op == "bwd_weight":
        runs.append((op, case, "bf16", ((b"patch_min_blocks", 1), (b"wgrad_slab_tile_x1000", 0))))
      runs += [(op, case, "bf16", ((b"patch_min_blocks", 1), (knob, cap))) for o2, c2, knob, cap in THIN_RUNS if (o2, c2) == (op, case) and minblk == 1]
  runs += [("fwd", case, "bf16", ((b"patch_min_blocks", 1), (b"s2c64", 1))) for case in S2C64_CASES]
  return runs


RUNS = make_runs()


def run_id(r):
  op, case, dtype, knobs = r
  return "%s-%s-%s-%s" % (op, "x".join(str(int(v)) for v in case), dtype, "-".join("%s%d" % (k.decode(), v) for k, v in knobs))


@contextlib.contextmanager
def knobs_set(knobs):
  L = _lib.lib()
  try:
    for k, v in knobs:
      assert L.vp_tune(k, v) == 0
    yield
  finally:
    for k, _ in knobs:
      L.vp_tune(k, KNOB_DEFAULTS[k])


def device_run(op, case, dtype, o, raw=True):
  kind, n, h, w, cin, cout, k, s, p, in_act, out_act, affine = case
  if op == "fwd":
    d = gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype, in_act, out_act)
    return gu.conv_fwd(d, o["a"], o["scale"], o["shift"], o["b"] * o["wscale"], o["bias"] * o["wscale"], dtype, raw=raw)
  if op == "bwd_data":
    return gu.conv_bwd_data(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype), o["a"], o["b"], dtype, raw=raw)
  d = gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype, in_act)
  return gu.conv_bwd_weight(d, o["a"], o["scale"], o["shift"], o["b"], (k, k, cin, cout) if kind == 0 else (4, 4, cout, cin), dtype, raw=raw)


CLASSES = {}      # run -> the profile's class names of its device call (filled by test_exact)


def exact_device(run, o):
  op, case, dtype, knobs = run
  out = []
  with knobs_set(knobs):
    CLASSES[run] = T._profile_classes(lambda: out.append(device_run(op, case, dtype, o)))        # (device_run asserts the guard bands)
  return out[0]


@gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_exact(run):
  op, case, dtype, knobs = run
  ref, o = exact_reference(case, op, recipe_of(case, op, dtype))
  reference_conditions(case, op, ref, o)
  got = exact_device(run, o)
  if op == "fwd" and case[10] == 3:
    t, bound = tanh_bound(ref, dtype)
    T.check_elements("exact tanh %s %s" % (dtype, case), got.float().numpy(), t, bound)
    return
  bad = exact_mismatch(got, ref, "f32" if op == "bwd_weight" else dtype)
  assert bad is None, "%s %s %s on %s: %s (coordinates: n, y, x, c - weight gradient: kh, kw, and the two channel axes)" % (
      op, dtype, case, sorted(CLASSES[run]), bad)


def rel_l2_side(op, case, dtype):
  """The device call test_conv_fwd / test_conv_bwd_data / test_conv_bwd_weight make for the case, on zeros: the planner sees the
  descriptor, which operands exist and the knobs, never a value (test_gpu_coverage.op_case_classes collects its classes the same way)."""
  kind, n, h, w, cin, cout, k, s, p, in_act, out_act, affine = case
  ho, wo = gu.out_hw(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype))
  x, dy = np.zeros((n, h, w, cin), np.float32), np.zeros((n, ho, wo, cout), np.float32)
  wt = np.zeros((k, k, cin, cout) if kind == 0 else (4, 4, cout, cin), np.float32)
  sc = np.zeros(cin, np.float32) if affine else None
  if op == "fwd":
    gu.conv_fwd(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype, in_act, out_act), x, sc, sc, wt, np.zeros(cout, np.float32), dtype)
  elif op == "bwd_data":
    gu.conv_bwd_data(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype), dy, wt, dtype)
  else:
    gu.conv_bwd_weight(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype, in_act), x, sc, sc, dy, wt.shape, dtype)


@gpu
def test_exact_runs_use_the_classes_of_the_rel_l2_cases():
  """The exact runs are worth what the rel-L2 cases are worth only if they land on the same kernels: run by run, the class names of the
  profile records (family, operand type, tile) collected while test_exact ran equal those of the rel-L2 test's call under the same
  knobs.  (A run test_exact did not make in this session is made here.)"""
  diff = []
  for run in RUNS:
    op, case, dtype, knobs = run
    if run not in CLASSES:
      exact_device(run, exact_operands(case, op, recipe_of(case, op, dtype)))
    with knobs_set(knobs):
      want = T._profile_classes(lambda: rel_l2_side(op, case, dtype))
    if want != CLASSES[run] or not want:
      diff.append((run_id(run), sorted(want), sorted(CLASSES[run])))
  assert not diff, diff[:5]
  every = set().union(*CLASSES.values())
  print("\n%d runs, %d classes: %s" % (len(RUNS), len(every), sorted(every)))
  for prefix in ("s2c64_", "cout8_", "dcout8_", "cin8_"):
    assert any(c.startswith(prefix) for c in every), prefix
  assert "wgrad_tr_exact_bf16_256x256" in every


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = [(0, 3, 9, 9, 32, 64, 4, 1, 1, 1, 0, True), (1, 2, 4, 4, 32, 16, 4, 2, 1, 2, 0, True), (0, 2, 16, 16, 8, 64, 4, 2, 1, 0, 0, False)]


def test_run_table():
  assert all(c in T.FWD_CASES for c in SMALL)
  cases = {r[1] for r in RUNS}
  assert cases == set(T.FWD_CASES) | {c for _, c in T.CLASS_CASES} | set(S2C64_CASES)
  for case in T.FWD_CASES + [c for _, c in T.CLASS_CASES]:
    for dtype in ("f32", "bf16"):
      assert ("fwd", case, dtype) in {r[:3] for r in RUNS}
      assert (("bwd_data", case, dtype) in {r[:3] for r in RUNS}) == bwd_able(case) == (("bwd_weight", case, dtype) in {r[:3] for r in RUNS})
  assert [c for c in T.FWD_CASES if bwd_able(c)] == T.BWD_CASES
  assert len({run_id(r) for r in RUNS}) == len(RUNS)
  assert sum(1 for r in RUNS if (b"patch_small_tiles", 0) in r[3]) == 2 * sum(1 for c in T.FWD_CASES if is_tile_variant_case(c)) > 0
  assert sum(1 for r in RUNS if (b"wgrad_slab_tile_x1000", 0) in r[3]) == sum(1 for c in T.FWD_CASES + [c for _, c in T.CLASS_CASES] if bwd_able(c))
  assert sum(1 for r in RUNS if any(k.startswith(b"thin_blocks") for k, _ in r[3])) == 3
  for _, knobs in {(r[0], r[3]) for r in RUNS}:
    assert all(k in KNOB_DEFAULTS for k, _ in knobs)


def test_leaky_relu_forms():
  """What the module docstring says of act_apply's leaky ReLU: on the float32 path the contracted form fma(0.6f, v, 0.4f |v|) misses
  the integer at EVERY negative multiple of 5 down to -60; rounded to bf16 all three forms give it; the non-negative pre-activations of
  the float32 recipe are reproduced by all three."""
  neg = np.arange(-60, 0, 5, dtype=np.float64)
  forms = lrelu_forms(neg)
  assert (forms[0][-4:] == neg[-4:] / 5).all()                           # the plain form is exact for the small ones ...
  assert (forms[1] != neg / 5).all()                                    # ... the contracted one never
  for fm in forms:
    assert (T.bf16_round(fm) == neg / 5).all()
  pos = np.float64([0, 1, 2, 4, 5, 6, 8, 9, 10, 12])
  assert all((fm == pos).all() for fm in lrelu_forms(pos))
  assert not all((fm == 7.0).all() for fm in lrelu_forms(np.float64([7])))      # (why the shifts are 0 4 8 and not 0 5 10 there)


@pytest.mark.parametrize("case", SMALL)
def test_exact_reference_against_the_oracle(case):
  """The torch float64 reference equals oracle/nn_ops.py on the exact operands, for every op and recipe of three small cases, and the
  three conditions hold; then each condition rejects a reference made to break it."""
  assert case in T.FWD_CASES
  for op in ("fwd", "bwd_data", "bwd_weight"):
    for dtype in ("f32", "bf16"):
      ref, o = exact_reference(case, op, recipe_of(case, op, dtype))
      want = T.conv_op(case, op, o["xa"], o["b"], o["bias"])
      assert ref.shape == want.shape and (ref == (np.maximum(want, 0) if op == "fwd" and case[10] == 2 else want)).all()
      reference_conditions(case, op, ref, o)
  ref, o = exact_reference(case, "fwd", recipe_of(case, "fwd", "bf16"))
  with pytest.raises(AssertionError):
    reference_conditions(case, "fwd", ref * 0, o)                        # vacuous
  with pytest.raises(AssertionError):
    reference_conditions(case, "fwd", ref * 300, o)                      # most of it above 256
  with pytest.raises(AssertionError):
    reference_conditions(case, "fwd", ref, dict(o, b=o["b"] * 2.0 ** 20))      # sums that float32 cannot hold in any order
  with pytest.raises(AssertionError):
    reference_conditions(case, "fwd", ref + 0.5, o)                      # not integers


def test_exact_conditions_hold_for_the_tanh_case():
  case = (1, 2, 8, 8, 128, 4, 4, 2, 1, 2, 3, True)
  assert case in T.FWD_CASES
  ref, o = exact_reference(case, "fwd", "")
  reference_conditions(case, "fwd", ref, o)
  assert o["wscale"] == 2.0 ** -6 and (ref * 64 == np.round(ref * 64)).all() and np.abs(ref).max() <= 4 and np.abs(ref).max() > 1
  t, bound = tanh_bound(ref, "bf16")
  assert (np.abs(T.bf16_round(np.tanh(ref).astype(np.float32)) - t) <= bound).all()
  assert not (np.abs(np.tanh(ref + 1.0 / 64) - t) <= bound).all()        # the neighbouring multiple of 1/64 is outside


def fma_chain32(terms):
  """s = fmaf(x, w, s) over the rows of `terms` (the exact products, float64): one float32 rounding per term."""
  s = np.zeros(terms[0].shape, np.float32)
  for row in terms:
    s = (s.astype(np.float64) + row).astype(np.float32)
  return s


def fwd_chain32(case, xa, wr, bias):
  """Forward of a kind-0 case as one float32 chain per output element, taps then channels in order, the bias last."""
  kind, n, h, w, cin, cout, k, s, p = case[:9]
  ho, wo = gu.out_hw(gu.conv_desc(kind, n, h, w, cin, cout, k, s, p, "f32"))
  xp = np.pad(xa, ((0, 0), (p, p), (p, p), (0, 0)))
  terms = [xp[:, i:i + s * ho:s, j:j + s * wo:s, c, None] * wr[i, j, c] for i in range(k) for j in range(k) for c in range(cin)]
  return fma_chain32(terms + [np.broadcast_to(bias, terms[0].shape)])


@pytest.mark.parametrize("case", SMALL)
def test_bound_holds_a_float32_restatement(case):
  """The per-element bound of test_gpu_ops.py on three small cases: a plain float32 chain of the forward (fmaf order; kind 0) and float32
  numpy evaluations of the backward ops stay inside it, on the operands of both dtypes; a relative error of 1e-4 does not."""
  f = np.float32
  for dtype in ("f32", "bf16"):
    ref, bound = T.fwd_reference(case, dtype)
    x, wt, b, sc, sh = T.make_case(case)
    for xa in T.input_candidates(x, sc, sh, case[9], dtype):
      wr = gu.rounded(wt, dtype)
      if case[0] == 0:
        got = fwd_chain32(case, xa.astype(np.float64), wr, f(b).astype(np.float64))
      else:
        got = T.conv_op(case, "fwd", xa.astype(f), wr.astype(f), f(b))
      got = T.ACTS[case[10]](got)
      got = T.bf16_round(got) if dtype == "bf16" else got
      assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert not (np.abs(ref * (1 + 1e-2 if dtype == "bf16" else 1 + 1e-4) - ref) <= bound).all()
    if not bwd_able(case):
      continue
    ho, wo = gu.out_hw(gu.conv_desc(*case[:9], dtype))
    dyr = gu.rounded(np.random.default_rng(7).normal(size=(case[1], ho, wo, case[5])), dtype)
    ref, bound = T.bwd_data_reference(case, dtype)
    got = T.conv_op(case, "bwd_data", dyr.astype(f), gu.rounded(wt, dtype).astype(f))
    got = T.bf16_round(got) if dtype == "bf16" else got
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    ref, bound = T.bwd_weight_reference(case, dtype)
    for xa in T.input_candidates(x, sc, sh, case[9], dtype):
      got = T.conv_op(case, "bwd_weight", xa.astype(f), dyr.astype(f))
      assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert not (np.abs(ref * (1 + 1e-4) - ref) <= bound).all()


def test_the_gap_demonstrated():
  """Three corruptions of a float64 result that the whole-tensor rel-L2 < 1e-2 accepts: a tap dropped at one border pixel and a K slab
  zeroed in one element (the exact comparison rejects both and names the place), a split-K partial rounded to bf16 (the per-element
  bound rejects it: the forward on the float32 path split by channels, the bf16 path's float32 weight gradient split by image).
  The bound's reach shrinks with K: gamma(K) S grows like K^1.5 u |ref| on random data, so from K of about 2000 a bf16 partial (4e-3 of
  the partial) fits inside it - there the exact test and the rel-L2 are what is left."""
  case = (0, 2, 33, 70, 32, 128, 4, 1, 1, 0, 0, False)
  assert case in T.FWD_CASES
  ref, o = exact_reference(case, "fwd", "")
  xp = np.pad(o["xa"], ((0, 0), (1, 1), (1, 1), (0, 0)))
  tap = ref.copy()
  tap[1, 0, 3] -= xp[1, 0 + 1, 3 + 0] @ o["b"][1, 0]                     # tap (1, 0) of border pixel (n 1, y 0, x 3), all channels
  slab = ref.copy()
  slab[1, 4, 5, 7] -= xp[1, 4 + 2, 5 + 1, 16:] @ o["b"][2, 1, 16:, 7]     # the upper half of the channels of one tap, one element
  for bad in (tap, slab):
    assert (bad != ref).any() and gu.rel_l2(bad, ref) < 1e-2
    for dtype in ("f32", "bf16"):
      assert exact_mismatch(ref.astype(np.float32), ref, dtype) is None
      assert "differ" in exact_mismatch(bad.astype(np.float32), ref, dtype)
  assert "first at [[1, 0, 3, " in exact_mismatch(tap.astype(np.float32), ref, "f32")
  assert "1 of %d elements differ; first at [[1, 4, 5, 7]]" % ref.size in exact_mismatch(slab.astype(np.float32), ref, "bf16")
  # the bound, on the random-normal data of test_gpu_ops.py
  case = SMALL[0]
  x, wt, b, sc, sh = T.make_case(case)
  ref, bound = T.fwd_reference(case, "f32")
  xa, wr = T.ref_input(x, sc, sh, case[9], "f32"), gu.rounded(wt, "f32")
  first = T.conv_op(case, "fwd", xa[..., :16], wr[:, :, :16])
  rest = T.conv_op(case, "fwd", xa[..., 16:], wr[:, :, 16:], np.float32(b).astype(np.float64))
  assert (np.abs(first + rest - ref) <= bound).all()
  got = T.bf16_round(first).astype(np.float64) + rest
  assert gu.rel_l2(got, ref) < 1e-2 and (np.abs(got - ref) > bound).mean() > 0.5
  ref, bound = T.bwd_weight_reference(case, "bf16")
  xa = T.ref_input(x, sc, sh, case[9], "bf16")
  dyr = gu.rounded(np.random.default_rng(7).normal(size=(3, 8, 8, 64)), "bf16")
  one = (0, 1) + case[2:]
  first, rest = T.conv_op(one, "bwd_weight", xa[:1], dyr[:1]), T.conv_op((0, 2) + case[2:], "bwd_weight", xa[1:], dyr[1:])
  assert (np.abs(first + rest - ref) <= bound).all()
  got = T.bf16_round(first).astype(np.float64) + rest
  assert gu.rel_l2(got, ref) < 1e-2 and (np.abs(got - ref) > bound).mean() > 0.5

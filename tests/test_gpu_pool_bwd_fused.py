"""-m gpu: the VGG pools' gradients expanded inside the conv_c64 backward-data loader (IgemmArgs::pool_src, vp_tune "pool_bwd_fused").
Where the forward pass wrote pool codes, the backward-data launch of conv1_2 / conv2_2 reads the POOLED gradient and the codes and builds
its input patch in LDS - the bits maxpool_bwd_code_kernel would have written to memory for it to read back.  Same kernel family and the
same arithmetic on both sides, so everything here is compared bit for bit; the unfused side is also held against the numpy oracle at
the bf16 backward-data tolerance of tests/test_gpu_ops.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import nn_ops as ops
from voicepuppet_amd import _lib
from voicepuppet_amd.engine import PixReferEngine

import gpu_util as gu

pytestmark = pytest.mark.gpu
P = gu.ptr
TOL_BF16 = 1e-2          # tests/test_gpu_ops.py TOL["bf16"]


@pytest.fixture(autouse=True)
def small_grids_on_the_patch_kernel():
  L = _lib.lib()
  L.vp_tune(b"patch_min_blocks", 1)
  yield
  L.vp_tune(b"patch_min_blocks", -1)


# ---- op level: vp_conv3x3_c64_bwd_data_pooled, fused = 1 against fused = 0 ---------------------------------------------------------------

# (n, h, w, c): tiles are 4 x 16 pixels; the grid is at most 1024 blocks (64 channels) / 256 blocks (128 channels)
OP_CASES = [
    (1, 16, 16, 64),       # the smallest grid the patch plans take: one column of tiles, left and right patch borders outside the image
    (1, 16, 32, 64),       # 4 x 2 tiles: a column seam
    (2, 32, 48, 64),       # conv1_2 geometry of tests/test_gpu_ops.py
    (3, 36, 80, 64),       # 135 tiles: a grid that is no multiple of 8 (no XCD remap)
    (5, 64, 256, 64),      # 1280 tiles on 1024 blocks: some blocks walk two tiles, most one
    (1, 16, 16, 128),
    (1, 16, 32, 128),
    (2, 32, 48, 128),      # conv2_2 geometry
    (3, 36, 80, 128),
    (3, 64, 128, 128),     # 384 tiles on 256 blocks
    (9, 32, 64, 128),      # 288 tiles on 256 blocks
]


def _make(n, h, w, c, seed):
  rng = np.random.default_rng(seed)
  ho, wo = h // 2, w // 2
  code = rng.integers(0, 5, size=(n, ho, wo, c)).astype(np.uint8)
  code[:, :, :, c // 2 + 3] = 0                                    # a channel without gradient anywhere
  zero_px = rng.random((n, ho, wo)) < 0.15                          # whole pooled pixels (windows of every channel) without gradient
  code[zero_px] = 0
  code[0, 0, 0, :] = 0                                              # ... the first corner's among them
  code[-1, -1, -1, :] = 4                                           # the last corner: every channel's gradient to the very last pixel
  if ho > 1:
    code[:, 1, :, : c // 4] = 1 + (np.arange(wo)[None, :, None] % 4)  # a row with a known pattern
  dy = rng.normal(size=(n, ho, wo, c)) * np.exp(rng.normal(size=(n, ho, wo, c)))      # both signs, several binades
  dy[rng.random(dy.shape) < 0.2] = 0.0                              # zero gradients
  dy[rng.random(dy.shape) < 0.02] = -0.0
  wt = rng.normal(0, 0.05, (3, 3, c, c))
  ref = np.maximum(rng.normal(size=(n, h, w, c)), 0.0)              # a relu output: about half of it zero
  return code, dy, wt, ref


def _expand(code, dy):
  n, ho, wo, c = code.shape
  full = np.zeros((n, 2 * ho, 2 * wo, c), np.float64)
  for k in range(4):
    full[:, (k >> 1)::2, (k & 1)::2, :] = np.where(code == k + 1, dy, 0.0)
  return full


def _run_op(n, h, w, c, code, dy, wt, ref, fused):
  L = _lib.lib()
  d = gu.conv_desc(0, n, h, w, c, c, 3, 1, 1, "bf16")
  nbytes = L.vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(ctypes.byref(d))
  assert nbytes > 0
  ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
  dyd, refd, wd = gu.to_dev(dy, "bf16"), gu.to_dev(ref, "bf16"), gu.dev_f32(wt)
  cdd = torch.tensor(code).cuda().contiguous()
  dx = torch.full((n, h, w, c), float("nan"), dtype=torch.bfloat16, device="cuda")
  _lib.check(L.vp_conv3x3_c64_bwd_data_pooled(ctypes.byref(d), P(dyd), P(cdd), P(wd), P(refd), P(dx), P(ws), fused, gu.stream()),
             "vp_conv3x3_c64_bwd_data_pooled")
  torch.cuda.synchronize()
  return dx.view(torch.int16).cpu().numpy(), dx.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", OP_CASES)
def test_fused_equals_unfused_bit_for_bit(case):
  n, h, w, c = case
  code, dy, wt, ref = _make(n, h, w, c, seed=n * 1000 + h + w + c)
  assert set(np.unique(code)) == {0, 1, 2, 3, 4}
  assert (dy < 0).any() and (dy == 0).any()
  bits0, dx0 = _run_op(n, h, w, c, code, dy, wt, ref, 0)
  bits1, dx1 = _run_op(n, h, w, c, code, dy, wt, ref, 1)
  print("case", case, "max |dx|", float(np.abs(dx0).max()), "differing elements", int((bits0 != bits1).sum()))
  assert np.isfinite(dx0).all() and np.isfinite(dx1).all() and np.abs(dx0).max() > 0
  # borders, corners and the pixels either side of every tile seam (tiles: 4 rows x 16 columns), then everything
  rows = sorted({0, h - 1} | {y for y in range(h) if y % 4 in (0, 3)})
  cols = sorted({0, w - 1} | {x for x in range(w) if x % 16 in (0, 15)})
  for y in (0, h - 1):
    for x in (0, w - 1):
      assert np.array_equal(bits0[:, y, x, :], bits1[:, y, x, :]), ("corner", y, x)
  for y in rows:
    assert np.array_equal(bits0[:, y], bits1[:, y]), ("row", y)
  for x in cols:
    assert np.array_equal(bits0[:, :, x], bits1[:, :, x]), ("column", x)
  assert np.array_equal(bits0, bits1)
  # the unfused side against the oracle: numpy expansion, float64 convolution gradient, relu'(ref)
  dyr, wr, refr = gu.rounded(dy, "bf16"), gu.rounded(wt, "bf16"), gu.rounded(ref, "bf16")
  dxr, _, _ = ops.conv2d_bwd(np.zeros((n, h, w, c)), wr, _expand(code, dyr), 1, 1, need_dw=False)
  dxr = dxr * (refr > 0)
  err = gu.rel_l2(dx0, dxr)
  print("case", case, "unfused against the oracle: rel L2", err)
  assert err < TOL_BF16, err


def test_one_hot_gradients_land_where_the_code_says():
  """One pooled element with a gradient, at each window position in turn and at image corners / tile seams: the fused launch must put it
  at exactly the full-resolution pixel the code names (seen through the 3x3 footprint of the convolution)."""
  n, h, w, c = 1, 16, 32, 64
  rng = np.random.default_rng(3)
  wt = rng.normal(0, 0.05, (3, 3, c, c))
  ref = np.ones((n, h, w, c))
  for (py, px) in [(0, 0), (0, 15), (7, 0), (7, 15), (1, 7), (1, 8), (2, 7), (2, 8)]:        # corners, and around the seam at (4, 16)
    for k in range(5):
      code = np.zeros((n, h // 2, w // 2, c), np.uint8)
      dy = np.zeros((n, h // 2, w // 2, c))
      code[0, py, px, :] = k
      dy[0, py, px, :] = rng.normal(size=c) + 2.0
      bits0, dx0 = _run_op(n, h, w, c, code, dy, wt, ref, 0)
      bits1, dx1 = _run_op(n, h, w, c, code, dy, wt, ref, 1)
      assert np.array_equal(bits0, bits1), (py, px, k)
      nz = np.argwhere(np.abs(dx1[0]).sum(axis=-1) > 0)
      if k == 0:
        assert len(nz) == 0, (py, px)
      else:
        y, x = 2 * py + ((k - 1) >> 1), 2 * px + ((k - 1) & 1)
        assert nz[:, 0].min() == max(y - 1, 0) and nz[:, 0].max() == min(y + 1, h - 1), (py, px, k)
        assert nz[:, 1].min() == max(x - 1, 0) and nz[:, 1].max() == min(x + 1, w - 1), (py, px, k)


def test_shapes_outside_the_kernel_are_refused():
  L = _lib.lib()
  for (h, w, c) in [(18, 16, 64), (16, 24, 64), (16, 16, 32), (16, 16, 256), (8, 16, 64), (16, 8, 64)]:
    d = gu.conv_desc(0, 1, h, w, c, c, 3, 1, 1, "bf16")
    assert L.vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(ctypes.byref(d)) == 0
  d = gu.conv_desc(0, 1, 16, 16, 64, 64, 3, 1, 1, "f32")
  assert L.vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(ctypes.byref(d)) == 0


# ---- step level: three steps with the knob on and off ------------------------------------------------------------------------------------

TENSORS = ("v/conv1/conv1_1:dy", "v/conv1/conv1_2:dy", "v/conv2/conv2_2:dy")


@functools.lru_cache(maxsize=None)
def _three_steps(fused, keep=0, c64=1):
  """Three training steps at N = 4, 256 x 256, bf16 on the shipped schedule (as tests/test_gpu_pool_code.py); fused = the
  vp_tune("pool_bwd_fused") value the plan is made with, keep = the store_first_raw option, c64 = vp_tune("c64")."""
  n = 4
  L = _lib.lib()
  L.vp_tune(b"pool_bwd_fused", fused)
  L.vp_tune(b"c64", c64)
  try:
    eng = PixReferEngine(n, 256, 8, 8, dtype="bf16", training=True)
  finally:
    L.vp_tune(b"c64", 1)
    L.vp_tune(b"pool_bwd_fused", 1)
  eng.load_params(eng.random_params(11))
  if keep:
    eng.set_option("store_first_raw", 1)
  g = torch.Generator(device="cpu").manual_seed(12)
  out = {"losses": [], "fused": [], "codes": []}
  for _ in range(3):
    batch = [torch.rand(n, 256, 256, c, generator=g).cuda() for c in (6, 6, 3, 3)]
    eng.forward(*batch); eng.backward()
    out["fused"].append(int(eng.L.vp_pixrefer_counter(eng.h, b"pool_bwd_fused")))
    out["codes"].append(int(eng.L.vp_pixrefer_counter(eng.h, b"pool_codes_written")))
    eng.adam_step(3e-4)
    torch.cuda.synchronize()
    out["losses"].append(eng.tensor("losses").float().cpu().numpy().copy())
  for k in TENSORS:
    out[k] = eng.tensor(k).float().cpu().numpy()
  out["params_g"] = eng.params_g.float().cpu().numpy()
  out["params_d"] = eng.params_d.float().cpu().numpy()
  del eng
  return out


@pytest.mark.parametrize("knob", [1, 4, 2, 3])
def test_three_steps_bit_identical_fused_and_unfused(knob):
  """knob 1: the default (at N = 4 conv1_2 takes the pooled-source form, conv2_2 does from 16 frames up); 4: both layers at every size;
  2 / 3: one layer only."""
  a, b = _three_steps(knob), _three_steps(0)
  assert a["fused"] == [1, 1, 1] and b["fused"] == [0, 0, 0]
  assert a["codes"] == [1, 1, 1] and b["codes"] == [1, 1, 1]
  for la, lb in zip(a["losses"], b["losses"]):
    assert np.isfinite(la).all() and np.abs(la).max() > 0 and np.array_equal(la, lb), (la, lb)
  for k in TENSORS + ("params_g", "params_d"):
    assert np.abs(a[k]).max() > 0, k
    assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


def test_old_path_with_stored_tensors_and_on_the_patch_kernels():
  """store_first_raw = 1 (no codes) and vp_tune("c64", 0) (codes, but the backward-data launches on the patch kernels) keep the pool
  backward kernels; the step is the same step."""
  a, b, p = _three_steps(1), _three_steps(1, keep=1), _three_steps(1, c64=0)
  assert b["fused"] == [0, 0, 0] and b["codes"] == [0, 0, 0]
  assert p["fused"] == [0, 0, 0] and p["codes"] == [1, 1, 1]
  for la, lb in zip(a["losses"], b["losses"]):
    assert np.array_equal(la, lb), (la, lb)
  for k in TENSORS + ("params_g", "params_d"):
    assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))
  # (the patch kernels sum in another order: that plan is compared with itself, knob on against off)
  q = _three_steps(0, c64=0)
  assert q["fused"] == [0, 0, 0]
  for la, lb in zip(p["losses"], q["losses"]):
    assert np.isfinite(la).all() and np.array_equal(la, lb), (la, lb)
  for k in TENSORS + ("params_g", "params_d"):
    assert np.array_equal(p[k], q[k]), k


def test_backward_follows_what_the_forward_wrote():
  """Forward and backward are separate calls.  An option or knob changed in between must not send the backward pass to codes the forward
  pass did not write, nor away from the ones it wrote."""
  n = 2
  L = _lib.lib()
  got = {}
  L.vp_tune(b"pool_bwd_fused", 4)                        # both layers on the pooled-source path at this small batch
  try:
    for name, before, between in (("plain", 0, None), ("raw_then_default", 1, 0), ("default_then_raw", 0, 1), ("knob_off_after_plan", 0, "knob")):
      eng = PixReferEngine(n, 256, 8, 8, dtype="bf16", training=True)
      eng.load_params(eng.random_params(13))
      g = torch.Generator(device="cpu").manual_seed(14)
      batch = [torch.rand(n, 256, 256, c, generator=g).cuda() for c in (6, 6, 3, 3)]
      if before:
        eng.set_option("store_first_raw", 1)
      eng.forward(*batch)
      if between == "knob":
        L.vp_tune(b"pool_bwd_fused", 0)                  # read when a plan is made: this plan keeps its path
      elif between is not None:
        eng.set_option("store_first_raw", between)
      eng.backward()
      L.vp_tune(b"pool_bwd_fused", 4)
      torch.cuda.synchronize()
      codes = int(eng.L.vp_pixrefer_counter(eng.h, b"pool_codes_written"))
      fused = int(eng.L.vp_pixrefer_counter(eng.h, b"pool_bwd_fused"))
      assert codes == (0 if before else 1), (name, codes)
      assert fused == codes, (name, fused, codes)          # fused exactly where the forward pass wrote codes
      got[name] = (eng.tensor("v/conv1/conv1_2:dy").float().cpu().numpy(), eng.tensor("v/conv2/conv2_2:dy").float().cpu().numpy(),
                   eng.tensor("v/conv1/conv1_1:dy").float().cpu().numpy(), eng.grads_g.clone().cpu().numpy())
      del eng
  finally:
    L.vp_tune(b"pool_bwd_fused", 1)
  for name in ("raw_then_default", "default_then_raw", "knob_off_after_plan"):
    for x, y in zip(got["plain"], got[name]):
      assert np.abs(x).max() > 0 and np.array_equal(x, y), name

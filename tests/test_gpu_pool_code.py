"""-m gpu: the VGG pools' arg-max codes.  On the shipped (overlapped) bf16 schedule the fake half of conv1_2 / conv2_2 writes its 2x2
max pool and one byte per pooled element (IgemmArgs::pool_code: 0 = window maximum <= 0, 1 + k = first arg-max k in the order (0,0), (0,1),
(1,0), (1,1)) instead of the full-resolution output, and the pool's backward pass reads the codes (maxpool_bwd_code_kernel).  The chosen
arg-max and the zero rule are those of maxpool_bwd_kernel on the stored tensor, so a step is bit-identical with and without
vp_pixrefer_set_option("store_first_raw", 1), which keeps the stored tensors and the old backward kernel."""
import functools

import numpy as np
import pytest
import torch

from voicepuppet_amd import _lib
from voicepuppet_amd._lib import VP_BF16, VP_F32
from voicepuppet_amd.engine import PixReferEngine

import gpu_util as gu

pytestmark = pytest.mark.gpu
P = gu.ptr

TENSORS = ("v/pool1", "v/pool2", "v/conv1/conv1_2:dy", "v/conv2/conv2_2:dy", "v/conv1/conv1_1:dy")
FULL = ("v/conv1/conv1_2", "v/conv2/conv2_2")


@functools.lru_cache(maxsize=None)
def _three_steps(keep, c64=1):
  """Three training steps at N = 4, 256 x 256, bf16 on the shipped schedule; keep = the store_first_raw option.  c64 = 0 plans the
  pooled layers on the patch kernels (vp_tune("c64", 0)): the staged epilogue's code writer instead of conv_c64.hip's."""
  n = 4
  L = _lib.lib()
  L.vp_tune(b"c64", c64)
  try:
    eng = PixReferEngine(n, 256, 8, 8, dtype="bf16", training=True)
  finally:
    L.vp_tune(b"c64", 1)
  eng.load_params(eng.random_params(11))
  if keep:
    eng.set_option("store_first_raw", 1)
  g = torch.Generator(device="cpu").manual_seed(12)
  out = {"losses": [], "codes_written": []}
  for _ in range(3):
    batch = [torch.rand(n, 256, 256, c, generator=g).cuda() for c in (6, 6, 3, 3)]
    eng.forward(*batch); eng.backward()
    out["codes_written"].append(int(eng.L.vp_pixrefer_counter(eng.h, b"pool_codes_written")))
    eng.adam_step(3e-4)
    torch.cuda.synchronize()
    out["losses"].append(eng.tensor("losses").float().cpu().numpy().copy())
  for k in TENSORS:
    out[k] = eng.tensor(k).float().cpu().numpy()
  out["params_g"] = eng.params_g.float().cpu().numpy()
  out["params_d"] = eng.params_d.float().cpu().numpy()
  out["full"] = {}
  for k in FULL:
    try:
      y = eng.tensor(k).float()
      out["full"][k] = (True, bool(torch.isfinite(y).all()) and float(y[n:].abs().max()) > 0)
    except RuntimeError as e:
      out["full"][k] = (False, str(e))
  del eng
  return out


def test_three_steps_bit_identical_with_and_without_the_stored_tensors():
  a, b = _three_steps(0), _three_steps(1)
  for la, lb in zip(a["losses"], b["losses"]):
    assert np.isfinite(la).all() and np.array_equal(la, lb), (la, lb)
  for k in TENSORS + ("params_g", "params_d"):
    assert np.abs(a[k]).max() > 0, k
    assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


def test_patch_kernel_epilogues_write_the_same_codes():
  """The same comparison with the pooled layers on the patch kernels (the other kernels a plan can pick for them)."""
  a, b = _three_steps(0, 0), _three_steps(1, 0)
  assert a["codes_written"] == [1, 1, 1] and b["codes_written"] == [0, 0, 0]
  for la, lb in zip(a["losses"], b["losses"]):
    assert np.array_equal(la, lb), (la, lb)
  for k in TENSORS + ("params_g", "params_d"):
    assert np.abs(a[k]).max() > 0, k
    assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


def test_the_code_path_ran_on_the_default_schedule_only():
  assert _three_steps(0)["codes_written"] == [1, 1, 1]
  assert _three_steps(1)["codes_written"] == [0, 0, 0]


def test_full_resolution_tensors_refused_without_the_option():
  for k in FULL:
    stored, what = _three_steps(0)["full"][k]
    assert not stored and "store_first_raw" in what, (k, what)
    stored, ok = _three_steps(1)["full"][k]
    assert stored and ok, k


def test_backward_follows_what_the_forward_wrote():
  """Forward and backward are separate calls: an option set in between must not send the backward pass to the tensors the forward pass
  did not store."""
  n = 2
  got = []
  for flip in (0, 1):
    eng = PixReferEngine(n, 256, 8, 8, dtype="bf16", training=True)
    eng.load_params(eng.random_params(13))
    g = torch.Generator(device="cpu").manual_seed(14)
    batch = [torch.rand(n, 256, 256, c, generator=g).cuda() for c in (6, 6, 3, 3)]
    eng.forward(*batch)
    if flip:
      eng.set_option("store_first_raw", 1)
    eng.backward()
    torch.cuda.synchronize()
    assert int(eng.L.vp_pixrefer_counter(eng.h, b"pool_codes_written")) == 1
    got.append((eng.tensor("v/conv1/conv1_2:dy").float().cpu().numpy(), eng.tensor("v/conv2/conv2_2:dy").float().cpu().numpy(), eng.grads_g.clone().cpu().numpy()))
    del eng
  for x, y in zip(*got):
    assert np.abs(x).max() > 0 and np.array_equal(x, y)


# ---- op level: vp_maxpool2x2_bwd_code against vp_maxpool2x2_bwd -------------------------------------------------------------------------

def _codes(win):
  """win [..., 4]: the window values in the order (0,0), (0,1), (1,0), (1,1) -> uint8 codes (first arg-max, strict >; 0 unless max > 0)."""
  best = np.argmax(win, axis=-1)                 # the first maximum
  m = np.max(win, axis=-1)
  return np.where(m > 0, 1 + best, 0).astype(np.uint8)


def _image(win):
  """win [n, ho, wo, c, 4] -> x [n, 2 ho, 2 wo, c]"""
  n, ho, wo, c, _ = win.shape
  x = np.empty((n, 2 * ho, 2 * wo, c), win.dtype)
  for k in range(4):
    x[:, (k >> 1)::2, (k & 1)::2, :] = win[..., k]
  return x


def _crafted():
  z = -0.0
  w = [(1.5, 1.5, 1.5, 1.5), (0.25, 0.25, 0.25, 0.25),                                         # all four equal and positive
       (2, 2, 1, 0), (1, 2, 2, 0), (0, 1, 2, 2), (2, 0, 2, 1), (1, 3, 0, 3), (3, 1, 1, 3), (0, 2, 1, 2), (2, 2, 2, 1), (1, 2, 2, 2),   # ties
       (-1, 2, 2, -3), (0.5, 0.5, -1, z),
       (0, 0, 0, 0), (-1, -2, 0, -0.5), (-1, -1, -1, -1), (-3, -2, -1, -0.5),                     # all <= 0
       (z, z, z, z), (z, 0, z, 0), (0, z, 0, z), (z, -1, z, -2), (-1, z, -2, 0),                  # negative zero
       (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),                                    # a lone positive in each position
       (1, -1, -2, z), (-1, 1, z, -2), (z, -2, 1, -1), (-2, z, -1, 1)]
  return np.array(w, np.float64)


def _run_both(win, dtype, seed):
  L = _lib.lib()
  td, code = gu.tdtype(dtype), (VP_BF16 if dtype == "bf16" else VP_F32)
  n, ho, wo, c, _ = win.shape
  x = _image(win)
  cd = _codes(win)
  rng = np.random.default_rng(seed)
  dy = gu.rounded(rng.normal(size=(n, ho, wo, c)) + 3.0, dtype)          # (no zero gradients: a misrouted one is seen)
  xd = torch.tensor(x, dtype=torch.float64).to(td).cuda().contiguous()
  assert np.array_equal(np.signbit(xd.float().cpu().numpy()), np.signbit(x)) and np.array_equal(xd.float().cpu().numpy(), x)
  dyd = torch.tensor(dy, dtype=torch.float64).to(td).cuda().contiguous()
  cdd = torch.tensor(cd).cuda().contiguous()
  old = torch.full(x.shape, float("nan"), dtype=td, device="cuda")
  new = torch.full(x.shape, float("nan"), dtype=td, device="cuda")
  _lib.check(L.vp_maxpool2x2_bwd(P(xd), P(dyd), P(old), n, 2 * ho, 2 * wo, c, code, gu.stream()))
  _lib.check(L.vp_maxpool2x2_bwd_code(P(cdd), P(dyd), P(new), n, 2 * ho, 2 * wo, c, code, gu.stream()))
  torch.cuda.synchronize()
  old, new = old.float().cpu().numpy(), new.float().cpu().numpy()
  want = _image(np.stack([np.where(cd == k + 1, dy, 0.0) for k in range(4)], axis=-1))
  assert np.array_equal(new, want)
  assert np.array_equal(new, old)
  return cd


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_code_backward_on_crafted_windows(dtype):
  w = _crafted()
  assert np.array_equal(gu.rounded(w, dtype), w)                       # every crafted value is a bf16 number
  # every crafted window at every channel slot of a 16-channel pixel and in several pixel positions: [1, 6, nw, 16] windows, rotated
  nw = len(w)
  win = np.empty((1, 6, nw, 16, 4), np.float64)
  for r in range(6):
    for c in range(16):
      win[0, r, :, c, :] = np.roll(w, r * 16 + c, axis=0)
  cd = _run_both(win, dtype, 3)
  assert set(np.unique(cd)) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_code_backward_on_random_windows_with_many_ties(dtype):
  rng = np.random.default_rng(5)
  levels = np.array([-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5])      # 8 levels, all bf16 numbers
  win = levels[rng.integers(0, 8, size=(2, 16, 24, 64, 4))]
  tie = (win == win.max(axis=-1, keepdims=True)).sum(axis=-1) > 1        # the maximum stands at two or more positions
  assert tie.mean() >= 0.20, tie.mean()
  _run_both(win, dtype, 6)

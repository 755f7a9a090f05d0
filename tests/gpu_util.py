"""Helpers for the -m gpu parity tests: call libvp_hip.so through its C ABI on torch device buffers."""
import ctypes

import numpy as np
import torch

from voicepuppet_amd import _lib
from voicepuppet_amd._lib import ConvDesc, VP_BF16, VP_F32


def ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def tdtype(dtype):
  return torch.bfloat16 if dtype == "bf16" else torch.float32


def to_dev(a, dtype="f32"):
  return torch.tensor(np.asarray(a), dtype=torch.float32).to("cuda").to(tdtype(dtype)).contiguous()


def dev_f32(a):
  return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


def rounded(a, dtype):
  """What the device actually sees: float32, or float32 rounded to bf16."""
  t = torch.tensor(np.asarray(a), dtype=torch.float32)
  if dtype == "bf16":
    t = t.to(torch.bfloat16).float()
  return t.numpy().astype(np.float64)


def rel_l2(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def conv_desc(kind, n, h, w, cin, cout, k, s, p, dtype, in_act=0, out_act=0):
  return ConvDesc(kind, n, h, w, cin, cout, k, s, p, VP_BF16 if dtype == "bf16" else VP_F32, in_act, out_act)


def out_hw(d):
  if d.kind == 1:
    return 2 * d.h, 2 * d.w
  return (d.h + 2 * d.pad - d.ksize) // d.stride + 1, (d.w + 2 * d.pad - d.ksize) // d.stride + 1


SENTINEL = -1536.0                      # exact in bf16 and f32
SENTINEL_BYTE = 0xA5                    # the band of a byte buffer (the convolution workspace)
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}


def guarded(shape, row_elems=0, dtype="f32", fill=None, band=None, min_bytes=0):
  """(whole buffer, view of `shape` inside it, guard length): the view lies between two guard bands of `band` (default: SENTINEL,
  SENTINEL_BYTE for "u8"), each at least `row_elems` elements and `min_bytes` bytes long and a multiple of 256 bytes, so the view starts
  as aligned as an allocation of its own (256 bytes).  fill: None - NaN (zero for "u8"), or the values the view starts with."""
  td = _TORCH[dtype]
  if band is None:
    band = SENTINEL_BYTE if dtype == "u8" else SENTINEL
  es = torch.empty((), dtype=td).element_size()
  g = -(-max(row_elems, -(-min_bytes // es), 1) // 256) * 256
  n = int(np.prod(shape))
  whole = torch.full((n + 2 * g,), band, dtype=td, device="cuda")
  view = whole[g:g + n].view(*shape)
  assert whole.data_ptr() % 256 == 0 and view.data_ptr() % 256 == 0
  if fill is None:
    view.fill_(0 if dtype == "u8" else float("nan"))
  else:
    view.copy_(torch.as_tensor(np.asarray(fill), dtype=torch.float32).to(td))
  return whole, view, g


def assert_guards(whole, g, what="guard band"):
  band = SENTINEL_BYTE if whole.dtype == torch.uint8 else SENTINEL
  lo, hi = (whole[:g] != band).nonzero(), (whole[-g:] != band).nonzero()
  assert len(lo) == 0 and len(hi) == 0, "%s written: %d elements below the buffer (the last %d before it), %d above (the first %d after it)" % (
      what, len(lo), g - int(lo[0]) if len(lo) else 0, len(hi), int(hi[0]) + 1 if len(hi) else 0)


GUARD_BYTES = 4096


def nan_banded(a, dtype="f32"):
  """An operand between two bands of NaN (at least 4 KiB each): a read outside it that enters a sum shows in the output."""
  return None if a is None else guarded(np.shape(a), 0, dtype, fill=a, band=float("nan"), min_bytes=GUARD_BYTES)[1]


class Guarded:
  """The buffers of one convolution call.  guard = True: operands between NaN bands, the output (NaN-prefilled) and the workspace
  (zeroed) between sentinel bands that check() asserts untouched; guard = False: plain allocations of exactly the right size."""

  def __init__(self, op, guard):
    self.op, self.guard, self.bands = op, guard, []

  def operand(self, a, dtype="f32"):
    if a is None:
      return None
    return nan_banded(a, dtype) if self.guard else (to_dev(a, dtype) if dtype != "f32" else dev_f32(a))

  def output(self, shape, dtype):
    if not self.guard:
      return torch.full(shape, float("nan"), dtype=tdtype(dtype), device="cuda")
    whole, view, g = guarded(shape, 0, dtype, min_bytes=GUARD_BYTES)
    self.bands.append((whole, g, "output"))
    return view

  def workspace(self, d):
    if not self.guard:
      return workspace(d)
    n = _lib.lib().vp_conv_workspace_bytes(ctypes.byref(d))
    assert n > 0
    whole, view, g = guarded((n,), 0, "u8", min_bytes=GUARD_BYTES)
    self.bands.append((whole, g, "workspace"))
    return view

  def check(self):
    torch.cuda.synchronize()
    for whole, g, name in self.bands:
      assert_guards(whole, g, "%s: guard band of the %s" % (self.op, name))


def workspace(d):
  n = _lib.lib().vp_conv_workspace_bytes(ctypes.byref(d))
  assert n > 0
  return torch.zeros(n, dtype=torch.uint8, device="cuda")


def conv_fwd(d, x, scale, shift, w, bias, dtype, guard=True, raw=False):
  """raw: the device tensor itself (its bits) instead of float64 values."""
  L = _lib.lib()
  ho, wo = out_hw(d)
  b = Guarded("vp_conv_fwd", guard)
  y = b.output((d.n, ho, wo, d.cout), dtype)
  ws = b.workspace(d)
  xd, wd = b.operand(x, dtype), b.operand(w)
  sc, sh, bs = b.operand(scale), b.operand(shift), b.operand(bias)
  _lib.check(L.vp_conv_fwd(ctypes.byref(d), ptr(xd), ptr(sc), ptr(sh), ptr(wd), ptr(bs), ptr(y), ptr(ws), stream()), "vp_conv_fwd")
  b.check()
  return y.cpu() if raw else y.float().cpu().numpy().astype(np.float64)


def conv_bwd_data(d, dy, w, dtype, guard=True, raw=False):
  L = _lib.lib()
  b = Guarded("vp_conv_bwd_data", guard)
  dx = b.output((d.n, d.h, d.w, d.cin), dtype)
  ws = b.workspace(d)
  dyd, wd = b.operand(dy, dtype), b.operand(w)
  _lib.check(L.vp_conv_bwd_data(ctypes.byref(d), ptr(dyd), ptr(wd), ptr(dx), ptr(ws), stream()), "vp_conv_bwd_data")
  b.check()
  return dx.cpu() if raw else dx.float().cpu().numpy().astype(np.float64)


def conv_bwd_weight(d, x, scale, shift, dy, wshape, dtype, guard=True, raw=False):
  L = _lib.lib()
  b = Guarded("vp_conv_bwd_weight", guard)
  dw = b.output(tuple(wshape), "f32")
  ws = b.workspace(d)
  xd, dyd = b.operand(x, dtype), b.operand(dy, dtype)
  sc, sh = b.operand(scale), b.operand(shift)
  _lib.check(L.vp_conv_bwd_weight(ctypes.byref(d), ptr(xd), ptr(sc), ptr(sh), ptr(dyd), ptr(dw), ptr(ws), stream()), "vp_conv_bwd_weight")
  b.check()
  return dw.cpu() if raw else dw.cpu().numpy().astype(np.float64)

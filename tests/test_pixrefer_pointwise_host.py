"""Host side of the PixReferNet pointwise entry points (include/vp_hip.h, "The PixReferNet training step's pointwise kernels one at a
time"): every class of bad argument an entry point documents comes back as VP_ERR_ARG with a message naming the entry point.  The
check precedes any launch, so nothing here needs a device.  Also the CPU half of tests/test_gpu_pixrefer_pointwise_ops.py's offset
case: a reduce pass with float32 accumulators violates the bound that case holds the kernel to."""
import ctypes

import numpy as np

from voicepuppet_amd import _lib
from voicepuppet_amd._lib import BN_PATH_ONE_LAUNCH as P1, BN_PATH_PLANNER as P0, BN_PATH_TWO_PASS as P2, VP_BF16 as BF, VP_F32 as F32

import test_gpu_pixrefer_pointwise_ops as ops

VP_ERR_ARG = -1
_page = ctypes.create_string_buffer(4096)                        # never dereferenced: every call below is refused first
B = ctypes.c_void_p(ctypes.addressof(_page))
N = None


def test_every_entry_point_refuses_its_bad_arguments():
  L = _lib.lib()
  fwd = lambda y=B, g=1, pg=8, c=8, dt=F32, gamma=B, beta=B, sc=B, sh=B, mu=B, rs=B, path=P0, ws=B: L.vp_bn_groups_fwd(
      y, g, pg, c, dt, gamma, beta, 1e-5, sc, sh, mu, rs, N, N, path, ws, N)
  bwd = lambda y=B, dz=B, dy=B, g=1, pg=8, c=8, dt=F32, gamma=B, mu=B, rs=B, c1=B, c2=B, dg=B, db=B, path=P0, ws=B: L.vp_bn_groups_bwd(
      y, dz, dy, g, pg, c, dt, gamma, mu, rs, c1, c2, dg, db, N, 0, path, ws, N)
  tail = lambda y=B, dz=B, dy=B, g=1, pg=8, c=8, dt=F32, part=B, nch=1, raw=0, c1=B, dg=B: L.vp_bn_groups_bwd_tail(
      y, dz, dy, g, pg, c, dt, B, B, B, part, nch, raw, c1, B, dg, B, N, 0, N)
  col = lambda x=B, g=1, pg=8, c=8, creal=4, dt=F32, o=B, ws=B: L.vp_colsum_groups(x, g, pg, c, creal, dt, o, 0, ws, N)
  act = lambda y=B, sc=B, sh=B, g=1, pg=8, c=8, dt=F32, a=B, b=B: L.vp_act_apply(y, sc, sh, g, pg, c, dt, a, b, N)
  comp = lambda y4=B, m=B, part=B, n=1, hw=8, dt=F32, din=B: L.vp_composite_fwd_train(y4, B, m, B, B, B, din, B, part, n, hw, dt, N)
  cbw = lambda o4=B, dd=B, dy=B, n=1, hw=8, dt=F32: L.vp_composite_bwd(o4, B, B, B, dd, B, dy, n, hw, 500.0, dt, N)
  calls = {
      "vp_bn_groups_fwd null y": lambda: fwd(y=N), "vp_bn_groups_fwd null gamma": lambda: fwd(gamma=N), "vp_bn_groups_fwd null rstd": lambda: fwd(rs=N),
      "vp_bn_groups_fwd groups=0": lambda: fwd(g=0), "vp_bn_groups_fwd pixels=0": lambda: fwd(pg=0), "vp_bn_groups_fwd c=6": lambda: fwd(c=6),
      "vp_bn_groups_fwd bf16 c=12": lambda: fwd(c=12, dt=BF), "vp_bn_groups_fwd dtype=2": lambda: fwd(dt=2), "vp_bn_groups_fwd path=3": lambda: fwd(path=3),
      "vp_bn_groups_fwd two-pass c=12 (256 % 3)": lambda: fwd(c=12, path=P2), "vp_bn_groups_fwd planner c=12 pixels=2049": lambda: fwd(c=12, pg=2049),
      "vp_bn_groups_fwd two-pass without workspace": lambda: fwd(path=P2, ws=N),
      "vp_bn_groups_bwd null dz": lambda: bwd(dz=N), "vp_bn_groups_bwd null c1": lambda: bwd(c1=N), "vp_bn_groups_bwd null dbeta": lambda: bwd(db=N),
      "vp_bn_groups_bwd pixels=-1": lambda: bwd(pg=-1), "vp_bn_groups_bwd c=4 bf16": lambda: bwd(c=4, dt=BF), "vp_bn_groups_bwd path=-1": lambda: bwd(path=-1),
      "vp_bn_groups_bwd two-pass c=24 bf16 (256 % 3)": lambda: bwd(c=24, dt=BF, path=P2), "vp_bn_groups_bwd two-pass without workspace": lambda: bwd(pg=4000, ws=N),
      "vp_bn_groups_bwd_tail null partial": lambda: tail(part=N), "vp_bn_groups_bwd_tail nchunk=0": lambda: tail(nch=0), "vp_bn_groups_bwd_tail raw=2": lambda: tail(raw=2),
      "vp_bn_groups_bwd_tail c=10": lambda: tail(c=10), "vp_bn_groups_bwd_tail groups=0": lambda: tail(g=0), "vp_bn_groups_bwd_tail null dgamma": lambda: tail(dg=N),
      "vp_colsum_groups creal=0": lambda: col(creal=0), "vp_colsum_groups creal>c": lambda: col(creal=9), "vp_colsum_groups c=12": lambda: col(c=12, creal=4),
      "vp_colsum_groups null out": lambda: col(o=N), "vp_colsum_groups pixels=0": lambda: col(pg=0), "vp_colsum_groups null workspace": lambda: col(ws=N),
      "vp_act_apply scale without shift": lambda: act(sh=N), "vp_act_apply no output": lambda: act(a=N, b=N), "vp_act_apply c=12 bf16": lambda: act(c=12, dt=BF),
      "vp_act_apply null y": lambda: act(y=N), "vp_act_apply groups=0": lambda: act(g=0),
      "vp_relu_bwd n=0": lambda: L.vp_relu_bwd(B, B, 0, F32, N), "vp_relu_bwd n=12 bf16": lambda: L.vp_relu_bwd(B, B, 12, BF, N),
      "vp_relu_bwd null d": lambda: L.vp_relu_bwd(B, N, 8, F32, N), "vp_relu_bwd dtype=7": lambda: L.vp_relu_bwd(B, B, 8, 7, N),
      "vp_tap_gather null bias": lambda: L.vp_tap_gather(B, N, B, 1, 5, 7, 4, 1, N), "vp_tap_gather ksize=5": lambda: L.vp_tap_gather(B, B, B, 1, 5, 7, 5, 1, N),
      "vp_tap_gather no output row": lambda: L.vp_tap_gather(B, B, B, 1, 1, 7, 4, 1, N), "vp_tap_gather n=0": lambda: L.vp_tap_gather(B, B, B, 0, 5, 7, 4, 1, N),
      "vp_tap_spread ld_dy=0": lambda: L.vp_tap_spread(B, 0, B, 1, 5, 7, 1, F32, N), "vp_tap_spread null dys": lambda: L.vp_tap_spread(B, 8, N, 1, 5, 7, 1, F32, N),
      "vp_tap_spread win=1": lambda: L.vp_tap_spread(B, 8, B, 1, 5, 1, 1, F32, N), "vp_tap_spread dtype=2": lambda: L.vp_tap_spread(B, 8, B, 1, 5, 7, 1, 2, N),
      "vp_pack_inputs fg_c=4": lambda: L.vp_pack_inputs(B, B, 4, B, B, B, B, 1, 8, 1, F32, N), "vp_pack_inputs train without din": lambda: L.vp_pack_inputs(B, B, 6, B, B, N, B, 1, 8, 1, F32, N),
      "vp_pack_inputs hw=0": lambda: L.vp_pack_inputs(B, B, 6, B, B, B, B, 1, 0, 0, F32, N), "vp_pack_inputs null gfg": lambda: L.vp_pack_inputs(B, B, 6, B, N, B, B, 1, 8, 0, F32, N),
      "vp_composite_fwd_train null masks": lambda: comp(m=N), "vp_composite_fwd_train null partial": lambda: comp(part=N), "vp_composite_fwd_train n=0": lambda: comp(n=0),
      "vp_composite_fwd_train null din": lambda: comp(din=N), "vp_composite_fwd_train dtype=3": lambda: comp(dt=3),
      "vp_composite_bwd null out4": lambda: cbw(o4=N), "vp_composite_bwd null d_din": lambda: cbw(dd=N), "vp_composite_bwd hw=0": lambda: cbw(hw=0),
      "vp_composite_bwd null dy4": lambda: cbw(dy=N),
      "vp_perceptual half=0": lambda: L.vp_perceptual(B, B, B, 0, 500.0, F32, N), "vp_perceptual half=12 bf16": lambda: L.vp_perceptual(B, B, B, 12, 500.0, BF, N),
      "vp_perceptual null partial": lambda: L.vp_perceptual(B, B, N, 8, 500.0, F32, N), "vp_perceptual half=6": lambda: L.vp_perceptual(B, B, B, 6, 500.0, F32, N),
      "vp_loss_final n_comp=0": lambda: L.vp_loss_final(B, 0, B, 1, 3.0, 3.0, 500.0, 1.0, B, N), "vp_loss_final n_out=0": lambda: L.vp_loss_final(B, 1, B, 1, 0.0, 3.0, 500.0, 1.0, B, N),
      "vp_loss_final null losses": lambda: L.vp_loss_final(B, 1, B, 1, 3.0, 3.0, 500.0, 1.0, N, N), "vp_loss_final null perc": lambda: L.vp_loss_final(B, 1, N, 1, 3.0, 3.0, 500.0, 1.0, B, N),
  }
  new = {"vp_bn_groups_fwd", "vp_bn_groups_bwd", "vp_bn_groups_bwd_tail", "vp_colsum_groups", "vp_act_apply", "vp_relu_bwd", "vp_tap_gather", "vp_tap_spread",
         "vp_pack_inputs", "vp_composite_fwd_train", "vp_composite_bwd", "vp_perceptual", "vp_loss_final"}
  assert {k.split()[0] for k in calls} == new
  for name, call in calls.items():
    assert call() == VP_ERR_ARG, name
    assert L.vp_last_error().startswith(name.split()[0].encode() + b":"), (name, L.vp_last_error())
  assert not any(_page.raw)                                      # nothing was written through the dummy pointer


def test_size_queries():
  L = _lib.lib()
  for g, pg, c, dtype in [(1, 1, 8, "f32"), (3, 5500, 512, "f32"), (1, 8209, 512, "f32"), (3, 180000, 8, "bf16"), (1, 300, 512, "bf16")]:
    assert L.vp_bn_groups_workspace_bytes(g, pg, c, ops.DT[dtype]) == g * ops.bn_nchunk(pg, c, g, dtype) * 2 * c * 8 + 1024
  assert [L.vp_bn_groups_workspace_bytes(*a) for a in [(0, 8, 8, F32), (1, 0, 8, F32), (1, 8, 6, F32), (1, 8, 12, F32), (1, 8, 8, 2), (1, 8, 8, BF - 2)]] == [0] * 6
  assert [L.vp_composite_nblocks(*a) for a in [(1, 7), (1, 512), (1, 262144 + 513), (0, 8), (1, 0)]] == [1, 2, 1024, 0, 0]
  assert [ops.composite_nblocks(*a) for a in [(1, 7), (1, 512), (1, 262144 + 513)]] == [1, 2, 1024]
  for dtype in ops.DTYPES:
    assert [L.vp_perceptual_nblocks(h, ops.DT[dtype]) for h in ops.perceptual_halves(dtype)] == [ops.perceptual_nblocks(h, dtype) for h in ops.perceptual_halves(dtype)]
  assert L.vp_perceptual_nblocks(0, F32) == 0 and L.vp_perceptual_nblocks(12, BF) == 0 and L.vp_perceptual_nblocks(8, 5) == 0


def test_float32_accumulators_violate_the_offset_case_bound():
  """What the GPU file's offset case (mean 100 .. 200, deviation 0.05, Pg = 4100) is for: bn_reduce_kernel with float32 accumulators,
  restated in numpy, leaves the variance bound by orders of magnitude; with float64 accumulators the same restatement holds it."""
  x, c, pg = ops.offset_case()
  ref = ops.bn_fwd_ref(x, np.ones(c), np.zeros(c), ops.BN_EPS, ops.bn_nchunk(pg, c, 1, "f32"))
  _, var32 = ops.bn_stats_float32_accumulators(x)
  excess = np.abs(var32 - ref["var"][0]) / ref["var"][1]
  assert excess.min() > 100, excess
  m64 = x[0].sum(0) / pg
  var64 = (x[0] * x[0]).sum(0) / pg - m64 * m64
  assert (np.abs(var64 - ref["var"][0]) <= ref["var"][1]).all()


def test_truncation_is_not_the_bf16_pack():
  """The planted values of the gradient-transport case separate nearest-even from truncation and from round-half-up."""
  x = ops.pack_plants()
  rne = ops.bf16_round(x).view(np.uint32)
  assert (ops.bf16_truncate(x).view(np.uint32) != rne).sum() >= 3
  half_up = ((x.view(np.uint32).astype(np.uint64) + 0x8000) & 0xffff0000).astype(np.uint32)
  assert (half_up != rne).sum() >= 2

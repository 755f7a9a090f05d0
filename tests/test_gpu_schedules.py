"""-m gpu: the schedule options that choose which executor lane (stream + its split-K scratch + its batch-norm partials) a pass runs
on.  tests/test_gpu_soak.py covers "overlap" 0 / 1 and streams = 1; here every other option is compared against the default schedule.
Two lanes that shared a scratch set, or a pass enqueued on the wrong lane, would race - so everything must stay bit-identical:
  * one engine per option setting against the default engine, small widths, several optimiser steps;
  * the staged generator backward of the data-parallel path with the foreground encoder chain on its own fourth stream against the
    same on three streams, full width (where the few-pixel and register-resident kernel families of those layers are chosen)."""
import pytest
import torch

from test_gpu_soak import _first_difference
from voicepuppet_amd import _lib
from voicepuppet_amd._handle import stream
from voicepuppet_amd.engine import PixReferEngine

pytestmark = pytest.mark.gpu

# batch 2 is the smallest at which the discriminator's three groups, the half-batch VGG plans and the float32 few-pixel tensors all exist
# ("bwd_sums_in_epilogue" is not a schedule option: 0 forms the batch-norm backward's sums in another kernel, in another order - gradients
# then differ in the last bits, 1.6e-5 at these shapes)
OPTIONS = [("use_streams", 3), ("d_backward_fork", 0), ("d_backward_fork", 1), ("d_beside_vgg", 0), ("vgg_real_fork", 0), ("vgg_real_fork", 9)]


def _batches(n, steps, seed):
  dev = torch.device("cuda", 0)
  g = torch.Generator(device=dev).manual_seed(seed)
  return [[torch.rand(n, 256, 256, c, device=dev, generator=g) for c in (6, 6, 3, 3)] for _ in range(steps)]


def test_every_schedule_option_is_bit_identical_to_the_default():
  n, ngf = 2, 8
  ref = PixReferEngine(n, 256, ngf, ngf, dtype="bf16", training=True)
  p = ref.random_params(seed=0)
  ref.load_params(p)
  engines = []
  for key, value in OPTIONS:
    e = PixReferEngine(n, 256, ngf, ngf, dtype="bf16", training=True)
    e.load_params(p)
    if key == "use_streams":
      e.use_streams(value)
    else:
      e.set_option(key, value)
    engines.append(e)
  for s, batch in enumerate(_batches(n, 3, seed=11)):
    for e in [ref] + engines:
      e.train_step(*batch, lr=3e-4)
    torch.cuda.synchronize()
    for (key, value), e in zip(OPTIONS, engines):
      diff = _first_difference(ref, e)
      assert diff is None, "step %d, %s = %d: %s" % (s, key, value, diff)
  assert torch.isfinite(ref.params_g).all() and torch.isfinite(ref.params_d).all()


def _staged_backward(e):
  """The backward pass as the data-parallel host drives it (engine.train_step with a group), without the collectives."""
  L = _lib.lib()
  _lib.check(L.vp_pixrefer_backward_d_fork(e.h, stream()), "vp_pixrefer_backward_d_fork")
  for stage in range(L.vp_pixrefer_backward_g_stages()):
    e.backward_g_stage(stage)
  _lib.check(L.vp_pixrefer_backward_d_join(e.h, stream()), "vp_pixrefer_backward_d_join")


def test_staged_backward_on_four_streams_matches_three():
  """The only path on which the fourth lane carries the foreground chain without the fused update running beside it."""
  n = 4
  a = PixReferEngine(n, 256, 64, 64, dtype="bf16", training=True)
  b = PixReferEngine(n, 256, 64, 64, dtype="bf16", training=True)
  p = a.random_params(seed=0)
  a.load_params(p)
  b.load_params(p)
  a.use_streams(4)
  b.use_streams(3)
  for s, batch in enumerate(_batches(n, 2, seed=12)):
    for e in (a, b):
      e.forward(*batch)
      _staged_backward(e)
      e.adam_step(3e-4)
    torch.cuda.synchronize()
    diff = _first_difference(a, b)
    assert diff is None, "step %d: %s" % (s, diff)
    assert a.grads_g.abs().sum() > 0 and a.grads_d.abs().sum() > 0

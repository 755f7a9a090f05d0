"""Streaming groups, host side (vp_bfmstream_group_*): bad descriptors are refused with a reason, the workspace grows with the slots, and
every bucket plan reduces each GEMM row as the batch-1 window plan does.  No GPU: these entry points are host-only."""
import ctypes

import pytest


def _lib():
  from voicepuppet_amd import _lib
  return _lib.lib()


def _desc(slots, **kw):
  from voicepuppet_amd.stream import group_desc
  return group_desc(slots, **kw)


def _bytes(d):
  return int(_lib().vp_bfmstream_group_workspace_bytes(ctypes.byref(d)))


def test_descriptor_size_matches_binding():
  from voicepuppet_amd._lib import BfmStreamGroupDesc
  assert _lib().vp_bfmstream_group_desc_size() == ctypes.sizeof(BfmStreamGroupDesc)


@pytest.mark.parametrize("field,value", [("struct_bytes", 4), ("struct_bytes", 36), ("slots", 0), ("slots", 129), ("slots", -1),
                                         ("max_chunk_frames", 0), ("max_chunk_frames", 1025), ("num_mel_bins", 64), ("trunk_dtype", 7),
                                         ("upper_hz", 9000.0)])
def test_bad_descriptors_are_refused(field, value):
  d = _desc(4)
  assert _bytes(d) > 0
  setattr(d, field, value)
  assert _bytes(d) == 0
  assert b"bad descriptor" in _lib().vp_last_error()


@pytest.mark.parametrize("slots,mcf", [(8, 1024), (128, 200), (16, 700)])
def test_chunks_past_the_addressing_limit_are_refused(slots, mcf):
  """A batch whose tensors would leave the 32-bit lane offsets of the kernels the one-stream plan runs is refused at create time, with
  the reason, instead of failing (or changing kernels, and so bits) at push time."""
  d = _desc(slots, max_chunk_frames=mcf)
  assert _bytes(d) == 0
  assert b"32-bit lane offsets" in _lib().vp_last_error()
  assert _bytes(_desc(1, max_chunk_frames=mcf)) > 0


def test_workspace_grows_with_slots():
  for dtype in ("f32", "bf16"):
    sizes = [_bytes(_desc(s, dtype=dtype)) for s in (1, 2, 4, 16, 64, 128)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes


@pytest.mark.parametrize("dtype,mcf", [("f32", 1), ("f32", 5), ("bf16", 1), ("bf16", 5)])
def test_bucket_plans_reduce_rows_as_the_batch1_plan(dtype, mcf):
  """Every GEMM of every bucket plan (batch 1, 2, 4, .., 64) has the batch-1 window plan's tile, K split and kernel."""
  L = _lib()
  d = _desc(64, max_chunk_frames=mcf, dtype=dtype)
  info = (ctypes.c_int * 8)()
  gemm, ref = 0, []
  while L.vp_bfmstream_group_plan_info(ctypes.byref(d), 0, gemm, info) == 0:
    assert info[0] == 1
    ref.append(tuple(info[1:4]))
    gemm += 1
  assert gemm > 40
  batches = []
  for b in range(1, 16):
    if L.vp_bfmstream_group_plan_info(ctypes.byref(d), b, 0, info) != 0:
      break
    batches.append(info[0])
    for g in range(gemm):
      assert L.vp_bfmstream_group_plan_info(ctypes.byref(d), b, g, info) == 0
      assert tuple(info[1:4]) == ref[g], (info[0], g)
  assert batches == [2, 4, 8, 16, 32, 64]
  assert any(r[1] > 1 for r in ref)       # (the batch-1 plan does split K somewhere: the pin matters)


def test_window_plans_unchanged_by_the_pin_option():
  """The batch-1 bucket plan is built without a pin: the existing plan_fwd path.  Its GEMMs' tile, K split and kernel are those the tree
  before stream groups chose for the same geometries (tests/golden/stream_window_plans.json), for both trunks and chunk sizes."""
  import json
  import os
  gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_window_plans.json")))
  want = {tuple(r[:4]): tuple(r[4:]) for r in gold["rows"]}
  L = _lib()
  info = (ctypes.c_int * 8)()
  seen = 0
  for dtype in ("f32", "bf16"):
    for mcf in (1, 5):
      d = _desc(1, max_chunk_frames=mcf, dtype=dtype)
      g = 0
      while L.vp_bfmstream_group_plan_info(ctypes.byref(d), 0, g, info) == 0:
        assert info[0] == 1
        assert tuple(info[1:4]) == want[tuple(info[4:8])], (dtype, mcf, g, tuple(info[4:8]))
        g += 1
        seen += 1
  assert seen > 160

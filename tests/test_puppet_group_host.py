"""Frames for stream groups, host side (vp_puppet_*, voicepuppet_amd.stream.PuppetRowPlan / launch_tables): the symbols are exported and
bound, bad descriptors are refused with a reason, the workspace grows with the slots, and the per-row table of a push is a pure function
of the frame counts.  No GPU: these entry points and functions are host-only."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("vp_puppet_desc_size", "vp_puppet_workspace_bytes", "vp_puppet_create", "vp_puppet_destroy", "vp_puppet_attach",
           "vp_puppet_set_backgrounds", "vp_puppet_splice", "vp_puppet_condition", "vp_puppet_tensor", "vp_puppet_slot_info",
           "vp_bfm_reconstruct_rows")


def _lib():
  from voicepuppet_amd import _lib
  return _lib.lib()


def _desc(slots, **kw):
  from voicepuppet_amd.stream import puppet_desc
  return puppet_desc(slots, **kw)


def _bytes(d):
  return int(_lib().vp_puppet_workspace_bytes(ctypes.byref(d)))


def test_symbols_are_exported_and_bound():
  from voicepuppet_amd import _lib as binding
  L = _lib()
  for name in SYMBOLS:
    assert name in binding.exported_symbols(), name
    assert getattr(L, name).argtypes is not None, name


def test_descriptor_size_matches_binding():
  from voicepuppet_amd._lib import PuppetDesc
  assert _lib().vp_puppet_desc_size() == ctypes.sizeof(PuppetDesc)


@pytest.mark.parametrize("field,value", [("slots", 0), ("slots", 129), ("slots", -1), ("frame_batch", 0), ("frame_batch", -3),
                                         ("frame_batch", 1025), ("img_size", 500), ("img_size", 128), ("img_size", 0), ("img_size", 8192),
                                         ("struct_bytes", 4), ("struct_bytes", 24), ("face_size", 0)])
def test_bad_descriptors_are_refused(field, value):
  d = _desc(4)
  assert _bytes(d) > 0
  setattr(d, field, value)
  assert _bytes(d) == 0
  msg = _lib().vp_last_error()
  assert b"bad descriptor" in msg and field.encode() in msg, msg


def test_create_refuses_a_bad_descriptor_and_a_small_workspace():
  L = _lib()
  h = ctypes.c_void_p()
  d = _desc(0)
  assert L.vp_puppet_create(ctypes.byref(d), ctypes.c_void_p(4096), 1 << 30, None, ctypes.byref(h)) != 0 and not h.value
  assert b"bad descriptor" in L.vp_last_error()
  d = _desc(2)
  assert L.vp_puppet_create(ctypes.byref(d), ctypes.c_void_p(4096), 1024, None, ctypes.byref(h)) != 0 and not h.value
  assert b"workspace too small" in L.vp_last_error()


def test_workspace_grows_with_slots_and_image_size():
  sizes = [_bytes(_desc(s)) for s in (1, 2, 4, 16, 64, 128)]
  assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
  # two float panels of H x H x 3 per slot are the bulk of it
  assert sizes[-1] >= 128 * 2 * 512 * 512 * 3 * 4
  assert _bytes(_desc(4, img_size=256)) < _bytes(_desc(4, img_size=512)) < _bytes(_desc(4, img_size=1024))


def test_row_plan_is_a_pure_function_of_the_frame_counts():
  """A scripted sequence of pushes over 3 slots with a reset_slot in the middle: each slot's angles concatenate to
  infer_bfmvid.angle_sequence(total) and its frame indices to 0 .. total-1, for the clip before the reset and the one after it."""
  from voicepuppet_amd.pixrefer.infer_bfmvid import angle_sequence
  from voicepuppet_amd.stream import PuppetRowPlan
  plan = PuppetRowPlan(3)
  script = [[0, 0, 0], [1, 0, 3], [2, 5, 0], [0, 1, 1], "reset 1", [7, 2, 0], [1, 1, 1], [0, 13, 4], [3, 0, 0]]
  clips = {s: [([], [])] for s in range(3)}
  for step in script:
    if isinstance(step, str):
      s = int(step.split()[1])
      plan.reset_slot(s)
      clips[s].append(([], []))
      continue
    slot, g, ang = plan.rows(step)
    assert slot.dtype == np.int32 and ang.dtype == np.float32 and ang.shape == (sum(step), 3)
    assert list(slot) == [s for s in range(3) for _ in range(step[s])]            # packed in slot order
    for s in range(3):
      clips[s][-1][0].extend(g[slot == s])
      clips[s][-1][1].extend(ang[slot == s])
  assert [len(c) for c in clips.values()] == [1, 2, 1]
  for s, cs in clips.items():
    for g, ang in cs:
      assert list(g) == list(range(len(g))), (s, g)
      assert np.array_equal(np.array(ang, np.float32).reshape(-1, 3), angle_sequence(len(g))), s
  assert [plan.frame[s] for s in range(3)] == [14, 16, 9]
  # the same script again from a fresh plan gives the same rows: no hidden state
  again = PuppetRowPlan(3)
  a = again.rows([5, 0, 2])
  b = PuppetRowPlan(3).rows([5, 0, 2])
  assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_launch_tables():
  """Rows of slots without coefficients are not rendered; one texture per rendered slot, taken from its first row; backgrounds by global
  frame index % 100; the last launch padded with the last row."""
  from voicepuppet_amd.stream import launch_tables
  slot = np.array([0, 0, 1, 2, 2, 2], np.int32)
  g = np.array([99, 100, 7, 0, 1, 2], np.int64)
  bg_row = np.full(100, -1, np.int32)
  bg_row[0], bg_row[99], bg_row[2] = 0, 1, 2
  render, tex_src, tex_row, cond = launch_tables(slot, g, [True, False, True], bg_row, 4)
  assert render[:, 0].tolist() == [0, 0, 2, 2, 2] and render[:, 1].tolist() == [0, 1, 3, 4, 5]
  assert tex_src.tolist() == [0, 2] and tex_row.tolist() == [0, 0, 1, 1, 1]
  assert cond.shape == (8, 4) and cond.dtype == np.int32
  assert cond[:6, 0].tolist() == slot.tolist() and cond[:6, 3].tolist() == g.tolist()
  assert cond[:6, 1].tolist() == [0, 1, -1, 2, 3, 4]
  assert cond[:6, 2].tolist() == [1, 0, -1, 0, -1, 2]
  assert (cond[6:] == cond[5]).all()
  render, tex_src, tex_row, cond = launch_tables(slot[2:3], g[2:3], [True, False, True], bg_row, 4)
  assert render.shape == (0, 4) and tex_src.size == 0 and cond.shape == (4, 4) and (cond[:, 1] == -1).all()

"""Host side of the VGG pool codes (no GPU): the op-level entry point is part of the C-ABI surface, and training plans - which now carve
the two code buffers - validate at the benchmark's batch sizes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_code_entry_point_is_in_the_c_abi_surface():
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  name = "vp_maxpool2x2_bwd_code"
  header = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  assert re.search(r"\bint\s+%s\s*\(" % name, header)
  assert hasattr(lib, name) and name in _lib.exported_symbols()
  # argument checks come before any launch: usable without a GPU
  null = ctypes.c_void_p(0)
  assert lib.vp_maxpool2x2_bwd_code(null, null, null, 1, 2, 2, 8, _lib.VP_BF16, null) == -1
  assert b"vp_maxpool2x2_bwd_code" in lib.vp_last_error()
  buf = (ctypes.c_char * 64)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert lib.vp_maxpool2x2_bwd_code(p, p, p, 1, 3, 2, 8, _lib.VP_BF16, null) == -1       # odd height
  assert lib.vp_maxpool2x2_bwd_code(p, p, p, 1, 2, 2, 4, _lib.VP_BF16, null) == -1       # bf16 wants whole 8-channel groups


@pytest.mark.parametrize("batch", [4, 8, 16, 32])
def test_training_plans_with_code_buffers_validate(batch):
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  sizes = {}
  for dtype in (1, 0):
    d = _lib.PixReferDesc(batch, 256, 64, 64, dtype, 1, 500.0, 1.0, 0)
    rc = lib.vp_pixrefer_validate_plan(ctypes.byref(d))
    assert rc == 0, lib.vp_last_error().decode()
    sizes[dtype] = lib.vp_pixrefer_workspace_bytes(ctypes.byref(d))
  # the two code buffers: one byte per pooled element of the fake half (64 channels at 128 x 128, 128 at 64 x 64)
  assert sizes[1] > batch * (128 * 128 * 64 + 64 * 64 * 128)

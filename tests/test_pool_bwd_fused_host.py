"""Host side of the pooled-source backward-data launches (no GPU): the new entry points are part of the C-ABI surface, the knob exists,
and training plans validate - kernel preconditions of the pooled-source form and the regions its loader reads included - at the
benchmark's batch sizes with the knob on and off."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_in_the_c_abi_surface():
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  header = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  for ret, name in (("int", "vp_conv3x3_c64_bwd_data_pooled"), ("size_t", "vp_conv3x3_c64_bwd_data_pooled_workspace_bytes")):
    assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
    assert hasattr(lib, name) and name in _lib.exported_symbols(), name
  # argument checks come before any launch: usable without a GPU
  null = ctypes.c_void_p(0)
  ok = _lib.ConvDesc(0, 2, 32, 48, 64, 64, 3, 1, 1, _lib.VP_BF16, 0, 0)
  assert lib.vp_conv3x3_c64_bwd_data_pooled(ctypes.byref(ok), null, null, null, null, null, null, 1, null) == -1
  assert b"vp_conv3x3_c64_bwd_data_pooled" in lib.vp_last_error()
  full = 2 * 32 * 48 * 64 * 2
  assert lib.vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(ctypes.byref(ok)) >= lib.vp_conv_workspace_bytes(ctypes.byref(ok)) + full
  buf = (ctypes.c_char * 64)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  for bad in (_lib.ConvDesc(0, 2, 32, 48, 64, 128, 3, 1, 1, _lib.VP_BF16, 0, 0),      # cin != cout
              _lib.ConvDesc(0, 2, 30, 48, 64, 64, 3, 1, 1, _lib.VP_BF16, 0, 0),       # height no multiple of 4
              _lib.ConvDesc(0, 2, 32, 40, 64, 64, 3, 1, 1, _lib.VP_BF16, 0, 0),       # width no multiple of 16
              _lib.ConvDesc(0, 2, 32, 48, 64, 64, 3, 1, 1, _lib.VP_F32, 0, 0),        # bf16 only
              _lib.ConvDesc(0, 2, 32, 48, 64, 64, 4, 1, 1, _lib.VP_BF16, 0, 0)):      # 3x3 only
    assert lib.vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.vp_conv3x3_c64_bwd_data_pooled(ctypes.byref(bad), p, p, p, p, p, p, 1, null) == -1


def test_the_knob_is_known():
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  assert lib.vp_tune(b"pool_bwd_fused", 0) == 0
  assert lib.vp_tune(b"pool_bwd_fused", 1) == 0


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("batch", [4, 8, 16, 32])
def test_training_plans_validate_with_the_knob_on_and_off(batch, knob):
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  assert lib.vp_tune(b"pool_bwd_fused", knob) == 0
  try:
    sizes = []
    for dtype in (1, 0):
      d = _lib.PixReferDesc(batch, 256, 64, 64, dtype, 1, 500.0, 1.0, 0)
      rc = lib.vp_pixrefer_validate_plan(ctypes.byref(d))
      assert rc == 0, lib.vp_last_error().decode()
      sizes.append(lib.vp_pixrefer_workspace_bytes(ctypes.byref(d)))
  finally:
    lib.vp_tune(b"pool_bwd_fused", 1)
  # the workspace does not depend on the knob (the full-resolution gradient buffers stay: vp_pixrefer_tensor materialises them on demand)
  lib.vp_tune(b"pool_bwd_fused", 1)
  for dtype, want in zip((1, 0), sizes):
    d = _lib.PixReferDesc(batch, 256, 64, 64, dtype, 1, 500.0, 1.0, 0)
    assert lib.vp_pixrefer_workspace_bytes(ctypes.byref(d)) == want

"""Streaming inference, host side (vp_bfmstream_*): the receptive field the library derives from MfccNet's layer table is tight, the
emission schedule emits exactly the frames whose receptive field has arrived (and pad_len frames in all), bad descriptors are refused.
No GPU: these entry points are host-only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
  from voicepuppet_amd.stream import stream_desc
  return stream_desc(**kw)


def _ctx(max_chunk_frames=1):
  from voicepuppet_amd.stream import stream_context
  return stream_context(_desc(max_chunk_frames=max_chunk_frames))


def test_context_numbers():
  L, R, Lf, Rf, Tw = _ctx(1)
  assert (Lf, Rf) == (-(-L // 5), -(-R // 5))
  assert Tw == 1 + Lf + Rf
  assert _ctx(7)[4] == 7 + Lf + Rf


def _pooled(p, mel, f):
  from oracle import audio_ref
  y = audio_ref.mfccnet_fwd(p, mel[None, :, :, None])[0]        # [T5, 3, 256]
  return y[5 * f:5 * f + 5].max(axis=(0, 1))                    # the MfccEncoder's [5,3] / [5,3] SAME pool of frame f


@pytest.mark.slow
def test_receptive_field_is_tight():
  """float64 oracle, random parameters, 30 video frames of mel: a change of mel row 5f - L - 1 or 5f + 4 + R + 1 leaves frame f's pooled
  encoding bit-identical; a change of row 5f - L or 5f + 4 + R changes it (for some draw)."""
  from oracle import audio_ref
  L, R = _ctx(1)[:2]
  T, f = 30, 13
  assert 5 * f - L - 1 >= 0 and 5 * f + 4 + R + 1 < 5 * T
  p = audio_ref.init_bfmnet_params(seed=3)
  rng = np.random.default_rng(4)
  mel = rng.normal(0, 2, (5 * T, 80))
  base = _pooled(p, mel, f)
  for row in (5 * f - L - 1, 5 * f + 4 + R + 1):
    m = mel.copy()
    m[row] += rng.normal(0, 5, 80)
    assert np.array_equal(_pooled(p, m, f), base), row
  for row in (5 * f - L, 5 * f + 4 + R):
    changed = False
    for _ in range(4):
      m = mel.copy()
      m[row] += rng.normal(0, 5, 80)
      if not np.array_equal(_pooled(p, m, f), base):
        changed = True
        break
    assert changed, row


def _frames_after(d, n, fin):
  from voicepuppet_amd import _lib
  return int(_lib.lib().vp_bfmstream_frames_after(ctypes.byref(d), n, fin))


def _chunkings(n, rng):
  yield [n]
  yield [640] * (n // 640) + ([n % 640] if n % 640 else [])
  yield [641] * (n // 641) + ([n % 641] if n % 641 else [])
  sizes, left = [], n
  while left > 0:
    k = int(min(left, rng.integers(1, 3000)))
    sizes.append(k)
    left -= k
  yield sizes
  if n <= 4000:
    yield [1] * n


def test_emission_schedule():
  """For wav lengths of 0 .. 3 T_win frames (exact multiples of 640 among them) and several chunkings: the frames emitted behind every
  push are exactly those whose receptive field lies in mel frames made of received samples (5f + 4 + R <= last complete mel row), never
  fewer, never revised; finish brings the total to pad_len = 1 + N // 640."""
  for cmax in (1, 5):
    d = _desc(max_chunk_frames=cmax)
    L, R, Lf, Rf, Tw = _ctx(cmax)
    rng = np.random.default_rng(cmax)
    lengths = sorted({0, 1, 511, 512, 640, 641, 1279, 1280} | {640 * k for k in range(3 * Tw + 1)} |
                     {int(x) for x in rng.integers(0, 640 * 3 * Tw + 640, 40)})
    for n in lengths:
      for sizes in _chunkings(n, rng):
        got, seen = 0, 0
        for s in sizes:
          seen += s
          k = _frames_after(d, seen, 0) - got
          assert k >= 0
          got += k
          mel = (seen - 512) // 128 + 1 if seen >= 512 else 0
          if got:
            assert 5 * (got - 1) + 4 + R <= mel - 1          # every emitted frame is exact
          assert 5 * got + 4 + R > mel - 1                     # and the next one is not yet
        got += _frames_after(d, n, 1) - got
        assert got == 1 + n // 640, (n, sizes[:4])


def test_bad_descriptors_are_refused():
  from voicepuppet_amd import _lib
  from voicepuppet_amd.stream import stream_desc
  lib = _lib.lib()
  assert lib.vp_bfmstream_desc_size() == ctypes.sizeof(_lib.BfmStreamDesc)
  good = stream_desc()
  assert lib.vp_bfmstream_workspace_bytes(ctypes.byref(good)) > 0
  bad = []
  d = stream_desc(); d.struct_bytes -= 4; bad.append(d)                  # size mismatch
  d = stream_desc(); d.struct_bytes += 4; bad.append(d)
  bad.append(stream_desc(max_chunk_frames=0))
  bad.append(stream_desc(max_chunk_frames=-3))
  bad.append(stream_desc(max_chunk_frames=1025))
  bad.append(stream_desc(num_mel_bins=64))
  d = stream_desc(); d.trunk_dtype = 7; bad.append(d)
  bad.append(stream_desc(upper_hz=9000.0))
  for d in bad:
    assert lib.vp_bfmstream_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.vp_bfmstream_frames_after(ctypes.byref(d), 1000, 0) == -1
    assert lib.vp_bfmstream_context(ctypes.byref(d), None, None, None, None, None) != 0
  assert lib.vp_bfmstream_frames_after(ctypes.byref(good), -1, 0) == -1
  # handle entry points refuse a NULL handle instead of dereferencing it
  assert lib.vp_bfmstream_ready(None, 640) == 0 and lib.vp_bfmstream_ready_finish(None) == 0
  assert lib.vp_bfmstream_push(None, None, 0, None, None, None) != 0
  assert lib.vp_bfmstream_finish(None, None, None, None) != 0
  assert lib.vp_bfmstream_create(ctypes.byref(stream_desc(max_chunk_frames=0)), None, 0, None, None, None) != 0


def test_session_is_a_one_slot_group():
  """A vp_bfmstream is a stream group of one slot: its workspace is that group's, for every chunk size and trunk."""
  from voicepuppet_amd import _lib
  from voicepuppet_amd.stream import group_desc, stream_desc
  lib = _lib.lib()
  for dtype in ("f32", "bf16"):
    for c in (1, 5, 64):
      n = lib.vp_bfmstream_workspace_bytes(ctypes.byref(stream_desc(max_chunk_frames=c, dtype=dtype)))
      assert n > 0 and n == lib.vp_bfmstream_group_workspace_bytes(ctypes.byref(group_desc(1, max_chunk_frames=c, dtype=dtype))), (dtype, c)


_ASAN_SCRIPT = r'''
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from voicepuppet_amd import _lib
from voicepuppet_amd.stream import stream_desc, stream_context
lib = _lib.lib()
for c in (1, 5, 64, 1024):
  d = stream_desc(max_chunk_frames=c, dtype="bf16" if c == 5 else "f32")
  assert lib.vp_bfmstream_workspace_bytes(ctypes.byref(d)) > 0
  stream_context(d)
  for n in (0, 511, 640, 10**6):
    assert lib.vp_bfmstream_frames_after(ctypes.byref(d), n, 0) >= 0
    assert lib.vp_bfmstream_frames_after(ctypes.byref(d), n, 1) == 1 + n // 640
d = stream_desc(max_chunk_frames=0)
assert lib.vp_bfmstream_workspace_bytes(ctypes.byref(d)) == 0
print("ok")
'''


def test_stream_host_layer_under_sanitizers():
  """The stream's planner (receptive field, workspace layout of the window and exact-size plans, schedule) in the `make host-asan`
  build: AddressSanitizer + UBSan, no GPU code."""
  import shutil
  csrc = os.path.join(ROOT, "voicepuppet_amd", "csrc")
  if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", csrc, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  so = os.path.join(ROOT, "voicepuppet_amd", "libvp_host_asan.so")
  rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
  assert os.path.exists(rt), rt
  env = dict(os.environ)
  env.update({"VP_LIB": so, "LD_PRELOAD": rt, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99",
              "UBSAN_OPTIONS": "halt_on_error=1:exitcode=98", "PYTHONMALLOC": "malloc"})
  r = subprocess.run([sys.executable, "-c", _ASAN_SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=600)
  assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_head_sway_carried_across_pushes_equals_the_clip_sequence():
  """PuppetStream's head-sway state: consecutive next(k) draws concatenate to infer_bfmvid.angle_sequence of the whole clip."""
  from voicepuppet_amd.pixrefer.infer_bfmvid import angle_sequence
  from voicepuppet_amd.stream import HeadSway
  s = HeadSway()
  got = np.concatenate([s.next(k) for k in (1, 4, 0, 7, 13, 2, 30)])
  assert np.array_equal(got, angle_sequence(got.shape[0]))

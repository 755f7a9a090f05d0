"""The stream ingest's definition and host layer, without a GPU: the C ABI (include/vp_hip.h vp_pcmin_*) refuses what it must, its filter
design and emission counts are scipy's, and the numpy restatement (tests/pcm_ref.py), which the device is compared with in
tests/test_gpu_pcm.py, is itself pinned against scipy.signal.resample_poly."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcm_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLED = [r for r in pr.COMMON_RATES if r != 16000]


def test_header_declares_the_pcmin_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.pcm  # noqa: F401  (importable without a GPU)
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  for name in ("vp_pcmin_desc_size", "vp_pcmin_ratio", "vp_pcmin_bank", "vp_pcmin_samples_after", "vp_pcmin_workspace_bytes", "vp_pcmin_create",
               "vp_pcmin_destroy", "vp_pcmin_open_slot", "vp_pcmin_ready", "vp_pcmin_push"):
    assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert name in _lib.exported_symbols()
  L = _lib.lib()
  assert L.vp_pcmin_desc_size() == ctypes.sizeof(_lib.PcmInDesc) == 52
  body = hdr[hdr.index("typedef struct vp_pcmin_desc {"):hdr.index("} vp_pcmin_desc;")]
  assert re.findall(r"\bint\s+(\w+)(?:\[\d+\])?;", body) == [n for n, _ in _lib.PcmInDesc._fields_]
  assert re.search(r"\bint\s+rates\[8\];", body) and _lib.PcmInDesc.rates.size == 32
  assert "#define VP_PCMIN_MAX_SLOTS %d" % _lib.PCMIN_MAX_SLOTS in hdr and "#define VP_PCMIN_MAX_CHANNELS %d" % _lib.PCMIN_MAX_CHANNELS in hdr
  assert re.search(r"VP_PCM_S16\s*=\s*%d\s*,\s*VP_PCM_F32\s*=\s*%d" % (_lib.PCM_S16, _lib.PCM_F32), hdr)


_REFUSALS = r"""
import ctypes, sys
sys.path.insert(0, %r)
from voicepuppet_amd import _lib
L = _lib.lib()
n = ctypes.sizeof(_lib.PcmInDesc)
common = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000]
def desc(size=n, slots=4, out_rate=16000, max_in=1 << 16, rates=(48000,), n_rates=None):
  return _lib.PcmInDesc(size, slots, out_rate, max_in, len(rates) if n_rates is None else n_rates, (ctypes.c_int * 8)(*rates))
bad = 0
for rates in (common[:8], common[3:], [48000], [16000]):
  for slots in (1, 128):
    ws = L.vp_pcmin_workspace_bytes(ctypes.byref(desc(slots=slots, rates=rates)))
    print("ok", slots, rates, ws)
    bad += ws == 0
for what, d in [("struct_bytes", desc(size=n - 4)), ("struct_bytes", desc(size=n + 4)), ("slots", desc(slots=0)), ("slots", desc(slots=129)),
                ("n_rates", desc(rates=(), n_rates=0)), ("n_rates", desc(n_rates=9)), ("rates[1]", desc(rates=(48000, 44101))),
                ("over the cap", desc(rates=(48000, 44101))), ("rates[0]", desc(rates=(0,))), ("rates[2]", desc(rates=(8000, 48000, 8000))),
                ("max_in_frames", desc(max_in=0)), ("out_rate", desc(out_rate=0))]:
  ws, msg = L.vp_pcmin_workspace_bytes(ctypes.byref(d)), L.vp_last_error().decode()
  h = ctypes.c_void_p()
  rc = L.vp_pcmin_create(ctypes.byref(d), None, 0, None, ctypes.byref(h))
  print("refused", what, ws, rc, msg)
  bad += ws != 0 or rc != -1 or what not in msg or h.value is not None
sys.exit(1 if bad else 0)
"""


def test_invalid_descriptors_are_refused_with_a_message_naming_the_field():
  r = subprocess.run([sys.executable, "-c", _REFUSALS % ROOT], capture_output=True, text=True, timeout=600)
  print(r.stdout)
  assert r.returncode == 0, r.stdout + r.stderr


def test_open_slot_and_the_host_queries_refuse_bad_arguments():
  """channels 0 / 9 and an unknown format are refused by vp_pcmin_open_slot before it looks at the handle (so this needs no device), with
  the field in the message; so are the host-only queries' bad rates and counts."""
  src = r"""
import ctypes, sys
sys.path.insert(0, %r)
from voicepuppet_amd import _lib
import voicepuppet_amd.pcm as pcm
L = _lib.lib()
for ch in (0, 9, -1):
  assert L.vp_pcmin_open_slot(None, 0, 48000, ch, _lib.PCM_S16, None) == -1
  assert "channels = %%d" %% ch in L.vp_last_error().decode(), L.vp_last_error()
assert L.vp_pcmin_open_slot(None, 0, 48000, 2, 7, None) == -1 and "format" in L.vp_last_error().decode()
assert L.vp_pcmin_open_slot(None, 0, 48000, 2, _lib.PCM_F32, None) == -1 and "handle" in L.vp_last_error().decode()
assert pcm.ratio(44100) == (160, 441, 4410, 56) and pcm.ratio(16000) == (1, 1, 0, 1)
assert L.vp_pcmin_ratio(0, 16000, None, None, None, None) == -1 and "in_rate" in L.vp_last_error().decode()
assert L.vp_pcmin_samples_after(48000, 16000, -1, 0) == -1 and "in_frames" in L.vp_last_error().decode()
assert L.vp_pcmin_ready(None, None, None, None) == -1
""" % ROOT
  r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("rate", RESAMPLED)
def test_restatement_against_resample_poly(rate):
  """The restatement with the float32 bank, summed in float64, against resample_poly(float64(x), up, down): within
  B = (taps per phase + 1) * 2^-24 * max_phase(sum |h|) * max |x| (the forward error bound of a float32 dot product of that length plus
  the rounding of the bank; pcm_ref.bound computes it from the bank itself)."""
  from scipy.signal import resample_poly
  up, down, half, T = pr.ratio(rate)
  x = pr.mono(pr.clip(rate, 1, "s16"), 1)
  want = resample_poly(x.astype(np.float64), up, down)
  got = pr.resample(x, rate)
  assert got.shape == want.shape == (-(-x.shape[0] * up // down),)
  B = pr.bound(rate, np.abs(x).max())
  d = float(np.abs(got - want).max())
  print("%d Hz: up %d down %d taps/phase %d, %d -> %d samples, max |d| %.3g, B %.3g" % (rate, up, down, T, x.shape[0], got.shape[0], d, B))
  assert d <= B, (d, B)
  # and WavLoader's own float32 evaluation of the same clip obeys the same bound around the float64 signal
  f32 = resample_poly(x, up, down)
  assert f32.dtype == np.float32 and float(np.abs(f32.astype(np.float64) - want).max()) <= B


def test_restatement_of_the_conversion_is_wavloaders(tmp_path):
  from scipy.io import wavfile
  from voicepuppet_amd.generator.loader import WavLoader
  for channels in (1, 2):
    for fmt in ("s16", "f32"):
      raw = pr.clip(16000, channels, fmt)
      path = str(tmp_path / ("c%d_%s.wav" % (channels, fmt)))
      wavfile.write(path, 16000, raw if channels > 1 else raw[:, 0])
      want = WavLoader(sr=16000).get_data(path)
      got = pr.mono(raw, channels)
      assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (channels, fmt)
  for channels in range(3, 9):
    raw = pr.clip(16000, channels, "f32")
    got, want = pr.mono(raw, channels), raw.astype(np.float64).mean(axis=1)
    assert np.abs(got - want).max() <= channels * 2.0 ** -24 * np.abs(raw).max()


@pytest.mark.parametrize("rate", RESAMPLED)
def test_filter_bank_is_scipys_design(rate):
  """vp_pcmin_bank against float32(firwin(...)) * up: every coefficient within one float32 ulp (two double evaluations of the Kaiser
  window can land on either side of a float32 rounding boundary)."""
  import voicepuppet_amd.pcm as pcm
  up, down, half, T = pcm.ratio(rate)
  assert (up, down, half, T) == pr.ratio(rate)
  got, want = pcm.bank(rate), pr.design(rate)
  assert got.shape == want.shape == (2 * half + 1,) and got.dtype == want.dtype == np.float32
  ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)))
  differ = int(np.count_nonzero(got != want))
  print("%d Hz: %d of %d coefficients differ from scipy's, worst %.2f ulp" % (rate, differ, got.size, float((np.abs(got - want) / ulp).max())))
  assert np.all(np.abs(got - want) <= ulp)


def test_pass_through_has_no_filter():
  import voicepuppet_amd.pcm as pcm
  assert pcm.ratio(16000) == (1, 1, 0, 1) and pcm.bank(16000).tolist() == [1.0]
  for n in (0, 1, 639, 640, 12345):
    assert pcm.samples_after(16000, n) == pcm.samples_after(16000, n, True) == n


@pytest.mark.parametrize("rate", pr.COMMON_RATES)
def test_emission_counts(rate):
  """vp_pcmin_samples_after equals the restatement over random cut points, is monotone, never counts a sample whose last tap has not
  arrived, is tight (the next sample does need a frame that has not arrived, or the clip's total is reached), and at finish equals
  len(resample_poly(x, up, down))."""
  import voicepuppet_amd.pcm as pcm
  from scipy.signal import resample_poly
  up, down, half, T = pr.ratio(rate)
  rng = np.random.default_rng(rate)
  cuts = sorted(set([0, 1, 2, half // up, half // up + 1] + [int(v) for v in rng.integers(0, 3 * rate, 300)] + [int(v) for v in rng.integers(0, 200, 50)]))
  prev = 0
  for n in cuts:
    k = pcm.samples_after(rate, n)
    total = pcm.samples_after(rate, n, True)
    assert k == pr.samples_after(rate, n) and total == pr.samples_after(rate, n, True), n
    assert prev <= k <= total
    prev = k
    if k:
      assert pr.last_input_needed(rate, k - 1) <= n - 1, (n, k)            # its last tap has arrived
    assert k == total or pr.last_input_needed(rate, k) >= n, (n, k)        # tight: the next one needs a frame still to come
  for n in (1, 2, 5, 100, 441, 1000, 4097):
    assert pcm.samples_after(rate, n, True) == len(resample_poly(np.zeros(n, np.float32), up, down)), n

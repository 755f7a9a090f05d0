"""Op-level float64 parity of the log-mel front end (vp_logmel_forward), BOTH of its paths: logmel512_kernel (csrc/audio_kernels.hip: the
one-launch radix-4 FFT form, win_length 512 and at most 80 mel bins) and the generic path (frame_window_kernel -> the DFT as a matrix
product on the float32 igemm kernel -> mag_mel_log_kernel) that every other descriptor admitted by logmel_ok takes.  The front end's
counterpart of test_gpu_bfmnet_ops.py; reference, bound, inputs and case table live in logmel_ref.py (CPU only).

Rules common to every GPU case
  * the C ABI is driven directly (vp_logmel_workspace_bytes / _create / _forward); PCM, output and workspace sit in gpu_util.guarded
    buffers: the output NaN-prefilled between sentinel bands, the workspace between byte bands, the PCM between NaN bands; all bands are
    checked after every call;
  * the device sees float32 PCM, the reference is the float64 of those values: oracle/audio_ref.stft_mag, linear_to_mel_weight_matrix
    with the descriptor's lower_hz / upper_hz / sample_rate cast to float32 and back, log(. + 1e-6);
  * every sample that no frame covers (the tail after the last frame; the gaps where hop > win) is NaN on the device: one read of it
    that reaches a result shows;
  * the clips of a batch differ in seed and scale (CLIP_SCALES), so a frame read from the neighbouring clip cannot pass;
  * before the device is touched the reference alone must satisfy (reference_conditions): at most 2 % of the elements with a log-domain
    bound above 1e-3 (the log of a near-empty mel bin is ill-conditioned; there the bound says nothing), and acc = 0 exactly wherever
    the mel column is all zero or the frame is silent.  Those elements are excluded from the share and asserted against
    log(1e-6f) under the K_LOG term alone.

The bound, per element, u = 2^-24, s_f = sum_n |x_n w_n| of the frame (derived from the operation counts, not fitted):
  magnitude, fused     |dmag_k| <= C_FUSED u s_f, C_FUSED = 61 =
                         2   the window value rounded to float32 and the window product (perturbations of x_n w_n: gain 1)
                       + 2 * 4 * 6   four radix-4 stages, on a path per stage: the twiddle rounded to float32 (1), a complex multiply
                             (sqrt 5 u < 3), two levels of complex adds (2); every intermediate is bounded by the 1-norm of its inputs,
                             so a stage adds 6 u s_f to |dZ_k|.  The untangling step forms xe = (Z_k + conj Z_{256-k}) / 2 and
                             xo = (Z_k - conj Z_{256-k}) / 2i and adds them: dZ_k and dZ_{256-k} both enter both, hence the factor 2
                       + 8   the untangling step itself: the add and the subtract (1 + 1, each on a value <= s_f), w512 rounded (1) and
                             its complex multiply (3), the final add of two values <= s_f (2)
                       + 3   re^2, im^2, their sum and sqrtf: 2.5 u |X| <= 3 u s_f
  magnitude, unfused   |dmag_k| <= (win_length + 14) u s_f: a win_length-term float32 FMA chain in any order (win_length), the window
                       value, the window product and the cos / -sin entry rounded to float32 (3), up to 8 partial sums of a K split
                       (8: igemm_splitk_cap), the magnitude step (3).  (The real and the imaginary chain are bounded together:
                       sum_n a_n (|cos|, |sin|) has norm <= sum_n a_n.)
  mel sum              dacc <= sum_k mel[k, m] dmag_k + (n_k + 2) u acc_ref, n_k = 257 fused (all rows run), nb unfused
  log                  darg = dacc + the rounding of 1e-6f + the rounding of the float32 sum acc + 1e-6f (u (acc + 1e-6));
                       |got - log(acc_ref + 1e-6)| <= log1p(darg / (acc_ref + 1e-6 - darg)) + K_LOG u |log(.)|
  K_LOG = 4            = 2 ulp of the result.  No copy of the HIP math accuracy table is installed with the toolchain; logf is commonly
                       stated at 1 ulp, and twice that is allowed (the margin covers the float64 -> float32 rounding of the
                       reference and nothing more).  Not measured on the kernel under test.

Signal families (logmel_ref.make_pcm)
  sweep    test_gpu_audio.synth_pcm per clip (noise 0.1 + sweep 0.3), scaled per clip
  tones    region r = samples [r win, (r + 1) win) carries a tone (3e-2) at the centre of one bin over a noise floor of 1e-2; bins 0 1 2 63
           64 65 127 128 129 191 192 255 256 (scaled by win / 512): DC, Nyquist, lane 0 / lane 63 and the quarters of the untangling step
  clicks   sparse clicks anywhere, about four per window (two above 512): broadband like noise, but s_f / |X_k| stays near 2
  impulse  ONE sample per frame at 0, 1, 255, 256, 257, 511 or an even / odd pair, every (clip, frame) its own amplitude and sign.  Only
           cases with hop >= win run it: their frames are disjoint, frame f owns samples [f hop, f hop + win) and the sample goes to
           f hop + n0 - so each frame sees exactly one.  Reference also in closed form: log(|a| w[n0] colsum(mel)[m] + 1e-6).
  silence  clip 0 silent, the other clips loud (B = 1: plain silence)
Which family runs where is decided by the 2 % cap on the REFERENCE, and that is a finding of its own: with C = win + 14 the unfused bound
is informative only where s_f / |X_k| is small.  Noise-like inputs (sweep, tones over a floor) have s_f / |X_k| ~ sqrt(win) and put
19 % of the one-bin mel bands of a 512 window above 1e-3 (84 % for the tones), so the unfused cases from win 256 up run clicks and
impulses (and silence), those of win 16 run every family, the fused cases (C = 61) run every family.

Case table (logmel_ref.FUSED_CASES / UNFUSED_CASES; `tail` > 0 wherever hop > 1)
  fused    B F = 1, 5, 31, 32 (B 2), 33 (B 3 x 11: block 0 ends inside clip 2, frame 32 is that block's last), 65 (B 5 x 13 and B 1);
           hop 128 160 1 512 640; nmel 80 79 40 1; lower / upper 300 / 3400; sample_rate 8000 with the default edges (the only
           descriptor here where bin 256 carries mel weight, and 18 all-zero columns above 4 kHz)
  unfused  (win, nmel) = (512, 81) (512, 128) (256, 80) (1024, 80) (16, 1) (16, 8) (4096, 128) with two frames; hop 1, win / 4, win,
           win + 16; B 1 and 3.  The igemm PIXEL tile plan_fwd picks for the P = B F rows of the DFT product (pick_igemm_cfg, conv_ops.h;
           rows = ncol is never a multiple of 64 here): IG_128x16 up to P = 16 and IG_128x32 for 17 .. 95 (win 16, ncol = 24 rows:
           IG_64x32 for every P below 96), the 128-pixel tiles (IG_128x128 / IG_64x128) from 96.  P = 15, 16, 17 at (512, 81); 31, 32, 33 around the 32-pixel tile; 96, 127, 128, 129 around the
           128-pixel one; P = 1, 2, 5, 6.
  both     the same clicks through nmel = 80 (fused) and nmel = 81 (unfused), each inside its own bound of one float64 spectrum.

CPU tests of the instrument: two independent float32 front ends (a radix-2 complex64 FFT, a float32 DFT matrix product) stay inside
the bound on every (case, family); the closed-form impulse reference equals the stft_mag route; the reference conditions hold on the
whole table and reject references made to break them; the mel matrix of the oracle equals vp_logmel_create's loops restated in float64
and cast to float32, bit for bit, at every descriptor of the table; the gap (test_the_gap_demonstrated): magnitudes rounded to bf16, bins
k <-> 256 - k swapped in one frame, frame 32 taken from the next clip and the Nyquist bin dropped are all rejected; of the old test's
two tolerances only max-abs < 5e-3 lets one of them through on the chosen input (bf16 magnitudes) - the others are rejection-only.

Measured on an MI355X (worst |got - ref| / bound over all cases of the path, elements with acc > 0; the acc = 0 elements sit at 0.347
of the K_LOG term everywhere - logf(1e-6f) is one float32 step from the float64 logarithm):
             sweep    tones    clicks   impulse  silence (its loud clips)
  fused      0.024    0.013    0.052    0.100    0.024
  unfused    0.131    0.176    0.189    0.252    0.129      (all five at win 16, where the chain is short and the bound tight)
  unfused by window, clicks / impulse: win 256 0.050 / 0.130, win 512 0.018 / 0.041, win 1024 0.011 / 0.027, win 4096 0.001 / 0.004
  (the bound is a worst case over win roundings; rel-L2 against the reference is 6e-8 .. 1.5e-7 at every case of both paths)
  both paths on the same clicks: 8.6e-08 (80 bins, fused) and 8.4e-08 (81 bins, unfused) rel-L2 against their float64 references.
  Between the two (per-frame mean mel energy, the 80- against 81-triangle difference of the references removed): rel-L2 3.0e-08.
  76 GPU cases, every guard band intact, 3.2 s for the file on the GPU (no case above 0.4 s, the first one with the library load); the 107 CPU tests take 8 s.
No kernel bug was found: both paths, the host-built DFT and mel matrices, the ncol padding and the s[nb + k] read hold at every
descriptor class logmel_ok admits that the table reaches.
"""
import ctypes

import numpy as np
import pytest

from oracle import audio_ref as ar

import logmel_ref as R
from logmel_ref import ALL_CASES, BOTH_PATHS, FUSED_CASES, UNFUSED_CASES, U

gpu = pytest.mark.gpu

CASE_FAMS = [(c, fam) for c in ALL_CASES for fam in c.fams]
IDS = ["%s-%s" % (c.name, fam) for c, fam in CASE_FAMS]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests of the instrument
# ---------------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_what_it_states():
  assert all(R.is_fused(c) for c in FUSED_CASES) and not any(R.is_fused(c) for c in UNFUSED_CASES)
  assert {c.b * c.frames for c in FUSED_CASES} >= {1, 5, 31, 32, 33, 65}
  assert {c.hop for c in FUSED_CASES} == {128, 160, 1, 512, 640} and {c.nmel for c in FUSED_CASES} == {80, 79, 40, 1}
  assert any(c.b > 1 and c.b * c.frames > 32 and 32 % c.frames for c in FUSED_CASES)          # a 32-frame block ends inside a clip
  assert any((c.lo, c.hi) != (80.0, 7600.0) for c in FUSED_CASES) and any(c.sr == 8000 for c in FUSED_CASES)
  assert {(c.win, c.nmel) for c in UNFUSED_CASES} == {(512, 81), (512, 128), (256, 80), (1024, 80), (16, 1), (16, 8), (4096, 128)}
  assert all(c.frames == 2 for c in UNFUSED_CASES if c.win == 4096)
  for win in (512, 256, 16):
    hops = {c.hop for c in UNFUSED_CASES if c.win == win}
    assert hops >= {1, win // 4, win, win + 16}, (win, hops)
  assert {c.b for c in UNFUSED_CASES} == {1, 3}
  ps = {c.b * c.frames for c in UNFUSED_CASES}
  assert ps >= {15, 16, 17, 31, 32, 33, 96, 127, 128, 129}
  assert [R.igemm_pixel_tile(512, p) for p in (16, 17, 95, 96)] == [16, 32, 32, 128] and [R.igemm_pixel_tile(16, p) for p in (1, 95, 96)] == [32, 32, 128]
  for c in ALL_CASES:
    assert c.tail > 0 or c.hop == 1, c.name
    assert 0 <= c.tail < max(c.hop, 2) and ("impulse" in c.fams) == (c.hop >= c.win), c.name
    assert (~R.covered(c)).sum() == c.tail + (c.frames - 1) * max(c.hop - c.win, 0)
  # every listed tone bin is the tone of some fused clip region, every impulse position of some impulse frame
  seen = {R.tone_of(c, b, r) for c in FUSED_CASES for b in range(c.b) for r in range(R.samples(c) // c.win)}
  assert seen == set(R.TONE_BINS_512)
  pos = {R.impulse_of(c, b, f)[0] for c in FUSED_CASES if "impulse" in c.fams for b in range(c.b) for f in range(c.frames)}
  assert pos >= set(R.IMPULSE_POS_512)
  amps = [R.impulse_of(FUSED_CASES[5], b, f)[1] for b in range(5) for f in range(13)]
  assert len(set(np.round(np.abs(amps), 9))) >= 40


def test_zero_columns_counted():
  """128 bins over 257 spectrogram bins and 80 over 129 have one all-zero mel column each; the default descriptor has none."""
  by = {(c.win, c.nmel, c.sr): len(R.zero_columns(c)) for c in ALL_CASES}
  assert by[(512, 128, 16000)] == 1 and by[(256, 80, 16000)] == 1 and by[(512, 80, 16000)] == 0 and by[(512, 81, 16000)] == 0
  assert by[(512, 80, 8000)] == 18
  c = [c for c in FUSED_CASES if c.sr == 8000][0]
  assert R.mel_matrix(c)[256].max() > 0.1                       # the one descriptor whose Nyquist bin carries weight
  assert all(R.mel_matrix(k)[-1].max() == 0 for k in ALL_CASES if k.sr == 16000)


@pytest.mark.parametrize("c", ALL_CASES + list(BOTH_PATHS), ids=lambda c: c.name)
def test_mel_matrix_equals_the_definition_in_create(c):
  """Separate from the kernels: the oracle's matrix (what the reference multiplies by) against vp_logmel_create's own loops."""
  want = R.mel_matrix(c).astype(np.float32)
  got = R.mel_matrix_as_created(c)
  assert got.dtype == np.float32 and got.shape == want.shape == (c.win // 2 + 1, c.nmel)
  assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("c,fam", CASE_FAMS, ids=IDS)
def test_reference_conditions_and_float32_front_ends(c, fam):
  """The 2 % cap and the acc = 0 condition on the reference; two independent float32 front ends inside the case's own bound."""
  pcm = R.make_pcm(c, fam)
  assert pcm.shape == (c.b, R.samples(c)) and np.array_equal(pcm, R.f32(pcm))
  ref = R.reference(c, pcm)
  R.reference_conditions(c, ref)
  assert np.isfinite(ref.log).all() and (ref.bound > 0).all()
  if c.b > 1 and fam != "silence":                               # no two clips alike
    assert R.vacuous_share(ref) <= R.VACUOUS_SHARE and not np.allclose(ref.log[0], ref.log[1], atol=1e-2)
  for name, fn in (("fft", R.logmel_f32_fft), ("dft", R.logmel_f32_dft)):
    ratio, ok = R.compare(c, fn(c, pcm), ref)
    assert ok, "%s %s %s: float32 %s front end at %.3f of the bound" % (c.name, fam, name, name, ratio.max())
  if fam == "impulse":
    closed = R.impulse_closed_form(c)
    assert np.abs(closed - ref.log).max() < 1e-12                # the closed form IS the stft_mag route
    assert (R.frame_sums(c, pcm) > 0).sum() >= 0.8 * c.b * c.frames   # (position 0 meets w[0] = 0: a silent frame)
  want = ar.extract_mfcc(pcm, c.sr, c.nmel, c.win, c.hop, c.win, c.lo, c.hi)      # the oracle's own call, edges threaded through
  assert np.abs(want - ref.log).max() < 1e-12
  if fam == "silence":
    assert ref.zero[0].all() and (ref.log[0] == np.log(1e-6)).all() and (c.b == 1 or not ref.zero[1:].all())


def test_reference_conditions_reject_broken_references():
  c = FUSED_CASES[4]
  ref = R.reference(c, R.make_pcm(c, "sweep"))
  R.reference_conditions(c, ref)
  t = np.arange(R.samples(c))
  quiet = R.reference(c, R.f32(np.tile(0.3 * np.cos(2 * np.pi * 64 * t / 512), (c.b, 1))))    # a bare tone: every other bin near-empty
  with pytest.raises(AssertionError, match="log-domain bound above"):
    R.reference_conditions(c, quiet)
  c2 = [k for k in UNFUSED_CASES if k.name == "u512x128_p33"][0]
  ref2 = R.reference(c2, R.make_pcm(c2, "clicks"))
  R.reference_conditions(c2, ref2)
  acc = ref2.acc.copy()
  acc[..., R.zero_columns(c2)[0]] = 1e-9
  with pytest.raises(AssertionError, match="non-zero reference energy"):
    R.reference_conditions(c2, ref2._replace(acc=acc))
  # and the unfused bound on a noise-like input (the reason the unfused 512 cases run clicks and impulses)
  c3 = BOTH_PATHS[1]
  with pytest.raises(AssertionError, match="log-domain bound above"):
    R.reference_conditions(c3, R.reference(c3, R.make_pcm(c3, "tones")))
  # zero elements: log(1e-6f) under the K_LOG term alone
  got = ref2.log.copy()
  z = tuple(np.argwhere(ref2.zero)[0])
  got[z] = R.LOG_EPS_F32 * (1 + 1.5 * R.K_LOG * U)
  assert not R.compare(c2, got, ref2)[1]
  got[z] = R.LOG_EPS_F32 * (1 + 0.5 * R.K_LOG * U)
  assert R.compare(c2, got, ref2)[1]
  got[z] = np.nan
  assert not R.compare(c2, got, ref2)[1]


def old_tolerances(got, ref):
  """test_gpu_audio.test_logmel_parity's two assertions."""
  return bool(np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-4 and np.abs(got - ref).max() < 5e-3)


def test_the_gap_demonstrated():
  """Four corruptions of the float64 magnitudes, carried through mel and log, on the old test's kind of input (the sweep family) at the
  default descriptor, B 3 x F 11.  All four are rejected here.  Against the old test's two tolerances, on this input:
    magnitudes rounded to bf16        inside max-abs < 5e-3 (3.5e-3), outside rel-L2 < 1e-4 (6.0e-4): the max-abs tolerance alone would
                                      accept bf16 magnitudes; here at 91 times the bound
    bins k and 256 - k swapped in one frame (k = 26, a noise-only pair)
                                      outside both (max abs 6.8e-2, rel-L2 8.9e-4): rejection only.  245 times the bound
    frame 32 taken from the next clip outside both (the clips differ in scale by design): rejection only
    the Nyquist bin dropped           changes nothing at the default descriptor - bin 256 (8 kHz) has mel weight 0 for any upper_hz up to
                                      Nyquist, so no output-level test can see it there.  At sample_rate 8000 with the default edges the
                                      bin carries weight: there it is outside both old tolerances as well (max abs 0.88) and rejected
                                      here: rejection only.
  So on an every-bin-loud input the old tolerances do catch a one-bin slip; what they let through is precision (bf16 magnitudes under
  the max-abs one) - and they never ran a descriptor where the Nyquist bin, the unfused path or a zero mel column exists."""
  c = FUSED_CASES[4]
  assert (c.b, c.frames, c.nmel) == (3, 11, 80)
  pcm = R.make_pcm(c, "sweep")
  ref = R.reference(c, pcm)
  s = R.frame_sums(c, pcm)
  carried = lambda case, mag, ss: R.from_mag(case, mag, ss).log
  assert R.compare(c, ref.log, ref)[1] and old_tolerances(ref.log, ref.log)

  import torch
  bf = torch.tensor(ref.mag, dtype=torch.float32).to(torch.bfloat16).double().numpy()
  got = carried(c, bf, s)
  print("\nbf16 magnitudes: max abs %.2e, rel-L2 %.2e, worst err / bound %.0f" % (
      np.abs(got - ref.log).max(), np.linalg.norm(got - ref.log) / np.linalg.norm(ref.log), R.compare(c, got, ref)[0].max()))
  assert not R.compare(c, got, ref)[1]
  assert np.abs(got - ref.log).max() < 5e-3 and not old_tolerances(got, ref.log)      # inside the max-abs tolerance, outside the rel-L2 one

  mag = ref.mag.copy()
  mag[1, 4, [230, 26]] = mag[1, 4, [26, 230]]
  got = carried(c, mag, s)
  ratio, ok = R.compare(c, got, ref)
  print("k <-> 256 - k at one frame: max abs %.2e, rel-L2 %.2e, worst err / bound %.0f" % (
      np.abs(got - ref.log).max(), np.linalg.norm(got - ref.log) / np.linalg.norm(ref.log), ratio.max()))
  assert not ok
  swap_passes_old = old_tolerances(got, ref.log)

  mag = ref.mag.reshape(33, 257).copy()
  src = ref.mag[0, 10]                                            # flattened frame 32 = (clip 2, frame 10); its next clip wraps to clip 0
  mag[32] = src
  got = carried(c, mag.reshape(3, 11, 257), s)
  assert not R.compare(c, got, ref)[1] and not old_tolerances(got, ref.log)

  mag = ref.mag.copy()
  mag[..., 256] = 0
  assert R.mel_matrix(c)[256].max() == 0 and np.abs(carried(c, mag, s) - ref.log).max() < 1e-13      # invisible at the default descriptor
  c8 = [k for k in FUSED_CASES if k.sr == 8000][0]
  pcm8 = R.make_pcm(c8, "sweep")
  ref8 = R.reference(c8, pcm8)
  mag = ref8.mag.copy()
  mag[..., 256] = 0
  got = carried(c8, mag, R.frame_sums(c8, pcm8))
  ratio, ok = R.compare(c8, got, ref8)
  print("Nyquist dropped at 8 kHz: max abs %.2e, worst err / bound %.0f, old tolerances %s; swap passes old: %s" % (
      np.abs(got - ref8.log).max(), ratio.max(), old_tolerances(got, ref8.log), swap_passes_old))
  assert not ok
  assert not swap_passes_old and not old_tolerances(got, ref8.log)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------------------
def device_logmel(c, pcm):
  """vp_logmel_forward through the C ABI on guarded buffers; returns the output as float64."""
  import torch
  from voicepuppet_amd import _lib
  import gpu_util as gu
  L = _lib.lib()
  n = R.samples(c)
  desc = _lib.LogMelDesc(c.sr, c.nmel, c.win, c.hop, c.win, c.lo, c.hi, c.b, n)
  nbytes = L.vp_logmel_workspace_bytes(ctypes.byref(desc))
  assert nbytes > 0 and L.vp_logmel_frames(ctypes.byref(desc)) == c.frames
  ws_whole, ws, ws_g = gu.guarded((nbytes,), 0, "u8", min_bytes=gu.GUARD_BYTES)
  x_whole, x, x_g = gu.guarded((c.b, n), c.win, "f32", fill=R.device_pcm(c, pcm), band=float("nan"), min_bytes=gu.GUARD_BYTES)
  y_whole, y, y_g = gu.guarded((c.b, c.frames, c.nmel), c.nmel, "f32", min_bytes=gu.GUARD_BYTES)
  assert int(torch.isnan(x).sum()) == c.b * int((~R.covered(c)).sum())
  h = ctypes.c_void_p()
  _lib.check(L.vp_logmel_create(ctypes.byref(desc), gu.ptr(ws), nbytes, gu.stream(), ctypes.byref(h)), "vp_logmel_create")
  try:
    _lib.check(L.vp_logmel_forward(h, gu.ptr(x), gu.ptr(y), gu.stream()), "vp_logmel_forward")
    torch.cuda.synchronize()
  finally:
    L.vp_logmel_destroy(h)
  gu.assert_guards(y_whole, y_g, "%s: guard band of the output" % c.name)
  gu.assert_guards(ws_whole, ws_g, "%s: guard band of the workspace" % c.name)
  assert bool(torch.isnan(x_whole[:x_g]).all()) and bool(torch.isnan(x_whole[-x_g:]).all()), "%s: guard band of the PCM written" % c.name
  assert torch.equal(torch.nan_to_num(x.cpu(), nan=7.0), torch.nan_to_num(torch.tensor(R.device_pcm(c, pcm)), nan=7.0)), "PCM changed"
  return y.cpu().numpy().astype(np.float64)


def check(c, fam, got, ref):
  ratio, ok = R.compare(c, got, ref)
  live = ~ref.zero
  worst = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
  print("\nLOGMEL %s %s %s: worst err/bound %.3f at %s (live %.3f, acc = 0 elements %.3f of %d), rel_l2 %.2e" % (
      "fused" if R.is_fused(c) else "unfused", fam, c.name, ratio[worst], worst, ratio[live].max() if live.any() else 0.0,
      ratio[ref.zero].max() if ref.zero.any() else 0.0, int(ref.zero.sum()), np.linalg.norm(got - ref.log) / np.linalg.norm(ref.log)))
  assert np.isfinite(got).all(), "%s %s: %d elements not written / not finite, first at %s" % (
      c.name, fam, int((~np.isfinite(got)).sum()), np.argwhere(~np.isfinite(got))[0])
  bad = np.argwhere(ratio > 1)
  assert ok, "%s %s: %d of %d elements outside the bound, e.g. (clip, frame, mel) %s: got %r want %r bound %.2e" % (
      c.name, fam, len(bad), ratio.size, bad[:8].tolist(), got[tuple(bad[0])], ref.log[tuple(bad[0])], ref.bound[tuple(bad[0])])


@gpu
@pytest.mark.parametrize("c,fam", CASE_FAMS, ids=IDS)
def test_logmel_per_element(c, fam):
  pcm = R.make_pcm(c, fam)
  ref = R.reference(c, pcm)
  R.reference_conditions(c, ref)                                   # on the reference alone, before the device call
  got = device_logmel(c, pcm)
  check(c, fam, got, ref)
  if fam == "impulse":                                             # the closed form, under the same bound
    assert (np.abs(got - R.impulse_closed_form(c))[~ref.zero] <= ref.bound[~ref.zero]).all()


@gpu
def test_both_paths_on_the_same_input():
  c80, c81 = BOTH_PATHS
  assert R.is_fused(c80) and not R.is_fused(c81) and R.samples(c80) == R.samples(c81)
  pcm = R.make_pcm(c80, "clicks")
  ref80, ref81 = R.reference(c80, pcm), R.reference(c81, pcm)
  assert np.array_equal(ref80.mag, ref81.mag)                      # one float64 spectrum
  R.reference_conditions(c80, ref80)
  R.reference_conditions(c81, ref81)
  got80, got81 = device_logmel(c80, pcm), device_logmel(c81, pcm)
  check(c80, "clicks", got80, ref80)
  check(c81, "clicks", got81, ref81)
  # the two paths against each other: band m of 80 and of 81 are different triangles, so the descriptors' own difference (known from the
  # float64 references) is taken out of the difference of the per-frame mean mel energies; only printed
  e80, e81 = np.exp(got80).mean(-1), np.exp(got81).mean(-1)
  r80, r81 = np.exp(ref80.log).mean(-1), np.exp(ref81.log).mean(-1)
  print("both paths: rel-L2 between the two, per-frame mean mel energy: %.2e as computed (80 against 81 triangles: the float64 references "
        "differ by %.2e), %.2e with the references' difference removed" % (
            np.linalg.norm(e80 - e81) / np.linalg.norm(e81), np.linalg.norm(r80 - r81) / np.linalg.norm(r81),
            np.linalg.norm((e80 - e81) - (r80 - r81)) / np.linalg.norm(r81)))
  d80, d81 = got80 - ref80.log, got81 - ref81.log
  print("both paths: rel-L2 against the float64 reference %.2e fused, %.2e unfused" % (
      np.linalg.norm(d80) / np.linalg.norm(ref80.log), np.linalg.norm(d81) / np.linalg.norm(ref81.log)))

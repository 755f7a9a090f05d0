"""Streaming inference on the device (voicepuppet_amd.stream.AudioStream, vp_bfmstream_*): mel frames, the stateful GRU and the emitted
coefficients against the offline path (LogMel + BFMNetEngine on the whole clip padded as prepare_pcm pads it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# bounds on max|streamed - offline| as a fraction of max|offline|.  Measured on an MI355X: f32 bit-identical for every clip of at most
# T_win frames tested (finish runs their last frames on the exact-size plan, and the window plan tiled like the offline one for the
# frames emitted earlier), 8.2e-6 / 9.2e-6 for 75 / 87 frames (the whole-clip plan tiles its trunk GEMMs differently), the same for
# every chunking; bf16 trunk 0 at 7 frames, 4.6e-2 at 87
F32_REL = 1e-5
BF16_REL = 1e-1


def _params(seed=0):
  from oracle import audio_ref
  return {k: v.astype(np.float32) for k, v in audio_ref.init_bfmnet_params(seed=seed).items()}


def _clip(frames, seed):
  """PCM of a clip whose pad_len is `frames`: 640 (frames - 1) + r samples."""
  rng = np.random.default_rng(seed)
  n = 640 * (frames - 1) + int(rng.integers(0, 640))
  return (0.3 * rng.standard_normal(n)).astype(np.float32)


def _offline(pcm, params, ears, dtype="f32"):
  import torch
  from voicepuppet_amd.audio import BFMNetEngine, LogMel
  pad_len = 1 + pcm.shape[0] // 640
  total = 128 * (5 * pad_len - 1) + 512
  x = np.zeros(total, np.float32)
  x[:pcm.shape[0]] = pcm
  lm = LogMel(1, total)
  mel = lm(torch.from_numpy(x).cuda().view(1, -1))
  eng = BFMNetEngine(1, pad_len, dtype=dtype)
  eng.load_params(params)
  out = eng.forward(torch.from_numpy(ears.reshape(1, pad_len, 1)).cuda(), mel, [pad_len])
  return mel[0], out[0]


def _sizes(n, how, rng):
  if how == "one":
    return [n]
  if how == "random":
    out, left = [], n
    while left > 0:
      k = int(min(left, rng.integers(1, 4000)))
      out.append(k)
      left -= k
    return out
  return [how] * (n // how) + ([n % how] if n % how else [])


def _stream(st, pcm, sizes, ears):
  """Push pcm in `sizes` pieces then finish; ears [pad_len] are handed out in order.  Returns [pad_len, 64]."""
  import torch
  outs, at, e = [], 0, 0
  for s in sizes:
    k = st.ready(s)
    outs.append(st.push(pcm[at:at + s], ears[e:e + k].reshape(k, 1)))
    assert outs[-1].shape[0] == k
    at += s
    e += k
  k = st.ready_finish()
  outs.append(st.finish(ears[e:e + k].reshape(k, 1)))
  e += k
  assert e == ears.shape[0] == 1 + pcm.shape[0] // 640
  return torch.cat(outs).cpu().numpy()


def test_mel_frames_bit_identical_to_logmel():
  """Every mel frame of the stream (computed once, as samples arrive, by vp_logmel_forward's kernel) equals LogMel on the padded clip."""
  import torch
  from voicepuppet_amd.stream import AudioStream
  st = AudioStream(_params(), max_chunk_frames=64)
  pcm = _clip(80, 1)
  pad_len = 80
  rng = np.random.default_rng(2)
  ears = (np.random.default_rng(3).random(pad_len) / 100).astype(np.float32)
  _stream(st, pcm, _sizes(pcm.shape[0], "random", rng), ears)
  mel_off, _ = _offline(pcm, _params(), ears)
  hist = st.mel_history()
  rows = hist.shape[0]
  assert rows >= 5 * pad_len
  torch.cuda.synchronize()
  assert torch.equal(hist[:5 * pad_len], mel_off)


def test_split_gru_is_bit_identical_to_whole_sequence():
  import ctypes
  import torch
  from voicepuppet_amd import _lib
  L = _lib.lib()
  B, T = 2, 37
  g = torch.Generator(device="cuda").manual_seed(0)
  xg = torch.randn(B, T, 512, device="cuda", generator=g)
  xc = torch.randn(B, T, 256, device="cuda", generator=g)
  whg = torch.randn(256, 512, device="cuda", generator=g) * 0.06
  whc = torch.randn(256, 256, device="cuda", generator=g) * 0.06
  seq = torch.full((B,), T, dtype=torch.int32, device="cuda")
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  whole = torch.empty(B, T, 256, device="cuda")
  _lib.check(L.vp_gru_seq(p(xg), p(xc), p(whg), p(whc), p(seq), p(whole), B, T, s), "vp_gru_seq")
  rng = np.random.default_rng(1)
  for _ in range(3):
    cuts = sorted(set(int(c) for c in rng.integers(1, T, 5)))
    h = torch.zeros(B, 256, device="cuda")
    piece = torch.full((B, T, 256), float("nan"), device="cuda")
    t0 = 0
    for t1 in cuts + [T]:
      _lib.check(L.vp_gru_seq_state(p(xg), p(xc), p(whg), p(whc), p(h), p(piece), B, T, t0, t1 - t0, s), "vp_gru_seq_state")
      t0 = t1
    torch.cuda.synchronize()
    assert torch.equal(piece, whole), cuts
    assert torch.equal(h, whole[:, T - 1])


def _check(got, ref, rel, what, exact=False):
  d = float(np.abs(got - ref).max())
  scale = float(np.abs(ref).max())
  print("%s: max|d| %.3g, max|offline| %.3g, bit-identical %s" % (what, d, scale, np.array_equal(got, ref)))
  if exact:
    assert np.array_equal(got, ref), (what, d, scale)
  assert d <= rel * scale, (what, d, scale)


def test_streamed_coefficients_match_offline_f32():
  """Clip lengths 1, 7, T_win - 1, T_win, 3 T_win + 3 frames; chunkings of one push, 640, 641, 2080 (130 ms) and random sizes; windows of
  1 and 5 frames.  Clips of at most T_win frames: bit-identical (measured, asserted).  Longer
  clips: max|d| <= 1e-5 max|offline|, the f32 parity bound (the whole-clip plan tiles its trunk GEMMs differently; measured 8.2e-6 and
  9.2e-6)."""
  from voicepuppet_amd.stream import AudioStream
  params = _params()
  for cmax in (1, 5):
    st = AudioStream(params, max_chunk_frames=cmax)
    Tw = st.window_frames
    for frames in (1, 7, Tw - 1, Tw, 3 * Tw + 3):
      pcm = _clip(frames, frames)
      ears = (np.random.default_rng(frames).random(frames) / 100).astype(np.float32)
      _, ref = _offline(pcm, params, ears)
      ref = ref.cpu().numpy()
      rng = np.random.default_rng(frames + 100)
      for how in ("one", 640, 641, 2080, "random"):
        st.reset()
        got = _stream(st, pcm, _sizes(pcm.shape[0], how, rng), ears)
        _check(got, ref, F32_REL, "f32 cmax %d frames %d chunk %s" % (cmax, frames, how), exact=frames <= Tw)


def test_streamed_coefficients_match_offline_bf16():
  """bf16 trunk against the offline bf16 forward: the same arithmetic per row up to GEMM tiling, but a bf16 rounding boundary crossed by
  one f32 ulp moves a value by a bf16 ulp, and the GRU carries that on: measured 0 at 7 frames (same plan size), 4.6e-2 of max|offline|
  at 87 frames; bound 1e-1 (the offline bf16 forward itself is ~1e-1 rel-L2 from the float64 oracle, tests/test_gpu_audio.py)."""
  from voicepuppet_amd.stream import AudioStream
  params = _params(1)
  st = AudioStream(params, max_chunk_frames=5, dtype="bf16")
  for frames in (7, 3 * st.window_frames + 3):
    pcm = _clip(frames, frames + 7)
    ears = (np.random.default_rng(frames).random(frames) / 100).astype(np.float32)
    _, ref = _offline(pcm, params, ears, dtype="bf16")
    st.reset()
    got = _stream(st, pcm, _sizes(pcm.shape[0], 2080, np.random.default_rng(0)), ears)
    _check(got, ref.cpu().numpy(), BF16_REL, "bf16 frames %d" % frames, exact=frames <= st.window_frames)


def test_reset_reproduces_and_streams_are_independent():
  from voicepuppet_amd.stream import AudioStream
  params = _params()
  a, b = AudioStream(params, max_chunk_frames=3), AudioStream(params, max_chunk_frames=3)
  pa, pb = _clip(40, 11), _clip(33, 12)
  ea = (np.random.default_rng(1).random(40) / 100).astype(np.float32)
  eb = (np.random.default_rng(2).random(33) / 100).astype(np.float32)
  solo_a = _stream(a, pa, _sizes(pa.shape[0], 1000, None), ea)
  a.reset()
  assert np.array_equal(_stream(a, pa, _sizes(pa.shape[0], 1000, None), ea), solo_a)
  solo_b = _stream(b, pb, _sizes(pb.shape[0], 777, None), eb)
  # interleaved pushes of two live sessions
  a.reset(); b.reset()
  import torch
  outs = {0: [], 1: []}
  pos, epos = [0, 0], [0, 0]
  clips, ears, sz = (pa, pb), (ea, eb), (1000, 777)
  while pos[0] < pa.shape[0] or pos[1] < pb.shape[0]:
    for i, st in enumerate((a, b)):
      if pos[i] >= clips[i].shape[0]:
        continue
      s = min(sz[i], clips[i].shape[0] - pos[i])
      k = st.ready(s)
      outs[i].append(st.push(clips[i][pos[i]:pos[i] + s], ears[i][epos[i]:epos[i] + k].reshape(k, 1)))
      pos[i] += s
      epos[i] += k
  for i, st in enumerate((a, b)):
    k = st.ready_finish()
    outs[i].append(st.finish(ears[i][epos[i]:epos[i] + k].reshape(k, 1)))
  assert np.array_equal(torch.cat(outs[0]).cpu().numpy(), solo_a)
  assert np.array_equal(torch.cat(outs[1]).cpu().numpy(), solo_b)


def test_push_runs_no_framework_kernel_but_copies():
  """Every ATen call of a push / finish is a copy, an allocation or a view: the arithmetic is the library's."""
  import torch
  from torch.utils._python_dispatch import TorchDispatchMode
  from voicepuppet_amd.stream import AudioStream
  st = AudioStream(_params(), max_chunk_frames=2)
  pcm = _clip(30, 5)
  st.push(pcm[:9000])                                   # (first window: folds and packs the weights)
  seen = []

  class Trace(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
      seen.append(func.__name__ if hasattr(func, '__name__') else str(func))
      return func(*args, **(kwargs or {}))

  with Trace():
    for at in range(9000, pcm.shape[0], 1300):
      st.push(pcm[at:at + 1300])
    st.finish()
  allowed = ('_to_copy', 'copy_', 'empty', 'empty_strided', 'lift_fresh', 'detach', 'alias', 'view', '_unsafe_view', 'as_strided', 'slice',
             'select', 'contiguous', 'clone', 'unsqueeze', 'reshape', '_reshape_alias', 'to', 'is_pinned', '_pin_memory', 'record_stream')
  bad = sorted({n for n in seen if n.split('.')[0] not in allowed})
  assert not bad, (bad, seen)
  assert seen

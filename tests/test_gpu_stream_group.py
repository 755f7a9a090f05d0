"""Streaming groups on the device (voicepuppet_amd.stream.AudioStreamGroup, vp_bfmstream_group_*): every slot's coefficients are
bit-identical to a single AudioStream fed the same chunks, whatever the other slots do (idle, zero-sample pushes, late starts, early
finishes, resets), whichever slot a stream is given and however many slots share a round (different bucket plans)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 6


def _params(seed=0):
  from oracle import audio_ref
  return {k: v.astype(np.float32) for k, v in audio_ref.init_bfmnet_params(seed=seed).items()}


def _clip(frames, seed):
  """PCM of a clip whose pad_len is `frames`: 640 (frames - 1) + r samples."""
  rng = np.random.default_rng(seed)
  n = 640 * (frames - 1) + int(rng.integers(0, 640))
  return (0.3 * rng.standard_normal(n)).astype(np.float32)


def _chunks(n, rng, zero_every=3):
  """Random chunk sizes summing to n, with zero-sample chunks mixed in."""
  out, left, i = [], n, 0
  while left > 0:
    i += 1
    if i % zero_every == 0:
      out.append(0)
      continue
    k = int(min(left, rng.integers(1, 3000)))
    out.append(k)
    left -= k
  return out


class Stream:
  """One clip cut into chunks; abort: the slot is reset after that many chunks instead of finishing."""

  def __init__(self, frames, seed, abort=None):
    rng = np.random.default_rng(100 + seed)
    self.pcm = _clip(frames, seed)
    self.sizes = _chunks(self.pcm.shape[0], rng)
    self.abort = abort
    self.ears = (rng.random(1 + self.pcm.shape[0] // 640) / 100).astype(np.float32)

  def pieces(self):
    n = len(self.sizes) if self.abort is None else self.abort
    at = 0
    for i in range(n):
      yield self.pcm[at:at + self.sizes[i]], self.abort is None and i == n - 1
      at += self.sizes[i]


def _single(streams, params, mcf, dtype):
  """Each stream alone on one AudioStream (reset between clips): its chunks, then finish after the last.  Returns [rows, 64] per stream."""
  import torch
  from voicepuppet_amd.stream import AudioStream
  st = AudioStream(params, max_chunk_frames=mcf, dtype=dtype)
  res = []
  for s in streams:
    st.reset()
    outs, e = [], 0
    for chunk, last in s.pieces():
      k = st.ready(chunk.shape[0])
      outs.append(st.push(chunk, s.ears[e:e + k].reshape(k, 1)))
      e += k
      if last:
        k = st.ready_finish()
        outs.append(st.finish(s.ears[e:e + k].reshape(k, 1)))
        e += k
    res.append(torch.cat(outs).cpu().numpy())
  return res


def _group(programs, streams, params, mcf, dtype, slots=S, idle=0.3, seed=0):
  """programs[slot]: (delay, [stream ids]) - the slot idles `delay` pushes, then serves its streams one after the other (reset_slot
  between them).  Each push, every busy slot takes part with probability 1 - idle.  Returns [rows, 64] per stream."""
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd.stream import AudioStreamGroup, stream_desc
  import ctypes
  g = AudioStreamGroup(params, slots=slots, max_chunk_frames=mcf, dtype=dtype)
  d = stream_desc(mcf, dtype)
  L = _lib.lib()
  frames_after = lambda n, fin: int(L.vp_bfmstream_frames_after(ctypes.byref(d), int(n), int(fin)))
  rng = np.random.default_rng(seed)
  queue = {s: list(ids) for s, (_, ids) in programs.items()}
  delay = {s: dl for s, (dl, _) in programs.items()}
  it, cur, got, eat, done = {}, {}, {i: [] for i in range(len(streams))}, {i: 0 for i in range(len(streams))}, {}
  samples = {}
  while any(queue[s] or s in cur for s in queue):
    pcm, fin, ears, who = {}, [], {}, {}
    for s in sorted(queue):
      if delay[s] > 0:
        delay[s] -= 1
        continue
      if s not in cur:
        if not queue[s]:
          continue
        cur[s] = queue[s].pop(0)
        it[s] = streams[cur[s]].pieces()
        samples[s] = 0
      if rng.random() < idle:
        continue
      nxt = next(it[s], None)
      if nxt is None:                       # an aborted stream: the slot starts over
        g.reset_slot(s)
        del cur[s]
        continue
      pcm[s], last = nxt
      if last:
        fin.append(s)
      who[s] = cur[s]
    k = g.ready({s: v.shape[0] for s, v in pcm.items()}, fin)
    for s, i in who.items():
      n0, n1 = samples[s], samples[s] + pcm[s].shape[0]
      want = frames_after(n1, s in fin) - frames_after(n0, False)
      assert k[s] == want, (s, k[s], want)
      ears[s] = streams[i].ears[eat[i]:eat[i] + k[s]].reshape(k[s], 1)
      eat[i] += k[s]
      samples[s] = n1
    out = g.push(pcm, finish=fin, ears={s: ears.get(s, np.zeros((0, 1), np.float32)) for s in range(slots)})
    for s, i in who.items():
      assert out[s].shape == (k[s], 64)
      got[i].append(out[s])
      if s in fin:
        g.reset_slot(s)
        del cur[s]
  return [torch.cat(got[i]).cpu().numpy() if got[i] else np.zeros((0, 64), np.float32) for i in range(len(streams))]


def _streams(Tw):
  # clips of 1, 7, T_win and ~80 frames, one aborted mid-stream (reset), and fillers
  return [Stream(1, 1), Stream(7, 2), Stream(Tw, 3), Stream(80, 4), Stream(30, 5, abort=6), Stream(13, 6), Stream(9, 7), Stream(Tw + 3, 8)]


def _tw(mcf):
  from voicepuppet_amd.stream import stream_context, stream_desc
  return stream_context(stream_desc(mcf))[4]


PROGRAMS = {0: (0, [0, 5]), 1: (2, [1]), 2: (0, [2]), 3: (1, [3]), 4: (0, [4, 6]), 5: (4, [7])}


@pytest.mark.parametrize("dtype,mcf", [("f32", 1), ("f32", 3), ("bf16", 2)])
def test_group_bit_identical_to_single_streams(dtype, mcf):
  p = _params()
  streams = _streams(_tw(mcf))
  ref = _single(streams, p, mcf, dtype)
  got = _group(PROGRAMS, streams, p, mcf, dtype)
  for i, (a, b) in enumerate(zip(got, ref)):
    assert a.shape == b.shape, (i, a.shape, b.shape)
    assert np.array_equal(a, b), (i, float(np.abs(a - b).max()))


def test_permuted_slots_and_bucket_sizes_give_the_same_bits():
  """The same streams on permuted slots, alone (bucket 1), three at a time (bucket 4) and all together (bucket S): the same bits."""
  p = _params(1)
  mcf = 2
  streams = _streams(_tw(mcf))
  ref = _single(streams, p, mcf, "f32")
  perm = {S - 1 - s: v for s, v in PROGRAMS.items()}
  runs = [_group(perm, streams, p, mcf, "f32", seed=3, idle=0.0),
          _group({0: (0, list(range(len(streams))))}, streams, p, mcf, "f32", slots=1, idle=0.0),
          _group({0: (0, [0, 3, 6]), 1: (0, [1, 4, 7]), 2: (0, [2, 5])}, streams, p, mcf, "f32", slots=3, idle=0.0)]
  for r in runs:
    for i, (a, b) in enumerate(zip(r, ref)):
      assert np.array_equal(a, b), i


def test_group_matches_offline_forward_f32():
  """Clips of at most T_win frames: bit-identical to BFMNetEngine.forward on the whole clip, as for a single AudioStream."""
  import torch
  from voicepuppet_amd.audio import BFMNetEngine, LogMel
  p = _params(2)
  Tw = _tw(1)
  streams = [Stream(1, 11), Stream(7, 12), Stream(Tw, 13), Stream(5, 14), Stream(12, 15)]
  got = _group({s: (s % 2, [s]) for s in range(5)}, streams, p, 1, "f32", slots=5)
  for s, out in zip(streams, got):
    pad_len = 1 + s.pcm.shape[0] // 640
    total = 128 * (5 * pad_len - 1) + 512
    x = np.zeros(total, np.float32)
    x[:s.pcm.shape[0]] = s.pcm
    mel = LogMel(1, total)(torch.from_numpy(x).cuda().view(1, -1))
    eng = BFMNetEngine(1, pad_len, dtype="f32")
    eng.load_params(p)
    off = eng.forward(torch.from_numpy(s.ears.reshape(1, pad_len, 1)).cuda(), mel, [pad_len])[0].cpu().numpy()
    assert np.array_equal(out, off), pad_len


def test_group_push_runs_no_framework_kernel_but_copies():
  """Every ATen call of a group push (with finishes) is a copy, an allocation or a view: the arithmetic is the library's."""
  from torch.utils._python_dispatch import TorchDispatchMode
  from voicepuppet_amd.stream import AudioStreamGroup
  g = AudioStreamGroup(_params(), slots=4, max_chunk_frames=2)
  pcm = [_clip(20 + 3 * s, 20 + s) for s in range(4)]
  g.push({s: pcm[s][:9000] for s in range(4)})          # (first window: folds and packs the weights)
  seen = []

  class Trace(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
      seen.append(func.__name__ if hasattr(func, '__name__') else str(func))
      return func(*args, **(kwargs or {}))

  with Trace():
    for at in range(9000, 12000, 1300):
      g.push({s: pcm[s][at:at + 1300] for s in range(3)})
    g.push({s: pcm[s][12000:] for s in range(4)}, finish=(0, 1, 2, 3))
  allowed = ('_to_copy', 'copy_', 'empty', 'empty_strided', 'lift_fresh', 'detach', 'alias', 'view', '_unsafe_view', 'as_strided', 'slice',
             'select', 'contiguous', 'clone', 'unsqueeze', 'reshape', '_reshape_alias', 'to', 'is_pinned', '_pin_memory', 'record_stream')
  bad = sorted({n for n in seen if n.split('.')[0] not in allowed})
  assert not bad, (bad, seen)
  assert seen


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_seventeen_active_slots_bit_identical(dtype):
  """17 slots pushed together: rounds of up to 17 active slots run the batch-32 bucket plan (pinned K splits on a 32x larger grid, the
  depthwise kernel cut into other segments) and still give each stream its single-session bits."""
  p = _params(3)
  streams = [Stream(8 + (i % 9), 40 + i) for i in range(17)]
  ref = _single(streams, p, 1, dtype)
  got = _group({s: (0, [s]) for s in range(17)}, streams, p, 1, dtype, slots=17, idle=0.0)
  for i, (a, b) in enumerate(zip(got, ref)):
    assert np.array_equal(a, b), (i, float(np.abs(a - b).max()) if a.shape == b.shape else (a.shape, b.shape))

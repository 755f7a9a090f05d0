"""Stream ingest on the device (voicepuppet_amd.pcm.PcmIngest, libvp_hip.so vp_pcmin_*, csrc/pcm_in.hip): pass-through is WavLoader bit for
bit, the output of a clip does not depend on how pushes cut it or on the other slots, it is the float64 restatement (tests/pcm_ref.py) and
WavLoader's signal within the float32 dot-product bound, a push only enqueues, and infer_streams --native_pcm writes what the host path
writes.  Wav fixtures are written into tmp_path."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcm_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 22050, 44100, 48000, 96000)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run(ing, slot, raw, sizes):
  """One clip through slot `slot` in chunks of `sizes` frames (the last push finishes): the concatenated output; every push's counts are
  checked against ready()."""
  import torch
  outs, at = [], 0
  for i, n in enumerate(sizes):
    fin = (slot,) if i == len(sizes) - 1 else ()
    want = ing.ready({slot: n}, fin)
    out, k = ing.push({slot: raw[at:at + n]}, finish=fin)
    assert k == want and out.numel() == sum(k) == k[slot], (i, n, k, want)
    outs.append(out)
    at += n
  assert at == raw.shape[0]
  return torch.cat(outs).cpu().numpy()


def _ragged(n, seed):
  rng = np.random.default_rng(seed)
  out, left, i = [], n, 0
  while left > 0:
    i += 1
    if i % 3 == 0:
      out.append(0)
      continue
    k = int(min(left, rng.integers(1, 1 + max(2, n // 6))))
    out.append(k)
    left -= k
  return out


def _wav(path, rate, raw):
  from scipy.io import wavfile
  wavfile.write(str(path), rate, raw if raw.shape[1] > 1 else raw[:, 0])
  return str(path)


def _params(seed=0):
  from oracle import audio_ref
  return {k: v.astype(np.float32) for k, v in audio_ref.init_bfmnet_params(seed=seed).items()}


@pytest.mark.parametrize("channels", [1, 2])
def test_pass_through_is_exact(tmp_path, channels):
  """16 kHz int16: the ingest's output is WavLoader.get_data of the same file bit for bit, and AudioStreamGroup coefficients through
  PcmIngest + push_device_packed are those of the same group fed the WavLoader floats."""
  import torch
  from voicepuppet_amd.generator.loader import WavLoader
  from voicepuppet_amd.pcm import PcmIngest
  from voicepuppet_amd.stream import AudioStreamGroup
  raw = pr.clip(16000, channels, "s16", seconds=1.3)
  want = WavLoader(sr=16000).get_data(_wav(tmp_path / "a.wav", 16000, raw))
  ing = PcmIngest(1, rates=(16000,))
  for sizes in ([raw.shape[0]], _ragged(raw.shape[0], 1), [640] * (raw.shape[0] // 640) + [raw.shape[0] % 640]):
    ing.open_slot(0, 16000, channels, "s16")
    got = _run(ing, 0, raw, sizes)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), sizes[:4]
  p = _params()
  ga, gb = AudioStreamGroup(p, slots=1, max_chunk_frames=2), AudioStreamGroup(p, slots=1, max_chunk_frames=2)
  ing.open_slot(0, 16000, channels, "s16")
  chunk = 1000
  ears = (np.random.default_rng(3).random(1 + raw.shape[0] // 640) / 100).astype(np.float32)
  a, b, row = [], [], 0
  for at in range(0, raw.shape[0], chunk):
    fin = (0,) if at + chunk >= raw.shape[0] else ()
    pcm, n = ing.push({0: raw[at:at + chunk]}, finish=fin)
    k = ga.ready({0: n[0]}, fin)[0]
    e = {0: ears[row:row + k].reshape(k, 1)}
    a.append(ga.push_device_packed(pcm, {0: n[0]}, fin, e)[0])
    b.append(gb.push({0: want[at:at + chunk]}, finish=fin, ears=e)[0])
    row += k
  a, b = torch.cat(a).cpu().numpy(), torch.cat(b).cpu().numpy()
  assert a.shape == b.shape == (1 + raw.shape[0] // 640, 64) and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_down_mix_of_three_to_eight_channels(fmt):
  """16 kHz, 3 .. 8 channels: the float32 left-to-right mean against the float64 mean, within c * 2^-24 * max |x|."""
  from voicepuppet_amd.pcm import PcmIngest
  ing = PcmIngest(1, rates=(16000,))
  for c in range(3, 9):
    raw = pr.clip(16000, c, fmt, seconds=0.1)
    ing.open_slot(0, 16000, c, fmt)
    got = _run(ing, 0, raw, [1000, raw.shape[0] - 1000])
    x = raw.astype(np.float64) / (32768.0 if fmt == "s16" else 1.0)
    d = float(np.abs(got - x.mean(axis=1)).max())
    assert got.shape == (raw.shape[0],) and d <= c * 2.0 ** -24 * np.abs(x).max(), (c, d)


@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", RATES)
def test_chunking_invariance_and_the_reference_signal(tmp_path, rate, channels, fmt):
  """The concatenated output is identical, bit for bit, for chunks of 1 frame, 40 ms, a ragged sequence with empty pushes in between and
  the whole clip at once, with per-push counts equal to vp_pcmin_ready (_run); it is within B of the float64 restatement and within 2 B of
  WavLoader.get_data on the same file (scipy's own float32 evaluation obeys the same bound), B = pcm_ref.bound: (taps per phase + 1) *
  2^-24 * max_phase(sum |h|) * max |x|."""
  from voicepuppet_amd.generator.loader import WavLoader
  from voicepuppet_amd.pcm import PcmIngest
  raw = pr.clip(rate, channels, fmt)
  N = raw.shape[0]
  ing = PcmIngest(1, rates=(rate,))
  ms40 = rate * 40 // 1000
  outs = {}
  for name, sizes in (("whole", [N]), ("40 ms", [ms40] * (N // ms40) + [N % ms40]), ("ragged", _ragged(N, rate + channels)), ("1 frame", [1] * N)):
    ing.open_slot(0, rate, channels, fmt)
    outs[name] = _run(ing, 0, raw, sizes)
  up, down, half, T = pr.ratio(rate)
  for name, y in outs.items():
    assert y.shape == (-(-N * up // down),), name
    assert np.array_equal(_bits(y), _bits(outs["whole"])), "%s differs from the whole clip at %d of %d samples" % (
        name, int(np.count_nonzero(_bits(y) != _bits(outs["whole"]))), y.size)
  x = pr.mono(raw, channels)
  B = pr.bound(rate, np.abs(x).max())
  d_ref = float(np.abs(outs["whole"] - pr.resample(x, rate)).max())
  loader = WavLoader(sr=16000).get_data(_wav(tmp_path / "a.wav", rate, raw))
  d_loader = float(np.abs(outs["whole"].astype(np.float64) - loader).max())
  print("%d Hz %d ch %s: max |d| to the float64 restatement %.3g, to WavLoader %.3g, B %.3g" % (rate, channels, fmt, d_ref, d_loader, B))
  assert loader.shape == outs["whole"].shape
  assert d_ref <= B, (d_ref, B)
  assert d_loader <= 2 * B, (d_loader, B)


GROUP = [(48000, 2, "s16"), (44100, 1, "f32"), (16000, 2, "s16"), None, (8000, 3, "s16"), (96000, 8, "s16"), (22050, 4, "f32"), (48000, 1, "f32")]


@pytest.mark.parametrize("perm", [list(range(8)), [5, 2, 7, 0, 3, 6, 1, 4]])
def test_groups_equal_slots_alone(perm):
  """Slots with different rates, channel counts and formats in one push (one idle, one restarted mid-way with open_slot), on the
  natural and on a permuted slot order: every slot's samples are those of the same clip run whole through a one-slot PcmIngest."""
  import torch
  from voicepuppet_amd.pcm import PcmIngest
  rates = sorted(set(g[0] for g in GROUP if g))
  clips = {i: pr.clip(g[0], g[1], g[2], seconds=0.2, seed=i) for i, g in enumerate(GROUP) if g}
  alone = {}
  for i, g in enumerate(GROUP):
    if g:
      one = PcmIngest(1, rates=(g[0],))
      one.open_slot(0, *g)
      alone[i] = _run(one, 0, clips[i], [clips[i].shape[0]])
  aborted = pr.clip(22050, 4, "f32", seconds=0.1, seed=99)      # what stream 6's slot carries before its restart
  one = PcmIngest(1, rates=(22050,))
  one.open_slot(0, 22050, 4, "f32")
  aborted_out = one.push({0: aborted})[0].cpu().numpy()
  assert aborted_out.size == pr.samples_after(22050, aborted.shape[0]) > 0

  ing = PcmIngest(8, rates=rates)
  for i, g in enumerate(GROUP):
    if g:
      ing.open_slot(perm[i], *g)
  rng = np.random.default_rng(7)
  at = {i: 0 for i in clips}
  got = {i: [] for i in clips}
  pre = []
  step = 0
  while any(at[i] < clips[i].shape[0] for i in clips):
    step += 1
    chunk, fin = {}, []
    if step <= 2:                                             # stream 6's slot first carries half of another clip, then restarts
      h = aborted.shape[0] // 2
      chunk[perm[6]] = aborted[(step - 1) * h:step * h if step == 1 else aborted.shape[0]]
    if step == 3:
      ing.open_slot(perm[6], *GROUP[6])
    for i in clips:
      if (i == 6 and step <= 2) or at[i] >= clips[i].shape[0] or rng.random() < 0.25:
        continue
      n = int(rng.integers(0, 1 + clips[i].shape[0] // 5))
      chunk[perm[i]] = clips[i][at[i]:at[i] + n]
      at[i] += n
      if at[i] >= clips[i].shape[0]:
        fin.append(perm[i])
    want = ing.ready({s: c.shape[0] for s, c in chunk.items()}, fin)
    out, k = ing.push(chunk, finish=fin)
    assert k == want and k[perm[3]] == 0
    o = 0
    for s in range(8):
      if k[s]:
        i = perm.index(s)
        (pre if (i == 6 and step <= 2) else got[i]).append(out[o:o + k[s]])
      o += k[s]
    assert o == out.numel()
  assert np.array_equal(_bits(torch.cat(pre).cpu().numpy()), _bits(aborted_out))
  for i in clips:
    y = torch.cat(got[i]).cpu().numpy()
    assert y.shape == alone[i].shape and np.array_equal(_bits(y), _bits(alone[i])), (i, GROUP[i])


def test_a_push_longer_than_max_in_frames_is_split():
  """The C entry point refuses more than max_in_frames per slot; the wrapper splits, and the result is the unsplit one."""
  from voicepuppet_amd.pcm import PcmIngest
  raw = pr.clip(48000, 2, "s16")
  a, b = PcmIngest(1, rates=(48000,)), PcmIngest(1, rates=(48000,), max_in_frames=1000)
  a.open_slot(0, 48000, 2, "s16")
  b.open_slot(0, 48000, 2, "s16")
  with pytest.raises(ValueError, match="max_in_frames"):
    b.ready({0: 1001})
  ya = _run(a, 0, raw, [raw.shape[0]])
  out, k = b.push({0: raw}, finish=(0,))                  # 13 launches of at most 1000 frames
  assert k == [ya.size] and np.array_equal(_bits(out.cpu().numpy()), _bits(ya))
  with pytest.raises(ValueError, match="finished"):
    a.ready({0: 1})


def _puppet():
  import test_gpu_puppet_group as pg
  return pg


def _raw_group(pg, fmt_by_slot):
  from voicepuppet_amd.stream import PuppetStreamGroup
  g = PuppetStreamGroup(pg.CFG, 4, frame_batch=4, ingest_rates=sorted(set(f[0] for f in fmt_by_slot)))
  for s, img in enumerate(pg._photos()):
    g.attach(s, img, pg.NPZ[s], *fmt_by_slot[s])
  return g


def test_push_raw_only_enqueues(tmp_path, monkeypatch):
  """The check of tests/test_gpu_puppet_group.py::test_push_only_enqueues for push_raw (48 kHz stereo int16 into 4 slots): with a 400 ms
  spin queued ahead on the stream, push_raw returns while the spin is still running, and afterwards the frames are those of an identical
  group that ran without the spin."""
  import torch
  pg = _puppet()
  monkeypatch.chdir(tmp_path)
  pg._assets(4, pg.SAMPLES)
  fmts = [(48000, 2, "s16")] * 4
  g, g2 = _raw_group(pg, fmts), _raw_group(pg, fmts)
  rng = np.random.default_rng(2)
  raw = np.clip(0.3 * rng.standard_normal((40, 4, 1920, 2)) * 32767, -32768, 32767).astype(np.int16)
  steady = 0
  for i in range(30):
    chunk = {s: raw[i, s] for s in range(4)}
    k = g.audio.ready({s: n for s, n in enumerate(g.ingest.ready({s: 1920 for s in range(4)}))})
    e = {s: np.full((k[s], 1), 0.005, np.float32) for s in range(4) if k[s]}
    g.push_raw(chunk, ears=e)
    g2.push_raw(chunk, ears=e)
    steady = steady + 1 if list(k) == [1, 1, 1, 1] else 0
  assert steady >= 5
  ears = {s: np.full((1, 1), 0.005, np.float32) for s in range(4)}
  spin_ms = 400.0
  cycles = pg._spin_cycles(spin_ms)
  torch.cuda.synchronize()
  chunk = {s: raw[30, s] for s in range(4)}
  want = g2.push_raw(chunk, ears=ears)
  want_frames = g2.last_frames.cpu().numpy()
  torch.cuda.synchronize()
  torch.cuda._sleep(cycles)
  ev = torch.cuda.Event()
  ev.record()
  t = time.perf_counter()
  res = g.push_raw(chunk, ears=ears)
  dt = 1000.0 * (time.perf_counter() - t)
  pending = not ev.query()
  print("push_raw returned after %.2f ms with the %.0f ms spin %s" % (dt, spin_ms, "still running" if pending else "ALREADY COMPLETE"))
  assert pending, "push_raw returned after %.1f ms, after the %.0f ms spin ahead of it had completed: it waited for the device" % (dt, spin_ms)
  assert dt < spin_ms / 2, dt
  torch.cuda.synchronize()
  assert {s: [i for i, _ in v] for s, v in res.items()} == {s: [i for i, _ in v] for s, v in want.items()}
  assert all(len(v) == 1 for v in res.values())
  assert np.array_equal(g.last_frames.cpu().numpy(), want_frames)


def _files(d):
  names = sorted(os.listdir(d), key=lambda f: int(f.split(".")[0]))
  return names, [open(os.path.join(d, f), "rb").read() for f in names]


def test_infer_streams_native_pcm(tmp_path, monkeypatch):
  """infer_streams --native_pcm on 16 kHz stereo int16 files writes, byte for byte, the files of the same command without the flag under
  the same --seed; on 48 kHz files it writes the same frame indices and count (no image tolerance is asserted there: a 1e-7 change of a
  sample may move a rasterised edge).  And the coefficients of push_raw are bit for bit those of the ingest's
  signal copied back and pushed as float32."""
  import torch
  from scipy.io import wavfile
  from voicepuppet_amd.pcm import PcmIngest
  from voicepuppet_amd.pixrefer import infer_streams
  from voicepuppet_amd.stream import AudioStreamGroup
  pg = _puppet()
  monkeypatch.chdir(tmp_path)
  pg._assets(2, pg.SAMPLES[:2])
  with open("talkers.txt", "w") as f:
    f.write("face0.jpg a0.wav photo0.npz\nface1.jpg a1.wav\n")
  common = ["--config_path", pg.CFG, "--frame_batch", "4", "--chunk_ms", "130", "--seed", "7"]
  for rate in (16000, 48000):
    for i in range(2):
      n = pg.SAMPLES[i] * rate // 16000 + 37
      t = np.arange(n) / float(rate)
      left = 0.3 * np.sin(2 * np.pi * (330 + 110 * i) * t) * np.sin(2 * np.pi * (3 + i) * t)
      right = 0.2 * np.sin(2 * np.pi * (500 + 70 * i) * t)
      wavfile.write("a%d.wav" % i, rate, (np.stack([left, right], axis=1) * 32767).astype(np.int16))
    infer_streams.main(common + ["--output_dir", "host%d" % rate, "talkers.txt"])
    infer_streams.main(common + ["--native_pcm", "--output_dir", "native%d" % rate, "talkers.txt"])
    for s in range(2):
      hn, hb = _files(os.path.join("host%d" % rate, str(s)))
      nn, nb = _files(os.path.join("native%d" % rate, str(s)))
      assert nn == hn == ["%d.jpg" % i for i in range(len(hn))] and len(hn) >= pg.FRAMES[s], (rate, s, nn, hn)
      if rate == 16000:
        assert nb == hb, "talker %d: %d of %d files differ" % (s, sum(a != b for a, b in zip(nb, hb)), len(hb))
  # coefficients: push_raw's path against its own signal copied back and pushed as float32
  rate, raw = 48000, wavfile.read("a1.wav")[1]
  p = _params(1)
  ga, gb = AudioStreamGroup(p, slots=1, max_chunk_frames=4), AudioStreamGroup(p, slots=1, max_chunk_frames=4)
  ing = PcmIngest(1, rates=(rate,))
  ing.open_slot(0, rate, 2, "s16")
  chunk = 130 * rate // 1000
  ears = (np.random.default_rng(3).random(8 + raw.shape[0] // 1920) / 100).astype(np.float32)
  a, b, row = [], [], 0
  for at in range(0, raw.shape[0], chunk):
    fin = (0,) if at + chunk >= raw.shape[0] else ()
    pcm, n = ing.push({0: raw[at:at + chunk]}, finish=fin)
    k = ga.ready({0: n[0]}, fin)[0]
    e = {0: ears[row:row + k].reshape(k, 1)}
    a.append(ga.push_device_packed(pcm, {0: n[0]}, fin, e)[0])
    b.append(gb.push({0: pcm.cpu().numpy()}, finish=fin, ears=e)[0])
    row += k
  a, b = torch.cat(a).cpu().numpy(), torch.cat(b).cpu().numpy()
  assert a.shape == b.shape and a.shape[0] == 1 + pr.samples_after(rate, raw.shape[0], True) // 640
  assert np.array_equal(_bits(a), _bits(b))

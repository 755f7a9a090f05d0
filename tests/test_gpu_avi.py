"""AVI segments on the device (voicepuppet_amd.avi.AviMuxer, libvp_hip.so vp_avimux_*, csrc/avi_mux.hip) against the numpy layout
(voicepuppet_amd.avi.host_segment), byte for byte and entry for entry, inside guarded buffers; then the muxer inside PuppetStreamGroup and
infer_stream, their files read back by tests/avi_ref.py.  The muxer does not look at its payload: most cases use synthetic byte rows."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avi_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL, SLACK = 256, 0xA5, 0xEE


class Call:
  """One vp_avimux_segment call on synthetic rows: inputs and blob inside 0xA5 arenas, the rows padded with 0xEE behind their lengths."""

  def __init__(self, lengths, frame_slot, samples, slots, row_bytes, src_shift=0, dst_shift=0, short=None, seed=0, pcm=None, rows=None):
    import torch
    from voicepuppet_amd.avi import AviMuxer
    rng = np.random.default_rng(seed)
    K = len(lengths)
    self.K, self.slots, self.lengths, self.frame_slot = K, slots, list(lengths), list(frame_slot)
    self.rows = rows or [rng.integers(0, 0x80, n).astype(np.uint8).tobytes() for n in lengths]          # no 0xEE in a payload
    counts = np.array([samples.get(s, 0) for s in range(slots)], np.int32)
    self.counts, self.offsets = counts, (np.cumsum(counts) - counts).astype(np.int32)
    total = int(counts.sum())
    # samples k / 32768 with k in 0 .. 199: neither byte of an int16 is 0xEE
    self.pcm = (rng.integers(0, 200, total).astype(np.float32) / np.float32(32768.0)) if pcm is None else np.asarray(pcm, np.float32)
    assert self.pcm.size == total
    self.mux = AviMuxer(max(K, 1), row_bytes, slots, max(total, 1))
    host = np.full(GUARD + src_shift + K * row_bytes + GUARD, FILL, np.uint8)
    base = GUARD + src_shift
    for r, row in enumerate(self.rows):
      host[base + r * row_bytes:base + (r + 1) * row_bytes] = SLACK
      host[base + r * row_bytes:base + r * row_bytes + len(row)] = np.frombuffer(row, np.uint8)
    self.arena_in = torch.from_numpy(host).cuda()
    self.data = self.arena_in[base:base + K * row_bytes].view(K, row_bytes) if K else None
    self.lengths_d = torch.tensor(self.lengths, dtype=torch.int32, device="cuda") if K else None
    self.slot_d = torch.tensor(self.frame_slot, dtype=torch.int32, device="cuda") if K else None
    pcm_host = np.full(64 + total + 64, np.float32(1e30), np.float32)           # a read past the samples would clamp to 0x7fff
    pcm_host[64:64 + total] = self.pcm
    self.pcm_arena = torch.from_numpy(pcm_host).cuda()
    self.pcm_d = self.pcm_arena[64:64 + total] if total else None
    self.table = self.mux.table_bytes(K)
    self.cap = self.mux.call_capacity(K, row_bytes, total)
    if short is not None:                                    # the bytes the call needs, less `short`
      self.cap = self.table + sum(len(v[0]) for v in self.expected().values()) - short
    self.arena_out = torch.full((GUARD + dst_shift + self.cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    self.out = self.arena_out[GUARD + dst_shift:GUARD + dst_shift + self.cap]
    self.dst_base = GUARD + dst_shift

  def expected(self):
    """{slot: (bytes, entries)} by host_segment, for the slots that have a frame or a sample and no refused frame."""
    from voicepuppet_amd.avi import host_segment
    exp = {}
    for s in range(self.slots):
      rows = [r for r in range(self.K) if self.frame_slot[r] == s]
      n = int(self.counts[s])
      if (rows or n) and all(self.lengths[r] >= 0 for r in rows):
        exp[s] = host_segment([self.rows[r] for r in rows], self.pcm[self.offsets[s]:self.offsets[s] + n])
    return exp

  def run(self):
    import torch
    self.seg = self.mux.segment(self.data, self.lengths_d, self.slot_d, self.pcm_d, self.offsets, self.counts, out=self.out)
    torch.cuda.synchronize()
    self.host = self.arena_out.cpu().numpy()
    self.blob = self.host[self.dst_base:self.dst_base + self.cap]
    t = self.blob[:self.table].view("<u4")
    self.head, self.slot_table, self.entries = t[:4], t[4:4 + 4 * self.slots].reshape(self.slots, 4), t[4 + 4 * self.slots:].reshape(-1, 4)
    return self

  def check(self, status=None):
    """The blob against host_segment: table, entries, segment bytes, and every byte the call had no business writing still 0xA5."""
    exp, status = self.expected(), status or {}
    blob, T = self.blob, self.table
    assert np.all(self.host[:self.dst_base] == FILL) and np.all(self.host[self.dst_base + self.cap:] == FILL)       # before and behind
    assert np.array_equal(self.arena_in.cpu().numpy()[:GUARD], np.full(GUARD, FILL, np.uint8))
    at, e0, used, written = T, 0, T, np.zeros(self.cap, bool)
    written[:16 + 16 * self.slots] = True
    for s in range(self.slots):
      off, nbytes, n, st = (int(v) for v in self.slot_table[s])
      assert st == status.get(s, 0), (s, st)
      if st == 1:
        assert (nbytes, n) == (0, 0)
        continue
      if s not in exp:
        assert (nbytes, n) == (0, 0), s
        continue
      want, want_e = exp[s]
      assert (off, nbytes, n) == (at, len(want), want_e.shape[0]), (s, off, nbytes, n, at, len(want))
      assert np.array_equal(self.entries[e0:e0 + n], want_e), s
      written[16 + 16 * self.slots + 16 * e0:16 + 16 * self.slots + 16 * (e0 + n)] = True
      if st == 0:
        assert blob[off:off + nbytes].tobytes() == want, "slot %d: segment differs from host_segment" % s
        written[off:off + nbytes] = True
        used = off + nbytes
      at += nbytes
      e0 += n
    assert [int(v) for v in self.head] == [T, used, e0, max([0] + list(status.values()))], self.head
    assert np.all(blob[~written] == FILL), "bytes outside the table and the segments were written: %s" % np.flatnonzero(blob[~written] != FILL)[:8]
    assert not np.any(blob[T:] == SLACK), "a byte from behind a row's length reached the blob"
    return self


SLOTS9 = [0, 0, 0, 2, 5, 5, 7, 7, 7]
SAMPLES9 = {0: 1, 1: 640, 2: 639, 5: 0, 6: 640, 7: 641}          # 1 and 6: audio only; 5: frames only; 3 and 4: nothing
LENGTHS = ([1, 2, 3, 4, 5, 63, 64, 65, 255], [257, 260, 5, 64, 1, 255, 3, 65, 2], [260, 257, 255, 65, 64, 63, 4, 2, 1])


@pytest.mark.parametrize("audio", [0, 1, 640])
def test_one_frame(audio):
  Call([77], [0], {0: audio}, 1, 260).run().check()


@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("src_shift,dst_shift", [(0, 0), (1, 4), (2, 8), (3, 12), (8, 0)])
def test_nine_rows_over_eight_slots(lengths, src_shift, dst_shift):
  """K = 9 over slots {0,0,0,2,5,5,7,7,7} of 8, row_bytes 260 (no multiple of 16), lengths 1 .. row_bytes, sample counts 0, 1, 639,
  640, 641, slots with audio only and with frames only; source and destination shifted against each other so that every copy width and
  both ragged ends run.  Segment and chunk offsets over the three length orders cover every even residue modulo 16."""
  c = Call(lengths, SLOTS9, SAMPLES9, 8, 260, src_shift, dst_shift, seed=len(lengths) + src_shift).run().check()
  got = c.mux.to_host(c.seg)
  exp = c.expected()
  assert sorted(got) == sorted(exp) == [0, 1, 2, 5, 6, 7]
  for s in exp:
    assert got[s][0].tobytes() == exp[s][0] and np.array_equal(got[s][1], exp[s][1]) and got[s][1].dtype == np.uint32


def test_offsets_cover_every_even_residue():
  """What the docstring above claims, from the layout alone (no device)."""
  seen = set()
  for lengths in LENGTHS:
    at = 16 + 16 * 8 + 16 * 17
    for s in range(8):
      n = SAMPLES9.get(s, 0)
      if n:
        seen.add(at % 16)
        at += 8 + 2 * n
      for r in range(9):
        if SLOTS9[r] == s:
          seen.add(at % 16)
          at += 8 + lengths[r] + (lengths[r] & 1)
  assert seen == set(range(0, 16, 2))


def test_long_chunks_and_many_rows():
  """Chunks longer than one 16 KB slice (a 40000-byte frame, 20001 samples) and 600 rows over 3 slots (more chunks than the layout
  workgroup has lanes); source and destination agree modulo 16 for the long row."""
  Call([40000, 39999, 16384, 16385], [0, 0, 1, 1], {0: 20001, 1: 8192}, 2, 40008, src_shift=8, dst_shift=0).run().check()
  rng = np.random.default_rng(3)
  lengths = rng.integers(0, 40, 600).tolist()
  slots = sorted(rng.integers(0, 3, 600).tolist())
  Call(lengths, slots, {0: 3, 2: 5}, 3, 40, seed=4).run().check()


def test_audio_without_frames_and_nothing_at_all():
  Call([], [], {1: 640, 3: 1}, 4, 260).run().check()
  c = Call([], [], {}, 4, 260).run().check()
  assert c.mux.to_host(c.seg) == {}


def test_refused_frame_marks_its_slot_only_and_the_host_rebuilds_it():
  """lengths[r] = -1 (the encoder's capacity rule) for a row of slot 5: status 1 for slot 5, nothing written for it, every other
  slot's segment what it is without the refusal; to_host rebuilds slot 5 from the raw frame with jpeg.host_jpeg."""
  import torch
  from voicepuppet_amd.avi import host_segment
  from voicepuppet_amd.jpeg import host_jpeg
  samples = {**SAMPLES9, 5: 7}
  good = Call(LENGTHS[0], SLOTS9, samples, 8, 260, seed=9).run().check()
  c = Call(LENGTHS[0], SLOTS9, samples, 8, 260, seed=9)      # the same inputs, but row 5 (slot 5's second) refused
  c.lengths[5] = -1
  c.lengths_d[5] = -1
  c.run().check(status={5: 1})
  for s in (0, 1, 2, 6, 7):
    a, b = [int(v) for v in good.slot_table[s][:2]], [int(v) for v in c.slot_table[s][:2]]
    assert a[1] == b[1] > 0 and good.blob[a[0]:a[0] + a[1]].tobytes() == c.blob[b[0]:b[0] + b[1]].tobytes()
  frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (9, 16, 16, 3)).astype(np.uint8)).cuda()
  with pytest.raises(RuntimeError):
    c.mux.to_host(c.seg)                                     # no raw frame to encode
  got = c.mux.to_host(c.seg, frames)
  want = host_segment([c.rows[4], host_jpeg(frames[5].cpu().numpy(), 75)], c.pcm[c.offsets[5]:c.offsets[5] + 7])
  assert bytes(got[5][0]) == want[0] and np.array_equal(got[5][1], want[1])
  exp = c.expected()
  for s in exp:
    assert bytes(got[s][0]) == exp[s][0] and np.array_equal(got[s][1], exp[s][1])


def test_capacity_one_byte_short_is_status_2_and_nothing_is_written_past_it():
  c = Call(LENGTHS[0], SLOTS9, SAMPLES9, 8, 260, short=1, seed=2).run()
  c.check(status={7: 2})                                     # slot 7's segment is the last: every byte of it, and behind, still 0xA5
  with pytest.raises(RuntimeError):
    c.mux.to_host(c.seg)
  Call(LENGTHS[0], SLOTS9, SAMPLES9, 8, 260, short=0, seed=2).run().check()             # exactly enough: all written


def test_a_slot_alone_and_among_seven_others_and_twice():
  """Slot 5's segment and entries are the same bytes alone in a call and among seven other slots; the same call twice gives the same blob."""
  rng = np.random.default_rng(6)
  lengths = [int(v) if v != SLACK else 237 for v in rng.integers(1, 261, 16)]      # (a length of 0xEE would put that byte into a header)
  slots = [0, 1, 2, 3, 4, 5, 5, 5, 6, 6, 7, 7, 7, 7, 7, 7]
  samples = {s: 640 + s for s in range(8)}
  many = Call(lengths, slots, samples, 8, 260, seed=7).run().check()
  alone = Call(lengths[5:8], [5, 5, 5], {5: 645}, 8, 260, rows=many.rows[5:8], pcm=many.pcm[many.offsets[5]:many.offsets[5] + 645]).run().check()
  a, b = many.mux.to_host(many.seg)[5], alone.mux.to_host(alone.seg)[5]
  assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
  first = many.blob.copy()
  many.run()
  assert np.array_equal(many.blob, first)


def test_sample_conversion_on_the_device():
  """clamp(rintf(x * 32768), -32768, 32767), half to even, NaN 0: the device's int16 equal avi.pcm_s16's for the edge values and for
  every int16 / 32768."""
  from voicepuppet_amd.avi import pcm_s16
  edge = np.array([1.0, -1.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 0.0, -0.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768,
                   -1.5 / 32768, -2.5 / 32768, 32766.5 / 32768, 32767.5 / 32768, -32767.5 / 32768, 0.49 / 32768, 0.51 / 32768], np.float32)
  every = np.arange(-32768, 32768).astype(np.float32) / np.float32(32768.0)
  x = np.concatenate([edge, every, np.random.default_rng(0).normal(0, 0.6, 5000).astype(np.float32)])
  c = Call([], [], {0: x.size}, 1, 16, pcm=x).run()
  off, nbytes, n, st = (int(v) for v in c.slot_table[0])
  assert (nbytes, n, st) == (8 + 2 * x.size, 1, 0)
  got = c.blob[off + 8:off + nbytes].view("<i2")
  assert np.array_equal(got, pcm_s16(x))
  assert got[:22].tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 0, 32767, -32768, 0, 0, 0, 2, 2, 0, -2, -2, 32766, 32767, -32768, 0, 1]
  assert np.array_equal(got[22:22 + 65536], np.arange(-32768, 32768))


def test_segment_refusals():
  import torch
  from voicepuppet_amd.avi import AviMuxer
  m = AviMuxer(4, 260, 2, 100)
  data = torch.zeros(5, 260, dtype=torch.uint8, device="cuda")
  lengths = torch.zeros(5, dtype=torch.int32, device="cuda")
  pcm = torch.zeros(101, dtype=torch.float32, device="cuda")
  with pytest.raises(RuntimeError, match="max_frames"):
    m.segment(data, lengths, lengths)
  with pytest.raises(RuntimeError, match="max_samples"):
    m.segment(None, None, None, pcm, [0, 0], [101, 0])
  with pytest.raises(RuntimeError, match="row_bytes"):
    m.segment(torch.zeros(2, 264, dtype=torch.uint8, device="cuda"), lengths[:2], lengths[:2])
  with pytest.raises(RuntimeError, match="table"):
    m.segment(data[:2], lengths[:2], lengths[:2], out=torch.zeros(64, dtype=torch.uint8, device="cuda"))
  with pytest.raises(ValueError):
    m.segment(data[:2], lengths[:2].to(torch.int64), lengths[:2])


def _pushed(group_pcm, s):
  return np.concatenate(group_pcm[s]) if group_pcm[s] else np.zeros(0, np.float32)


def test_stream_group_records_avi_beside_unchanged_frames(tmp_path, monkeypatch):
  """PuppetStreamGroup(jpeg_quality=75, avi=True), two slots, frame_batch 4 (the configuration of tests/test_gpu_puppet_group.py), 40 ms
  pushes (slot 1 stops earlier) and a finish, record / write_avi / stop: each file passes the reader, its frames are last_jpeg()'s bytes
  of the same pushes, its audio the pushed signal under the conversion rule; a group without avi=True gives bit-identical frames."""
  import torch
  import test_gpu_puppet_group as pg
  from voicepuppet_amd.avi import pcm_s16
  from voicepuppet_amd.generator.loader import ImageLoader, WavLoader
  from voicepuppet_amd.stream import PuppetStreamGroup
  monkeypatch.chdir(tmp_path)
  n = (5, 3)
  pg._assets(2, [640 * k for k in n])
  photos = [ImageLoader().get_data("face%d.jpg" % i)[:, :, ::-1] for i in range(2)]
  pcm = [WavLoader(sr=16000).get_data("a%d.wav" % i).astype(np.float32) for i in range(2)]
  groups = [PuppetStreamGroup(pg.CFG, 2, frame_batch=4, jpeg_quality=75, avi=True), PuppetStreamGroup(pg.CFG, 2, frame_batch=4, jpeg_quality=75)]
  assert groups[1].avi is None and groups[1].audio.keep_pcm is False
  with pytest.raises(RuntimeError):
    groups[1].last_avi()
  with pytest.raises(ValueError):
    PuppetStreamGroup(pg.CFG, 2, frame_batch=4, avi=True)
  for g in groups:
    g.attach(0, photos[0], "photo0.npz")
    g.attach(1, photos[1], None)
  g = groups[0]
  g.record(0, "t0.avi")
  g.record(1, "t1.avi")
  rng = np.random.default_rng(2)
  steps = [({s: pcm[s][640 * i:640 * (i + 1)] for s in range(2) if i < n[s]}, ()) for i in range(max(n))] + [({}, (0, 1))]
  jpegs, pushed = {0: [], 1: []}, {0: [], 1: []}
  for chunks, fin in steps:
    k = g.audio.ready({s: len(c) for s, c in chunks.items()}, fin)
    ears = {s: rng.uniform(size=(k[s], 1)).astype(np.float32) / 100 for s in range(2) if k[s]}
    res = [x.push(chunks, finish=fin, ears=ears) for x in groups]
    for s, c in chunks.items():
      pushed[s].append(c)
    segs = g.write_avi()
    assert sorted(segs) == sorted(s for s in res[0] if res[0][s] or s in chunks)
    if groups[0].last_frames is not None:
      assert torch.equal(groups[0].last_frames, groups[1].last_frames)
      files, other = g.last_jpeg(), groups[1].last_jpeg()
      for s in files:
        assert [f for _, f in files[s]] == [f for _, f in other[s]]
        jpegs[s] += [f for _, f in files[s]]
    else:
      assert groups[1].last_frames is None
  assert [len(jpegs[s]) for s in range(2)] == [n[0] + 1, n[1] + 1]
  assert g.stop(0) == ["t0.avi"] and g.stop(0) is None
  g.reset_slot(1)                                            # a reset stops the recording
  assert g._writers == {}
  for s in range(2):
    a = avi_ref.check("t%d.avi" % s, 512, 512)
    assert a.video == jpegs[s]
    assert np.array_equal(np.frombuffer(b"".join(a.audio), "<i2"), pcm_s16(_pushed(pushed, s)))
    assert len(a.audio) == n[s]


def _run_cli(tmp_path, monkeypatch):
  import test_gpu_stream_cli as sc
  from voicepuppet_amd.pixrefer import infer_stream
  monkeypatch.chdir(tmp_path)
  sc._assets(8000)
  np.random.seed(7)
  infer_stream.main(["--config_path", sc.CFG, "--frame_batch", "4", "--bfmcoeff", "photo.npz", "--chunk_ms", "130", "--avi", "--output_dir", "s",
                     "face.jpg", "a.wav"])


def test_infer_stream_cli_avi_holds_the_jpg_files_and_the_wav(tmp_path, monkeypatch):
  """infer_stream.main --avi on the 0.5 s clip of tests/test_gpu_stream_cli.py: s.avi passes the reader, its frames are the s/<i>.jpg
  files of the same run byte for byte, its audio the wav's int16 samples."""
  from scipy.io import wavfile
  _run_cli(tmp_path, monkeypatch)
  a = avi_ref.check("s.avi", 512, 512)
  names = sorted(os.listdir("s"), key=lambda f: int(f.split(".")[0]))
  assert names == ["%d.jpg" % i for i in range(13)]
  assert a.video == [open(os.path.join("s", f), "rb").read() for f in names]
  assert np.array_equal(np.frombuffer(b"".join(a.audio), "<i2"), wavfile.read("a.wav")[1])


def test_ffprobe_reads_the_cli_file(tmp_path, monkeypatch):
  if not shutil.which("ffprobe"):
    pytest.skip("no ffprobe on this machine: no real player has read a file yet (DESIGN.md section 11)")
  import json
  _run_cli(tmp_path, monkeypatch)
  r = subprocess.run(["ffprobe", "-v", "error", "-count_frames", "-show_streams", "-of", "json", "s.avi"], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr
  st = json.loads(r.stdout)["streams"]
  assert [s["codec_name"] for s in st] == ["mjpeg", "pcm_s16le"]
  assert int(st[0]["nb_read_frames"]) == 13

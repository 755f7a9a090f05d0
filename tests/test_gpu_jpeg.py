"""The device JPEG encoder (libvp_hip.so vp_jpeg_*, voicepuppet_amd.jpeg) against the numpy restatement of its stream (tests/jpeg_ref.py,
itself pinned against libjpeg in tests/test_jpeg_host.py): coefficients, the entropy coder bit for bit, libjpeg's decode of every file,
independence of batch rows, the overflow path, and the encoder inside PuppetStreamGroup and infer_streams."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as jr  # noqa: E402
from test_jpeg_host import PSNR_MARGIN_DB, fixtures, pil_decode, pil_encode  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "params.yml")


def _frames():
  fx = fixtures()
  fx["noise"] = np.random.default_rng(5).integers(0, 256, (512, 512, 3), dtype=np.uint8)
  fx["constant"] = np.full((256, 256, 3), 77, np.uint8)
  return fx


def _encode(frame, quality=75, want_coef=True):
  """One frame through JpegEncoder -> (int16 coefficients [H/16, 6 W/16, 64] or None, file bytes)"""
  import torch
  from voicepuppet_amd.jpeg import JpegEncoder
  enc = JpegEncoder(frame.shape[0], frame.shape[1], 1, quality=quality)
  coef = enc.coefficients() if want_coef else None
  dev = torch.from_numpy(np.ascontiguousarray(frame)).to("cuda")[None]
  data, lengths = enc.encode(dev)
  files = enc.to_host(data, lengths)
  assert files[0][:len(enc.header())] == enc.header() == jr.header(frame.shape[0], frame.shape[1], quality)
  return (coef[0].cpu().numpy() if want_coef else None), files[0]


@pytest.mark.parametrize("name", ["sample22_panel", "background_1", "background_10", "sample22_256", "noise"])
def test_coefficients_equal_the_restatement(name):
  """Equal, except by exactly 1 where the float64 unquantised value lies within 2^-8 of a rounding boundary (k + 1/2) Q: |sample| <= 128,
  |coefficient| <= 1024, two separable 8-term float32 passes, error <= 32 * 2^-24 * 1024 = 2^-9, doubled; such coefficients are at most
  0.1 % of the frame's."""
  frame = _frames()[name]
  got, _ = _encode(frame)
  raw = jr.unquantised(frame)
  want = jr.quantise(raw, 75)
  assert got.shape == want.shape and got.dtype == np.int16
  diff = got.astype(np.int64) - want
  differs = diff != 0
  near = jr.near_boundary(raw, 75)
  print("%s: %d of %d coefficients differ (%.4f %%), %.4f %% lie near a boundary, max |difference| %d" %
        (name, differs.sum(), differs.size, 100.0 * differs.mean(), 100.0 * near.mean(), np.abs(diff).max()))
  assert np.abs(diff).max() <= 1
  assert not (differs & ~near).any(), "%d coefficients differ away from every rounding boundary" % (differs & ~near).sum()
  assert differs.mean() <= 1e-3


@pytest.mark.parametrize("name,quality", [("sample22_panel", 75), ("background_1", 75), ("background_10", 75), ("sample22_256", 75), ("noise", 75),
                                          ("constant", 75), ("sample22_panel", 100), ("sample22_panel", 10)])
def test_entropy_coder_bit_for_bit(name, quality):
  """The restatement's Huffman / stuffing / framing stage fed with the device's own coefficients gives exactly the device's bytes."""
  frame = _frames()[name]
  coef, data = _encode(frame, quality)
  want = jr.entropy_encode(coef, frame.shape[0], frame.shape[1], quality)
  scan = data[len(jr.header(frame.shape[0], frame.shape[1], quality)):]
  print("%s q%d: %d bytes, %d stuffed 0xFF, %d non-zero coefficients" % (name, quality, len(data), scan.count(b"\xff\x00"), np.count_nonzero(coef)))
  assert len(data) == len(want)
  assert data == want
  if name == "constant":
    assert np.count_nonzero(coef[:, :, 1:]) == 0 and np.count_nonzero(np.diff(coef[:, 0::6, 0], axis=1)) == 0
  if name == "noise":
    assert scan.count(b"\xff\x00") > 100


@pytest.mark.parametrize("name", ["sample22_panel", "background_1", "background_10", "sample22_256", "noise", "constant"])
def test_libjpeg_decodes_every_device_file(name):
  frame = _frames()[name]
  _, data = _encode(frame, want_coef=False)
  im = pil_decode(data)
  assert im.size == (frame.shape[1], frame.shape[0]) and im.mode == "RGB"
  info = jr.parse(data)
  assert info["dri"] == frame.shape[1] // 16 and info["rst"] == [i % 8 for i in range(frame.shape[0] // 16 - 1)]
  ours, theirs = jr.psnr(np.asarray(im), frame), jr.psnr(np.asarray(pil_decode(pil_encode(frame))), frame)
  print("%s: device %d bytes %.3f dB, PIL %.3f dB" % (name, len(data), ours, theirs))
  assert ours >= theirs - PSNR_MARGIN_DB, (ours, theirs)


def test_batch_rows_are_independent():
  import torch
  from voicepuppet_amd.jpeg import JpegEncoder
  fx = _frames()
  frame = fx["sample22_panel"]
  enc = JpegEncoder(512, 512, 64)
  alone = enc.to_host(*enc.encode(torch.from_numpy(frame).to("cuda")[None]))[0]
  rng = np.random.default_rng(9)
  batch = rng.integers(0, 256, (64, 512, 512, 3), dtype=np.uint8)
  batch[1::2] = (batch[1::2] >> 3) + 100         # every other frame nearly flat: rows of very different lengths
  for r in (0, 17, 63):
    batch[r] = frame
  files = enc.to_host(*enc.encode(torch.from_numpy(batch).to("cuda")))
  for r in (0, 17, 63):
    assert files[r] == alone, r
  assert pil_decode(files[5]).size == (512, 512) and files[5] != files[6]
  # frames < max_frames: the rows behind stay as they were
  out = torch.full((64, enc.capacity), 0xa5, dtype=torch.uint8, device="cuda")
  lengths = torch.full((64,), -77, dtype=torch.int32, device="cuda")
  enc.encode(torch.from_numpy(batch[:10]).to("cuda"), out, lengths)
  torch.cuda.synchronize()
  assert (lengths[10:] == -77).all() and (lengths[:10] > 0).all()
  assert (out[10:] == 0xa5).all()
  assert bytes(out[0, :int(lengths[0])].cpu().numpy()) == alone


def test_overflow_is_reported_not_written():
  """out_row_bytes smaller than the frame needs: out_bytes -1, the guard band behind each row intact, success returned, and the next
  encode on the same handle is correct.  (A length check inside the kernels, not a fault.)"""
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd.jpeg import JpegEncoder
  fx = _frames()
  frames = np.stack([fx["sample22_panel"], fx["noise"], fx["sample22_panel"]])
  dev = torch.from_numpy(frames).to("cuda")
  enc = JpegEncoder(512, 512, 4)
  good = enc.to_host(*enc.encode(dev))
  assert len(good[0]) < 40000 < len(good[1])
  row, guard = 40000, 4096                  # the panel fits 40000 bytes, the noise frame does not
  buf = torch.full((3, row + guard), 0x5a, dtype=torch.uint8, device="cuda")
  lengths = torch.full((3,), 7, dtype=torch.int32, device="cuda")
  L = _lib.lib()
  # rows of `row` bytes inside the larger buffer: what lies behind the three rows is guard band too
  flat = buf.view(-1)
  rc = L.vp_jpeg_encode(enc.h, ctypes.c_void_p(dev.data_ptr()), 3, ctypes.c_void_p(flat.data_ptr()), row, ctypes.c_void_p(lengths.data_ptr()),
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == 0
  torch.cuda.synchronize()
  assert lengths.tolist() == [len(good[0]), -1, len(good[2])]
  host = flat.cpu().numpy()
  assert host[:len(good[0])].tobytes() == good[0] and host[2 * row:2 * row + len(good[2])].tobytes() == good[2]
  assert (host[len(good[0]):row] == 0x5a).all() and (host[row:2 * row] == 0x5a).all() and (host[2 * row + len(good[2]):] == 0x5a).all()
  # a row too small for even the header
  lengths.fill_(7)
  buf.fill_(0x5a)
  rc = L.vp_jpeg_encode(enc.h, ctypes.c_void_p(dev.data_ptr()), 3, ctypes.c_void_p(flat.data_ptr()), 100, ctypes.c_void_p(lengths.data_ptr()),
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == 0
  torch.cuda.synchronize()
  assert lengths.tolist() == [-1, -1, -1] and (buf == 0x5a).all()
  # to_host falls back to the host encoder for such a row
  data = torch.zeros(3, row, dtype=torch.uint8, device="cuda")
  data, n = enc.encode(dev, data, torch.zeros(3, dtype=torch.int32, device="cuda"))
  files = enc.to_host(data, n, dev)
  assert files[0] == good[0] and files[2] == good[2] and files[1] == pil_encode(frames[1])
  # and the handle is as good as new
  assert enc.to_host(*enc.encode(dev)) == good


def _stream_assets(talkers, samples, H=512):
  """tests/test_gpu_puppet_group.py's recipe (its own copy): face<i>.jpg, a<i>.wav, photo<i>.npz per talker, a synthetic face model, both
  checkpoints (random, saved), three backgrounds."""
  from PIL import Image
  from scipy.io import savemat, wavfile
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.pixrefer import infer_bfmvid
  geometry = [(1.0, [512, 512, 1.0, 0.0, 0.0], 256, 256), (2.0, [512, 512, 1.0, 30.0, -50.0], 200, 300), (1.2, [512, 512, 1.0, 0.0, 0.0], 100, 90)]
  for i in range(talkers):
    rng = np.random.default_rng(10 + i)
    Image.fromarray((rng.uniform(size=(H, 3 * H, 3)) * 255).astype(np.uint8)).save("face%d.jpg" % i)
    t = np.arange(samples[i]) / 16000.0
    wavfile.write("a%d.wav" % i, 16000, (0.3 * np.sin(2 * np.pi * (330 + 110 * i) * t) * np.sin(2 * np.pi * (3 + i) * t) * 32767).astype(np.int16))
    ratio, tp, cx, cy = geometry[i]
    coeff, _ = br.synthetic_coeffs(1, 5 + i)
    np.savez("photo%d.npz" % i, bfmcoeff=coeff.reshape(1, 257), transform_params=np.array(tp, np.float32), center_x=cx, center_y=cy, ratio=ratio)
  fm = br.synthetic_facemodel(3)
  os.makedirs("BFM")
  savemat(os.path.join("BFM", "BFM_model_front.mat"),
          {"meanshape": fm.meanshape, "idBase": fm.idBase, "exBase": fm.exBase, "meantex": fm.meantex, "texBase": fm.texBase,
           "point_buf": fm.point_buf, "tri": fm.tri, "keypoints": (fm.keypoints + 1).reshape(1, -1)})
  os.makedirs("ckpt_bfmnet")
  np.savez(infer_bfmvid.BFMNET_CKPT + ".npz", **random_variables(seed=11))
  gen = infer_bfmvid.load_generator(CFG, 4, H)[0]
  os.makedirs("ckpt_pixrefer")
  np.savez(infer_bfmvid.PIX_CKPT + ".npz", **gen.engine.get_params(0))
  os.makedirs("background")
  rng = np.random.default_rng(1)
  for i in (1, 2, 5):
    Image.fromarray((rng.uniform(size=(H, H, 3)) * 255).astype(np.uint8)).save(os.path.join("background", "%d.jpg" % i))


FRAMES = (13, 30, 51)
SAMPLES = tuple(640 * (f - 1) for f in FRAMES)


def test_stream_group_emits_jpeg_beside_unchanged_frames(tmp_path, monkeypatch):
  """PuppetStreamGroup(jpeg_quality=75), random weights, two slots: one last_jpeg entry per emitted frame, each decoding to within the PSNR
  the restatement reaches on that very last_frames row; last_frames bit-identical to a group without the keyword on the same inputs."""
  import torch
  from voicepuppet_amd.generator.loader import ImageLoader, WavLoader
  from voicepuppet_amd.stream import PuppetStreamGroup
  monkeypatch.chdir(tmp_path)
  _stream_assets(2, SAMPLES[:2])
  photos = [ImageLoader().get_data("face%d.jpg" % i)[:, :, ::-1] for i in range(2)]
  pcm = [WavLoader(sr=16000).get_data("a%d.wav" % i).astype(np.float32) for i in range(2)]
  groups = [PuppetStreamGroup(CFG, 2, frame_batch=4, jpeg_quality=q) for q in (75, None)]
  for g in groups:
    g.attach(0, photos[0], "photo0.npz")
    g.attach(1, photos[1], None)
  assert groups[1].jpeg is None
  with pytest.raises(RuntimeError):
    groups[1].last_jpeg()
  rng = np.random.default_rng(2)
  chunk, emitted = 2080, 0
  steps = [({s: pcm[s][at:at + chunk] for s in range(2) if at < len(pcm[s])}, ()) for at in range(0, len(pcm[1]), chunk)] + [({}, (0, 1))]
  for chunks, fin in steps:
    k = groups[0].audio.ready({s: len(c) for s, c in chunks.items()}, fin)
    ears = {s: rng.uniform(size=(k[s], 1)).astype(np.float32) / 100 for s in range(2) if k[s]}
    res = [g.push(chunks, finish=fin, ears=ears) for g in groups]
    n = sum(len(v) for v in res[0].values())
    if not n:
      assert groups[0].last_jpeg() == {}
      continue
    a, b = groups[0].last_frames, groups[1].last_frames
    assert a.shape == b.shape and torch.equal(a, b)
    files = groups[0].last_jpeg()
    assert {s: [i for i, _ in v] for s, v in files.items()} == {s: [i for i, _ in v] for s, v in res[0].items() if v}
    raw = a.cpu().numpy()
    row = 0
    for s in sorted(files):
      for i, data in files[s]:
        im = pil_decode(data)
        assert im.size == (512, 512)
        got = jr.psnr(np.asarray(im), raw[row])
        want = jr.psnr(np.asarray(pil_decode(jr.encode(raw[row], 75)[1])), raw[row])
        print("slot %d frame %d: device %.3f dB, restatement %.3f dB, %d bytes" % (s, i, got, want, len(data)))
        assert got >= want - PSNR_MARGIN_DB
        row += 1
        emitted += 1
  assert emitted == FRAMES[0] + FRAMES[1]


def _jpgs(d):
  from PIL import Image
  names = sorted(os.listdir(d), key=lambda f: int(f.split(".")[0]))
  assert names == ["%d.jpg" % i for i in range(len(names))], (d, names)
  return names, [Image.open(os.path.join(d, f)) for f in names]


def test_infer_streams_device_jpeg(tmp_path, monkeypatch):
  """infer_streams.main with --device_jpeg on a three-line list writes the file names of a run without the flag; every file opens at
  512 x 512 and decodes as close to the frame the other run wrote (that run's decoded .jpg) as the restatement's coding of the same raw
  frame does, less the margin of tests/test_jpeg_host.py.  The raw frames are recorded from the run without the flag by a wrapper around
  PuppetStreamGroup.push that changes nothing.

  (Measured against the host run's file, not against a re-coding of it: coding an already coded frame again is nearly lossless - on the
  sample22 panel the float64 restatement of the decoded PIL file returns 56.0 dB while the restatement of the raw panel lies 48.2 dB from
  that file - so a threshold taken from a re-coding would refuse the restatement itself.)"""
  from voicepuppet_amd import stream
  from voicepuppet_amd.pixrefer import infer_streams
  monkeypatch.chdir(tmp_path)
  _stream_assets(3, SAMPLES)
  with open("talkers.txt", "w") as f:
    f.write("face0.jpg a0.wav photo0.npz\nface1.jpg a1.wav\n\nface2.jpg a2.wav photo2.npz\n")
  raw = {}
  push = stream.PuppetStreamGroup.push

  def recording_push(self, *a, **k):
    res = push(self, *a, **k)
    if self.last_frames is not None:
      frames, row = self.last_frames.cpu().numpy(), 0
      for s in sorted(res):
        for i, _ in res[s]:
          raw[(s, i)] = frames[row]
          row += 1
    return res
  args = ["--config_path", CFG, "--frame_batch", "4", "--chunk_ms", "130", "--seed", "7"]
  with monkeypatch.context() as m:
    m.setattr(stream.PuppetStreamGroup, "push", recording_push)
    infer_streams.main(args + ["--output_dir", "host", "talkers.txt"])
  infer_streams.main(args + ["--device_jpeg", "--output_dir", "device", "talkers.txt"])
  assert len(raw) == sum(FRAMES)
  for s in range(3):
    names, want = _jpgs(os.path.join("host", str(s)))
    got_names, got = _jpgs(os.path.join("device", str(s)))
    assert got_names == names and len(names) == FRAMES[s]
    for i in range(len(names)):
      assert got[i].size == (512, 512) and got[i].mode == "RGB"
      other = np.asarray(want[i])
      near = jr.psnr(np.asarray(got[i]), other)
      ref = jr.psnr(np.asarray(pil_decode(jr.encode(raw[(s, i)], 75)[1])), other)
      print("talker %d frame %d: against the host run's file: device %.3f dB, restatement %.3f dB" % (s, i, near, ref))
      assert near >= ref - PSNR_MARGIN_DB

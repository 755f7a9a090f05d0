"""AviReader on the device (voicepuppet_amd.avi_read): the frames of Motion-JPEG clips against PIL's decode of every video chunk, the
index path, ranges, dropped frames, and the two tools that take a clip (make_triptychs.py --clip_avi, compare_frames.py)."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import avi_files as af  # noqa: E402
from test_jpeg_dec_422_host import strip_dht  # noqa: E402
from test_jpeg_dec_host import _image, _pil, _pil_rgb  # noqa: E402

W, H = 48, 32


def _write(path, data):
  with open(path, "wb") as f:
    f.write(data)
  return str(path)


def test_a_clip_of_the_device_muxer_reads_back(tmp_path):
  import torch
  from voicepuppet_amd.avi import AviMuxer, AviWriter, pcm_s16
  from voicepuppet_amd.avi_read import AviReader
  from voicepuppet_amd.jpeg import JpegEncoder
  frames = torch.from_numpy(np.stack([_image(W, H, 70 + i) for i in range(5)])).cuda()
  sig = np.random.default_rng(3).uniform(-1, 1, 3200).astype(np.float32)
  enc = JpegEncoder(H, W, 5, quality=90)
  data, lengths = enc.encode(frames)
  mux = AviMuxer(5, enc.capacity, 1, sig.size)
  seg = mux.segment(data, lengths, torch.zeros(5, dtype=torch.int32, device="cuda"), torch.from_numpy(sig).cuda(), [0], [sig.size])
  blob, entries = mux.to_host(seg)[0]
  path = str(tmp_path / "mux.avi")
  w = AviWriter(path, W, H, sample_rate=16000)
  w.append(blob, entries)
  w.close()
  r = AviReader(path)
  assert (r.frames, r.width, r.height, r.fps) == (5, W, H, 25.0) and r.check_index() == [] and not r.truncated
  rate, samples, fmt = r.audio()
  assert (rate, fmt) == (16000, "s16") and np.array_equal(samples[:, 0], pcm_s16(sig))
  got = r.read(0, 5).cpu().numpy()
  jpegs = enc.to_host(data, lengths)
  for i in range(5):
    assert r.frame_bytes(i) == jpegs[i]
    assert np.array_equal(got[i], _pil_rgb(jpegs[i])), i
  assert r.fallbacks == 0
  bgr = r.read(0, 5, bgr=True).cpu().numpy()
  assert np.array_equal(bgr, got[..., ::-1])


def _mixed_clip(tmp_path):
  """Frames 0 .. 3: PIL 4:2:2 without Huffman tables; 4: 4:2:0 with its tables; 5: progressive; then a dropped frame."""
  jpegs = [strip_dht(_pil(_image(W, H, 80 + i, i == 2), subsampling=1, quality=85)) for i in range(4)]
  jpegs.append(_pil(_image(W, H, 84), quality=85))
  jpegs.append(_pil(_image(W, H, 85), quality=85, progressive=True))
  parts = [af.chunk(b"00dc", j) for j in jpegs] + [af.chunk(b"00dc", b"")]
  data, _ = af.avi(W, H, [af.video_strl(W, H)], parts)
  return _write(tmp_path / "mixed.avi", data), jpegs + [jpegs[-1]]


def test_tableless_422_frames_a_420_frame_and_a_progressive_frame(tmp_path):
  from voicepuppet_amd.avi_read import AviReader
  from voicepuppet_amd.jpeg_dec import parse
  path, jpegs = _mixed_clip(tmp_path)
  assert parse(jpegs[0], accept_422=True).refused and parse(jpegs[0], accept_422=True, default_huffman=True).sampling == 3
  r = AviReader(path, scan_chunk_bytes=32)
  assert r.frames == 7 and r.describe() == "7 frames 4:2:2" and r.audio_format is None
  want = np.stack([_pil_rgb(j) for j in jpegs])
  got = r.read(0, 7)
  assert got.shape == (7, H, W, 3) and np.array_equal(got.cpu().numpy(), want)
  assert r.fallbacks == 1
  rows = -(-H // 8)
  assert r.last_segments == [rows] * 4 + [H // 16, 0, 0]           # the scan held at first sight; gaps for the PIL frame and the copy
  # the second read runs from the index, and gives the same bytes
  again = r.read(0, 7)
  assert r.last_segments == [rows] * 4 + [H // 16, 0, 0] and r.fallbacks == 2
  assert np.array_equal(again.cpu().numpy(), want)
  dec = r._decoder(False)
  keys = sorted(k[0] for k in dec.index)
  assert keys == ["%s#%d" % (os.path.abspath(path), i) for i in range(5)] and all(k[1] == os.path.getsize(path) for k in dec.index)
  # the index travels through a file to another reader, whose first read then needs no scan
  r.save_index(str(tmp_path / "index.npz"))
  other = AviReader(path, scan_chunk_bytes=None)
  other.load_index(str(tmp_path / "index.npz"))
  assert np.array_equal(other.read(0, 5).cpu().numpy(), want[:5]) and other.last_segments == [rows] * 4 + [H // 16]
  # a range, into a caller's tensor; a dropped frame at the head of a range is decoded from the frame it repeats
  import torch
  out = torch.full((3, H, W, 3), 9, dtype=torch.uint8, device="cuda")
  part = r.read(2, 2, out=out)
  assert part.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy()[:2], want[2:4]) and (out[2] == 9).all()
  assert np.array_equal(r.read(6, 1).cpu().numpy()[0], want[5]) and np.array_equal(r.read(5, 2).cpu().numpy(), want[5:7])
  with pytest.raises(IndexError):
    r.read(5, 3)
  # batches smaller than the run: the dropped frame at the head of the last batch is copied from the batch before it
  small = AviReader(path, batch=2)
  assert np.array_equal(small.read(0, 7).cpu().numpy(), want) and small.fallbacks == 1


def test_a_range_equals_rows_of_the_whole_and_a_repeat_equals_its_predecessor(tmp_path):
  from voicepuppet_amd.avi_read import AviReader
  jpegs = [_pil(_image(W, H, 90 + i), subsampling=1, quality=90) for i in range(4)]
  parts = [af.chunk(b"00dc", jpegs[0]), af.chunk(b"00dc", jpegs[1]), af.chunk(b"00dc", b""), af.chunk(b"00dc", jpegs[2]), af.chunk(b"00dc", jpegs[3])]
  data, _ = af.avi(W, H, [af.video_strl(W, H)], parts)
  r = AviReader(_write(tmp_path / "five.avi", data))
  whole = r.read(0, 5).cpu().numpy()
  assert np.array_equal(r.read(2, 2).cpu().numpy(), whole[2:4])
  assert np.array_equal(whole[2], whole[1]) and not np.array_equal(whole[3], whole[2])
  assert np.array_equal(whole[[0, 1, 3, 4]], np.stack([_pil_rgb(j) for j in jpegs]))


def test_make_triptychs_clip_avi_end_to_end(tmp_path, monkeypatch, capsys):
  """Six frames of the matte scene as <i>.jpg and as one AVI file with a stereo 44.1 kHz track: --clip_avi writes the triptychs, the
  coefficients and the list line of --clip_dir, and the audio.wav WavLoader reads back to the signal; compare_frames.py finds the clip
  and the folder equal frame by frame."""
  from PIL import Image
  import bfm_fit_ref as fr
  import matte_clean_ref as mr
  from oracle import bfm_ref as br
  from test_gpu_bfm_fit import write_bfm_assets
  from voicepuppet_amd.datasets import make_triptychs as mt
  from voicepuppet_amd.generator.loader import WavLoader
  from voicepuppet_amd.pixrefer import compare_frames as cf
  S_ = 256
  monkeypatch.chdir(tmp_path)
  g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")))
  write_bfm_assets(br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True), g["lm3d68"])
  xy = np.stack([fr.photo_landmarks(g["landmarks_2d"][f], 0.7, (50.0, 45.0)) for f in range(6)])
  frames, _, _ = mr.scene(S_, S_, seed=11, n=6, spill_levels=10.0)
  os.makedirs("clip")
  jpegs = []
  for i in range(6):
    b = io.BytesIO()
    Image.fromarray(frames[i]).save(b, "JPEG", quality=95, subsampling=1 if i % 2 else 2)
    jpegs.append(b.getvalue())
    _write(os.path.join("clip", "%d.jpg" % i), jpegs[-1])
  np.savetxt("_landmark.txt", xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  pcm = np.random.default_rng(8).integers(-20000, 20000, (44100 * 6 // 25, 2)).astype("<i2")
  parts = []
  for i in range(6):
    parts += [af.chunk(b"01wb", pcm[1764 * i:1764 * (i + 1)].tobytes()), af.chunk(b"00dc", strip_dht(jpegs[i]) if i % 2 else jpegs[i])]
  data, _ = af.avi(S_, S_, [af.video_strl(S_, S_), af.audio_strl(1, 2, 44100, 16)], parts)
  _write("clip.avi", data)
  common = ["--landmarks", "_landmark.txt", "--rounds", "1", "--id_steps", "1", "--frame_batch", "4", "--list", "train.txt", "--key_matte"]
  mt.main(["--clip_dir", "clip", "--out_dir", "from_dir"] + common)
  line_dir = capsys.readouterr().out.strip().splitlines()[-1]
  mt.main(["--clip_avi", "clip.avi", "--out_dir", "from_avi"] + common)
  line_avi = capsys.readouterr().out.strip().splitlines()[-1]
  print(line_avi)
  assert line_avi.endswith("; avi: 6 frames 4:2:0, audio 44100 Hz x 2 -> audio.wav")
  assert " 0 read with PIL" not in line_dir and " 0 read with PIL" in line_avi     # the folder's 4:2:2 files went to PIL, the clip's did not
  for i in range(6):
    assert open(os.path.join("from_dir", "%d.jpg" % i), "rb").read() == open(os.path.join("from_avi", "%d.jpg" % i), "rb").read(), i
  for name in ("bfmcoeff.txt", "ear.txt"):
    assert open(os.path.join("from_dir", name)).read() == open(os.path.join("from_avi", name)).read()
  assert open("train.txt").read() == "from_dir|6\nfrom_avi|6\n" and not os.path.exists(os.path.join("from_dir", "audio.wav"))
  from scipy.signal import resample_poly
  got = WavLoader(sr=16000).get_data(os.path.join("from_avi", "audio.wav"))
  assert np.array_equal(got, resample_poly((pcm.astype(np.float32) / 32768.0).mean(axis=1), 160, 441).astype(np.float32))
  assert np.array_equal(got, WavLoader(sr=16000).get_data("clip.avi"))
  with pytest.raises(SystemExit):
    mt.parse_options(["--clip_dir", "clip", "--clip_avi", "clip.avi", "--landmarks", "l", "--out_dir", "o"])

  for a, b in (("clip.avi", "clip"), ("clip", "clip.avi"), ("clip.avi", "clip.avi")):
    res = cf.main([a, b])
    assert res["kind"] == "jpg" and len(res["frames"]) == 6
    assert all(f["MSE"] == 0.0 and f["L1"] == 0.0 for f in res["frames"])
  capsys.readouterr()

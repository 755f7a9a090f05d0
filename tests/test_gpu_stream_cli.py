"""The streaming CLI end to end (voicepuppet_amd/pixrefer/infer_stream.py, PuppetStream) against infer_bfmvid on the same inputs: the
synthetic BFM face model and photo coefficients of test_infer_bfmvid_cli_through_the_clip_renderer, checkpoints of both networks
written once (so that every run restores the same weights), the same np.random.seed (the ears)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "params.yml")


def _assets(n_samples):
  from PIL import Image
  from scipy.io import savemat, wavfile
  from oracle import bfm_ref as br
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.pixrefer import infer_bfmvid
  rng = np.random.default_rng(0)
  Image.fromarray((rng.uniform(size=(512, 1536, 3)) * 255).astype(np.uint8)).save("face.jpg")
  t = np.arange(n_samples) / 16000.0
  wavfile.write("a.wav", 16000, (0.3 * np.sin(2 * np.pi * 440 * t) * np.sin(2 * np.pi * 3 * t) * 32767).astype(np.int16))
  fm = br.synthetic_facemodel(3)
  os.makedirs("BFM")
  savemat(os.path.join("BFM", "BFM_model_front.mat"),
          {"meanshape": fm.meanshape, "idBase": fm.idBase, "exBase": fm.exBase, "meantex": fm.meantex, "texBase": fm.texBase,
           "point_buf": fm.point_buf, "tri": fm.tri, "keypoints": (fm.keypoints + 1).reshape(1, -1)})
  coeff, _ = br.synthetic_coeffs(1, 5)
  np.savez("photo.npz", bfmcoeff=coeff.reshape(1, 257), transform_params=np.array([512, 512, 1.0, 0.0, 0.0], np.float32),
           center_x=256, center_y=256, ratio=0.9)
  os.makedirs("ckpt_bfmnet")
  np.savez(infer_bfmvid.BFMNET_CKPT + ".npz", **random_variables(seed=11))
  gen = infer_bfmvid.load_generator(CFG, 4, 512)[0]          # random generator weights, saved so that every run restores them
  os.makedirs("ckpt_pixrefer")
  np.savez(infer_bfmvid.PIX_CKPT + ".npz", **gen.engine.get_params(0))


def _frames(d):
  from PIL import Image
  names = sorted(os.listdir(d), key=lambda f: int(f.split(".")[0]))
  assert names == ["%d.jpg" % i for i in range(len(names))]
  return np.stack([np.asarray(Image.open(os.path.join(d, f))) for f in names])


def _run_both(n, chunks):
  from PIL import Image
  from voicepuppet_amd.pixrefer import infer_bfmvid, infer_stream
  _assets(n)
  os.makedirs("background")
  rng = np.random.default_rng(1)
  for i in (1, 2, 5):                               # some frames have a background, the others take the 0.5 grey
    Image.fromarray((rng.uniform(size=(512, 512, 3)) * 255).astype(np.uint8)).save(os.path.join("background", "%d.jpg" % i))
  args = ["--config_path", CFG, "--frame_batch", "4", "--bfmcoeff", "photo.npz"]
  np.random.seed(7)
  infer_bfmvid.main(args + ["face.jpg", "a.wav"])
  ref = _frames("output")
  assert ref.shape[0] == 1 + n // 640
  assert any(not np.array_equal(ref[0], ref[i]) for i in range(1, ref.shape[0]))      # the frames do move
  out = {}
  for ms in chunks:
    np.random.seed(7)
    infer_stream.main(args + ["--chunk_ms", str(ms), "--output_dir", "s%d" % ms, "face.jpg", "a.wav"])
    got = _frames("s%d" % ms)
    assert got.shape == ref.shape, (ms, got.shape, ref.shape)
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print("%d samples, chunk %d ms: max |d| %d, mean |d| %.4f, pixels |d| > 8: %.5f, frames equal %d of %d" % (
        n, ms, d.max(), d.mean(), (d > 8).mean(), sum(np.array_equal(got[i], ref[i]) for i in range(ref.shape[0])), ref.shape[0]))
    out[ms] = d
  return out


def test_infer_stream_cli_matches_infer_bfmvid(tmp_path, monkeypatch):
  """A 0.5 s clip (13 frames, shorter than either stream window): infer_stream at --chunk_ms 40 and 130 writes infer_bfmvid's frames,
  the same number and the same decoded pixels bit for bit.  No frame is ready before finish, and finish runs the exact-size plan,
  so the coefficients are bit-identical; the renderer and the generator work per frame and see the same coefficients, head-sway
  angles, ears and backgrounds by global frame index."""
  monkeypatch.chdir(tmp_path)
  for ms, d in _run_both(8000, (40, 130)).items():
    assert d.max() == 0, ms


def test_infer_stream_cli_long_clip_within_bound(tmp_path, monkeypatch):
  """A 2 s clip (51 frames): frames are emitted while the audio arrives, on the window plan, whose trunk GEMMs are tiled unlike the
  whole-clip plan's (coefficients within 1e-5 of max|offline|, tests/test_gpu_stream.py).  A 1e-5 change can still move a rasterised
  edge pixel, so decoded frames are compared by a bound: the same frame count, mean |d| <= 0.5 grey levels, and at most 1 % of the
  pixels off by more than 8 levels.  Measured (40 and 130 ms alike): 37 of 51 frames bit-identical, mean |d| 0.23, 0.14 % of the
  pixels off by more than 8, max |d| 33."""
  monkeypatch.chdir(tmp_path)
  for ms, d in _run_both(32000, (40, 130)).items():
    assert d.mean() <= 0.5 and (d > 8).mean() <= 0.01, (ms, float(d.mean()), float((d > 8).mean()))

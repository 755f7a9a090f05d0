"""Key mattes on the device (voicepuppet_amd.matte.KeyMatte; csrc/key_matte.hip: vp_keymatte_*) against the numpy restatement
tests/key_matte_ref.py, which tests/test_key_matte_host.py pins: the border moments exactly, the model bit for bit, the raw key and
the matte byte for byte over every pixel.  Then views, guards, refusals, and the dataset launcher end to end on six frames of the
synthetic studio scene."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_matte_ref as kr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")
# (n, H, W): one tile and less; 3 x 3 tiles, ragged; odd sizes; 8 x 8 tiles; one tile row / column with a window wider than the image
SIZES = [(1, 16, 16), (3, 96, 80), (5, 33, 47), (2, 256, 256)]
THIN = [(1, 17, 64), (1, 64, 17)]
# explicit (band, side_rows) per size: 2 * band == W and side_rows == H among them
EXPLICIT = {(1, 16, 16): (8, 16), (3, 96, 80): (5, 60), (5, 33, 47): (23, 33), (2, 256, 256): (128, 256)}
RADII = (0, 1, 4, 16)
EPS = (0.01, 25.0, 400.0)


@functools.lru_cache(maxsize=None)
def _scene(n, H, W):
  frames, alpha = kr.scene(H, W, seed=H * 1000 + W, n=n)
  frames.setflags(write=False)
  return frames


@functools.lru_cache(maxsize=None)
def _fit(n, H, W, band=None, side_rows=None):
  S, model = kr.fit(_scene(n, H, W), band, side_rows)
  S.setflags(write=False)
  model.setflags(write=False)
  return S, model


@functools.lru_cache(maxsize=None)
def _keyer():
  from voicepuppet_amd.matte import KeyMatte
  return KeyMatte(5, 256, 256)


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the cached references are read-only)


def _bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.int64)


def _solve_host(S, sigma_min=2.0):
  import ctypes
  from voicepuppet_amd import _lib
  out = (ctypes.c_double * kr.MODEL_DOUBLES)()
  assert _lib.lib().vp_keymatte_solve_host((ctypes.c_int64 * 21)(*[int(v) for v in S]), sigma_min, out) == 0
  return np.array(out[:], np.float64)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_moments_exact_and_model_bit_for_bit(size, explicit):
  band, side_rows = EXPLICIT[size] if explicit else (None, None)
  if explicit:
    assert 2 * EXPLICIT[(1, 16, 16)][0] == 16 and EXPLICIT[(2, 256, 256)] == (128, 256)
  S, model = _fit(*size, band, side_rows)
  km = _keyer().fit(_dev(_scene(*size)), band=band, side_rows=side_rows)
  got_S = km.tensor("moments").cpu().numpy()
  got = km.model().cpu().numpy()
  assert got_S.dtype == np.int64 and got_S.shape == (2, 21) and np.array_equal(got_S, S), (got_S - S)
  want = _solve_host(got_S[1])
  want[kr.KEPT] = float(got_S[1, 20]) / float(got_S[0, 20])
  assert np.array_equal(_bits(got), _bits(want)), (got, want)
  assert np.array_equal(_bits(got), _bits(model))
  rep = km.report()
  assert rep == {"status": int(model[kr.STATUS]), "N": int(S[1, 20]), "kept": float(model[kr.KEPT]), "residual_rms": float(model[kr.RESIDUAL_RMS])}
  assert np.array_equal(_bits(km.tensor("model").cpu().numpy()), _bits(got))


@pytest.mark.parametrize("size", SIZES + THIN)
def test_raw_key_and_matte_byte_for_byte(size):
  import torch
  frames, (_, model) = _scene(*size), _fit(*size)
  km = _keyer().set_model(_dev(model))
  dev = _dev(frames)
  raw_want = kr.raw_key(model, frames)
  guide = kr.guide(frames)
  for radius in RADII:
    for eps in EPS if radius else EPS[1:2]:
      raw = torch.zeros(size, dtype=torch.uint8, device="cuda")
      got = km.matte(dev, radius=radius, eps=eps, raw=raw).cpu().numpy()
      assert np.array_equal(raw.cpu().numpy(), raw_want), (radius, eps)
      want = kr.guided(guide, raw_want, radius, eps)
      assert got.shape == want.shape and np.array_equal(got, want), (radius, eps, int((got != want).sum()), np.argwhere(got != want)[:4])
      if radius == 0:
        assert np.array_equal(got, raw_want)
  # other thresholds move the raw key
  got = km.matte(dev, lo=2.0, hi=5.0, radius=0).cpu().numpy()
  assert np.array_equal(got, kr.raw_key(model, frames, 2.0, 5.0)) and not np.array_equal(got, raw_want)


def test_all_backdrop_and_all_foreground_frames():
  n, H, W = 3, 96, 80
  _, model = _fit(n, H, W)
  rng = np.random.default_rng(4)
  yy, xx = np.mgrid[0:H, 0:W]
  plane = lambda c: model[3 * c] + model[3 * c + 1] * xx + model[3 * c + 2] * yy
  back = np.stack([plane(c) for c in range(3)], -1) + rng.normal(0, 3.0, (H, W, 3))
  fore = np.stack([205.0 + 12.0 * np.sin(xx * 0.9), 160.0 + 9.0 * np.cos(yy * 0.7), 135.0 + 0 * xx], -1) + rng.normal(0, 2.0, (H, W, 3))
  frames = np.clip(np.floor(np.stack([back, fore]) + 0.5), 0, 255).astype(np.uint8)
  km = _keyer().set_model(_dev(model))
  for radius in (0, 4, 16):
    want_raw, want = kr.matte(model, frames, radius=radius)
    got = km.matte(_dev(frames), radius=radius).cpu().numpy()
    assert np.array_equal(got, want), radius
    assert (want[0] == 0).mean() > 0.95 and np.all(want[1] == 255)


def test_padded_strided_view_equals_its_dense_copy():
  import torch
  n, H, W = 3, 96, 80
  frames = _scene(n, H, W)
  base = torch.full((n, H + 3, W + 5, 3), 255, dtype=torch.uint8, device="cuda")
  view = base[:, 1:H + 1, 2:W + 2]
  view.copy_(_dev(frames))
  assert not view.is_contiguous()
  km = _keyer()
  dense_model = km.fit(_dev(frames)).model().cpu().numpy()
  dense = km.matte(_dev(frames), radius=4).cpu().numpy()
  view_model = km.fit(view).model().cpu().numpy()
  assert np.array_equal(_bits(view_model), _bits(dense_model)) and np.array_equal(_bits(dense_model), _bits(_fit(n, H, W)[1]))
  assert np.array_equal(km.matte(view, radius=4).cpu().numpy(), dense)
  assert np.array_equal(km.matte(view[1:2], radius=4).cpu().numpy(), dense[1:2])
  with pytest.raises(ValueError, match="strides"):
    km.matte(base[:, :H, ::2])                                    # every other pixel of a row: not a frame layout


def test_out_and_raw_are_honoured_and_guards_stay_intact():
  """the outputs sit between poisoned guard frames; the handle lives in the middle of a poisoned buffer and runs at its largest sizes"""
  import ctypes
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd.matte import KeyMatte
  n, H, W = 3, 96, 80
  frames, (_, model) = _scene(n, H, W), _fit(n, H, W)
  km = KeyMatte(n, H, W, max_radius=16)
  need, guard = km.workspace.numel(), 4096
  big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
  km.close()
  h = ctypes.c_void_p()
  _lib.check(km.L.vp_keymatte_create(ctypes.byref(km.desc), ctypes.c_void_p(big.data_ptr() + guard), need, ctypes.byref(h)), "create")
  km.workspace, km.h = big[guard:guard + need], h
  out = torch.full((n + 2, H, W), 0x5A, dtype=torch.uint8, device="cuda")
  raw = torch.full((n + 2, H, W), 0x5A, dtype=torch.uint8, device="cuda")
  km.fit(_dev(frames))
  before = km.tensor("moments").clone(), km.tensor("model").clone()
  got = km.matte(_dev(frames), radius=16, out=out[1:n + 1], raw=raw[1:n + 1])
  torch.cuda.synchronize()
  assert got.data_ptr() == out[1].data_ptr() and tuple(got.shape) == (n, H, W)
  want_raw, want = kr.matte(model, frames, radius=16)
  assert np.array_equal(out[1:n + 1].cpu().numpy(), want) and np.array_equal(raw[1:n + 1].cpu().numpy(), want_raw)
  for t in (out, raw):
    assert bool((t[0] == 0x5A).all()) and bool((t[n + 1] == 0x5A).all())
  assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + need:] == 0xA5).all())
  assert torch.equal(km.tensor("moments"), before[0]) and torch.equal(km.tensor("model").view(torch.int64), before[1].view(torch.int64))
  # a smaller call through the same handle leaves the frames behind it alone
  out.fill_(0x5A)
  km.matte(_dev(frames[:1]), radius=4, out=out[1:])
  assert np.array_equal(out[1].cpu().numpy(), kr.matte(model, frames[:1])[1][0]) and bool((out[2:] == 0x5A).all()) and bool((out[0] == 0x5A).all())
  km.close()


def test_a_frame_alone_equals_the_frame_in_a_batch_and_set_model_is_the_identity():
  n, H, W = 5, 33, 47
  frames = _scene(n, H, W)
  km = _keyer().fit(_dev(frames))
  model = km.model()
  batch = km.matte(_dev(frames)).cpu().numpy()
  batch_raw = km.matte(_dev(frames), radius=0).cpu().numpy()
  km.set_model(model)
  assert np.array_equal(_bits(km.model().cpu().numpy()), _bits(model.cpu().numpy()))
  assert np.array_equal(km.matte(_dev(frames)).cpu().numpy(), batch)
  for k in range(n):
    assert np.array_equal(km.matte(_dev(frames[k:k + 1])).cpu().numpy()[0], batch[k]), k
    assert np.array_equal(km.matte(_dev(frames[k:k + 1]), radius=0).cpu().numpy()[0], batch_raw[k]), k
  assert len({b.tobytes() for b in batch}) == n


def test_bad_arguments_raise_before_anything_is_enqueued():
  import torch
  from voicepuppet_amd.matte import KeyMatte
  H, W = 40, 48
  km = KeyMatte(2, H, W, max_radius=4).set_model(_dev(_fit(3, 96, 80)[1]))
  model = km.model().cpu().numpy()
  out = torch.full((2, H, W), 0x5A, dtype=torch.uint8, device="cuda")
  ok = torch.zeros(2, H, W, 3, dtype=torch.uint8, device="cuda")
  with pytest.raises(ValueError, match="uint8"):
    km.matte(ok.float(), out=out)
  with pytest.raises(ValueError, match="uint8"):
    km.fit(ok.float())
  with pytest.raises(RuntimeError, match="max_height"):
    km.matte(torch.zeros(1, H + 1, W, 3, dtype=torch.uint8, device="cuda"), out=torch.full((1, H + 1, W), 0x5A, dtype=torch.uint8, device="cuda"))
  with pytest.raises(RuntimeError, match="max_height"):
    km.fit(torch.zeros(1, H + 1, W, 3, dtype=torch.uint8, device="cuda"))
  with pytest.raises(RuntimeError, match="max_frames"):
    km.matte(torch.zeros(3, H, W, 3, dtype=torch.uint8, device="cuda"), out=torch.zeros(3, H, W, dtype=torch.uint8, device="cuda"))
  with pytest.raises(RuntimeError, match="radius 5"):
    km.matte(ok, radius=5, out=out)
  with pytest.raises(RuntimeError, match="lo"):
    km.matte(ok, lo=10.0, hi=10.0, out=out)
  with pytest.raises(RuntimeError, match="eps"):
    km.matte(ok, eps=0.0, out=out)
  with pytest.raises(RuntimeError, match="band"):
    km.fit(ok, band=W // 2 + 1)
  with pytest.raises(RuntimeError, match="side_rows"):
    km.fit(ok, side_rows=H + 1)
  with pytest.raises(ValueError, match="out must be"):
    km.matte(ok, out=out[:1])
  torch.cuda.synchronize()
  assert bool((out == 0x5A).all())
  assert np.array_equal(_bits(km.model().cpu().numpy()), _bits(model))
  with pytest.raises(ValueError, match="max_radius"):
    KeyMatte(2, H, W, max_radius=17)


# ---- the launcher end to end -------------------------------------------------------------------------------------------------------------
def _rgb(path):
  from PIL import Image
  return np.asarray(Image.open(path).convert("RGB"))


def test_alpha_dir_takes_panel_size_mattes_as_they_are(tmp_path):
  """what --write_alpha wrote is panel size: with --crop or --size it is not the frames' size, and goes through no crop and no resize"""
  from PIL import Image
  from voicepuppet_amd.datasets import make_triptychs as mt

  class Reader:
    h, w, size = 40, 48, 32

    def fit_to_panel(self, frames):
      raise AssertionError("panel-size mattes are not resized")
  planes = np.random.default_rng(8).integers(0, 256, (2, 32, 32), dtype=np.uint8)
  for i in range(2):
    Image.fromarray(planes[i]).save(str(tmp_path / ("%d.png" % (3 + i))))
  got = mt.read_alpha(Reader(), str(tmp_path), 3, 2)
  assert got.is_cuda and np.array_equal(got.cpu().numpy(), planes)
  Image.fromarray(planes[0, :31]).save(str(tmp_path / "5.png"))
  with pytest.raises(ValueError, match="5.png is 32 x 31"):
    mt.read_alpha(Reader(), str(tmp_path), 4, 2)


def test_launcher_key_matte_end_to_end(tmp_path, monkeypatch, capsys):
  """Six JPEG frames of the studio scene through make_triptychs.py --key_matte --write_alpha.  JPEG noise: at quality 95 the luma
  quantiser steps are 1 .. 10, a coefficient is off by at most half a step, so a grey panel's error has an rms of about
  sqrt(64 * 5^2 / 12) / 8 = 1.4 levels plus the rounding of the colour conversion: the mean absolute difference is held to 2 levels.
  Step 6's layout keeps the frame itself in panel 1 (make_data_from_GRID.py:693); what is black where the matte is 0 is the product
  panel 1 x panel 3 that PuppetStreamGroup.attach forms."""
  import torch
  from PIL import Image
  import bfm_fit_ref as fr
  from test_gpu_bfm_fit import write_bfm_assets
  from voicepuppet_amd.datasets import make_triptychs as mt
  from voicepuppet_amd.matte import KeyMatte
  S = 256
  monkeypatch.chdir(tmp_path)
  g = dict(np.load(GOLDEN))
  write_bfm_assets(br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True), g["lm3d68"])
  xy = np.stack([fr.photo_landmarks(g["landmarks_2d"][f], 0.7, (50.0, 45.0)) for f in range(6)])
  frames, _ = kr.scene(S, S, seed=11, n=6)
  os.makedirs("clip")
  for i in range(6):
    Image.fromarray(frames[i]).save(os.path.join("clip", "%d.jpg" % i), "JPEG", quality=95)
  np.savetxt(os.path.join("clip", "_landmark.txt"), xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  common = ["--clip_dir", "clip", "--landmarks", os.path.join("clip", "_landmark.txt"), "--rounds", "1", "--id_steps", "1", "--frame_batch", "4"]

  res = mt.main(common + ["--out_dir", "keyed", "--key_matte", "--write_alpha", "alpha"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  assert "triptych status 0:6, 0 repeated" in line and "key matte: kept " in line and " levels" in line
  assert res["key_matte"]["status"] == 0 and res["key_matte"]["kept"] > 0.9 and 1.0 < res["key_matte"]["residual_rms"] < 4.5

  # the matte KeyMatte returns for the decoded panel-size frames: the model of the first device batch (4 frames), applied to all six
  reader = mt.FrameReader("clip", 4, None, None)
  decoded = torch.cat([reader.read(0, 4), reader.read(4, 2)])
  km = KeyMatte(6, S, S).fit(decoded[:4])
  assert km.report() == res["key_matte"]
  want = km.matte(decoded).cpu().numpy()
  assert np.array_equal(want, kr.matte(kr.fit(decoded[:4].cpu().numpy())[1], decoded.cpu().numpy())[1])
  assert (want == 0).mean() > 0.4 and (want == 255).mean() > 0.15
  for i in range(6):
    assert np.array_equal(np.asarray(Image.open(os.path.join("alpha", "%d.png" % i))), want[i]), i
    img = _rgb(os.path.join("keyed", "%d.jpg" % i))
    assert img.shape == (S, 3 * S, 3)
    p1, p2, p3 = img[:, :S].astype(np.float64), img[:, S:2 * S], img[:, 2 * S:].astype(np.float64)
    diff = np.abs(p3 - want[i][..., None]).mean()
    product = (p1 * p3 / 255.0)[want[i] == 0].mean()
    print("frame %d: panel 3 against the device matte, mean |difference| %.3f levels; panel 1 x panel 3 where the matte is 0: %.3f" % (i, diff, product))
    assert diff <= 2.0 and product <= 2.0
    side, y0, x0 = res["geometry"][i]
    assert p2[0, 0].max() < 30 and p2[y0:y0 + side, x0:x0 + side].max() > p2[0, 0].max()   # the render on black
  assert not os.path.exists(os.path.join("alpha", "6.png"))

  # the written mattes as --alpha_dir: the same files
  mt.main(common + ["--out_dir", "reread", "--alpha_dir", "alpha"])
  for i in range(6):
    assert open(os.path.join("reread", "%d.jpg" % i), "rb").read() == open(os.path.join("keyed", "%d.jpg" % i), "rb").read(), i

  # without either option: the path as it was.  build() is handed the frames, the render and the face mask and no matte, and the files
  # are those a fresh TriptychBuilder writes from the same arguments (step 5's layout)
  from voicepuppet_amd.triptych import TriptychBuilder
  calls, real = [], TriptychBuilder.build

  def spy(self, frames, render, face_mask, geometry, alpha=None, out=None):
    calls.append((frames.clone(), render.clone(), face_mask.clone(), np.array(geometry), alpha))
    return real(self, frames, render, face_mask, geometry, alpha=alpha, out=out)
  monkeypatch.setattr(TriptychBuilder, "build", spy)
  monkeypatch.setattr(KeyMatte, "__init__", lambda self, *a, **k: pytest.fail("KeyMatte built without --key_matte"))
  res5 = mt.main(common + ["--out_dir", "plain"])
  monkeypatch.undo()
  monkeypatch.chdir(tmp_path)
  line5 = capsys.readouterr().out.strip().splitlines()[-1]
  assert "key matte" not in line5 and "key_matte" not in res5 and "triptych status 0:6, 0 repeated" in line5
  assert open(os.path.join("keyed", "bfmcoeff.txt")).read() == open(os.path.join("plain", "bfmcoeff.txt")).read()
  assert len(calls) == 2 and all(c[4] is None for c in calls)
  assert torch.equal(torch.cat([c[0] for c in calls]), decoded)
  os.makedirs("direct")
  builder, first = TriptychBuilder(S, 4), 0
  for frames_, render, face_mask, geometry, _ in calls:
    trip, st = builder.build(frames_, render, face_mask, geometry)
    builder.write(trip, st, "direct", first)
    first += int(frames_.shape[0])
  for i in range(6):
    plain = open(os.path.join("plain", "%d.jpg" % i), "rb").read()
    assert plain == open(os.path.join("direct", "%d.jpg" % i), "rb").read(), i
    assert plain != open(os.path.join("keyed", "%d.jpg" % i), "rb").read()
    side, y0, x0 = res5["geometry"][i]
    p3 = _rgb(os.path.join("plain", "%d.jpg" % i))[:, 2 * S:]
    assert p3[y0:y0 + side, x0:x0 + side].max() > 200 and p3[0, 0].max() < 30          # the face mask, not a matte

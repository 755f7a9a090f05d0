"""Training triptychs on the device (voicepuppet_amd.triptych.TriptychBuilder; csrc/triptych.hip: vp_triptych_*) against the numpy
restatement tests/triptych_ref.py, which tests/test_triptych_host.py pins to scipy and to a float64 Gaussian.  Every comparison is
byte-exact over every element: the hole fill, the mask chain (resize, erosion, quantisation, blur), the panels, the rows left untouched.
Then the launcher end to end on six synthetic frames, and the written files through the existing PixRefer input pipeline."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import triptych_ref as tr  # noqa: E402
import test_triptych_host as host  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")
CFG = os.path.join(ROOT, "config", "params.yml")
S, FACE = 256, 224
# touching the canvas edge exactly; an odd side; the rectangle one pixel outside; side 10 (below the blur's REFLECT_101 limit)
GEOMETRY = np.array([[100, 156, 156], [151, 30, 50], [100, 157, 0], [10, 5, 5]], np.int64)
SIDES = (11, 12, 63, 224, 225, 256)
CASES = dict(host.fill_cases())


def _frame(seed, size=S):
  """a smooth ramp with noise (the content of the JPEG tests)"""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:size, 0:size]
  img = np.stack([xx * 255 // (size - 1), yy * 255 // (size - 1), ((xx + yy) * 5) % 256], -1)
  return (img + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)


def _device_fill(masks):
  import torch
  from voicepuppet_amd.triptych import fill_holes
  out = fill_holes(torch.from_numpy(np.ascontiguousarray(masks)).cuda())
  torch.cuda.synchronize()
  return out.cpu().numpy()


# ---- stage a, through vp_triptych_fill_holes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fill_holes(name):
  m = CASES[name]
  want = tr.fill_holes(m)
  if name == "diagonal":
    from scipy import ndimage
    assert np.array_equal(want, ndimage.binary_fill_holes(m > 0).astype(np.uint8)) and want[20, 20] == 1
  assert np.array_equal(_device_fill(m[None])[0], want)
  assert np.array_equal(_device_fill(m[None] * 255)[0], want)


def test_fill_holes_batch_equals_single_calls():
  masks = np.stack([host.ring(), host.letter_c(), host.hole_at_border(), host.diagonal_leak(), host.random_mask(40, 52, 9)])
  got = _device_fill(masks)
  for i in range(5):
    assert np.array_equal(got[i], _device_fill(masks[i:i + 1])[0]) and np.array_equal(got[i], tr.fill_holes(masks[i])), i
  assert len({g.tobytes() for g in got}) == 5


# ---- stages b-d ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builder():
  from voicepuppet_amd.triptych import TriptychBuilder
  return TriptychBuilder(S, len(SIDES))


def test_mask_chain(builder):
  import torch
  disc = host.disc_with_holes()
  masks = torch.from_numpy(np.stack([disc * 255] * len(SIDES))).cuda()
  geometry = np.array([[s, 0, 0] for s in SIDES])
  got = builder.mask(masks, geometry, fill=False).cpu().numpy()
  for i, side in enumerate(SIDES):
    want = tr.mask_chain(disc, side)
    assert want.shape == (side, side) and 0 < want.max() and (side < 63 or want.min() == 0)
    assert np.array_equal(got[i, :side, :side], want), side
  filled = tr.fill_holes(disc)
  assert filled.sum() > disc.sum()
  got = builder.mask(masks[:2], geometry[2:4], fill=True).cpu().numpy()          # with stage a in front: sides 63 and 224
  assert np.array_equal(builder.tensor("filled")[:2].cpu().numpy(), np.stack([filled, filled]))
  for i, side in enumerate(SIDES[2:4]):
    assert np.array_equal(got[i, :side, :side], tr.mask_chain(filled, side)), side


# ---- the full build --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
  """four frames, the synthetic model's renders and masks of four golden coefficient rows, and the reference triptychs, computed once"""
  import torch
  from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer
  g = dict(np.load(GOLDEN))
  renderer = ClipRenderer(br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True))
  render, face_mask = renderer.render_view(g["coeff"][:4].astype(np.float32), view=0)
  frames = np.stack([_frame(40 + i) for i in range(4)])
  r, m = render.cpu().numpy(), face_mask.cpu().numpy()
  assert all(1000 < (m[i] > 0).sum() < FACE * FACE for i in range(4))
  want = [tr.triptych(frames[i], r[i], m[i], GEOMETRY[i]) for i in range(4)]
  return {"torch": torch, "frames": torch.from_numpy(frames).cuda(), "render": render, "mask": face_mask, "np": (frames, r, m), "want": want}


def test_build_panels_statuses_and_untouched_rows(scene):
  from voicepuppet_amd.triptych import TriptychBuilder
  torch = scene["torch"]
  b = TriptychBuilder(S, 4)
  out = torch.full((4, S, 3 * S, 3), 0xA5, dtype=torch.uint8, device="cuda")
  trip, status = b.build(scene["frames"], scene["render"], scene["mask"], GEOMETRY, out=out)
  trip, status = trip.cpu().numpy(), status.cpu().numpy()
  assert status.tolist() == [0, 0, 3, 1] and [w[1] for w in scene["want"]] == [0, 0, 3, 1]
  for i in (0, 1):
    want = scene["want"][i][0]
    assert np.array_equal(trip[i, :, :S], scene["np"][0][i])
    assert np.array_equal(trip[i, :, 2 * S:], want[:, 2 * S:]), "mask panel of frame %d" % i
    assert np.array_equal(trip[i], want), "frame %d" % i
    assert want[:, 2 * S:].max() > 200 and (want[:, S:2 * S] != want[:, :S]).any()
  assert np.all(trip[2:] == 0xA5)
  # a frame's bytes are the same at T = 1 and inside the batch
  for i in (0, 1):
    one, st = b.build(scene["frames"][i:i + 1], scene["render"][i:i + 1], scene["mask"][i:i + 1], GEOMETRY[i:i + 1])
    assert st.cpu().tolist() == [0] and np.array_equal(one.cpu().numpy()[0], trip[i])
  # a fresh output is zeros where nothing is built, and max_side below a frame's side is its own status
  small = TriptychBuilder(S, 4, max_side=120)
  trip2, st2 = small.build(scene["frames"], scene["render"], scene["mask"], GEOMETRY)
  assert st2.cpu().tolist() == [0, 2, 3, 1] and np.array_equal(trip2[0].cpu().numpy(), trip[0]) and not trip2[1:].any()


def test_matte_mode_equals_resize_paste_of_the_frame_alone(scene):
  from voicepuppet_amd.triptych import TriptychBuilder
  from voicepuppet_amd.utils.cv_resize import resize_paste_u8
  torch = scene["torch"]
  alpha = torch.from_numpy(np.stack([_frame(60 + i)[..., 0] for i in range(4)])).cuda()
  b = TriptychBuilder(S, 4)
  # the four geometries of the build, then the copy (side = face), the exact halving, a down-scale and an up-scale-free large side
  for geometry, statuses in ((GEOMETRY, [0, 0, 3, 1]), (np.array([[224, 10, 20], [112, 0, 0], [63, 100, 100], [256, 0, 0]]), [0, 0, 0, 0])):
    out = torch.full((4, S, 3 * S, 3), 0xA5, dtype=torch.uint8, device="cuda")
    trip, status = b.build(scene["frames"], scene["render"], None, geometry, alpha=alpha, out=out)
    assert status.cpu().tolist() == statuses
    for i in range(4):
      if statuses[i]:
        assert bool((trip[i] == 0xA5).all())
        continue
      side, y0, x0 = (int(v) for v in geometry[i])
      pasted = resize_paste_u8(scene["render"][i:i + 1], side, side, (S, S), y0, x0, swap_rb=True)[0]
      assert torch.equal(trip[i, :, S:2 * S], pasted), i
      assert torch.equal(trip[i, :, :S], scene["frames"][i]) and torch.equal(trip[i, :, 2 * S:], alpha[i][..., None].expand(-1, -1, 3))
      want, _ = tr.triptych(scene["np"][0][i], scene["np"][1][i], None, geometry[i], alpha=alpha[i].cpu().numpy())
      assert np.array_equal(trip[i].cpu().numpy(), want), i


def test_arguments_are_refused_before_anything_is_enqueued(scene):
  import ctypes
  from voicepuppet_amd._handle import ptr
  from voicepuppet_amd.triptych import TriptychBuilder
  torch = scene["torch"]
  b = TriptychBuilder(S, 2)
  with pytest.raises(ValueError, match="1 .. 2"):
    b.build(scene["frames"], scene["render"], scene["mask"], GEOMETRY)
  with pytest.raises(ValueError, match="geometry"):
    b.build(scene["frames"][:2], scene["render"][:2], scene["mask"][:2], GEOMETRY[:2].astype(np.float64))
  with pytest.raises(ValueError, match="render"):
    b.build(scene["frames"][:2], scene["render"][:2, :100], scene["mask"][:2], GEOMETRY[:2])
  f, r, m = scene["frames"], scene["render"], scene["mask"]
  g = torch.zeros(9, dtype=torch.int32, device="cuda")
  out, st = torch.zeros(2, S, 3 * S, 3, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
  L = b.L
  assert L.vp_triptych_build(b.h, ptr(f), ptr(r), ptr(m), ptr(g), None, 3, ptr(out), ptr(st), None) == -1 and b"max_frames" in L.vp_last_error()
  assert L.vp_triptych_build(b.h, ptr(f), ptr(r), None, ptr(g), None, 1, ptr(out), ptr(st), None) == -1 and b"face_mask" in L.vp_last_error()
  assert L.vp_triptych_build(b.h, ptr(f), ptr(r), ptr(m), ctypes.c_void_p(g.data_ptr() + 2), None, 1, ptr(out), ptr(st), None) == -1
  assert b"4-byte" in L.vp_last_error()
  assert L.vp_triptych_mask(b.h, ptr(m), ptr(g), 0, 1, None) == -1 and b"max_frames" in L.vp_last_error()
  q, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
  assert L.vp_triptych_tensor(b.h, b"nothing", ctypes.byref(q), shp) == -1 and b"mask, filled" in L.vp_last_error()
  with pytest.raises(ValueError, match="descriptor.*max_side"):
    TriptychBuilder(S, 2, max_side=S + 1)


def test_write_repeats_the_frame_before_and_refuses_a_first_frame(scene, tmp_path):
  from PIL import Image
  from voicepuppet_amd.triptych import TriptychBuilder
  b = TriptychBuilder(S, 4)
  trip, status = b.build(scene["frames"], scene["render"], scene["mask"], GEOMETRY)
  assert b.write(trip, status, str(tmp_path), 0) == [2, 3]
  files = [(tmp_path / ("%d.jpg" % i)).read_bytes() for i in range(4)]
  assert files[2] == files[1] and files[3] == files[1] and files[0] != files[1]
  assert Image.open(io.BytesIO(files[0])).size == (3 * S, S)
  assert b.write(trip[2:], status[2:], str(tmp_path), 4) == [4, 5] and (tmp_path / "5.jpg").read_bytes() == files[1]
  empty = tmp_path / "empty"
  empty.mkdir()
  with pytest.raises(ValueError, match="frame 0 cannot be built.*not wholly inside"):
    b.write(trip[2:], status[2:], str(empty), 0)
  assert not os.listdir(str(empty))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _psnr(a, b):
  d = a.astype(np.float64) - b.astype(np.float64)
  return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


def _decode(data):
  from PIL import Image
  return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_jpeg_fidelity_at_quality_95(scene):
  """PSNR of the device-encoded file against the raw triptych >= that of the host encoder at the same quality - 0.18 dB: twice the 0.09 dB
  recorded at quality 75 (profiles/jpeg_encode.json), because quality 95 had not been measured when the bound was set.  Measured here:
  -0.003 and -0.001 dB on these two triptychs, -0.011 dB at worst on eight others (profiles/triptych.json)."""
  from voicepuppet_amd.jpeg import host_jpeg
  from voicepuppet_amd.triptych import TriptychBuilder
  b = TriptychBuilder(S, 4)
  trip, status = b.build(scene["frames"], scene["render"], scene["mask"], GEOMETRY)
  files = b.encode(trip[:2], 95)
  raw = trip[:2].cpu().numpy()
  for i in range(2):
    dev, hst = _psnr(_decode(files[i]), raw[i]), _psnr(_decode(host_jpeg(raw[i], 95)), raw[i])
    print("triptych %d at quality 95: device %.3f dB, host %.3f dB, difference %+.3f dB" % (i, dev, hst, dev - hst))
    assert dev >= hst - 0.18


def test_launcher_end_to_end_and_the_input_pipeline(tmp_path, monkeypatch, capsys):
  import random
  import torch
  from PIL import Image
  import bfm_fit_ref as fr
  from test_gpu_bfm_fit import write_bfm_assets
  from voicepuppet_amd.datasets import make_triptychs as mt
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  from voicepuppet_amd.generator.loader import BFMCoeffLoader
  from voicepuppet_amd.jpeg import host_jpeg
  monkeypatch.chdir(tmp_path)
  g = dict(np.load(GOLDEN))
  write_bfm_assets(br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True), g["lm3d68"])
  # landmarks taken from the synthetic model's own projection, placed in a 256 x 256 frame
  xy = np.stack([fr.photo_landmarks(g["landmarks_2d"][f], 0.7, (50.0, 45.0)) for f in range(6)])
  os.makedirs("clip")
  for i in range(6):
    Image.fromarray(_frame(80 + i)).save(os.path.join("clip", "%d.jpg" % i), "JPEG", quality=95)
  np.savetxt(os.path.join("clip", "_landmark.txt"), xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  out_dir = str(tmp_path / "data" / "clip0")
  res = mt.main(["--clip_dir", "clip", "--landmarks", os.path.join("clip", "_landmark.txt"), "--out_dir", out_dir, "--list", "train.txt",
                 "--rounds", "1", "--id_steps", "1", "--frame_batch", "4"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  assert "6 frames" in line and "reprojection mean" in line and "triptych status 0:6, 0 repeated" in line
  assert res["status"].tolist() == [0] * 6 and res["geometry"].shape == (6, 3)
  for i in range(6):
    with Image.open(os.path.join(out_dir, "%d.jpg" % i)) as im:
      assert im.size == (768, 256) and im.mode == "RGB"
      img = np.asarray(im)
    # panel 1 is frame i and no other: the six frames differ by their noise alone (the bytes of a panel are compared in the tests above)
    seen = [np.asarray(Image.open(os.path.join("clip", "%d.jpg" % k)).convert("RGB")) for k in range(6)]
    fidelity = [_psnr(img[:, :S], f) for f in seen]
    print("frame %d: panel 1 against the decoded inputs %s dB; host re-encode of input %d: %.2f dB" % (
        i, " ".join("%.2f" % v for v in fidelity), i, _psnr(_decode(host_jpeg(seen[i], 95)), seen[i])))
    assert int(np.argmax(fidelity)) == i
    side, y0, x0 = res["geometry"][i]
    panel3 = img[:, 2 * S:]
    assert panel3[y0:y0 + side, x0:x0 + side].max() > 200 and panel3[0, 0].max() < 30                       # the mask: face inside, black corner
  assert not os.path.exists(os.path.join(out_dir, "6.jpg"))
  ears = [float(v) for v in open(os.path.join(out_dir, "ear.txt")).read().split()]
  assert len(ears) == 6 and all(abs(e - mt.ear_value(xy[i].reshape(-1).tolist())) < 1e-9 for i, e in enumerate(ears))
  rows = BFMCoeffLoader().get_data(os.path.join(out_dir, "bfmcoeff.txt"))
  assert rows.shape == (6, 257) and np.all(np.isfinite(rows)) and np.all(rows[:, 144:224] == rows[0, 144:224])
  assert open("train.txt").read() == "%s|6\n" % out_dir
  # the existing PixRefer input pipeline yields a batch from that list, decoding the written files on the device
  gen = PixReferDataGenerator(CFG)
  p = gen.params
  p.dataset_path, p.batch_size, p.img_size, p.shuffle_bufsize = "train.txt", 2, S, 1
  amd = dict(p.get('amd') or {})
  amd['device_jpeg_decode'] = True
  p.amd = amd
  gen.set_params(p)
  random.seed(5)
  batch = gen.get_device_dataset().make_one_shot_iterator().next_batch()
  torch.cuda.synchronize()
  assert [tuple(t.shape) for t in batch] == [(2, S, S, 6), (2, S, S, 6), (2, S, S, 3), (2, S, S, 3)]
  assert all(bool(torch.isfinite(t).all()) for t in batch) and float(batch[3].max()) > 0.7

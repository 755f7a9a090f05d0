"""The matte clean-up and the foreground estimate on the device (voicepuppet_amd.matte_clean.MatteCleaner, KeyMatte.foreground;
csrc/matte_clean.hip, csrc/key_matte.hip) against the numpy restatement tests/matte_clean_ref.py, which tests/test_matte_clean_host.py
pins: labels and report exactly, the cleaned matte and the foreground byte for byte over every pixel.  Then the labelling's worst cases,
the parameter grid, batch independence, views, refusals, and the dataset launcher end to end on six frames of the scene."""
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
import matte_clean_ref as mr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")
# (n, H, W): one tile and less; 3 x 3 tiles, ragged; odd sizes (an odd width: the last pixel pair of a row is half outside); 8 x 8 tiles;
# one tile row / column
SIZES = [(1, 16, 16), (3, 96, 80), (5, 33, 47), (2, 256, 256), (1, 17, 64), (1, 64, 17)]


@functools.lru_cache(maxsize=None)
def _scene(n, H, W):
  """frames, model, KeyMatte's matte (the restatement's), anchors: read-only"""
  frames, _, _ = mr.scene(H, W, seed=H * 1000 + W, n=n, spill_levels=10.0)
  _, model = kr.fit(frames)
  _, matte = kr.matte(model, frames)
  res = (frames, model, matte, mr.landmarks(H, W, n))
  for a in res:
    a.setflags(write=False)
  return res


@functools.lru_cache(maxsize=None)
def _want(n, H, W):
  res = mr.clean(_scene(n, H, W)[2], _scene(n, H, W)[3])
  for a in res:
    a.setflags(write=False)
  return res


@functools.lru_cache(maxsize=None)
def _cleaner():
  from voicepuppet_amd.matte_clean import MatteCleaner
  return MatteCleaner(14, 256, 256)


@functools.lru_cache(maxsize=None)
def _keyer():
  from voicepuppet_amd.matte import KeyMatte
  return KeyMatte(5, 256, 256, max_radius=0)


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the cached references are read-only)


def _run(matte, anchors=None, cleaner=None, **kw):
  """-> (cleaned, labels, report) of the device, as host arrays"""
  c = cleaner or _cleaner()
  n, H, W = matte.shape
  out = c.clean(_dev(matte), anchors=None if anchors is None else _dev(np.asarray(anchors, np.int32)), **kw)
  rep = c.report()
  lab = c.tensor("labels")
  assert tuple(lab.shape) == (c.max_frames, H, W) and rep.shape == (n, 8)
  return out.cpu().numpy(), lab[:n].cpu().numpy(), rep


def _same(got, want, what=""):
  for name, g, w in zip(("cleaned matte", "labels", "report"), got, want):
    assert g.dtype == w.dtype and np.array_equal(g, w), "%s %s: %d values differ" % (what, name, int((g != w).sum()))
  assert not (got[2][:, 6] & 2).any() and not got[2][:, 7].any(), what


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_labels_report_and_cleaned_matte_equal_the_restatement(size):
  frames, model, matte, anchors = _scene(*size)
  _same(_run(matte, anchors), _want(*size), str(size))
  want = _want(*size)
  if size[1] >= 96:
    assert (want[2][:, 0] > want[2][:, 1]).all() and (want[2][:, 4] >= 1).all()      # the scene does its work: components go, the logo is filled


@pytest.mark.parametrize("size", SIZES)
def test_foreground_equals_the_restatement(size):
  frames, model, matte, _ = _scene(*size)
  cleaned = _want(*size)[0]
  k = _keyer().set_model(_dev(model))
  assert mr.spill(model, size[1], size[2])[1] >= 16.0 and k.spill(size[1], size[2])["active"]
  for m in (matte, cleaned):
    for despill in (0.0, 0.5, 1.0):
      got = k.foreground(_dev(frames), _dev(m), despill=despill).cpu().numpy()
      want = mr.foreground(model, frames, m, despill)
      assert np.array_equal(got, want), "%s despill %g: %d bytes differ" % (size, despill, int((got != want).sum()))
  assert not np.array_equal(mr.foreground(model, frames, matte, 1.0), mr.foreground(model, frames, matte, 0.0))


# ---- worst cases of the labelling ----------------------------------------------------------------------------------------------------------
def test_worst_case_patterns():
  """Paths that cross every tile border of 3 x 3 tiles (serpentine, spiral), a component per pixel (checkerboard, whose inverse is 3840
  four-connected holes), teeth, a diagonal, nothing and everything, and the inverse of each: the device's labels are the
  restatement's, and no step cap is reached."""
  H, W = 96, 80
  pats = mr.patterns(H, W)
  matte = np.stack([p for p in pats.values()] + [255 - p for p in pats.values()])
  assert matte.shape[0] == 14
  for kw in (dict(keep="all", min_area=0, max_hole=H * W, grow=0), dict(keep="anchored", min_area=2, max_hole=1, grow=1)):
    _same(_run(matte, **kw), mr.clean(matte, **kw), str(kw))
  # the same through a core between the two values: the component pass keeps everything, the hole pass sees the pattern's inverse
  soft = (matte // 255 * 155 + 100).astype(np.uint8)
  kw = dict(keep="all", min_area=0, max_hole=H * W, grow=0, support=100, core=200)
  want = mr.clean(soft, **kw)
  assert (want[2][:, 0] == 1).all() and want[2][:, 4].max() > 1000
  _same(_run(soft, **kw), want, "soft")


def test_random_blobs_at_1024():
  """the index width: labels up to 2^20 - 1, one frame of 32 x 32 tiles"""
  from voicepuppet_amd.matte_clean import MatteCleaner
  matte = mr.blobs(1024, 1024, seed=7)[None]
  anchors = np.array([[[512, 512], [1023, 1023], [0, 0], [1024, 5]]], np.int32)
  c = MatteCleaner(1, 1024, 1024)
  want = mr.clean(matte, anchors)
  assert want[1].max() > 2 ** 19 and want[2][0, 0] > 100
  _same(_run(matte, anchors, cleaner=c), want, "1024")
  c.close()


# ---- parameters ----------------------------------------------------------------------------------------------------------------------------
GRID = [dict(support=100, core=100), dict(support=1), dict(core=255), dict(grow=0), dict(grow=16), dict(max_hole=0), dict(min_area=0),
        dict(keep="all"), dict(keep="all", min_area=0, max_hole=0, grow=0), dict(keep="anchored", min_area=40, max_hole=5),
        dict(support=255, core=1), dict(min_area=96 * 80, max_hole=96 * 80)]


@functools.lru_cache(maxsize=None)
def _grid_input():
  """three frames of 96 x 80: the scene's matte, random blobs, blobs with the scene's anchors far from anything"""
  matte = np.stack([_scene(3, 96, 80)[2][0], mr.blobs(96, 80, seed=5), mr.blobs(96, 80, seed=6, smooth=1)])
  anchors = np.array(_scene(3, 96, 80)[3])
  matte.setflags(write=False)
  return matte, anchors


@pytest.mark.parametrize("kw", GRID, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_parameter_grid(kw):
  matte, anchors = _grid_input()
  _same(_run(matte, anchors, **kw), mr.clean(matte, anchors, **kw), str(kw))


def test_anchors_off_frame_none_and_the_fallback():
  matte, anchors = _grid_input()
  off = np.array(anchors)
  off[..., 0] += 1000
  off[..., 1] = -off[..., 1] - 1
  islands = np.array(matte)
  islands[:, -8:] = 0                                              # nothing reaches the bottom row
  for a in (off, None, np.zeros((3, 0, 2), np.int32), anchors):
    want = mr.clean(islands, a)
    _same(_run(islands, a), want, "anchors")
  kept_all = mr.clean(islands, None, max_hole=0)
  assert (kept_all[2][:, 6] == 1).all() and np.array_equal(kept_all[0][islands >= 32], islands[islands >= 32])    # every component stays
  assert (mr.clean(islands, anchors)[2][0, 6] == 0)


def test_a_frame_alone_equals_the_frame_in_a_batch():
  size = (5, 33, 47)
  _, _, matte, anchors = _scene(*size)
  full = _run(matte, anchors)
  alone = _run(matte[3:4], anchors[3:4])
  for f, a in zip(full, alone):
    assert np.array_equal(f[3], a[0])
  other = np.array(matte[[4, 3, 2, 1, 0]])
  again = _run(other, np.array(anchors[[4, 3, 2, 1, 0]]))
  for f, a in zip(full, again):
    assert np.array_equal(f[3], a[1])


def test_out_is_honoured_and_guards_stay_intact():
  import torch
  _, _, matte, anchors = _scene(3, 96, 80)
  c = _cleaner()
  buf = torch.full((5, 96, 80), 77, dtype=torch.uint8, device="cuda")
  got = c.clean(_dev(matte), anchors=_dev(anchors), out=buf[1:])
  assert got.data_ptr() == buf[1].data_ptr() and np.array_equal(got.cpu().numpy(), _want(3, 96, 80)[0])
  assert (buf[0] == 77).all() and (buf[4] == 77).all()
  src = _dev(matte)
  same = c.clean(src, anchors=_dev(anchors), out=src)              # in place
  assert same.data_ptr() == src.data_ptr() and np.array_equal(src.cpu().numpy(), _want(3, 96, 80)[0])


# ---- foreground: views and backdrops ------------------------------------------------------------------------------------------------------
def test_foreground_on_a_padded_view_and_on_green_and_neutral_backdrops():
  import torch
  n, H, W = 3, 96, 80
  frames, model, matte, _ = _scene(n, H, W)
  k = _keyer()
  padded = torch.full((n, H + 8, W + 16, 3), 201, dtype=torch.uint8, device="cuda")   # a JpegDecoder output: whole MCUs, a view of the image
  padded[:, :H, :W] = _dev(frames)
  view = padded[:, :H, :W]
  assert not view.is_contiguous()
  neutral = np.array(model)
  neutral[[0, 3, 6]] = (120.0, 130.0, 125.0)
  neutral[[1, 2, 4, 5, 7, 8]] = 0.0
  for md, active in ((model, True), (neutral, False)):
    k.set_model(_dev(md))
    assert k.spill(H, W)["active"] == active == (mr.spill(md, H, W)[1] >= 16.0)
    for despill in (0.0, 0.5, 1.0):
      want = mr.foreground(md, frames, matte, despill)
      assert np.array_equal(k.foreground(view, _dev(matte), despill=despill).cpu().numpy(), want), (active, despill)
      if not active:
        assert np.array_equal(want, mr.foreground(md, frames, matte, 0.0))
  out = torch.full((n + 1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
  got = k.foreground(view, _dev(matte), out=out)
  assert got.data_ptr() == out.data_ptr() and (out[n] == 9).all() and np.array_equal(got.cpu().numpy(), mr.foreground(neutral, frames, matte))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched():
  import torch
  c, k = _cleaner(), _keyer()
  matte = torch.zeros(2, 64, 48, dtype=torch.uint8, device="cuda")
  out = torch.full((2, 64, 48), 55, dtype=torch.uint8, device="cuda")
  anchors = torch.zeros(2, 4, 2, dtype=torch.int32, device="cuda")
  bad = [dict(support=0), dict(support=256), dict(core=0), dict(core=256), dict(min_area=-2), dict(min_area=64 * 48 + 1), dict(max_hole=-3),
         dict(max_hole=64 * 48 + 1), dict(grow=-1), dict(grow=17), dict(anchors=torch.zeros(2, 257, 2, dtype=torch.int32, device="cuda"))]
  for kw in bad:
    with pytest.raises(RuntimeError, match="vp_matteclean_clean"):
      c.clean(matte, out=out, **kw)
  for m, kw in [(matte, dict(keep="some")), (matte.cpu(), {}), (matte.float(), {}), (matte[:, :, ::2], {}), (matte[0], {}),
                (matte, dict(anchors=anchors[:1])), (matte, dict(anchors=anchors.long())), (matte, dict(anchors=anchors[:, :, :1])),
                (matte, dict(anchors=anchors.cpu())), (matte, dict(out=out[:1])), (matte, dict(out=out[:, :, :40])), (matte, dict(out=out.cpu()))]:
    with pytest.raises(ValueError):
      c.clean(m, **dict(dict(out=out), **kw))
  for shape in ((15, 64, 48), (1, 15, 48), (1, 64, 15), (1, 257, 48), (1, 64, 257)):      # n, height and width against the descriptor
    big = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="vp_matteclean_clean"):
      c.clean(big, out=torch.empty_like(big))
  frames = torch.zeros(2, 64, 48, 3, dtype=torch.uint8, device="cuda")
  fout = torch.full((2, 64, 48, 3), 55, dtype=torch.uint8, device="cuda")
  for despill in (-0.5, 1.01, float("nan")):
    with pytest.raises(RuntimeError, match="despill"):
      k.foreground(frames, matte, despill=despill, out=fout)
  for f, m, o in [(frames, matte[:1], fout), (frames, matte[:, :, ::2], fout), (frames, matte.float(), fout), (frames, matte, fout[:1]),
                  (frames, matte, fout[..., :2]), (frames[..., :2], matte, fout), (frames, matte.cpu(), fout)]:
    with pytest.raises(ValueError):
      k.foreground(f, m, out=o)
  with pytest.raises(RuntimeError, match="max_frames"):
    k.foreground(torch.zeros(6, 64, 48, 3, dtype=torch.uint8, device="cuda"), torch.zeros(6, 64, 48, dtype=torch.uint8, device="cuda"))
  torch.cuda.synchronize()
  assert (out == 55).all() and (fout == 55).all()


# ---- the dataset tool ----------------------------------------------------------------------------------------------------------------------
def _rgb(path):
  from PIL import Image
  return np.asarray(Image.open(path).convert("RGB"))


def test_launcher_clean_matte_and_key_foreground_end_to_end(tmp_path, monkeypatch, capsys):
  """Six JPEG frames of the scene through make_triptychs.py --key_matte --clean_matte --key_foreground --write_alpha: the written PNGs
  are the restatement's cleaned mattes of the device's key matte (which tests/test_gpu_key_matte.py holds equal to its restatement),
  the summary line and the results carry the restatement's counts, and the frame panel holds the foreground estimate.  JPEG noise on
  that panel: about 1.4 levels rms as in test_gpu_key_matte.py (held to 2 there), plus the ringing of the cut at the matte's edge, which the
  blocks that hold it (under a tenth of the frame) carry at under 10 levels: the mean absolute difference is held to 3 levels."""
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
  frames, _, _ = mr.scene(S, S, seed=11, n=6)
  os.makedirs("clip")
  for i in range(6):
    Image.fromarray(frames[i]).save(os.path.join("clip", "%d.jpg" % i), "JPEG", quality=95)
  np.savetxt(os.path.join("clip", "_landmark.txt"), xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  common = ["--clip_dir", "clip", "--landmarks", os.path.join("clip", "_landmark.txt"), "--rounds", "1", "--id_steps", "1", "--frame_batch", "4"]

  res = mt.main(common + ["--out_dir", "cleaned", "--key_matte", "--clean_matte", "--key_foreground", "--write_alpha", "alpha"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  reader = mt.FrameReader("clip", 4, None, None)
  decoded = torch.cat([reader.read(0, 4), reader.read(4, 2)])
  km = KeyMatte(6, S, S).fit(decoded[:4])
  keyed = km.matte(decoded).cpu().numpy()
  anchors = np.floor(np.loadtxt(os.path.join("clip", "_landmark.txt"), delimiter=",").reshape(6, 68, 2)).astype(np.int32)
  want, _, rep = mr.clean(keyed, anchors)
  assert np.array_equal(res["clean"], rep) and (rep[:, 0] > rep[:, 1]).all() and (rep[:, 4] >= 1).all() and not rep[:, 6].any()
  assert "triptych status 0:6, 0 repeated" in line and "key matte: kept " in line and ("; clean: " + mr.summary(rep)) in line
  fore = mr.foreground(km.model().cpu().numpy(), decoded.cpu().numpy(), want)
  for i in range(6):
    assert np.array_equal(np.asarray(Image.open(os.path.join("alpha", "%d.png" % i))), want[i]), i
    img = _rgb(os.path.join("cleaned", "%d.jpg" % i))
    p1, p3 = img[:, :S].astype(np.float64), img[:, 2 * S:].astype(np.float64)
    d1, d3 = np.abs(p1 - fore[i]).mean(), np.abs(p3 - want[i][..., None]).mean()
    print("frame %d: mean |difference| of panel 1 against the foreground %.3f, of panel 3 against the cleaned matte %.3f levels" % (i, d1, d3))
    assert d1 <= 3.0 and d3 <= 2.0
  assert not np.array_equal(want, keyed)

  # the written mattes as --alpha_dir, cleaned again: cleaning a cleaned matte removes nothing more
  res2 = mt.main(common + ["--out_dir", "again", "--alpha_dir", "alpha", "--clean_matte", "--clean_max_hole", "0", "--key_foreground"])
  line2 = capsys.readouterr().out.strip().splitlines()[-1]
  assert "clean: removed 0 components / 0 px, filled 0 holes / 0 px" in line2 and "key matte: kept" not in line2
  assert (res2["clean"][:, 0] == 1).all() and not res2["clean"][:, 2].any()
  for i in range(6):
    p1 = _rgb(os.path.join("again", "%d.jpg" % i))[:, :S].astype(np.float64)
    assert np.abs(p1 - fore[i]).mean() <= 3.0

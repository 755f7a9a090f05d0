"""-m gpu: BFMNet's visual evaluation on the device against the reference-captured golden (tests/golden/bfm_visual.npz) and its numpy
restatement (tests/bfm_visual_ref.py): vp_bfm_reconstruct_view, vp_sheet_tile_u8, vp_landmark_distance, MeshSheet / plot_bfm_coeff_seq,
and the two launchers that use them.

Tolerances: float64 outputs within 1e-12 relative (tests/test_bfm_recon.py's bound: the 144-term sums are ordered differently from
numpy's); float32 vertices, integer colours, tiles and sheets IDENTICAL; the landmark distance within 1e-12 relative (68 terms, one
square root each); a .jpg at most 0.2 dB below PIL's own file of the same array at the same quality and subsampling."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avi_ref  # noqa: E402
import bfm_visual_ref as vr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402
from test_bfm_visual_host import golden, rel  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "params.yml")
F64 = ["face_shape", "face_texture", "face_color", "face_projection", "z_buffer", "landmarks_2d"]
# a landmark distance from the device's own projections against one from the restatement's: each coordinate is within 1e-12 * 224 px of
# the other's (the bound above), a distance moves by at most 2 * sqrt(2) times that, 6.4e-10 px
LMD_ATOL = 1e-9
_CACHE = {}


def model():
  """The golden's face model on the device, once."""
  from voicepuppet_amd.utils import reconstruct_mesh as vrm
  if "model" not in _CACHE:
    _CACHE["model"] = vrm.DeviceFaceModel(golden()[1])
  return _CACHE["model"]


def long_sequences():
  """real [2,40,257] / pred [2,40,64] (the second sequence must never show) and, per seq_len, the restatement's montage - drawn once."""
  if "seq" not in _CACHE:
    _CACHE["seq"] = vr.synthetic_sequences(40, 77, batch=2)
  return _CACHE["seq"]


def want_montage(seq_len, branch=False):
  key = ("montage", seq_len, branch)
  if key not in _CACHE:
    g, fm, _ = golden()
    if seq_len == 12 and not branch:
      _CACHE[key] = vr.montage(fm, g["seq_len"], g["real"], g["pred"], tiles=(g["real_tiles"], g["pred_tiles"]))
    else:
      real, pred = long_sequences()
      if branch:                                       # (the reference's tile of id_coeff [1,1,80] only fits a batch of one)
        real, pred, (idc, texc) = real[:1], pred[:1], branch_coeffs()
        _CACHE[key] = vr.montage(fm, [seq_len, 3], real, pred, idc, texc)
      else:
        if "tiles30" not in _CACHE:                    # the 30 + 30 tiles of the long clip serve every shorter seq_len
          _CACHE["tiles30"] = (vr.tiles_of(real[0, :30], fm), vr.tiles_of(vr.splice(real, pred)[0, :30], fm))
        _CACHE[key] = vr.montage(fm, [seq_len, 3], real, pred, tiles=_CACHE["tiles30"])
  return _CACHE[key]


def branch_coeffs():
  rng = np.random.default_rng(4)
  return rng.normal(size=(1, 1, 80)).astype(np.float32), rng.normal(size=(1, 1, 80)).astype(np.float32)


def psnr(a, b):
  mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
  return 10 * np.log10(255.0 ** 2 / mse)


def pil_file(arr, quality):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=2)
  return buf.getvalue()


def decode(data):
  from PIL import Image
  return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("view,scale", [(0, 1.0), (1, 1.0), (1, 3.0)])
def test_reconstruct_view_matches_the_reference_golden(view, scale):
  from voicepuppet_amd.utils import reconstruct_mesh as vrm
  g, fm, spliced = golden()
  for tag, coeff in (("real", g["real"][0]), ("pred", spliced[0])):
    out = vrm.reconstruct_view(coeff, model(), view=view, scale=scale)
    for n in F64:
      assert rel(out[n].cpu().numpy(), g["%s_%s" % (tag, n)]) < 1e-12, (tag, n)
    assert np.array_equal(out["translation"].cpu().numpy(), g[tag + "_translation"])
    if view == 0 or scale == 3.0:
      want_v = g["%s_vertices_view%d" % (tag, view)]
    else:
      want_v = vr.pack_view({n: g["%s_%s" % (tag, n)] for n in vr.NAMES}, 1, 1)[0]
    assert np.array_equal(out["vertices"].cpu().numpy(), want_v), tag
    assert np.array_equal(out["colors"].cpu().numpy(), g[tag + "_colors"]), tag


@pytest.mark.parametrize("shared", [False, True])
def test_reconstruct_view_33_frames_against_the_restatement(shared):
  """More than one 32-frame pass of the basis kernel; identity and texture constant over the clip (so that one shared texture is the
  per-frame one), expression and pose per frame."""
  from voicepuppet_amd.utils import reconstruct_mesh as vrm
  fm = golden()[1]
  coeff, _ = br.synthetic_coeffs(33, 8)
  coeff[:, 224:227] += np.random.default_rng(1).normal(0, 0.2, size=(33, 3)).astype(np.float32)
  want = vr.reconstruction(coeff, fm)
  for view, scale in ((0, 1.0), (1, 3.0)):
    out = vrm.reconstruct_view(coeff, model(), view=view, scale=scale, shared_texture=shared)
    for n in F64:
      w = want[n][:1] if shared and n == "face_texture" else want[n]
      assert out[n].shape == w.shape and rel(out[n].cpu().numpy(), w) < 1e-12, (view, n)
    v, c = vr.pack_view(want, view, 3)
    assert np.array_equal(out["vertices"].cpu().numpy(), v) and np.array_equal(out["colors"].cpu().numpy(), c), view
  lean = vrm.reconstruct_view(coeff, model(), view=1, scale=3.0, shared_texture=shared, full=False)
  assert sorted(lean) == ["colors", "vertices"] and np.array_equal(lean["vertices"].cpu().numpy(), v)


def test_reconstruction_has_the_reference_signature():
  from voicepuppet_amd.utils import reconstruct_mesh as vrm
  g, fm, _ = golden()
  res = vrm.Reconstruction(g["real"][0, 1:2], fm)                      # one frame, the reference's BFM object, numpy in / numpy out
  assert len(res) == 7
  for n, r in zip(vr.NAMES, res):
    want = g["real_" + n][1:2]
    assert isinstance(r, np.ndarray) and r.dtype == want.dtype and r.shape == want.shape and rel(r, want) < 1e-12, n


def test_external_pose_entry_is_unchanged_after_a_view_call_on_the_same_model():
  """vp_bfm_reconstruct on the golden of tests/test_bfm_recon.py, before and after a view-1 call that shares the model's workspace."""
  from voicepuppet_amd.utils import reconstruct_mesh as vrm
  g = np.load(os.path.join(ROOT, "tests", "golden", "bfm_recon.npz"))
  m = vrm.DeviceFaceModel(br.synthetic_facemodel(int(g["model_seed"])))
  before = {k: v.cpu().numpy() for k, v in vrm.reconstruct_clip(g["coeff"], m, g["angles"]).items()}
  vrm.reconstruct_view(br.synthetic_coeffs(9, 2)[0], m, view=1, scale=3.0, shared_texture=True)
  after = {k: v.cpu().numpy() for k, v in vrm.reconstruct_clip(g["coeff"], m, g["angles"]).items()}
  for k in before:
    assert np.array_equal(before[k], after[k]), k
  assert np.array_equal(after["vertices"], g["vertices"]) and np.array_equal(after["colors"], g["colors"])
  for n in F64:
    assert rel(after[n], g[n]) < 1e-12, n


def place_numpy(sheet, tiles, cols, first_cell, swap):
  n, h, w = tiles.shape[:3]
  for i in range(n):
    r, c = divmod(first_cell + i, cols)
    sheet[r * h:(r + 1) * h, c * w:(c + 1) * w] = tiles[i][..., ::-1] if swap else tiles[i]
  return sheet


SHEET_CASES = [
    (1, 224, 224, 9, 10, 0), (1, 224, 224, 9, 10, 30), (13, 224, 224, 9, 10, 0), (13, 224, 224, 9, 10, 30),      # 13 tiles wrap a row of 10
    (4, 672, 672, 2, 3, 0), (4, 672, 672, 5, 7, 30),                                                            # wrap after 3; cells 30..33 of 35
    (5, 30, 30, 4, 3, 0), (5, 30, 30, 12, 3, 30), (3, 7, 5, 2, 2, 1),                                            # odd row widths: the byte path
]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("n,h,w,rows,cols,first", SHEET_CASES)
def test_sheet_tile_byte_for_byte(n, h, w, rows, cols, first, swap):
  import torch
  from voicepuppet_amd.bfmnet import visual
  rng = np.random.default_rng(n * 1000 + h + first)
  tiles = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
  sheet = torch.full((rows * h, cols * w, 3), 0xAB, dtype=torch.uint8, device="cuda")
  visual.sheet_tile(torch.from_numpy(tiles).cuda(), sheet, first, swap)
  want = place_numpy(np.full((rows * h, cols * w, 3), 0xAB, np.uint8), tiles, cols, first, swap)
  assert np.array_equal(sheet.cpu().numpy(), want)                     # the written cells, and 0xAB everywhere else


@pytest.mark.parametrize("swap", [False, True])
def test_sheet_tile_unaligned_bases_take_the_byte_path(swap):
  """w a multiple of 4 but tiles / sheet one byte off a dword boundary: same bytes, and the guard bytes around both stay."""
  import torch
  from voicepuppet_amd.bfmnet import visual
  rng = np.random.default_rng(5)
  tiles = rng.integers(0, 256, (3, 6, 8, 3)).astype(np.uint8)
  src = torch.zeros(3 * 6 * 8 * 3 + 8, dtype=torch.uint8, device="cuda")
  src[1:-7] = torch.from_numpy(tiles.reshape(-1)).cuda()
  arena = torch.full((2 * 6 * 2 * 8 * 3 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
  for shift_src, shift_dst in ((1, 0), (0, 3), (1, 3)):
    arena.fill_(0xAB)
    t = (src[1:-7] if shift_src else torch.from_numpy(tiles).cuda().reshape(-1)).view(3, 6, 8, 3)
    sheet = arena[shift_dst:shift_dst + 2 * 6 * 2 * 8 * 3].view(12, 16, 3)
    visual.sheet_tile(t, sheet, 1, swap)
    want = place_numpy(np.full((12, 16, 3), 0xAB, np.uint8), tiles, 2, 1, swap)
    host = arena.cpu().numpy()
    assert np.array_equal(host[shift_dst:shift_dst + want.size].reshape(12, 16, 3), want)
    assert np.all(host[:shift_dst] == 0xAB) and np.all(host[shift_dst + want.size:] == 0xAB)


def test_sheet_tile_refuses_a_cell_outside_the_sheet():
  import torch
  from voicepuppet_amd.bfmnet import visual
  tiles = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device="cuda")
  sheet = torch.full((16, 24, 3), 0xAB, dtype=torch.uint8, device="cuda")          # 6 cells
  for first in (3, 6, -1):
    with pytest.raises(RuntimeError, match="outside"):
      visual.sheet_tile(tiles, sheet, first)
  torch.cuda.synchronize()
  assert bool((sheet == 0xAB).all())
  visual.sheet_tile(tiles, sheet, 2)                                               # cells 2..5: the last one that fits
  assert bool((sheet[8:] == 0).all()) and bool((sheet[:8, :16] == 0xAB).all())


@pytest.mark.parametrize("frames", [1, 12, 70])
def test_landmark_distance(frames):
  import torch
  from voicepuppet_amd.bfmnet import visual
  rng = np.random.default_rng(frames)
  N = 300
  a, b = rng.uniform(0, 224, (frames, N, 2)), rng.uniform(0, 224, (frames, N, 2))
  kp = rng.choice(N, 68, replace=False).astype(np.int32)
  kp_d = torch.from_numpy(kp).cuda()
  got = visual.landmark_distance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), kp_d).cpu().numpy()
  want = vr.lmd(a, b, kp)
  assert got.shape == (frames, 2) and np.abs(got / want - 1).max() < 1e-12
  assert np.all(got[:, 0] != got[:, 1])
  f = frames // 2                                                      # a frame alone gives the bits it has inside the batch
  alone = visual.landmark_distance(torch.from_numpy(a[f:f + 1]).cuda(), torch.from_numpy(b[f:f + 1]).cuda(), kp_d).cpu().numpy()
  assert np.array_equal(alone[0], got[f])
  same = visual.landmark_distance(torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda(), kp_d).cpu().numpy()
  assert np.array_equal(same, np.zeros((frames, 2)))


def test_mesh_sheet_render_against_the_restatement():
  """seq_len 40 (clamped to 30), then 12 (the golden's clip: reference-made tiles), then 5: each sheet is the restatement's, rows 6-8
  are zero, and the shorter clips leave nothing of the longer ones behind."""
  from voicepuppet_amd.bfmnet.visual import MeshSheet
  g, fm, _ = golden()
  ms = MeshSheet(model())
  real, pred = long_sequences()
  for seq_len in (40, 12, 5):
    r, p = (g["real"], g["pred"]) if seq_len == 12 else (real, pred)
    sheet, lmd = ms.render(np.array([seq_len, 3], np.int32), r, p)
    big, want_lmd = want_montage(seq_len)
    host = sheet.cpu().numpy()
    assert host.shape == (2016, 2240, 3) and host.dtype == np.uint8
    assert np.array_equal(host, big[..., ::-1]), seq_len                # the file's RGB: the reference's big_img with R and B exchanged
    assert not host[6 * 224:].any() and host[:224].any() and host[3 * 224:4 * 224].any()
    time = min(seq_len, 30)
    assert lmd.shape == (time, 2) and str(lmd.dtype) == "torch.float64"
    assert np.abs(lmd.cpu().numpy() - want_lmd).max() < LMD_ATOL
  # the reference's in-memory array, and device tensors as input
  import torch
  sheet, _ = MeshSheet(model(), swap_rb=True).render([12], torch.from_numpy(g["real"]).cuda(), torch.from_numpy(g["pred"]).cuda())
  assert np.array_equal(sheet.cpu().numpy(), want_montage(12)[0])


def test_mesh_sheet_id_and_texture_branch():
  from voicepuppet_amd.bfmnet.visual import MeshSheet
  real, pred = long_sequences()
  idc, texc = branch_coeffs()
  sheet, lmd = MeshSheet(model()).render([7], real[:1], pred[:1], idc, texc)
  big, want_lmd = want_montage(7, branch=True)
  assert np.array_equal(sheet.cpu().numpy(), big[..., ::-1])
  assert np.abs(lmd.cpu().numpy() - want_lmd).max() < LMD_ATOL
  assert not np.array_equal(big, want_montage(5)[0])


def test_plot_bfm_coeff_seq_writes_the_sheet_as_jpeg(tmp_path):
  """bfmnet_<step>.jpg decodes to 2016 x 2240; its PSNR against the sheet is at most 0.2 dB below that of PIL's quality-95 4:2:0 file of
  the same array (the encoder's record on faces is 0.09 dB, profiles/jpeg_encode.json; a sheet of flat-shaded triangles on black is the
  harder image).  Measured on an MI355X: device 36.602 dB, PIL 36.596 dB, 557817 bytes."""
  from voicepuppet_amd.bfmnet import visual
  g, fm, _ = golden()
  ms = visual.MeshSheet(model())
  got = visual.plot_bfm_coeff_seq(str(tmp_path), ms, 7, g["seq_len"], g["real"], g["pred"])
  big, want_lmd = want_montage(12)
  assert np.abs(np.array(got) - want_lmd.mean(axis=0)).max() < LMD_ATOL
  path = tmp_path / "bfmnet_7.jpg"
  assert sorted(os.listdir(tmp_path)) == ["bfmnet_7.jpg"]
  rgb = np.ascontiguousarray(big[..., ::-1])
  dev = decode(path.read_bytes())
  assert dev.shape == (2016, 2240, 3)
  p_dev, p_pil = psnr(dev, rgb), psnr(decode(pil_file(rgb, 95)), rgb)
  print("sheet jpeg: device %.3f dB, PIL %.3f dB, %d bytes" % (p_dev, p_pil, path.stat().st_size))
  assert p_dev >= p_pil - 0.2
  # the reference's BFM object instead of a kept MeshSheet, numpy in: the same file
  visual.plot_bfm_coeff_seq(str(tmp_path), fm, 8, g["seq_len"], g["real"], g["pred"])
  assert (tmp_path / "bfmnet_8.jpg").read_bytes() == path.read_bytes()


def _write_mat(fm):
  from scipy.io import savemat
  os.makedirs("BFM")
  savemat(os.path.join("BFM", "BFM_model_front.mat"),
          {"meanshape": fm.meanshape, "idBase": fm.idBase, "exBase": fm.exBase, "meantex": fm.meantex, "texBase": fm.texBase,
           "point_buf": fm.point_buf, "tri": fm.tri, "keypoints": (fm.keypoints + 1).reshape(1, -1)})


def test_train_launcher_writes_the_montage_only_when_asked(tmp_path, monkeypatch, capsys):
  from PIL import Image
  from voicepuppet_amd.bfmnet import train_bfmnet
  monkeypatch.chdir(tmp_path)
  _write_mat(golden()[1])
  args = ["--config_path", CFG, "--steps", "2", "--batch_size", "2", "--eval_step", "1", "--save_step", "100"]
  train_bfmnet.main(args)
  plain = capsys.readouterr().out
  assert plain.count("Evaluation >>> Loss=") == 2 and "LMD" not in plain
  assert sorted(os.listdir(".")) == ["BFM", "ckpt_bfmnet"]              # nothing else written
  train_bfmnet.main(args + ["--eval_visual_dir", "vis"])
  out = capsys.readouterr().out
  assert out.count("Evaluation >>> Loss=") == 2 and out.count("LMD= ") == 2 and "px, mouth " in out
  assert sorted(os.listdir("vis")) == ["bfmnet_1.jpg", "bfmnet_2.jpg"]
  img = np.asarray(Image.open(os.path.join("vis", "bfmnet_2.jpg")))
  # a training clip has 24 frames: rows 0-2 and 3-5 are drawn on; rows 6-8 are black (the decoder's chroma upsampling smears row 5's last
  # pixels over the edge of its MCU row, hence the 16)
  assert img.shape == (2016, 2240, 3) and img[:224].max() > 64 and img[3 * 224:4 * 224].max() > 64 and img[6 * 224 + 16:].max() < 4
  lines = [l for l in out.splitlines() if not l.startswith("LMD= ")]
  assert len(lines) == len(plain.splitlines())                          # the other lines are the ones a plain run prints


def test_infer_bfmnet_cli_frames_and_avi(tmp_path, monkeypatch):
  """A 1 s clip: 26 frames of 672 x 672; frame 0 is the restatement's view-1 raster of the clip's first coefficients through a
  quality-75 JPEG (at most 0.2 dB below PIL's file of that raster); --avi_only writes a 672 x 672 AVI of 26 frames the reader accepts."""
  from scipy.io import wavfile
  from voicepuppet_amd.bfmnet import infer_bfmnet
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.pixrefer import infer_bfmvid
  monkeypatch.chdir(tmp_path)
  fm = golden()[1]
  _write_mat(fm)
  t = np.arange(16000) / 16000.0
  wavfile.write("a.wav", 16000, (0.3 * np.sin(2 * np.pi * 440 * t) * np.sin(2 * np.pi * 3 * t) * 32767).astype(np.int16))
  np.savez("photo.npz", bfmcoeff=br.synthetic_coeffs(1, 5)[0].reshape(1, 257))
  os.makedirs("ckpt_bfmnet")
  np.savez(infer_bfmvid.BFMNET_CKPT + ".npz", **random_variables(seed=11))
  args = ["--config_path", CFG, "--bfmcoeff", "photo.npz"]
  infer_bfmnet.main(args + ["--device_jpeg", "--output_dir", "out", "face.jpg", "a.wav"])
  names = sorted(os.listdir("out"), key=lambda f: int(f.split(".")[0]))
  assert names == ["%d.jpg" % i for i in range(26)]
  frames = [decode(open(os.path.join("out", f), "rb").read()) for f in names]
  assert all(f.shape == (672, 672, 3) for f in frames)
  assert any(not np.array_equal(frames[0], f) for f in frames[1:])      # the mouth moves
  coeff = infer_bfmnet.predict_coefficients(CFG, "a.wav", "photo.npz")[0]
  assert coeff.shape == (26, 257)
  v, c = vr.pack_view(vr.reconstruction(coeff[:1], fm), 1, 3)
  want = vr.raster(v[0], c[0], fm, 672)
  assert want.any()
  p_dev, p_pil = psnr(frames[0], want), psnr(decode(pil_file(want, 75)), want)
  print("mesh frame jpeg: device %.3f dB, PIL %.3f dB" % (p_dev, p_pil))
  assert p_dev >= p_pil - 0.2
  infer_bfmnet.main(args + ["--avi_only", "--frame_batch", "5", "--output_dir", "clip", "face.jpg", "a.wav"])
  assert os.listdir("clip") == []
  a = avi_ref.check("clip.avi", 672, 672)
  assert len(a.video) == 26
  assert psnr(decode(a.video[0]), want) >= p_pil - 0.2

"""BFMNet visual evaluation, the parts that need no GPU: the numpy restatement (tests/bfm_visual_ref.py) against what the reference's
own reconstruct_mesh.Reconstruction returned (tests/golden/bfm_visual.npz, made by tests/golden/make_bfm_visual_golden.py), the
arithmetic helpers of voicepuppet_amd/bfmnet/visual.py against the reference's index lines, the binding, and the two launchers' option
parsers.

Tolerances as tests/test_bfm_recon.py: float64 outputs within 1e-13 relative of the reference's (its per-frame matmuls against the
batched ones here); the float32 vertices, integer colours and rasterised tiles IDENTICAL."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfm_visual_ref as vr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bfm_visual.npz")
_CACHE = {}


def golden():
  """(npz, face model, spliced sequence) - loaded once, never written to."""
  if "g" not in _CACHE:
    g = np.load(GOLD)
    fm = br.synthetic_facemodel(int(g["model_seed"]))
    chk = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(), float(fm.tri.sum()),
                    float(fm.point_buf.sum()), float(fm.keypoints.sum())])
    assert np.array_equal(chk, g["model_checksum"]), "seeded face model differs from the one the golden was made with"
    _CACHE["g"] = ({k: g[k] for k in g.files}, fm, vr.splice(g["real"], g["pred"]))
  return _CACHE["g"]


def rel(a, b):
  return np.abs(a - b).max() / np.abs(b).max()


def sequences():
  g, fm, spliced = golden()
  return (("real", g["real"][0]), ("pred", spliced[0]))


def test_golden_inputs_are_the_seeded_ones():
  g, fm, _ = golden()
  real, pred = vr.synthetic_sequences(12, int(g["seq_seed"]))
  assert np.array_equal(real, g["real"]) and np.array_equal(pred, g["pred"]) and g["seq_len"].tolist() == [12]
  assert g["real"].shape == (1, 12, 257) and g["pred"].shape == (1, 12, 64) and g["real"].dtype == np.float32


@pytest.mark.parametrize("tag", ["real", "pred"])
def test_restatement_matches_the_reference_reconstruction(tag):
  g, fm, _ = golden()
  coeff = dict(sequences())[tag]
  out = vr.reconstruction(coeff, fm)
  for n in vr.NAMES:
    want = g["%s_%s" % (tag, n)]
    assert out[n].shape == want.shape, n
    assert rel(out[n], want) < 1e-13, n
  assert np.array_equal(out["translation"], coeff[:, 254:])
  # one rotation, not two, and not none: the unrotated shape is returned and the projection differs from the unrotated one
  rot = br.reconstruction_rotation(coeff, fm, coeff[:, 224:227])
  assert rel(rot["face_projection"], g[tag + "_face_projection"]) > 1e-4
  v0, c = vr.pack_view(out, 0)
  v1, c1 = vr.pack_view(out, 1, 3)
  assert v0.dtype == np.float32 and np.array_equal(v0, g[tag + "_vertices_view0"])
  assert np.array_equal(v1, g[tag + "_vertices_view1"])
  assert np.array_equal(c, g[tag + "_colors"]) and np.array_equal(c1, c)


def test_restatement_tiles_match_the_reference_rasteriser():
  g, fm, _ = golden()
  for tag, coeff in sequences():
    tiles = vr.tiles_of(coeff[[0, 5, 11]], fm)
    assert np.array_equal(tiles, g[tag + "_tiles"][[0, 5, 11]]), tag
    assert tiles.any()


def test_montage_layout_and_lmd():
  g, fm, spliced = golden()
  big, lmd = vr.montage(fm, g["seq_len"], g["real"], g["pred"], tiles=(g["real_tiles"], g["pred_tiles"]))
  assert big.shape == (2016, 2240, 3) and big.dtype == np.uint8
  assert np.array_equal(big[0:224, 224:448], g["real_tiles"][1][..., ::-1])                     # frame 1: row 0, column 1
  assert np.array_equal(big[224:448, 224:448], g["real_tiles"][11][..., ::-1])                  # frame 11: row 1, column 1
  assert np.array_equal(big[4 * 224:5 * 224, 0:224], g["pred_tiles"][10][..., ::-1])            # predicted frame 10: row 3 + 1, column 0
  assert not big[448:672].any() and not big[5 * 224:].any() and not big[224:448, 448:].any()    # rows 6-8 (and the unused cells) stay black
  kp = fm.keypoints
  d = np.linalg.norm(g["real_landmarks_2d"] - g["pred_landmarks_2d"], axis=2)
  assert lmd.shape == (12, 2)
  assert np.allclose(lmd[:, 0], d.mean(1), rtol=1e-12) and np.allclose(lmd[:, 1], d[:, 48:].mean(1), rtol=1e-12)
  assert np.array_equal(g["real_landmarks_2d"], g["real_face_projection"][:, kp]) and lmd.min() > 0


@pytest.mark.parametrize("time", [1, 10, 11, 30])
def test_sheet_cells_against_the_reference_index_arithmetic(time):
  from voicepuppet_amd.bfmnet import visual
  for h_index in (0, 3):
    want = []
    for i in range(time):                                  # bfm_visual.py:127-128
      r0, c0 = (i // 10 + h_index) * 224, (i % 10) * 224
      want.append((r0 // 224, c0 // 224))
    assert visual.sheet_cells(time, h_index) == want
    assert max(r for r, _ in want) < 6                     # never reaches rows 6-8
  assert visual.sheet_cells(5, 1, cols=4) == [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0)]


def test_splice_predicted_both_branches_and_clip_time():
  from voicepuppet_amd.bfmnet import visual
  g, fm, spliced = golden()
  real, pred = np.tile(g["real"], (2, 1, 1)), np.tile(g["pred"], (2, 1, 1))
  got = visual.splice_predicted(real, pred)
  assert got.dtype == np.float32 and np.array_equal(got[:1], spliced) and np.array_equal(got, vr.splice(real, pred))
  rng = np.random.default_rng(0)
  idc, texc = rng.normal(size=(1, 1, 80)).astype(np.float32), rng.normal(size=(1, 1, 80)).astype(np.float32)
  got = visual.splice_predicted(real[:1], pred[:1], idc, texc)
  assert got.shape == (1, 12, 257) and np.array_equal(got, vr.splice(real[:1], pred[:1], idc, texc))
  assert np.array_equal(got[0, 7, :80], idc[0, 0]) and np.array_equal(got[0, 7, 144:224], texc[0, 0]) and np.array_equal(got[..., 224:], real[:1, :, 224:])
  # one of the two alone is the first branch (bfm_visual.py:147: `or`)
  assert np.array_equal(visual.splice_predicted(real, pred, id_coeff=idc), vr.splice(real, pred))
  import torch
  t = visual.splice_predicted(torch.from_numpy(real[:1]), torch.from_numpy(pred[:1]), torch.from_numpy(idc), torch.from_numpy(texc))
  assert np.array_equal(t.numpy(), got)
  for n, want in ((5, 5), (30, 30), (40, 30)):
    assert visual.clip_time([n, 99]) == want == vr.clip_time([n, 99])
    assert visual.clip_time(np.array([n], np.int32)) == want


def test_strip_assembly_renumbers_restart_markers():
  """_assemble_strips on hand-made strip files: per MCU row the strips' intervals left to right, markers RST0..7 in sequence, the width
  patched in the frame header."""
  from voicepuppet_amd.bfmnet import visual
  header = b"\xff\xd8" + b"\xff\xc0\x00\x11\x08" + bytes([0, 32, 0, 16]) + b"rest-of-header"
  a = header + b"a0" + b"\xff\xd0" + b"a1" + b"\xff\xd9"
  b = header + b"b0\xff\x00" + b"\xff\xd0" + b"b1" + b"\xff\xd9"
  out = visual._assemble_strips(header, [a, b], 32)
  want_head = b"\xff\xd8" + b"\xff\xc0\x00\x11\x08" + bytes([0, 32, 0, 32]) + b"rest-of-header"
  assert out == want_head + b"a0" + b"\xff\xd0" + b"b0\xff\x00" + b"\xff\xd1" + b"a1" + b"\xff\xd2" + b"b1" + b"\xff\xd9"


def test_strip_assembly_of_host_encoded_strips_decodes_like_the_whole_sheet():
  """The same assembly on real files: the golden's sheet cut into four 560-wide strips, each encoded by the host encoder of the device
  encoder's format (jpeg.host_jpeg: one restart interval per MCU row), joined, decodes to exactly what PIL's file of the whole sheet
  decodes to - the restart intervals of a strip are those of the sheet."""
  import io
  from PIL import Image
  from voicepuppet_amd.bfmnet import visual
  from voicepuppet_amd.jpeg import host_jpeg
  g, fm, _ = golden()
  big, _ = vr.montage(fm, g["seq_len"], g["real"], g["pred"], tiles=(g["real_tiles"], g["pred_tiles"]))
  rgb = np.ascontiguousarray(big[..., ::-1])
  files = [host_jpeg(np.ascontiguousarray(rgb[:, i * visual.STRIP_W:(i + 1) * visual.STRIP_W]), 95) for i in range(4)]
  sos = files[0].index(b"\xff\xda")
  header = files[0][:sos + 2 + ((files[0][sos + 2] << 8) | files[0][sos + 3])]
  out = visual._assemble_strips(header, files, 2240)
  whole = io.BytesIO()
  Image.fromarray(rgb).save(whole, "JPEG", quality=95, subsampling=2)
  got, want = np.asarray(Image.open(io.BytesIO(out)).convert("RGB")), np.asarray(Image.open(whole).convert("RGB"))
  assert got.shape == (2016, 2240, 3) and np.array_equal(got, want)


def test_every_new_symbol_of_the_header_is_bound():
  from voicepuppet_amd import _lib
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header))
  new = {"vp_bfm_reconstruct_view", "vp_sheet_tile_u8", "vp_landmark_distance"}
  assert new <= declared and new <= set(_lib.exported_symbols())
  lib = _lib.lib()
  for name in new:
    assert getattr(lib, name).argtypes is not None, name
  assert len(lib.vp_bfm_reconstruct_view.argtypes) == 17 and lib.vp_bfm_reconstruct_view.argtypes[6] is __import__("ctypes").c_double
  # host-side refusals need no device: nothing is enqueued for an out-of-range cell or a bad view
  import ctypes
  buf = (ctypes.c_ubyte * 64)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  assert lib.vp_sheet_tile_u8(p, 2, 2, 2, p, 1, 2, 1, 0, None) == -1 and b"outside" in lib.vp_last_error()
  assert lib.vp_sheet_tile_u8(p, 1, 2, 2, p, 1, 2, -1, 0, None) == -1
  assert lib.vp_landmark_distance(None, p, p, 1, 4, p, None) == -1
  m = _lib.BfmModel()
  assert lib.vp_bfm_reconstruct_view(ctypes.byref(m), p, p, 1, 0, 2, 1.0, None, None, None, None, None, p, p, p, 64, None) == -1
  assert b"view" in lib.vp_last_error()


def test_train_launcher_parses_without_the_new_flags_and_keeps_the_visual_path_off(tmp_path, monkeypatch, caplog):
  from voicepuppet_amd.bfmnet import train_bfmnet as tb
  opts, rest = tb.parse_options(["--config_path", "c.yml", "--steps", "3"])
  assert (opts.eval_visual_dir, opts.eval_visual, opts.steps, opts.batch_size, opts.eval_step, opts.save_step) == (None, False, 3, 4, 1000, 5000)
  assert tb.visual_dir(opts) is None and tb.mesh_sheet(None) is None and rest == []
  assert tb.visual_dir(tb.parse_options(["--eval_visual"])[0]) == "log/eval_bfmnet"              # the reference's directory
  assert tb.visual_dir(tb.parse_options(["--eval_visual", "--eval_visual_dir", "x"])[0]) == "x"
  monkeypatch.chdir(tmp_path)                              # no BFM/BFM_model_front.mat here: one warning, no sheet, no directory made
  with caplog.at_level("WARNING"):
    assert tb.mesh_sheet("vis") is None
  assert "BFM_model_front.mat" in caplog.text and not os.path.exists("vis")


def test_infer_bfmnet_option_parser_and_ears():
  from voicepuppet_amd.bfmnet import infer_bfmnet as ib
  from voicepuppet_amd.pixrefer import infer_bfmvid
  assert ib.parse_options is infer_bfmvid.parse_options and ib.prepare_pcm is infer_bfmvid.prepare_pcm       # shared, not copied
  assert ib.splice_coeff is infer_bfmvid.splice_coeff and ib.restore_or_init is infer_bfmvid.restore_or_init
  opts, rest = ib.parse_options(["--config_path", "c.yml", "face.jpg", "a.wav"])
  assert rest == ["face.jpg", "a.wav"]
  assert (opts.frame_batch, opts.bfmcoeff, opts.output_dir, opts.device_jpeg, opts.avi, opts.avi_only) == (8, None, "output", False, False, False)
  opts, _ = ib.parse_options(["--config_path", "c.yml", "--frame_batch", "3", "--bfmcoeff", "p.npz", "--output_dir", "o", "--avi_only", "i", "a"])
  assert (opts.frame_batch, opts.bfmcoeff, opts.output_dir, opts.avi_only) == (3, "p.npz", "o", True)
  ears = ib.ears_sequence(7)                               # infer_bfmnet.py:162-164
  assert ears.shape == (1, 7, 1) and ears.dtype == np.float32
  assert np.array_equal(ears[0, :, 0], np.array([0.2, 0.2, 0.2, 0.9, 0.9, 0.9, 0.9], np.float32))
  assert (ib.IMG_SIZE, ib.SCALE) == (672, 3)
  assert os.path.exists(os.path.join(ROOT, "voicepuppet", "bfmnet", "infer_bfmnet.py"))

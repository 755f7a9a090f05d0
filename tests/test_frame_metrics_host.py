"""The frame metrics' definition and host layer, without a GPU: known answers of the numpy restatement (tests/frame_metrics_ref.py) the
device kernel is compared with in tests/test_gpu_frame_metrics.py, the C ABI's surface and refusals, and compare_frames.py's argument
handling and JSON shape with the device part stubbed by the restatement."""
import ctypes
import io
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_metrics_ref as fr  # noqa: E402


def _image(w, h, seed):
  """a smooth ramp with +-20 of noise (the content of the JPEG tests)"""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), ((xx + yy) * 5) % 256], -1)
  return (img + rng.integers(-20, 20, img.shape)).clip(0, 255).astype(np.uint8)


def _noise(h, w, seed):
  return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_identical_images():
  a = _noise(24, 31, 0)
  l1, mse, psnr, ssim = fr.metrics(a, a.copy())
  assert l1 == 0 and mse == 0 and psnr == np.inf and abs(ssim - 1.0) <= 1e-15
  assert fr.sums(a, a) == (0, 0)


@pytest.mark.parametrize("c1,c2", [(0, 255), (10, 200), (77, 78), (255, 255)])
def test_constant_images(c1, c2):
  a, b = np.full((13, 17, 3), c1, np.uint8), np.full((13, 17, 3), c2, np.uint8)
  l1, mse, psnr, ssim = fr.metrics(a, b)
  assert l1 == abs(c1 - c2) and mse == (c1 - c2) ** 2
  assert psnr == (np.inf if c1 == c2 else 10.0 * np.log10(255.0 ** 2 / (c1 - c2) ** 2))
  want = (2.0 * c1 * c2 + fr.C1) / (c1 * c1 + c2 * c2 + fr.C1)        # variances and covariance 0: the C2 factors cancel
  assert abs(ssim - want) <= 1e-10


def test_one_window_equals_the_hand_written_formula():
  a, b = _noise(11, 11, 1), _noise(11, 11, 2)
  g = [np.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
  g = [v / sum(g) for v in g]
  total = 0.0
  for c in range(3):
    ea = eb = eaa = ebb = eab = 0.0
    for y in range(11):
      for x in range(11):
        w, p, q = g[y] * g[x], float(a[y, x, c]), float(b[y, x, c])
        ea += w * p; eb += w * q; eaa += w * p * p; ebb += w * q * q; eab += w * p * q
    va, vb, cov = eaa - ea * ea, ebb - eb * eb, eab - ea * eb
    total += ((2 * ea * eb + 6.5025) * (2 * cov + 58.5225)) / ((ea * ea + eb * eb + 6.5025) * (va + vb + 58.5225))
  m = fr.ssim_map(a, b)
  assert m.shape == (1, 1, 3) and abs(m.mean() - total / 3) <= 1e-12
  assert abs(fr.C1 - 6.5025) < 1e-12 and abs(fr.C2 - 58.5225) < 1e-12 and abs(fr.window().sum() - 1) < 1e-15


def test_restatement_equals_skimage():
  skm = pytest.importorskip("skimage.metrics")
  for seed, (h, w) in enumerate([(11, 11), (23, 40), (64, 48)]):
    a, b = _noise(h, w, 10 + seed), _noise(h, w, 20 + seed)
    full = skm.structural_similarity(a, b, gaussian_weights=True, use_sample_covariance=False, data_range=255, channel_axis=-1, full=True)[1]
    assert abs(full[5:h - 5, 5:w - 5].mean() - fr.metrics(a, b)[3]) <= 1e-12


def test_map_f32_clamps_and_inverts_the_uint8_scale():
  u = np.arange(256, dtype=np.uint8)
  x = (u.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
  assert np.abs(fr.map_f32(x) - u).max() < 2e-5
  assert fr.map_f32(np.float32([-3.0, 1.5, np.nan])).tolist() == [0.0, 255.0, 0.0]
  assert fr.map_f32(np.float32([300.0, -1.0, 7.25]), 1.0, 0.0).tolist() == [255.0, 0.0, 7.25]


def test_header_declares_the_frame_metrics_abi_and_the_binding_mirrors_it():
  from voicepuppet_amd import _lib
  import voicepuppet_amd.metrics as vm  # importable without a GPU
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  names = ("vp_frame_metrics_desc_size", "vp_frame_metrics_workspace_bytes", "vp_frame_metrics_create", "vp_frame_metrics_destroy",
           "vp_frame_metrics_u8", "vp_frame_metrics_f32", "vp_frame_metrics_tensor")
  for name in names:
    assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols(), name
  body = hdr[hdr.index("typedef struct vp_frame_metrics_desc {"):hdr.index("} vp_frame_metrics_desc;")]
  assert re.findall(r"\b(?:u?int32_t)\s+(\w+);", body) == [n for n, _ in _lib.FrameMetricsDesc._fields_]
  assert ctypes.sizeof(_lib.FrameMetricsDesc) == 16
  assert "#define VP_FRAME_METRICS_MAX_FRAMES %d" % _lib.FRAME_METRICS_MAX_FRAMES in hdr
  assert "structural_similarity" in hdr and "use_sample_covariance=False" in hdr
  src = open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  assert "frame_metrics.hip" in src.split("SRCS =")[1].split("\n")[0]
  assert vm.COLUMNS == ("L1", "MSE", "PSNR", "SSIM") and (vm.L1, vm.MSE, vm.PSNR, vm.SSIM) == (0, 1, 2, 3)


def test_library_answers_and_refuses_with_the_field_named():
  from voicepuppet_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libvp_hip.so is not built: desc_size, workspace_bytes and the refusals are unexercised")
  names = [n for n in _lib.exported_symbols() if n.startswith("vp_frame_metrics_")]
  assert len(names) == 7
  L = _lib.lib()
  for name in names:
    assert hasattr(L, name), name
  n = ctypes.sizeof(_lib.FrameMetricsDesc)
  assert L.vp_frame_metrics_desc_size() == n
  # one record of 40 bytes per tile of 16 x 16 windows and frame
  assert L.vp_frame_metrics_workspace_bytes(ctypes.byref(_lib.FrameMetricsDesc(n, 64, 512, 512))) >= 64 * 32 * 32 * 40
  for what, d in [("max_frames", _lib.FrameMetricsDesc(n, 0, 64, 64)), ("max_frames", _lib.FrameMetricsDesc(n, 4097, 64, 64)),
                  ("max_height", _lib.FrameMetricsDesc(n, 1, 10, 64)), ("max_height", _lib.FrameMetricsDesc(n, 1, 9000, 64)),
                  ("max_width", _lib.FrameMetricsDesc(n, 1, 64, 10)), ("max_width", _lib.FrameMetricsDesc(n, 1, 64, 9000)),
                  ("struct_bytes", _lib.FrameMetricsDesc(n - 4, 1, 64, 64))]:
    assert L.vp_frame_metrics_workspace_bytes(ctypes.byref(d)) == 0 and what in L.vp_last_error().decode(), what
    h = ctypes.c_void_p()
    assert L.vp_frame_metrics_create(ctypes.byref(d), None, 0, ctypes.byref(h)) == -1 and not h.value
    assert what in L.vp_last_error().decode()
  # create is host only: with a workspace address that is never touched, the call-time refusals answer without a GPU
  good = _lib.FrameMetricsDesc(n, 2, 64, 64)
  ws = L.vp_frame_metrics_workspace_bytes(ctypes.byref(good))
  h = ctypes.c_void_p()
  assert L.vp_frame_metrics_create(ctypes.byref(good), ctypes.c_void_p(4096), ws - 1, ctypes.byref(h)) == -3 and not h.value
  assert L.vp_frame_metrics_create(ctypes.byref(good), ctypes.c_void_p(4096), ws, ctypes.byref(h)) == 0 and h.value
  p = ctypes.c_void_p(1 << 20)
  for what, args in [("height", (1, 10, 64)), ("width", (1, 64, 10)), ("n ", (3, 64, 64)), ("max_height", (1, 65, 64)), ("max_width", (1, 64, 65))]:
    cnt, hh, ww = args
    assert L.vp_frame_metrics_u8(h, p, 3 * ww, 3 * ww * hh, p, 3 * ww, 3 * ww * hh, cnt, hh, ww, p, None) == -1
    assert what in L.vp_last_error().decode(), (what, L.vp_last_error())
  assert L.vp_frame_metrics_u8(h, p, 3 * 64 - 1, 3 * 64 * 64, p, 3 * 64, 3 * 64 * 64, 1, 64, 64, p, None) == -1 and b"a_row_pitch" in L.vp_last_error()
  assert L.vp_frame_metrics_u8(h, p, 3 * 64, 3 * 64 * 64, p, 3 * 64, 3 * 64 * 64 - 1, 1, 64, 64, p, None) == -1 and b"b_frame_stride" in L.vp_last_error()
  assert L.vp_frame_metrics_f32(h, p, 12 * 64 + 2, 12 * 64 * 64 + 128, p, 12 * 64, 12 * 64 * 64, 1, 64, 64, 127.5, 127.5, p, None) == -1
  assert b"multiples of 4" in L.vp_last_error()
  assert L.vp_frame_metrics_u8(h, p, 3 * 64, 3 * 64 * 64, p, 3 * 64, 3 * 64 * 64, 1, 64, 64, ctypes.c_void_p((1 << 20) + 4), None) == -1
  assert b"8-byte" in L.vp_last_error()
  assert L.vp_frame_metrics_u8(h, p, 3 * 64, 1 << 49, p, 3 * 64, 3 * 64 * 64, 1, 64, 64, p, None) == -1 and b"a_frame_stride" in L.vp_last_error()
  q, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
  assert L.vp_frame_metrics_tensor(h, b"abs_sum", ctypes.byref(q), shp) == 0 and shp[0] == 2
  assert L.vp_frame_metrics_tensor(h, b"nothing", ctypes.byref(q), shp) == -1 and b"abs_sum, sq_sum" in L.vp_last_error()
  L.vp_frame_metrics_destroy(h)


# ---- compare_frames.py with the device part stubbed by the restatement -----------------------------------------------------------------
def _jpeg(img, quality):
  from PIL import Image
  b = io.BytesIO()
  Image.fromarray(img).save(b, "JPEG", quality=quality)
  return b.getvalue()


def _pil_rgb(path):
  from PIL import Image
  return np.asarray(Image.open(path).convert("RGB"))


def _stub(a, b):
  return fr.batch(a, b)


def _dirs(tmp_path, n=3, missing=None):
  da, db = tmp_path / "a", tmp_path / "b"
  da.mkdir(); db.mkdir()
  for i in range(n):
    img = _image(64, 48, 70 + i)
    (da / ("%d.jpg" % i)).write_bytes(_jpeg(img, 95))
    if i != missing:
      (db / ("%d.jpg" % i)).write_bytes(_jpeg(img, 50))
  return str(da), str(db)


def test_compare_frames_json_shape_and_arguments(tmp_path, capsys):
  from voicepuppet_amd.pixrefer import compare_frames as cf
  da, db = _dirs(tmp_path)
  out = str(tmp_path / "m.json")
  res = cf.main([da, db, "--out", out], load=lambda paths: [_pil_rgb(p) for p in paths], compare=_stub)
  text = capsys.readouterr().out
  with open(out) as f:
    saved = json.load(f)
  assert saved == json.loads(json.dumps(res))
  assert saved["a"] == da and saved["b"] == db and saved["kind"] == "jpg" and [f["index"] for f in saved["frames"]] == [0, 1, 2]
  want = np.stack([fr.metrics(_pil_rgb(os.path.join(da, "%d.jpg" % i)), _pil_rgb(os.path.join(db, "%d.jpg" % i))) for i in range(3)])
  for i, f in enumerate(saved["frames"]):
    assert [f[k] for k in ("L1", "MSE", "PSNR", "SSIM")] == want[i].tolist()
  s = saved["summary"]
  assert s["frames"] == 3
  for j, k in enumerate(("L1", "MSE", "PSNR", "SSIM")):
    assert s[k]["mean"] == want[:, j].mean() and s[k]["min"] == want[:, j].min() and s[k]["max"] == want[:, j].max()
  assert s["PSNR"]["worst"] == int(np.argmin(want[:, 2])) and s["SSIM"]["worst"] == int(np.argmin(want[:, 3]))
  assert s["L1"]["worst"] == int(np.argmax(want[:, 0]))
  assert len([l for l in text.splitlines() if l.startswith("frame ")]) == 3 and "mean" in text and "worst" in text


def test_compare_frames_refuses_what_it_cannot_pair(tmp_path):
  from voicepuppet_amd.pixrefer import compare_frames as cf
  da, db = _dirs(tmp_path, missing=1)
  with pytest.raises(SystemExit) as e:
    cf.main([da, db], load=lambda paths: [_pil_rgb(p) for p in paths], compare=_stub)
  assert "1.jpg" in str(e.value)
  with pytest.raises(SystemExit):
    cf.main([da, str(tmp_path / "nowhere")], compare=_stub)
  empty = tmp_path / "empty"
  empty.mkdir()
  with pytest.raises(SystemExit) as e:
    cf.main([str(empty), str(empty)], compare=_stub)
  assert "no " in str(e.value)


def test_compare_frames_takes_dumped_generator_outputs(tmp_path):
  """two bench.py --dump-outputs directories: Outputs.npy, float32 [N, H, H, 3] in [0, 1]"""
  from voicepuppet_amd.pixrefer import compare_frames as cf
  rng = np.random.default_rng(5)
  a = rng.uniform(size=(2, 16, 16, 3)).astype(np.float32)
  b = (a + rng.normal(0, 0.02, a.shape)).astype(np.float32)
  for name, arr in (("a", a), ("b", b)):
    (tmp_path / name).mkdir()
    np.save(str(tmp_path / name / "Outputs.npy"), arr)
  seen = {}

  def compare(x, y, **kw):
    seen.update(kw, dtype=x.dtype)
    return fr.batch(fr.map_f32(x, 255.0, 0.0), fr.map_f32(y, 255.0, 0.0))
  res = cf.main([str(tmp_path / "a"), str(tmp_path / "b")], compare=compare)
  assert res["kind"] == "npy" and res["summary"]["frames"] == 2 and seen == {"value_range": (0, 1), "dtype": np.float32}
  np.save(str(tmp_path / "b" / "Outputs.npy"), b[:, :12])
  with pytest.raises(SystemExit) as e:
    cf.main([str(tmp_path / "a"), str(tmp_path / "b")], compare=compare)
  assert "shape" in str(e.value)


def test_launcher_options_and_the_deterministic_crop(tmp_path):
  from voicepuppet_amd.pixrefer.train_pixrefer import parse_options
  from voicepuppet_amd.pixrefer import heldout
  o = parse_options(["--config_path", "c.yml"])
  assert o.eval_list is None and o.eval_step is None and o.eval_frames is None        # absent by default
  o = parse_options(["--config_path", "c.yml", "--eval_list", "held.txt", "--eval_step", "500", "--eval_frames", "16"])
  assert (o.eval_list, o.eval_step, o.eval_frames) == ("held.txt", 500, 16)
  for size in (64, 256, 512):
    rx, ry, rsize = heldout.centre_crop(size, 0.9)
    assert int(size * 0.9) <= rsize <= size and rx == ry == (size - rsize) // 2 and rx + rsize <= size
  lst = tmp_path / "l.txt"
  lst.write_text("/d/a|2\n\n/d/b|3\n")
  assert heldout.first_pairs(str(lst), 4) == [("/d/a/0.jpg", "/d/a/0.jpg"), ("/d/a/0.jpg", "/d/a/1.jpg"), ("/d/b/0.jpg", "/d/b/0.jpg"),
                                              ("/d/b/0.jpg", "/d/b/1.jpg")]
  assert len(heldout.first_pairs(str(lst), 99)) == 5

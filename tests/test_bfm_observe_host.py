"""CPU checks for FaceFitter.observe's self-occlusion test and area pre-filter (csrc/bfm_observe.hip: vp_bfmfit_observe_ex;
csrc/raster_dense.hip: vp_raster_vertex_visibility): the C ABI's names and host-side refusals, the workspace query, known answers of the
visibility rule, the conditions the GPU fixtures were chosen for, and what each option buys, all on the numpy restatement
tests/bfm_observe_ref.py.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_appearance_ref as ar  # noqa: E402
import bfm_observe_ref as orf  # noqa: E402

NEW = {"vp_raster_vertex_visibility", "vp_bfmfit_observe_opts_size", "vp_bfmfit_observe_ex_workspace_bytes", "vp_bfmfit_observe_ex"}
YAWS = (0.0, 0.6, -0.6)
MARGIN = 1e-4


def opts(lib_module, visibility=1, ss=2, prefilter=1, tol=0.01, struct_bytes=None):
  o = lib_module.BfmObserveOpts()
  o.struct_bytes = ctypes.sizeof(lib_module.BfmObserveOpts) if struct_bytes is None else struct_bytes
  o.visibility, o.raster_scale, o.prefilter, o.depth_tol = visibility, ss, prefilter, tol
  return o


def test_abi_exports_and_refusals():
  """The header declares the new names and the library exports them; every refusal happens on the host, before anything is enqueued (no
  device is touched: the pointers are host dummies)."""
  from voicepuppet_amd import _lib
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vp_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header))
  assert NEW <= declared and NEW <= set(_lib.exported_symbols())
  assert "vp_bfmfit_observe_opts" in header and "bfm_observe.hip" in open(os.path.join(ROOT, "voicepuppet_amd", "csrc", "Makefile")).read()
  lib = _lib.lib()
  for name in NEW:
    assert getattr(lib, name).argtypes is not None, name
  assert lib.vp_bfmfit_observe_opts_size() == ctypes.sizeof(_lib.BfmObserveOpts) == 20
  buf = (ctypes.c_ubyte * 4096)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  m = _lib.BfmModel()
  m.nver, m.ntri = 252, 442
  for k in ("meanshape", "idBase", "exBase", "meantex", "texBase", "tri", "point_buf"):
    setattr(m, k, ctypes.addressof(buf))
  big = 1 << 40
  good = opts(_lib)

  def ex(frames=1, photo=p, pf=1, h=96, w=128, ws=big, o=good, model=m):
    return lib.vp_bfmfit_observe_ex(ctypes.byref(model), p, p, frames, photo, pf, h, w, p, None, p, p, p, p, ws, None,
                                    ctypes.byref(o) if o is not None else None, None)

  def size(o, nver=252, ntri=442, frames=1):
    return lib.vp_bfmfit_observe_ex_workspace_bytes(nver, ntri, frames, ctypes.byref(o) if o is not None else None)

  bad_opts = {"struct_bytes": opts(_lib, struct_bytes=16), "raster_scale 3": opts(_lib, ss=3), "raster_scale 0": opts(_lib, ss=0),
              "raster_scale 8": opts(_lib, ss=8), "depth_tol < 0": opts(_lib, tol=-1e-3), "depth_tol nan": opts(_lib, tol=float("nan")),
              "depth_tol inf": opts(_lib, tol=float("inf")), "visibility 2": opts(_lib, visibility=2), "prefilter -1": opts(_lib, prefilter=-1)}
  for what, o in bad_opts.items():
    assert ex(o=o) == -1, what
    msg = lib.vp_last_error()
    assert b"vp_bfmfit_observe_ex" in msg and b"options" in msg, (what, msg)
    assert size(o) == 0, what
  assert ex(o=bad_opts["struct_bytes"]) == -1 and b"struct_bytes 16" in lib.vp_last_error()
  assert ex(o=bad_opts["raster_scale 3"]) == -1 and b"raster_scale 3" in lib.vp_last_error()
  assert ex(o=bad_opts["depth_tol < 0"]) == -1 and b"depth_tol" in lib.vp_last_error()
  assert ex(o=None) == -1 and size(None) == 0
  # everything vp_bfmfit_observe refuses
  assert ex(frames=65536) == -1 and b"65535" in lib.vp_last_error()
  assert ex(frames=0) == -1 and ex(photo=None) == -1 and ex(h=1) == -1 and ex(w=1) == -1 and ex(pf=2) == -1
  empty = _lib.BfmModel()
  empty.nver, empty.ntri = 252, 442
  assert ex(model=empty) == -1
  assert size(good, nver=0) == 0 and size(good, ntri=0) == 0 and size(good, frames=0) == 0
  # a short workspace, for every combination of the options
  for vis in (0, 1):
    for pre in (0, 1):
      o = opts(_lib, visibility=vis, prefilter=pre)
      need = size(o)
      assert need > 0
      assert ex(ws=need - 1, o=o) == -1 and b"workspace" in lib.vp_last_error(), (vis, pre)
  # vp_raster_vertex_visibility
  vis = lambda nver=8, h=16, w=16, batch=1, tol=0.0, v=p, d=p, out=p: lib.vp_raster_vertex_visibility(v, d, out, nver, h, w, batch, tol, None)
  for kw in (dict(h=1), dict(w=1), dict(nver=0), dict(batch=0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(v=None),
             dict(d=None), dict(out=None)):
    assert vis(**kw) == -1, kw
    assert b"vp_raster_vertex_visibility" in lib.vp_last_error()


def test_workspace_is_linear_in_frames():
  """frames x (a per-frame size) + a constant: the raster buffers are those of one chunk of 8 frames whatever the clip's length, 28 bytes
  per pixel of the (224 ss)^2 raster (depth, triangle id, three weights, the rasteriser's 8-byte key)."""
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  size = lambda o, frames, nver=35709, ntri=70789: lib.vp_bfmfit_observe_ex_workspace_bytes(nver, ntri, frames, ctypes.byref(o))
  for ss in (1, 2, 4):
    for vis in (0, 1):
      o = opts(_lib, visibility=vis, ss=ss, prefilter=1)
      per = size(o, 2) - size(o, 1)
      raw = 8 * 3 * (35709 + 70790) + vis * 13 * 35709
      assert raw <= per < raw + 256, (ss, vis, per, raw)
      for frames in (3, 8, 9, 64, 250):
        assert size(o, frames) == size(o, 1) + (frames - 1) * per, (ss, vis, frames)
      const = size(o, 1) - per
      pixels = 8 * (224 * ss) ** 2
      print("ss %d visibility %d: %d bytes per frame + %d (%.1f MB)" % (ss, vis, per, const, const / 1e6))
      assert (const < 4096) if not vis else (28 * pixels <= const <= 28 * pixels + 4096)
  # without either option: vp_bfmfit_observe's arrays, nothing else
  plain = opts(_lib, visibility=0, prefilter=0)
  assert size(plain, 250) <= lib.vp_bfmfit_observe_workspace_bytes(35709, 70789, 250) + 250 * 256 + 512


def test_two_plate_known_answers():
  """The rule on hand-written depths: hidden, edge, empty pixel, off the buffer, NaN, and z + tol == m exactly."""
  v, tri, depth, expected = orf.two_plates()
  assert v.shape == (8, 3) and tri.shape == (4, 3) and depth.shape == (16, 16)
  vis, margin = orf.vertex_visibility(v, depth, orf.TWO_PLATES_TOL)
  print(vis, margin)
  assert np.array_equal(vis, expected) and vis.dtype == np.uint8
  assert margin[7] == 0.0 and np.isinf(margin[5]) and np.isinf(margin[6])
  half, _ = orf.vertex_visibility(v, depth, orf.TWO_PLATES_TOL / 2)
  assert half[7] == 0 and np.array_equal(half[:7], expected[:7])
  zero, _ = orf.vertex_visibility(v, depth, 0.0)
  assert np.array_equal(zero, half)
  # the hidden vertex comes back when the tolerance spans the gap between the plates
  assert orf.vertex_visibility(v, depth, 4.0)[0].all()


@pytest.fixture(scope="module")
def models():
  plain = orf.plain_model(14, 18)
  nose, height = orf.nose_model(14, 18)
  return {"plain": plain, "nose": nose, "height": height}


def test_fixture_conditions(models):
  """What the pose (bfm_observe_ref.POSE_T) was chosen for, asserted from the restatement alone: the convex model hides no camera-facing
  vertex at yaw 0 and +-0.6; the nose hides at least 5 at +-0.6 (10 of 216 at every setting below); no vertex of any case lies within 1e-4
  of the visibility threshold |z + tol - m| or of a pixel boundary, so a float32 rounding difference cannot flip a result."""
  worst_t, worst_p = np.inf, np.inf
  for name in ("plain", "nose"):
    fm = models[name]
    for yaw in YAWS:
      c = orf.pose_coeff(yaw)
      nz = orf.facing(fm, c)
      assert np.abs(nz).min() >= 1e-6
      for ss in (1, 2):
        rv = orf.raster_vertices(fm, c, ss)
        depth, _, _ = orf.depth_raster(fm, rv, ss)
        pm = orf.pixel_margin(rv, 224 * ss)
        for tol in (0.0, 0.01):
          vis, margin = orf.vertex_visibility(rv, depth, tol)
          hidden = int(((vis == 0) & (nz > 0)).sum())
          print("%s yaw %+.1f ss %d tol %.2f: %d camera-facing, %d of them hidden (%d hidden in all); threshold margin %.3e, pixel margin %.3e"
                % (name, yaw, ss, tol, int((nz > 0).sum()), hidden, int((vis == 0).sum()), margin.min(), pm))
          worst_t, worst_p = min(worst_t, margin.min()), min(worst_p, pm)
          if name == "plain":
            assert hidden == 0
          elif yaw != 0.0:
            assert hidden >= 5
          else:
            assert hidden == 0
  print("worst threshold margin %.3e, worst pixel margin %.3e" % (worst_t, worst_p))
  assert worst_t >= MARGIN and worst_p >= MARGIN


def occluder_case(models, yaw=0.6):
  """The painted-occluder photo: the nose model's own colours at the truth p*, the bump's vertices 80 grey levels brighter."""
  fm = models["nose"]
  c = orf.pose_coeff(yaw, seed=11)
  extra = np.where(models["height"] > 0.2, 80.0, 0.0)
  return fm, c, orf.painted_photo(fm, c, extra), np.array([1.0, 0.0, 0.0]), extra


def test_visibility_lowers_the_data_term_at_the_truth(models):
  """A 224 x 224 photo (a = 1) painted from the nose model's own colours T(delta*) L(gamma*) at yaw 0.6, the bump's vertices 80 grey levels
  brighter (an occluder whose colour the model does not predict).  The far cheek's vertices behind the nose sample the nose.  Data term
  at the truth, bfm_appearance_ref.data_term(fm, obs, p*): 567.61 without the visibility test, 537.63 with it (10 of 216 camera-facing
  vertices dropped); what is left is the bump's own +80 and the interpolation of the painting."""
  fm, c, photo, aff, extra = occluder_case(models)
  assert int((extra > 0).sum()) >= 6
  p_star = ar.coeff_to_p(c)
  without = orf.observe_ex(fm, c, photo, aff)
  with_vis = orf.observe_ex(fm, c, photo, aff, visibility=True, ss=2, tol=0.01)
  dropped = int(((without[1] > 0) & (with_vis[1] == 0)).sum())
  e0, e1 = ar.data_term(fm, without[:3], p_star), ar.data_term(fm, with_vis[:3], p_star)
  print("data term at the truth: %.4f without, %.4f with visibility; %d of %d weighted vertices dropped" % (e0, e1, dropped, int((without[1] > 0).sum())))
  assert dropped >= 5 and np.array_equal(without[0], with_vis[0]) and np.array_equal(without[2], with_vis[2])
  assert e1 < e0


PREFILTER_SHARE = 0.02


def test_prefilter_is_nearer_to_the_area_mean(models):
  """a = 4.3 on a 1024 x 1024 photo: a smooth field plus a +-40 checkerboard of 1 px period.  The exact area mean of the photo over a
  vertex's 4.3 x 4.3 pixels is the smooth field's (the checkerboard cancels to within a boundary row).  The 5 x 5 pre-filtered observation
  is nearer to it than the single tap for every inside vertex but a share of at most PREFILTER_SHARE = 2 % (measured: 1 of 252; RMS distance
  from the area mean 0.22 grey levels against 13.2 for the single tap).  A single tap at a non-integer position keeps up to the full +-40."""
  fm = models["plain"]
  c = orf.pose_coeff(0.0, seed=11)
  photo, field = orf.checkerboard_photo(1024, 1024)
  aff = np.array([4.3, 20.0, 30.0])
  _, proj = ar.geometry(fm, c, orf.rotation_of(c))
  px, py = aff[0] * proj[:, 0] + aff[1], aff[0] * proj[:, 1] + aff[2]
  single, inside = ar.bilinear(photo, px, py)
  filtered, inside2 = orf.prefiltered(photo, px, py, aff[0])
  assert orf.filter_taps(4.3) == 5 and orf.filter_taps(0.7) == 1 and orf.filter_taps(1.0) == 1 and orf.filter_taps(17.0) == 16 and orf.filter_taps(16.2) == 16
  assert np.array_equal(inside, inside2) and inside.sum() >= 200
  exact = orf.area_mean(field, px[inside], py[inside], aff[0])
  d_single = np.abs(single[inside] - exact).max(axis=1)
  d_filtered = np.abs(filtered[inside] - exact).max(axis=1)
  worse = int((d_filtered >= d_single).sum())
  print("inside %d; pre-filter not nearer for %d; RMS distance from the area mean: single tap %.3f, pre-filtered %.3f grey levels"
        % (inside.sum(), worse, np.sqrt((d_single ** 2).mean()), np.sqrt((d_filtered ** 2).mean())))
  assert worse <= PREFILTER_SHARE * inside.sum()
  # a <= 1: the single tap's bits
  small = orf.prefiltered(photo, px / 4.3, py / 4.3, 0.9)[0]
  assert np.array_equal(small, ar.bilinear(photo, px / 4.3, py / 4.3)[0])


def test_cli_options_default_off():
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  from voicepuppet_amd.datasets import make_triptychs as mt
  o, _ = fl.parse_options(["--photo", "lm.txt", "--image", "face.jpg", "--out", "photo.npz"])
  assert o.visibility is False and o.prefilter is False
  o, _ = fl.parse_options(["--photo", "lm.txt", "--image", "face.jpg", "--out", "photo.npz", "--visibility", "--prefilter"])
  assert o.visibility is True and o.prefilter is True
  o, _ = mt.parse_options(["--clip_dir", "c", "--landmarks", "l", "--out_dir", "o"])
  assert o.appearance_visibility is False and o.appearance_prefilter is False and o.appearance == "first"
  o, _ = mt.parse_options(["--clip_dir", "c", "--landmarks", "l", "--out_dir", "o", "--appearance_visibility", "--appearance_prefilter"])
  assert o.appearance_visibility is True and o.appearance_prefilter is True


def test_python_signatures():
  """The options are keyword arguments that default to off; the documentation no longer says they are left out."""
  import inspect
  from voicepuppet_amd import bfmfit
  from voicepuppet_amd.utils import mesh_core
  sig = inspect.signature(bfmfit.FaceFitter.observe).parameters
  assert [sig[k].default for k in ("visibility", "prefilter", "raster_scale", "depth_tol", "return_visible")] == [False, False, 2, 0.01, False]
  for fn in (bfmfit.FaceFitter.fit_appearance, bfmfit.FaceFitter.enroll):
    s = inspect.signature(fn).parameters
    assert s["visibility"].default is False and s["prefilter"].default is False
  assert "a default, not a tuned value" in " ".join(bfmfit.FaceFitter.observe.__doc__.split())
  assert list(inspect.signature(mesh_core.vertex_visibility).parameters) == ["vertices", "depth_buffer", "tol", "out"]
  for path in ("include/vp_hip.h", "voicepuppet_amd/bfmfit.py"):
    text = open(os.path.join(ROOT, path)).read()
    assert "Left out: self-occlusion" not in text and "No self-occlusion test and no pre-filter" not in text, path

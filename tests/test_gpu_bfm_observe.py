"""FaceFitter.observe's self-occlusion test and area pre-filter on the device (csrc/bfm_observe.hip: vp_bfmfit_observe_ex;
csrc/raster_dense.hip: vp_raster_vertex_visibility; mesh_core.vertex_visibility) against the numpy restatement tests/bfm_observe_ref.py.
The fixtures are those of tests/test_bfm_observe_host.py, whose test_fixture_conditions shows that no vertex lies within 1e-4 of a
threshold: a float32 rounding difference between the device's raster vertices and numpy's (one ulp at 448 is 3e-5) cannot flip a result.

Tolerances: the 0 / 1 masks and the weights are compared exactly; a pre-filtered observation is a float64 sum of <= 256 terms <= 255 in
another order than numpy's, 1e-9 relative; the fit is judged as tests/test_gpu_bfm_appearance.py judges (its `judge`)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bfm_appearance_ref as ar  # noqa: E402
import bfm_fit_ref as fr  # noqa: E402
import bfm_observe_ref as orf  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YAWS = (0.6, -0.6, 0.0)
MARGIN = 1e-4


@pytest.fixture(scope="module")
def ctx():
  import torch
  from voicepuppet_amd.bfmfit import FaceFitter
  plain = orf.plain_model(14, 18)
  nose, height = orf.nose_model(14, 18)
  coeff = np.stack([orf.pose_coeff(y, seed=11) for y in YAWS])
  extra = np.where(height > 0.2, 80.0, 0.0)
  photo = orf.painted_photo(nose, coeff[0], extra)                     # the painted occluder of the host test, yaw 0.6
  return {"torch": torch, "plain": plain, "nose": nose, "coeff": coeff, "photo": photo, "fit_nose": FaceFitter(nose), "fit_plain": FaceFitter(plain),
          "ref_vis": {}}


def ref_visibility(ctx, row, ss, tol=0.01):
  """The restatement's (mask, margin) for fixture row `row` of the nose model, once per (row, ss, tol)."""
  key = (row, ss, tol)
  if key not in ctx["ref_vis"]:
    rv = orf.raster_vertices(ctx["nose"], ctx["coeff"][row], ss)
    depth, _, _ = orf.depth_raster(ctx["nose"], rv, ss)
    ctx["ref_vis"][key] = orf.vertex_visibility(rv, depth, tol)
  return ctx["ref_vis"][key]


def batch(a, frames):
  return np.stack([a[i % len(a)] for i in range(frames)])


def observe_ex_raw(fitter, coeff, photo, affine, visibility, prefilter, ss=2, tol=0.01):
  """vp_bfmfit_observe_ex itself (FaceFitter.observe takes vp_bfmfit_observe when both options are off)."""
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd._handle import ptr, stream
  from voicepuppet_amd.utils.reconstruct_mesh import Compute_rotation_matrix
  dev, N = fitter.model.device, fitter.model.nver
  T = coeff.shape[0]
  c = torch.from_numpy(np.ascontiguousarray(coeff, np.float32)).to(dev)
  rot = torch.from_numpy(Compute_rotation_matrix(np.asarray(coeff[:, 224:227], np.float32))).to(dev)
  img = torch.from_numpy(np.ascontiguousarray(photo)).to(dev)
  aff = torch.from_numpy(np.ascontiguousarray(affine, np.float64)).to(dev)
  sh = torch.empty(T, N, 9, dtype=torch.float64, device=dev)
  weight = torch.empty(T, N, dtype=torch.float64, device=dev)
  observed = torch.empty(T, N, 3, dtype=torch.float64, device=dev)
  visible = torch.full((T, N), 7, dtype=torch.uint8, device=dev)
  o = _lib.BfmObserveOpts(ctypes.sizeof(_lib.BfmObserveOpts), visibility, ss, prefilter, tol)
  n = _lib.lib().vp_bfmfit_observe_ex_workspace_bytes(N, fitter.model.ntri, T, ctypes.byref(o))
  ws = torch.empty(n, dtype=torch.uint8, device=dev)
  _lib.check(_lib.lib().vp_bfmfit_observe_ex(ctypes.byref(fitter.model.c), ptr(c), ptr(rot), T, ptr(img), 1, photo.shape[0], photo.shape[1], ptr(aff),
                                             None, ptr(sh), ptr(weight), ptr(observed), ptr(ws), n, stream(), ctypes.byref(o), ptr(visible)),
             "vp_bfmfit_observe_ex")
  torch.cuda.synchronize()
  return sh.cpu().numpy(), weight.cpu().numpy(), observed.cpu().numpy(), visible.cpu().numpy()


def test_vertex_visibility_two_plates(ctx):
  torch = ctx["torch"]
  from voicepuppet_amd.utils import mesh_core
  v, _, depth, expected = orf.two_plates()
  dv, dd = torch.from_numpy(v[None]).cuda(), torch.from_numpy(depth[None]).cuda()
  for tol in (orf.TWO_PLATES_TOL, orf.TWO_PLATES_TOL / 2, 0.0, 4.0):
    got = mesh_core.vertex_visibility(dv, dd, tol=tol).cpu().numpy()[0]
    want, _ = orf.vertex_visibility(v, depth, tol)
    print("tol %.3f: %s" % (tol, got))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
  assert np.array_equal(mesh_core.vertex_visibility(dv, dd, tol=orf.TWO_PLATES_TOL).cpu().numpy()[0], expected)
  out = torch.zeros(1, 8, dtype=torch.uint8, device="cuda")
  assert mesh_core.vertex_visibility(dv, dd, tol=0.0, out=out) is out
  with pytest.raises(RuntimeError):
    mesh_core.vertex_visibility(dv, dd, tol=-1.0)
  with pytest.raises(RuntimeError):
    mesh_core.vertex_visibility(dv, dd[:, :1], tol=0.0)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("ss", [1, 2])
def test_vertex_visibility_nose(ctx, ss, frames):
  """The kernel on the device's own float32 inputs - raster vertices from reconstruct_view's float64 projection, the depth buffer the
  device's rasteriser left - byte-equal to the restatement on the same arrays; a row is the same in any batch."""
  torch = ctx["torch"]
  from voicepuppet_amd.utils import mesh_core
  from voicepuppet_amd.utils.reconstruct_mesh import reconstruct_view
  fitter = ctx["fit_nose"]
  out = reconstruct_view(ctx["coeff"][:frames], fitter.model)
  rv = torch.cat([ss * out["face_projection"], out["z_buffer"]], dim=2).to(torch.float32).contiguous()
  if ss == 1:
    assert torch.equal(rv, out["vertices"])                           # what view 0 packs
  side = 224 * ss
  depth = torch.full((frames, side, side), float(orf.DEPTH_CLEAR), dtype=torch.float32, device="cuda")
  ids = torch.full((frames, side, side), -1, dtype=torch.int32, device="cuda")
  bary = torch.zeros(frames, side, side, 3, dtype=torch.float32, device="cuda")
  tri = torch.from_numpy((np.asarray(ctx["nose"].tri) - 1).astype(np.int32)).cuda()
  mesh_core.rasterize_triangles(rv, tri, depth, ids, bary)
  for tol in (0.0, 0.01):
    got = mesh_core.vertex_visibility(rv, depth, tol=tol).cpu().numpy()
    for f in range(frames):
      want, margin = orf.vertex_visibility(rv[f].cpu().numpy(), depth[f].cpu().numpy(), tol)
      nz = orf.facing(ctx["nose"], ctx["coeff"][f])
      print("ss %d frame %d tol %.2f: %d hidden, %d of them camera-facing; margin %.3e" % (ss, f, tol, int((want == 0).sum()),
                                                                                           int(((want == 0) & (nz > 0)).sum()), margin.min()))
      assert np.array_equal(got[f], want)
      if YAWS[f] != 0.0:
        assert int(((want == 0) & (nz > 0)).sum()) >= 5
    if frames == 3:
      alone = mesh_core.vertex_visibility(rv[1:2].contiguous(), depth[1:2].contiguous(), tol=tol).cpu().numpy()
      assert np.array_equal(alone[0], got[1])


@pytest.mark.parametrize("frames", [1, 11])
def test_observe_ex_options_off_is_observe(ctx, frames):
  """visibility = prefilter = 0: the three outputs are vp_bfmfit_observe's bits (and `visible` is not written); prefilter = 1 at a <= 1
  likewise."""
  fitter = ctx["fit_nose"]
  c = batch(ctx["coeff"], frames)
  photo = ar.smooth_photo()
  aff = np.stack([np.array([0.55 + 0.01 * (i % 6), 2.4 + 0.7 * (i % 6), -13.6]) for i in range(frames)])
  plain = [t.cpu().numpy() for t in fitter.observe(c, photo, aff)]
  assert np.any(plain[1] > 0) and np.any(plain[1] == 0)
  for prefilter in (0, 1):
    sh, w, obs, vis = observe_ex_raw(fitter, c, photo, aff, 0, prefilter)
    for a, b in zip(plain, (sh, w, obs)):
      assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.all(vis == 7)
  again = [t.cpu().numpy() for t in fitter.observe(c, photo, aff, prefilter=True)]
  for a, b in zip(plain, again):
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("frames", [3, 11])
@pytest.mark.parametrize("ss", [1, 2])
def test_observe_visibility(ctx, ss, frames):
  """visible = the restatement's mask; weight = vp_bfmfit_observe's weight times the mask, bit for bit; sh and observed untouched.  11
  frames are two chunks of the raster buffers.  A flip is tolerated only where the restatement's own margin is below 1e-4: nowhere."""
  fitter = ctx["fit_nose"]
  c = batch(ctx["coeff"], frames)
  aff = np.tile(np.array([1.0, 0.0, 0.0]), (frames, 1))
  plain = [t.cpu().numpy() for t in fitter.observe(c, ctx["photo"], aff)]
  sh, w, obs, vis = (t.cpu().numpy() for t in fitter.observe(c, ctx["photo"], aff, visibility=True, raster_scale=ss, return_visible=True))
  assert vis.dtype == np.uint8 and vis.shape == (frames, 252)
  for f in range(frames):
    want, margin = ref_visibility(ctx, f % 3, ss)
    flips = np.flatnonzero(vis[f] != want)
    print("ss %d frame %d: %d hidden, %d flips, smallest margin %.3e" % (ss, f, int((want == 0).sum()), len(flips), margin.min()))
    assert margin.min() >= MARGIN
    assert np.all(margin[flips] < MARGIN)                             # (empty, by the line above)
    assert np.array_equal(w[f].view(np.uint64), (plain[1][f] * vis[f].astype(np.float64)).view(np.uint64))
    if YAWS[f % 3] != 0.0:
      assert int(((plain[1][f] > 0) & (w[f] == 0)).sum()) >= 5
  assert np.array_equal(sh.view(np.uint64), plain[0].view(np.uint64)) and np.array_equal(obs.view(np.uint64), plain[2].view(np.uint64))
  three = fitter.observe(c, ctx["photo"], aff, visibility=True, raster_scale=ss)
  assert len(three) == 3 and np.array_equal(three[1].cpu().numpy(), w)
  with pytest.raises(ValueError):
    fitter.observe(c, ctx["photo"], aff, visibility=True, raster_scale=3)
  with pytest.raises(ValueError):
    fitter.observe(c, ctx["photo"], aff, return_visible=True)


PREFILTER_CASES = {0.7: dict(shape=(96, 128), k=1, affine=(0.7, 2.4, -13.6), frames=3),
                   4.3: dict(shape=(1024, 1024), k=5, affine=(4.3, 20.0, -150.0), frames=3),
                   17.0: dict(shape=(3400, 3400), k=16, affine=(17.0, -250.5, -300.25), frames=1)}


@pytest.mark.parametrize("a", sorted(PREFILTER_CASES))
def test_observe_prefilter(ctx, a):
  """observed within 1e-9 relative of the restatement's k x k mean (float64 sums of <= 256 terms <= 255 in another order); sh and weight
  are vp_bfmfit_observe's bits; at a <= 1 so is observed; a frame's numbers are the same bits alone and in a batch.  Noise photos: every
  tap matters."""
  case = PREFILTER_CASES[a]
  fitter = ctx["fit_plain"]
  frames = case["frames"]
  assert orf.filter_taps(a) == case["k"]
  photo = np.random.default_rng(int(a * 10)).integers(0, 256, size=case["shape"] + (3,), dtype=np.uint8)
  c = batch(ctx["coeff"], frames)
  aff = np.tile(np.array(case["affine"]), (frames, 1))
  plain = [t.cpu().numpy() for t in fitter.observe(c, photo, aff)]
  sh, w, obs = (t.cpu().numpy() for t in fitter.observe(c, photo, aff, prefilter=True))
  assert np.array_equal(sh.view(np.uint64), plain[0].view(np.uint64)) and np.array_equal(w.view(np.uint64), plain[1].view(np.uint64))
  for f in range(frames):
    _, _, want, _, _ = orf.observe_ex(ctx["plain"], c[f], photo, aff[f], prefilter=True)
    inside = np.abs(want).sum(axis=1) > 0
    rel = np.abs(obs[f] - want) / np.maximum(np.abs(want), 1.0)
    print("a %.1f frame %d: k %d, %d inside, %d outside; worst relative difference %.3e; differs from the single tap at %d vertices"
          % (a, f, case["k"], int(inside.sum()), int((~inside).sum()), rel.max(), int((obs[f] != plain[2][f]).any(axis=1).sum())))
    assert rel.max() <= 1e-9
    assert np.all(obs[f][~inside] == 0) and inside.sum() >= 100
    if a <= 1:
      assert np.array_equal(obs[f].view(np.uint64), plain[2][f].view(np.uint64))
    else:
      assert (obs[f] != plain[2][f]).any(axis=1).sum() >= 0.9 * inside.sum()
  if a == 4.3:
    assert (np.abs(obs).sum(axis=2) == 0).any()                          # this case pushes vertices off the photo's top
  if frames > 1:
    alone = fitter.observe(c[1:2], photo, aff[1:2], prefilter=True)[2].cpu().numpy()
    assert np.array_equal(alone[0].view(np.uint64), obs[1].view(np.uint64))
  if a == 4.3:                                                           # a per-frame scale: frame 1 keeps its single tap
    mixed = aff.copy()
    mixed[1] = (0.9, 20.0, 5.0)
    m_plain = fitter.observe(c, photo, mixed)[2].cpu().numpy()
    m_obs = fitter.observe(c, photo, mixed, prefilter=True)[2].cpu().numpy()
    assert np.array_equal(m_obs[1].view(np.uint64), m_plain[1].view(np.uint64)) and np.array_equal(m_obs[0].view(np.uint64), obs[0].view(np.uint64))


def test_fit_appearance_with_visibility(ctx):
  """The painted-occluder photo (tests/test_bfm_observe_host.py): fit_appearance(visibility=True) from zero texture and lighting reaches
  the restatement's fit on the restatement's observation within tests/test_gpu_bfm_appearance.py's two bounds (stationarity, agreement
  with p*), and its observation has the lower data term at the truth than the default path's."""
  from test_gpu_bfm_appearance import judge
  fm, fitter = ctx["nose"], ctx["fit_nose"]
  truth = ctx["coeff"][:1]
  p_star = ar.coeff_to_p(truth[0])
  start = truth.copy()
  start[:, 144:224] = 0
  start[:, 227:254] = 0
  aff = np.array([[1.0, 0.0, 0.0]])
  want = orf.observe_ex(fm, start[0], ctx["photo"], aff[0], visibility=True)

  class Case:
    pass
  case = Case()
  case.fm, case.star = fm, {}
  coeff, report = fitter.fit_appearance(start, photo=ctx["photo"], affine=aff, visibility=True)
  p = fitter.last_appearance.cpu().numpy()
  report = report.cpu().numpy()
  print(report)
  assert report[0, 0] == 0
  judge(case, "occluder", 0, want[:3], p[0], ar.coeff_to_p(start[0]))
  dev_vis = [t.cpu().numpy()[0] for t in fitter.observe(start, ctx["photo"], aff, visibility=True)]
  dev_plain = [t.cpu().numpy()[0] for t in fitter.observe(start, ctx["photo"], aff)]
  e_vis, e_plain = ar.data_term(fm, dev_vis, p_star), ar.data_term(fm, dev_plain, p_star)
  _, report_plain = fitter.fit_appearance(start, photo=ctx["photo"], affine=aff)
  print("data term at the truth: %.4f with visibility, %.4f without; fitted E %.4f / %.4f" % (e_vis, e_plain, report[0, 2], report_plain.cpu().numpy()[0, 2]))
  assert e_vis < e_plain


def photo_case():
  g = dict(np.load(os.path.join(GOLDEN, "bfm_fit.npz")))
  xy = fr.photo_landmarks(g["landmarks_2d"][0], 1.7, (130.0, 60.0))
  return g, xy, ar.smooth_photo(480, 640, seed=5)


def test_enroll_with_options(ctx):
  """enroll(image=, visibility=True, prefilter=True) returns the documented dictionary: the geometry columns are enroll()'s, texture and
  lighting are those of fit_appearance with the same options; with the options off nothing changes."""
  from voicepuppet_amd import bfmfit
  fitter = ctx["fit_plain"]
  g, xy, image = photo_case()
  plain = fitter.enroll(xy, 480, 640, g["lm3d68"], image=image)
  off = fitter.enroll(xy, 480, 640, g["lm3d68"], image=image, visibility=False, prefilter=False)
  got = fitter.enroll(xy, 480, 640, g["lm3d68"], image=image, visibility=True, prefilter=True)
  rep = fitter.last_appearance_report.cpu().numpy()
  print("enroll with both options: appearance report", rep)
  assert set(got) == {"bfmcoeff", "transform_params", "center_x", "center_y", "ratio"} and rep.shape == (1, 4) and rep[0, 0] in (0, 1, 2)
  assert got["bfmcoeff"].shape == (1, 257) and got["bfmcoeff"].dtype == np.float32
  assert np.array_equal(off["bfmcoeff"].view(np.uint32), plain["bfmcoeff"].view(np.uint32))
  for k in ("transform_params", "center_x", "center_y", "ratio"):
    assert np.array_equal(got[k], plain[k])
  assert np.array_equal(got["bfmcoeff"][:, :144], plain["bfmcoeff"][:, :144]) and np.array_equal(got["bfmcoeff"][:, 224:227], plain["bfmcoeff"][:, 224:227])
  aff = bfmfit.photo_affine(xy, 480, 640, g["lm3d68"])
  assert aff[0] > 1.0                                                 # the pre-filter has work to do
  lm_new, _ = bfmfit.preprocess_landmarks(bfmfit.crop_alignment(xy, 480, 640)[0], g["lm3d68"])
  coeff, _ = fitter.fit(lm_new.reshape(1, 68, 2))
  coeff, _ = fitter.fit_appearance(coeff, photo=image, affine=aff, visibility=True, prefilter=True)
  assert np.array_equal(got["bfmcoeff"].view(np.uint32), coeff.cpu().numpy().view(np.uint32))
  assert np.any(got["bfmcoeff"][:, 144:224] != plain["bfmcoeff"][:, 144:224])


def test_cli_with_options(ctx, tmp_path, monkeypatch, capsys):
  """fit_landmarks.py --photo LANDMARKS --image FILE --visibility --prefilter, files in a temporary directory: the npz is bit-equal to
  enroll(image=, visibility=True, prefilter=True) on the decoded pixels."""
  from PIL import Image
  from voicepuppet_amd.bfmnet import fit_landmarks as fl
  from test_gpu_bfm_fit import write_bfm_assets
  monkeypatch.chdir(tmp_path)
  g, xy, image = photo_case()
  write_bfm_assets(ctx["plain"], g["lm3d68"])
  np.savetxt("landmarks.txt", xy.reshape(1, 136), delimiter=",", fmt="%.10f")
  Image.fromarray(image).save("photo.png")
  fl.main(["--photo", "landmarks.txt", "--image", "photo.png", "--out", "photo.npz", "--visibility", "--prefilter"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  assert "1 frames" in line and "appearance status " in line
  got = np.load("photo.npz")
  lms = np.loadtxt("landmarks.txt", delimiter=",").reshape(68, 2)
  want = ctx["fit_plain"].enroll(lms, 480, 640, g["lm3d68"], image=image, visibility=True, prefilter=True)
  assert set(got.files) == set(want) and np.array_equal(got["bfmcoeff"].view(np.uint32), want["bfmcoeff"].view(np.uint32))
  default = ctx["fit_plain"].enroll(lms, 480, 640, g["lm3d68"], image=image)
  assert not np.array_equal(got["bfmcoeff"], default["bfmcoeff"])

"""The trimap and the closed-form matting solve on the device (voicepuppet_amd.matte_solve.MatteSolver, csrc/matte_solve.hip) against the
numpy restatement tests/matte_solve_ref.py, which tests/test_matte_solve_host.py pins: the trimap byte for byte, the single Laplacian
op and the solve within tolerances measured with the restatement itself (E and S below), then batch and order independence in bits,
views, the degenerate clauses, refusals, and the dataset launcher end to end."""
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
import matte_solve_ref as sr  # noqa: E402
from oracle import bfm_ref as br  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_fit.npz")
# (n, H, W): one tile and less; 3 x 3 ragged tiles; odd sizes; one tile row / column; 8 x 8 tiles (the solve and the trimap only)
SIZES = [(1, 16, 16), (3, 96, 80), (5, 33, 47), (1, 17, 64), (1, 64, 17)]
BIG = (2, 256, 256)
# E: the largest difference between the restatement's Laplacian in float64 and in numpy.longdouble (x87, 64-bit mantissa), relative to
# max |L p|, over SIZES and BIG, the first two frames of each, radius 1 2 3, eps 1, p a standard normal plane and p = k: 1.336e-12
# (256 x 256, radius 3).  The device is held to 16 E of the float64 restatement: it sums the same terms in another association.
E = 1.336e-12
# S: over every frame of SIZES and BIG at radius 1, eps 1, tol 1e-6, the larger of (a) the restatement's spread in alpha over three
# dot-product orders (numpy.sum, math.fsum, a running sum): 1.694e-6 at most (17 x 64), no matte byte differs between them; (b) the
# distance of the fsum run from the restatement's own tol = 1e-12 solution: 3.221e-5 at most (33 x 47, frame 0).  The device is held to
# 8 S of the fsum run: 2.6e-4, 0.066 of a matte level.
S = 3.221e-5
TOL = 1e-6


def _freeze(res):
  for a in res:
    a.setflags(write=False)
  return res


@functools.lru_cache(maxsize=None)
def _scene(n, H, W):
  """frames, the true alpha, KeyMatte's matte and the cleaned matte (both the restatements'), the trimap of the cleaned matte: read-only"""
  frames, alpha, _ = mr.scene(H, W, seed=H * 1000 + W, n=n, spill_levels=10.0)
  _, model = kr.fit(frames)
  _, matte = kr.matte(model, frames)
  cleaned, _, _ = mr.clean(matte, mr.landmarks(H, W, n))
  return _freeze((frames, alpha, matte, cleaned, sr.trimap(cleaned)))


@functools.lru_cache(maxsize=None)
def _want(n, H, W, radius=1, iters=256, tol=TOL):
  frames, _, _, _, tri = _scene(n, H, W)
  alpha, matte, rep = sr.solve(frames, tri, radius=radius, eps=1.0, iters=iters, tol=tol)
  return _freeze((alpha, matte)) + (rep,)


@functools.lru_cache(maxsize=None)
def _solver():
  from voicepuppet_amd.matte_solve import MatteSolver
  return MatteSolver(5, 256, 256, max_radius=3)


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the cached references are read-only)


def _solve(frames, tri, solver=None, **kw):
  """-> (alpha float64 [n, H, W], matte uint8, report) of the device, as host arrays"""
  s = solver or _solver()
  n, H, W = tri.shape
  out = s.solve(_dev(frames), _dev(tri), **kw)
  rep = s.report()
  alpha = s.tensor("alpha")
  assert tuple(alpha.shape) == (s.max_frames, H, W) and len(rep["status"]) == n
  return alpha[:n].cpu().numpy(), out.cpu().numpy(), rep


# ---- trimap -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [BIG])
def test_trimap_equals_the_restatement(size):
  """KeyMatte's matte, the cleaned matte, a 0 / 255 mask and random blobs; the default squares, even and odd ones, 1 and 64"""
  n, H, W = size
  _, _, matte, cleaned, tri = _scene(*size)
  s = _solver()
  binary = np.where(cleaned >= 128, 255, 0).astype(np.uint8)
  blobs = np.stack([mr.blobs(H, W, seed=f) for f in range(n)])
  for name, m in (("key", matte), ("cleaned", cleaned), ("binary", binary), ("blobs", blobs)):
    for kw in ({}, dict(erode=4, dilate=7), dict(erode=1, dilate=1), dict(erode=64, dilate=64), dict(erode=9, dilate=2, support=100, core=101)):
      if size == BIG and kw and name != "cleaned":
        continue
      got = s.trimap(_dev(m), **kw).cpu().numpy()
      want = sr.trimap(m, **kw)
      assert np.array_equal(got, want), "%s %s %s: %d bytes differ" % (size, name, kw, int((got != want).sum()))
      tiles = s.tensor("tiles")[:n].cpu().numpy()
      ty, tx = (H + 31) // 32, (W + 31) // 32
      flags = np.array([[[(want[f, 32 * y:32 * y + 32, 32 * x:32 * x + 32] == 127).any() for x in range(tx)] for y in range(ty)] for f in range(n)])
      assert tiles.shape == (n, ty, tx) and np.array_equal(tiles != 0, flags), (size, name, kw)
  assert np.array_equal(sr.trimap(cleaned), tri) and set(np.unique(tri)) <= {0, 127, 255}


# ---- the single op ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_laplacian_is_within_16_e_of_the_restatement(size, radius):
  """Every element of L p for a random plane and for p = k, against the float64 restatement, in units of max |L p|.  E (above) is what
  float64 itself loses against numpy.longdouble in the restatement: 1.336e-12."""
  n, H, W = size
  frames, _, _, _, tri = _scene(*size)
  rng = np.random.default_rng(H * W + radius)
  for name, p in (("random", rng.standard_normal((n, H, W))), ("k", (tri == 255).astype(np.float64))):
    got = _solver().laplacian(_dev(frames), _dev(p), radius=radius, eps=1.0).cpu().numpy()
    for f in range(n):
      want = sr.Laplacian(frames[f], radius, 1.0).apply(p[f])
      err = np.abs(got[f] - want).max() / np.abs(want).max()
      print("%s radius %d %s frame %d: max |device - restatement| / max |L p| = %.3e (16 E = %.3e)" % (size, radius, name, f, err, 16 * E))
      assert err <= 16 * E, (size, radius, name, f, err)


# ---- the solve ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [BIG])
def test_solve_is_within_8_s_of_the_restatement(size):
  """alpha against the restatement's fsum run at the same tol (S above: 3.221e-5); the matte equal but for pixels within 8 S * 255 of a
  rounding boundary, at most 0.1 % of the band; the reported residual at most tol; at most one iteration more than the restatement."""
  n, H, W = size
  frames, truth, _, cleaned, tri = _scene(*size)
  want_alpha, want_matte, want_rep = _want(*size)
  alpha, matte, rep = _solve(frames, tri, tol=TOL)
  U = (tri != 0) & (tri != 255)
  for f in range(n):
    err = np.abs(alpha[f] - want_alpha[f]).max()
    print("%s frame %d: %d unknown, iterations %d (restatement %d), residual %.3e, max |alpha - restatement| %.3e (8 S = %.3e)"
          % (size, f, rep["unknown"][f], rep["iterations"][f], want_rep[f]["iterations"], rep["residual"][f], err, 8 * S))
    assert rep["unknown"][f] == want_rep[f]["unknown"] == U[f].sum() and rep["status"][f] == 0 == want_rep[f]["status"]
    assert err <= 8 * S
    assert rep["residual"][f] <= TOL and rep["iterations"][f] <= want_rep[f]["iterations"] + 1
    differ = matte[f] != want_matte[f]
    frac = want_alpha[f] * 255.0 + 0.5
    near = np.abs(frac - np.round(frac)) <= 8 * S * 255
    assert not (differ & ~near).any() and not differ[~U[f]].any() and differ.sum() <= 0.001 * U[f].sum(), (size, f, int(differ.sum()))
    assert np.abs(differ * (matte[f].astype(int) - want_matte[f])).max() <= 1
  assert np.array_equal(matte[~U], tri[~U]) and np.array_equal(alpha[~U], (tri[~U] == 255).astype(np.float64))
  if H >= 96:
    mae_c, mae_s = kr.quality(cleaned, truth)[0], kr.quality(matte, truth)[0]
    print("%s: matte MAE %.5f cleaned, %.5f solved" % (size, mae_c, mae_s))
    assert mae_s <= mae_c / 3


def test_radius_2_and_3_against_the_restatement():
  size = (3, 96, 80)
  frames, _, _, _, tri = _scene(*size)
  for radius in (2, 3):
    want_alpha, want_matte, want_rep = _want(*size, radius=radius)
    alpha, matte, rep = _solve(frames, tri, radius=radius, tol=TOL)
    err = np.abs(alpha - want_alpha).max()
    print("radius %d: iterations %s (restatement %s), max |alpha - restatement| %.3e" % (radius, rep["iterations"], [r["iterations"] for r in want_rep], err))
    assert err <= 8 * S and (rep["residual"] <= TOL).all() and not rep["status"].any()
    assert (rep["iterations"] <= np.array([r["iterations"] for r in want_rep]) + 1).all()
    assert np.abs(matte.astype(int) - want_matte).max() <= 1 and (matte != want_matte).sum() <= 0.001 * rep["unknown"].sum()


# ---- batch and order independence ---------------------------------------------------------------------------------------------------------
def test_a_frame_has_the_same_bits_alone_anywhere_in_a_batch_and_on_a_second_run():
  size = (5, 33, 47)
  frames, _, _, _, tri = _scene(*size)
  full = _solve(frames, tri)
  again = _solve(frames, tri)
  order = [4, 3, 2, 1, 0]
  moved = _solve(frames[order], tri[order])
  alone = _solve(frames[3:4], tri[3:4])
  assert full[2]["iterations"][3] > 10
  for other, at in ((again, 3), (moved, 1), (alone, 0)):
    assert np.array_equal(full[0][3].view(np.int64), other[0][at].view(np.int64)) and np.array_equal(full[1][3], other[1][at])
    assert full[2]["iterations"][3] == other[2]["iterations"][at] and full[2]["residual"][3] == other[2]["residual"][at]
  assert np.array_equal(full[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(full[2]["iterations"], again[2]["iterations"])


def test_a_batch_mixes_a_frame_that_stops_early_with_one_that_runs_to_iters():
  """frame 0: all of the band but four pixels made known (at most a handful of iterations); frame 1: the whole band, 12 iterations allowed"""
  frames, _, _, cleaned, tri = _scene(3, 96, 80)
  U = (tri[0] != 0) & (tri[0] != 255)
  ys, xs = np.nonzero(U[:-2, :-2] & (cleaned[0][:-2, :-2] >= 128))               # inside the subject: known-1 neighbours, b is not 0
  small = np.where(U, np.where(cleaned[0] >= 128, 255, 0), tri[0]).astype(np.uint8)
  mid = len(ys) // 2
  small[ys[mid]:ys[mid] + 2, xs[mid]:xs[mid] + 2] = 127
  f2, t2 = np.stack([frames[0], frames[1]]), np.stack([small, tri[1]])
  both = _solve(f2, t2, iters=12)
  assert 0 < both[2]["iterations"][0] < 12 and both[2]["residual"][0] <= TOL and both[2]["unknown"][0] == 4
  assert both[2]["iterations"][1] == 12 and both[2]["residual"][1] > TOL and not both[2]["status"].any()
  for f in range(2):
    alone = _solve(f2[f:f + 1], t2[f:f + 1], iters=12)
    assert np.array_equal(both[0][f].view(np.int64), alone[0][0].view(np.int64)) and np.array_equal(both[1][f], alone[1][0])
    assert both[2]["iterations"][f] == alone[2]["iterations"][0] and both[2]["residual"][f] == alone[2]["residual"][0]
  want = sr.solve_frame(frames[1], tri[1], iters=12, tol=TOL)
  assert want["iterations"] == 12 and np.abs(both[0][1] - want["alpha"]).max() <= 8 * S
  assert abs(both[2]["residual"][1] - want["residual"]) <= 1e-6 * want["residual"]


# ---- views, out, degenerate clauses -------------------------------------------------------------------------------------------------------
def test_padded_view_out_reuse_and_solving_into_the_trimap():
  import torch
  n, H, W = 3, 96, 80
  frames, _, _, _, tri = _scene(n, H, W)
  s = _solver()
  ref = _solve(frames, tri)
  padded = torch.full((n, H + 8, W + 16, 3), 201, dtype=torch.uint8, device="cuda")   # a JpegDecoder output: whole MCUs, a view of the image
  padded[:, :H, :W] = _dev(frames)
  view = padded[:, :H, :W]
  assert not view.is_contiguous()
  buf = torch.full((5, H, W), 77, dtype=torch.uint8, device="cuda")
  got = s.solve(view, _dev(tri), out=buf[1:])
  assert got.data_ptr() == buf[1].data_ptr() and np.array_equal(got.cpu().numpy(), ref[1]) and (buf[0] == 77).all() and (buf[4] == 77).all()
  assert np.array_equal(s.tensor("alpha")[:n].cpu().numpy().view(np.int64), ref[0].view(np.int64))
  t = _dev(tri)
  same = s.solve(view, t, out=t)
  assert same.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), ref[1])
  big = torch.cat([t, t])
  with pytest.raises(RuntimeError, match="overlaps"):                                 # the same buffer a frame further on
    s.solve(view, big[1:n + 1], out=big[:n])
  # a trimap of another size leaves the layout of the solution: "alpha" keeps the solve's extents, "tiles" takes the trimap's
  s.trimap(torch.zeros(2, 40, 70, dtype=torch.uint8, device="cuda"))
  assert tuple(s.tensor("alpha").shape) == (s.max_frames, H, W) and tuple(s.tensor("tiles").shape) == (s.max_frames, 2, 3)
  assert np.array_equal(s.tensor("alpha")[:n].cpu().numpy().view(np.int64), ref[0].view(np.int64))
  tbuf = torch.full((4, H, W), 9, dtype=torch.uint8, device="cuda")
  tri_dev = s.trimap(_dev(_scene(n, H, W)[3]), out=tbuf)
  assert tri_dev.data_ptr() == tbuf.data_ptr() and np.array_equal(tri_dev.cpu().numpy(), tri) and (tbuf[3] == 9).all()


def test_degenerate_clauses_and_a_band_on_the_frames_edge():
  H, W = 33, 47
  frames, _, _, cleaned, tri = _scene(5, H, W)
  known = np.where(cleaned[:1] >= 128, 255, 0).astype(np.uint8)                       # no unknown pixel
  no_one = np.where(tri[1:2] == 255, 127, tri[1:2]).astype(np.uint8)                  # a band, and no known-1 pixel: b = 0
  stripe = np.array(tri[2:3])
  stripe[0, :, 20:27] = 127                                                           # a band from the top edge to the bottom edge
  stripe[0, 10:14, :] = 127                                                           # and from the left edge to the right
  t3, f3 = np.concatenate([known, no_one, stripe]), frames[:3]
  alpha, matte, rep = _solve(f3, t3)
  want_alpha, want_matte, want_rep = sr.solve(f3, t3, tol=TOL)
  assert [r["status"] for r in want_rep] == [1, 1, 0] and rep["status"].tolist() == [1, 1, 0]
  assert rep["iterations"].tolist()[:2] == [0, 0] and rep["residual"].tolist()[:2] == [0.0, 0.0] and rep["unknown"][0] == 0 and rep["unknown"][1] > 0
  assert np.array_equal(matte[0], known[0]) and not matte[1].any() and not alpha[1].any()
  assert np.abs(alpha[2] - want_alpha[2]).max() <= 8 * S and rep["residual"][2] <= TOL and rep["iterations"][2] <= want_rep[2]["iterations"] + 1
  assert np.abs(matte[2].astype(int) - want_matte[2]).max() <= 1
  one = _solve(f3[2:], t3[2:], iters=1)
  want = sr.solve_frame(f3[2], t3[2], iters=1, tol=TOL)
  assert one[2]["iterations"][0] == 1 == want["iterations"] and np.abs(one[0][0] - want["alpha"]).max() <= 8 * S and one[2]["residual"][0] > TOL


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched():
  import torch
  from voicepuppet_amd.matte_solve import MatteSolver
  s = _solver()
  frames = torch.zeros(2, 64, 48, 3, dtype=torch.uint8, device="cuda")
  tri = torch.full((2, 64, 48), 127, dtype=torch.uint8, device="cuda")
  out = torch.full((2, 64, 48), 55, dtype=torch.uint8, device="cuda")
  for kw in (dict(radius=0), dict(radius=4), dict(eps=0.0), dict(eps=float("nan")), dict(iters=0), dict(iters=1025), dict(tol=-1.0), dict(tol=float("inf"))):
    with pytest.raises(RuntimeError, match="vp_mattesolve_solve"):
      s.solve(frames, tri, out=out, **kw)
  for f, t, o in [(frames, tri[:1], out), (frames, tri[:, :, ::2], out), (frames, tri.float(), out), (frames, tri, out[:1]), (frames, tri, out[:, :, :40]),
                  (frames[..., :2], tri, out), (frames.cpu(), tri, out), (frames, tri.cpu(), out), (frames[:, :, ::2], tri[:, :, :24].contiguous(), out)]:
    with pytest.raises(ValueError):
      s.solve(f, t, out=o)
  for shape in ((6, 64, 48), (1, 15, 48), (1, 64, 15), (1, 257, 48), (1, 64, 257)):
    with pytest.raises(RuntimeError, match="vp_mattesolve_solve"):
      s.solve(torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda"), torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="vp_mattesolve_trimap"):
      s.trimap(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
  for kw in (dict(support=0), dict(support=256), dict(core=0), dict(core=256), dict(erode=-1), dict(erode=65), dict(dilate=-1), dict(dilate=65)):
    with pytest.raises(RuntimeError, match="vp_mattesolve_trimap"):
      s.trimap(tri, out=out, **kw)
  with pytest.raises(RuntimeError, match="overlaps"):
    s.trimap(tri, out=tri)
  for m, o in [(tri.cpu(), out), (tri.float(), out), (tri[:, :, ::2], out), (tri[0], out), (tri, out[:1]), (tri, out.cpu())]:
    with pytest.raises(ValueError):
      s.trimap(m, out=o)
  p = torch.zeros(2, 64, 48, dtype=torch.float64, device="cuda")
  for args, kw in (((frames, p.float()), {}), ((frames, p[:1]), {}), ((frames, p.cpu()), {})):
    with pytest.raises(ValueError):
      s.laplacian(*args, **kw)
  with pytest.raises(RuntimeError, match="radius"):
    s.laplacian(frames, p, radius=4)
  small = MatteSolver(1, 64, 64, max_radius=1)
  with pytest.raises(RuntimeError, match="max_radius"):
    small.solve(frames[:1], tri[:1], radius=2, out=out)
  for bad in ((0, 64, 64, 1), (1, 8, 64, 1), (1, 64, 2000, 1), (1, 64, 64, 0), (1, 64, 64, 4)):
    with pytest.raises(ValueError, match="invalid matte solver descriptor"):
      MatteSolver(*bad)
  small.close()
  torch.cuda.synchronize()
  assert (out == 55).all()


# ---- the dataset tool ---------------------------------------------------------------------------------------------------------------------
def _rgb(path):
  from PIL import Image
  return np.asarray(Image.open(path).convert("RGB"))


# measured with the restatement on clutter_scene(256, 256, seed=1): matte MAE of the 0 / 255 segmentation alpha > 0.5 and of the solve
CLUTTER_MAE = (0.0071, 0.0046)


def test_launcher_solve_matte_end_to_end(tmp_path, monkeypatch, capsys):
  """Six JPEG frames of the scene through make_triptychs.py: without --solve_matte the new options change no byte of what the existing
  options write; with it the matte panel is the device's solve of the cleaned key matte (the solver run here on the same decoded
  frames gives the same bytes), closer to the known alpha than the cleaned matte, and the summary line carries the report.  Then the
  cluttered clip with 0 / 255 masks as --alpha_dir: the third panel against the known alpha."""
  import torch
  from PIL import Image
  import bfm_fit_ref as fr
  from test_gpu_bfm_fit import write_bfm_assets
  from voicepuppet_amd.datasets import make_triptychs as mt
  from voicepuppet_amd.matte import KeyMatte
  from voicepuppet_amd.matte_solve import MatteSolver, summary
  S_ = 256
  monkeypatch.chdir(tmp_path)
  g = dict(np.load(GOLDEN))
  write_bfm_assets(br.synthetic_facemodel(seed=int(g["model_seed"]), smooth=True), g["lm3d68"])
  xy = np.stack([fr.photo_landmarks(g["landmarks_2d"][f], 0.7, (50.0, 45.0)) for f in range(6)])
  frames, truth, _ = mr.scene(S_, S_, seed=11, n=6, spill_levels=10.0)
  cframes, ctruth, _ = sr.clutter_scene(S_, S_, seed=1, n=6)
  for name, clip in (("clip", frames), ("clutter", cframes)):
    os.makedirs(name)
    for i in range(6):
      Image.fromarray(clip[i]).save(os.path.join(name, "%d.jpg" % i), "JPEG", quality=95)
    np.savetxt(os.path.join(name, "_landmark.txt"), xy.reshape(6, 136), delimiter=",", fmt="%.10f")
  os.makedirs("masks")
  seg = np.where(ctruth > 0.5, 255, 0).astype(np.uint8)
  for i in range(6):
    Image.fromarray(seg[i]).save(os.path.join("masks", "%d.png" % i))

  def common(name):
    return ["--clip_dir", name, "--landmarks", os.path.join(name, "_landmark.txt"), "--rounds", "1", "--id_steps", "1", "--frame_batch", "4"]
  existing = ["--key_matte", "--clean_matte", "--key_foreground"]
  mt.main(common("clip") + ["--out_dir", "plain"] + existing)
  line0 = capsys.readouterr().out.strip().splitlines()[-1]
  mt.main(common("clip") + ["--out_dir", "unused"] + existing + ["--solve_radius", "2", "--solve_eps", "5", "--solve_iters", "7", "--solve_erode", "9"])
  line1 = capsys.readouterr().out.strip().splitlines()[-1]
  assert "solve:" not in line0 and line1 == line0
  for i in range(6):
    assert open(os.path.join("plain", "%d.jpg" % i), "rb").read() == open(os.path.join("unused", "%d.jpg" % i), "rb").read(), i

  res = mt.main(common("clip") + ["--out_dir", "solved", "--solve_matte", "--write_alpha", "alpha"] + existing)
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  reader = mt.FrameReader("clip", 4, None, None)
  decoded = torch.cat([reader.read(0, 4), reader.read(4, 2)])
  keyed = KeyMatte(6, S_, S_).fit(decoded[:4]).matte(decoded).cpu().numpy()
  anchors = np.floor(np.loadtxt(os.path.join("clip", "_landmark.txt"), delimiter=",").reshape(6, 68, 2)).astype(np.int32)
  cleaned, _, _ = mr.clean(keyed, anchors)
  ms = MatteSolver(6, S_, S_)
  want = ms.solve(decoded, ms.trimap(_dev(cleaned))).cpu().numpy()
  rep = ms.report()
  assert sr.wrongly_known(sr.trimap(cleaned), truth) == 0
  assert all(np.array_equal(res["solve"][k], rep[k]) for k in rep) and not rep["status"].any() and (rep["residual"] <= TOL).all()
  assert "triptych status 0:6, 0 repeated" in line and ("; " + summary(rep)[0]) in line and summary(rep, 512, TOL)[1:] == (0, 0)
  mae_c, mae_s = kr.quality(cleaned, truth)[0], kr.quality(want, truth)[0]
  print("matte MAE: cleaned %.5f, solved %.5f" % (mae_c, mae_s))
  assert mae_s <= mae_c / 3
  for i in range(6):
    assert np.array_equal(np.asarray(Image.open(os.path.join("alpha", "%d.png" % i))), want[i]), i
    p3 = _rgb(os.path.join("solved", "%d.jpg" % i))[:, 2 * S_:].astype(np.float64)
    assert np.abs(p3 - want[i][..., None]).mean() <= 2.0

  # the cluttered clip: 0 / 255 masks, the solve, the foreground
  res = mt.main(common("clutter") + ["--out_dir", "cluttered", "--alpha_dir", "masks", "--solve_matte", "--key_foreground"])
  line = capsys.readouterr().out.strip().splitlines()[-1]
  print(line)
  reader = mt.FrameReader("clutter", 4, None, None)
  decoded = torch.cat([reader.read(0, 4), reader.read(4, 2)])
  want = ms.solve(decoded, ms.trimap(_dev(seg))).cpu().numpy()
  assert sr.wrongly_known(sr.trimap(seg), ctruth) == 0 and "solve: " in line and not res["solve"]["status"].any()
  mae_seg, mae_s = kr.quality(seg, ctruth)[0], kr.quality(want, ctruth)[0]
  panel = np.stack([_rgb(os.path.join("cluttered", "%d.jpg" % i))[:, 2 * S_:].astype(np.float64).mean(-1) for i in range(6)])
  mae_p = float(np.abs(panel / 255.0 - ctruth).mean())
  print("cluttered clip: matte MAE segmentation %.5f, solved %.5f, the third panel (after JPEG) %.5f" % (mae_seg, mae_s, mae_p))
  assert mae_s < mae_seg and mae_s <= 1.5 * CLUTTER_MAE[1]
  assert np.abs(panel - want).mean() <= 2.0 and mae_p <= 1.5 * CLUTTER_MAE[1] + 2.0 / 255.0
  ms.close()

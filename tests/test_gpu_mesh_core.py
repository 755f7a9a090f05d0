"""The dense half of mesh_core on the device (voicepuppet_amd/csrc/raster_dense.hip through voicepuppet_amd.utils.mesh_core) against the
goldens the reference's compiled mesh_core.cpp produced and the numpy restatements of tests/mesh_core_ref.py.  BIT-EXACT throughout:
uint32 views of the float buffers, exact triangle ids."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_core_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "mesh_core_dense.npz")


def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
  return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def gold():
  return dict(np.load(GOLD))


def dev(a):
  import torch
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("tag", list(mr.MESHES))
def test_core_signatures_on_numpy_arrays_match_the_goldens(gold, tag):
  from voicepuppet_amd.utils import mesh_core
  v, t, h, w = mr.mesh(tag)
  nver, ntri = v.shape[0], t.shape[0]
  depth, ids, bary, _ = mr.fresh_buffers(h, w)
  assert mesh_core.rasterize_triangles_core(v.copy(), t.copy(), depth, ids, bary.reshape(h, w * 3), nver, ntri, h, w) is None
  assert np.array_equal(ids, gold[tag + "_ids"])
  assert same(depth, gold[tag + "_depth"]) and same(bary, gold[tag + "_weights"])
  for mode in (0, 1):
    d, _, _, image = mr.fresh_buffers(h, w)
    mesh_core.render_texture_core(image, v.copy(), t.copy(), gold[tag + "_texture"], gold[tag + "_tex_coords"], gold[tag + "_tex_triangles"], d,
                                  nver, nver, ntri, h, w, 3, 16, 16, 3, mode)
    assert same(image, gold["%s_tex%d_image" % (tag, mode)]), mode
    assert same(d, gold["%s_tex%d_depth" % (tag, mode)]), mode
  normal = gold[tag + "_normal0"].copy()
  mesh_core.get_normal_core(normal, gold[tag + "_tri_normal"], t.copy(), ntri)
  assert same(normal, gold[tag + "_normal"])


@pytest.fixture(scope="module")
def clip(gold):
  """Three frames of the 40 x 36 mesh sharing its triangle list: the fixture as it is (its large near triangles hide the ellipsoid), then
  two with those triangles pushed behind the cleared depth, jittered, with scaled depth.  The restatement's buffers, computed once."""
  v0, t, h, w = mr.mesh("m5")
  n0 = v0.shape[0] - 12                                          # synthetic_mesh appends 12 extra vertices
  rng = np.random.default_rng(11)
  frames = [v0]
  for f in (1, 2):
    v = v0.copy()
    v[:, :2] += rng.normal(0, 1.5, size=(1, 2)).astype(np.float32)
    v[:, 2] *= np.float32(1 + 0.07 * f)
    v[n0:, 2] = np.float32(-2000000.0 - f)                         # below the cleared depth: candidates that never win
    frames.append(v)
  texture, tex_coords, tex_triangles = gold["m5_texture"], gold["m5_tex_coords"], gold["m5_tex_triangles"]
  want, want_tex = [], []
  for v in frames:
    depth, ids, bary, _ = mr.fresh_buffers(h, w)
    want.append(mr.rasterize_triangles_py(v, t, depth, ids, bary, h, w))
    rows = []
    for mode in (0, 1):
      d, _, _, image = mr.fresh_buffers(h, w)
      rows.append(mr.render_texture_py(image, v, t, texture, tex_coords, tex_triangles, d, h, w, mode))
    want_tex.append(rows)
  assert 0.2 < (want[1][1] >= 0).mean() < 0.95 and len(np.unique(want[1][1])) > 20      # the ellipsoid shows, with background
  return dict(frames=np.stack(frames), tri=t, h=h, w=w, want=want, want_tex=want_tex, texture=texture, tex_coords=tex_coords,
              tex_triangles=tex_triangles)


def _fresh_device(F, h, w):
  import torch
  return (torch.full((F, h, w), float(mr.DEPTH_INIT), dtype=torch.float32, device="cuda"),
          torch.full((F, h, w), -1, dtype=torch.int32, device="cuda"), torch.zeros(F, h, w, 3, dtype=torch.float32, device="cuda"))


def test_batch_of_frames_alone_and_again(clip):
  import torch
  from voicepuppet_amd.utils import mesh_core
  h, w, F = clip["h"], clip["w"], 3
  V, T = dev(clip["frames"]), dev(clip["tri"])
  depth, ids, bary = _fresh_device(F, h, w)
  mesh_core.rasterize_triangles(V, T, depth, ids, bary)
  for f in range(F):
    wd, wi, wb = clip["want"][f]
    assert np.array_equal(ids[f].cpu().numpy(), wi), f
    assert same(depth[f].cpu().numpy(), wd) and same(bary[f].cpu().numpy(), wb), f
  # a frame alone gives the bits it gives in the batch
  d1, i1, b1 = _fresh_device(1, h, w)
  mesh_core.rasterize_triangles(V[1:2].contiguous(), T, d1, i1, b1)
  assert torch.equal(i1[0], ids[1]) and torch.equal(d1[0].view(torch.int32), depth[1].view(torch.int32))
  assert torch.equal(b1[0].view(torch.int32), bary[1].view(torch.int32))
  # a second call over the same buffers changes nothing (strict > against the depths already written)
  before = (depth.clone(), ids.clone(), bary.clone())
  mesh_core.rasterize_triangles(V, T, depth, ids, bary)
  assert torch.equal(before[0].view(torch.int32), depth.view(torch.int32)) and torch.equal(before[1], ids)
  assert torch.equal(before[2].view(torch.int32), bary.view(torch.int32))
  # the *_core signature on CUDA tensors works where they lie
  d2, i2, b2 = _fresh_device(1, h, w)
  mesh_core.rasterize_triangles_core(V[2].contiguous(), T, d2[0], i2[0], b2[0], V.shape[1], T.shape[0], h, w)
  assert torch.equal(i2[0], ids[2]) and torch.equal(d2[0].view(torch.int32), depth[2].view(torch.int32))


def test_texture_batch_both_modes(clip):
  import torch
  from voicepuppet_amd.utils import mesh_core
  h, w, F = clip["h"], clip["w"], 3
  V, T = dev(clip["frames"]), dev(clip["tri"])
  tex, tc, tt = dev(clip["texture"]), dev(clip["tex_coords"]), dev(clip["tex_triangles"])
  for mode in (0, 1):
    depth, _, image = _fresh_device(F, h, w)
    mesh_core.render_texture(image, V, T, tex, tc, tt, depth, mapping_type=mode)
    for f in range(F):
      wi, wd = clip["want_tex"][f][mode]
      assert same(image[f].cpu().numpy(), wi) and same(depth[f].cpu().numpy(), wd), (mode, f)
    before = image.clone()
    mesh_core.render_texture(image, V, T, tex, tc, tt, depth, mapping_type=mode)
    assert torch.equal(before.view(torch.int32), image.view(torch.int32))
  image = torch.zeros(F, h, w, 4, dtype=torch.float32, device="cuda")
  with pytest.raises(ValueError):
    mesh_core.render_texture(image, V, T, tex, tc, tt, depth)                        # c > tex_c
  with pytest.raises(ValueError):
    mesh_core.render_texture(torch.zeros(F, h, w, 3, device="cuda"), V, T, tex, tc[:-1].contiguous(), tt, depth)   # too few tex_coords rows


def test_no_triangles_leave_the_buffers_as_given():
  import torch
  from voicepuppet_amd.utils import mesh_core
  rng = np.random.default_rng(3)
  depth0, bary0 = rng.normal(size=(2, 9, 7)).astype(np.float32), rng.normal(size=(2, 9, 7, 3)).astype(np.float32)
  ids0 = rng.integers(-1, 5, size=(2, 9, 7)).astype(np.int32)
  depth, ids, bary = dev(depth0), dev(ids0), dev(bary0)
  V = dev(rng.uniform(0, 8, size=(2, 5, 3)).astype(np.float32))
  none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
  mesh_core.rasterize_triangles(V, none, depth, ids, bary)
  assert same(depth.cpu().numpy(), depth0) and np.array_equal(ids.cpu().numpy(), ids0) and same(bary.cpu().numpy(), bary0)
  image0 = rng.normal(size=(2, 9, 7, 3)).astype(np.float32)
  image = dev(image0)
  mesh_core.render_texture(image, V, none, dev(np.ones((4, 4, 3), np.float32)), dev(np.zeros((5, 3), np.float32)), none, depth)
  assert same(image.cpu().numpy(), image0) and same(depth.cpu().numpy(), depth0)
  normal0 = rng.normal(size=(2, 5, 3)).astype(np.float32)
  normal = dev(normal0)
  mesh_core.vertex_normals(normal, torch.zeros(2, 0, 3, device="cuda"), none)
  assert same(normal.cpu().numpy(), normal0)


def test_one_triangle_over_the_whole_image_and_a_nan_depth():
  """A 64 x 64 image under one triangle (a 4096-pixel box: the wave-wide scan), a small triangle in front of it (the lane's own scan), and
  a nearer triangle with a NaN z, which the reference's '>' never lets win - also not in the border ring."""
  from voicepuppet_amd.utils import mesh_core
  h = w = 64
  v = np.array([[-10, -10, 1], [200, -10, 2], [-10, 200, 3],             # covers everything
                [20.3, 20.6, 9], [24.1, 20.2, 9.5], [21.7, 24.9, 10],    # small, nearer
                [-5, -5, np.nan], [90, -5, 50], [-5, 90, 50]], np.float32)   # NaN z at one corner: every p_depth is NaN
  t = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
  want = mr.fresh_buffers(h, w)
  mr.rasterize_triangles_py(v, t, want[0], want[1], want[2], h, w)
  assert (want[1] == 0).sum() > 4000 and 0 < (want[1] == 1).sum() < 32 and not (want[1] == 2).any() and not np.isnan(want[0]).any()
  depth, ids, bary, _ = mr.fresh_buffers(h, w)
  mesh_core.rasterize_triangles_core(v, t, depth, ids, bary, 9, 3, h, w)
  assert np.array_equal(ids, want[1]) and same(depth, want[0]) and same(bary, want[2])
  # the NaN triangle alone: nothing wins, the buffers stay as given
  depth, ids, bary, _ = mr.fresh_buffers(h, w)
  mesh_core.rasterize_triangles_core(v, t[2:].copy(), depth, ids, bary, 9, 1, h, w)
  assert (ids == -1).all() and (depth == mr.DEPTH_INIT).all() and not bary.any()


def test_interpolate_matches_its_restatement_and_skips_negative_ids(clip):
  import torch
  from voicepuppet_amd.utils import mesh_core
  h, w, F = clip["h"], clip["w"], 3
  nver = clip["frames"].shape[1]
  rng = np.random.default_rng(7)
  attr = rng.normal(size=(F, nver, 5)).astype(np.float32)
  ids = np.stack([x[1] for x in clip["want"]])
  bary = np.stack([x[2] for x in clip["want"]])
  assert (ids < 0).any() and (ids >= 0).any()
  out0 = rng.normal(size=(F, h, w, 5)).astype(np.float32)
  want = out0.copy()
  for f in range(F):
    mr.interpolate_py(ids[f], bary[f], clip["tri"], attr[f], want[f])
  out = dev(out0)
  got = mesh_core.interpolate(dev(ids), dev(bary), dev(clip["tri"]), dev(attr), out=out)
  assert got is out and same(out.cpu().numpy(), want)
  assert same(out.cpu().numpy()[ids < 0], out0[ids < 0])                 # negative ids: left alone
  fresh = mesh_core.interpolate(dev(ids), dev(bary), dev(clip["tri"]), dev(attr))
  assert not fresh.cpu().numpy()[ids < 0].any() and same(fresh.cpu().numpy()[ids >= 0], want[ids >= 0])
  # the vertex positions interpolated through the buffers give back the pixel's own depth to rounding: the buffers are a correspondence
  pos = mesh_core.interpolate(dev(ids), dev(bary), dev(clip["tri"]), dev(clip["frames"])).cpu().numpy()
  depth = np.stack([x[0] for x in clip["want"]])
  assert same(pos[..., 2][ids >= 0], depth[ids >= 0])


def test_vertex_normals_order_repeats_and_batches():
  import torch
  from voicepuppet_amd.utils import mesh_core
  rng = np.random.default_rng(9)
  # a fan of 50 triangles around vertex 0 (its list is long enough for the heap sort), small lists elsewhere, a triangle that names
  # vertex 3 twice and one that names it three times
  nver = 60
  tri = [[0, 1 + k, 2 + k] for k in range(50)] + [[3, 3, 7], [3, 3, 3], [58, 59, 0]]
  tri = np.array(tri, np.int32)[rng.permutation(len(tri))]
  F = 2
  normal0 = rng.normal(size=(F, nver, 3)).astype(np.float32)
  tn = (rng.normal(size=(F, tri.shape[0], 3)) * 10.0 ** rng.integers(-3, 4, size=(F, tri.shape[0], 1))).astype(np.float32)   # order matters
  want = np.stack([mr.get_normal_py(normal0[f].copy(), tn[f], tri) for f in range(F)])
  T = dev(tri)
  runs = []
  for _ in range(3):
    n = dev(normal0)
    mesh_core.vertex_normals(n, dev(tn), T)
    runs.append(n.cpu().numpy())
  assert same(runs[0], want)
  assert same(runs[1], runs[0]) and same(runs[2], runs[0])               # repeated calls: identical bits
  adj = mesh_core.vertex_adjacency(T, nver)
  assert mesh_core.vertex_adjacency(T, nver) is adj                      # built once per triangle tensor
  n_off = np.frombuffer(adj.cpu().numpy().tobytes(), np.int32)
  offsets, entries = n_off[:nver + 1], n_off[nver + 1:nver + 1 + 3 * tri.shape[0]]
  assert offsets[0] == 0 and offsets[-1] == 3 * tri.shape[0] and np.array_equal(np.diff(offsets), np.bincount(tri.reshape(-1), minlength=nver))
  for v in range(nver):
    e = entries[offsets[v]:offsets[v + 1]]
    assert np.array_equal(e, np.nonzero(tri.reshape(-1) == v)[0]), v     # 3 * triangle + corner, ascending
  # a repeated index counts twice: one triangle (3, 3, 7) onto zeros
  one = torch.zeros(1, 8, 3, device="cuda")
  mesh_core.vertex_normals(one, torch.tensor([[[1.0, 2.0, 4.0]]], device="cuda"), torch.tensor([[3, 3, 7]], dtype=torch.int32, device="cuda"))
  got = one.cpu().numpy()[0]
  assert got[3].tolist() == [2.0, 4.0, 8.0] and got[7].tolist() == [1.0, 2.0, 4.0] and not got[[0, 1, 2, 4, 5, 6]].any()

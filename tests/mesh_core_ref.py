"""Checkers for the dense half of mesh_core (voicepuppet_amd/csrc/raster_dense.hip): _rasterize_triangles_core (utils/cython/mesh_core.cpp:108-166),
_render_texture_core (:234-333), _get_normal_core (:85-105) and the interpolation of per-vertex attributes through the buffers.

  * *_py  : plain numpy restatements, float32 arithmetic in the reference's evaluation order (the style of oracle/raster_ref.py's _in_tri),
            in place like the C++;
  * *_ref : the reference's own mesh_core.cpp as oracle/Makefile compiles it into oracle/_ref/libmesh_core_ref.so, through ctypes.
            tests/golden/mesh_core_dense.npz holds what it produced (tests/golden/make_mesh_core_golden.py).
TEST INFRASTRUCTURE ONLY: nothing under voicepuppet_amd imports this."""
import ctypes
import warnings

import numpy as np

from oracle import raster_ref as rr

F = np.float32


def _uv(px, py, p0, p1, p2):
  """u, v of isPointInTri / get_point_weight (mesh_core.cpp:23-46, :53-76: the same arithmetic), px / py float32 arrays."""
  v0x, v0y = F(p2[0] - p0[0]), F(p2[1] - p0[1])
  v1x, v1y = F(p1[0] - p0[0]), F(p1[1] - p0[1])
  v2x, v2y = (px - p0[0]).astype(F), (py - p0[1]).astype(F)
  dot00 = F(F(v0x * v0x) + F(v0y * v0y))
  dot01 = F(F(v0x * v1x) + F(v0y * v1y))
  dot02 = (v0x * v2x).astype(F) + (v0y * v2y).astype(F)
  dot11 = F(F(v1x * v1x) + F(v1y * v1y))
  dot12 = (v1x * v2x).astype(F) + (v1y * v2y).astype(F)
  den = F(F(dot00 * dot11) - F(dot01 * dot01))
  inv = F(0) if den == 0 else F(F(1) / den)
  u = ((dot11 * dot02).astype(F) - (dot01 * dot12).astype(F)).astype(F) * inv
  v = ((dot00 * dot12).astype(F) - (dot01 * dot02).astype(F)).astype(F) * inv
  return u.astype(F), v.astype(F)


def _candidates(vertices, tri, t, depth, h, w):
  """The pixels of triangle t that pass :148 / :292 and beat `depth`: (ys, xs, w0, w1, w2, p_depth) or None."""
  i0, i1, i2 = tri[t]
  p0, p1, p2 = vertices[i0], vertices[i1], vertices[i2]
  x_min = max(int(np.ceil(min(p0[0], p1[0], p2[0]))), 0)
  x_max = min(int(np.floor(max(p0[0], p1[0], p2[0]))), w - 1)
  y_min = max(int(np.ceil(min(p0[1], p1[1], p2[1]))), 0)
  y_max = min(int(np.floor(max(p0[1], p1[1], p2[1]))), h - 1)
  if x_max < x_min or y_max < y_min:
    return None
  ys, xs = np.mgrid[y_min:y_max + 1, x_min:x_max + 1]
  u, v = _uv(xs.astype(F), ys.astype(F), p0, p1, p2)
  border = (xs < 2) | (xs > w - 3) | (ys < 2) | (ys > h - 3)
  inside = (u >= 0) & (v >= 0) & ((u + v).astype(F) < 1)
  w0 = ((F(1) - u).astype(F) - v).astype(F)                                     # weight[0] = 1 - u - v; weight[1] = v; weight[2] = u
  pd = (((w0 * p0[2]).astype(F) + (v * p1[2]).astype(F)).astype(F) + (u * p2[2]).astype(F)).astype(F)
  hit = (border | inside) & (pd > depth[ys, xs])                                # false for a NaN depth, as in the C++
  if not hit.any():
    return None
  return ys[hit], xs[hit], w0[hit], v[hit], u[hit], pd[hit]


def rasterize_triangles_py(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, h, w):
  """In place on depth_buffer f32 [h,w], triangle_buffer i32 [h,w], barycentric_weight f32 [h,w,3]."""
  vertices = np.asarray(vertices, F).reshape(-1, 3)
  tri = np.asarray(triangles, np.int32).reshape(-1, 3)
  with warnings.catch_warnings(), np.errstate(all="ignore"):
    warnings.simplefilter("ignore")
    for t in range(tri.shape[0]):
      c = _candidates(vertices, tri, t, depth_buffer, h, w)
      if c is None:
        continue
      ys, xs, w0, w1, w2, pd = c
      depth_buffer[ys, xs] = pd
      triangle_buffer[ys, xs] = t
      barycentric_weight[ys, xs, 0], barycentric_weight[ys, xs, 1], barycentric_weight[ys, xs, 2] = w0, w1, w2
  return depth_buffer, triangle_buffer, barycentric_weight


def _clamp(x, top):
  """max(min(x, top), 0) with std::min / std::max's comparisons (:304-305)."""
  m = np.where(F(top) < x, F(top), x).astype(F)
  return np.where(m < 0, F(0), m).astype(F)


def _round_half_away(x):
  x = x.astype(np.float64)                                                       # |x| + 0.5 is exact in double
  return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def render_texture_py(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, h, w, mapping_type):
  """In place on image f32 [h,w,c] and depth_buffer f32 [h,w]; the indexing of :270-272 as written."""
  vertices = np.asarray(vertices, F).reshape(-1, 3)
  tri = np.asarray(triangles, np.int32).reshape(-1, 3)
  ttri = np.asarray(tex_triangles, np.int32).reshape(-1, 3)
  tc = np.asarray(tex_coords, F).reshape(-1, 3)
  tex_h, tex_w, _ = texture.shape
  c = image.shape[2]
  for t in range(tri.shape[0]):
    cand = _candidates(vertices, tri, t, depth_buffer, h, w)
    if cand is None:
      continue
    ys, xs, w0, w1, w2, pd = cand
    tx = (((w0 * tc[ttri[t, 0], 0]).astype(F) + (w1 * tc[ttri[t, 1], 0]).astype(F)).astype(F) + (w2 * tc[ttri[t, 2], 0]).astype(F)).astype(F)
    ty = (((w0 * tc[tri[t, 0], 1]).astype(F) + (w1 * tc[tri[t, 1], 1]).astype(F)).astype(F) + (w2 * tc[tri[t, 2], 1]).astype(F)).astype(F)
    tx, ty = _clamp(tx, tex_w - 1), _clamp(ty, tex_h - 1)
    if mapping_type == 0:
      image[ys, xs] = texture[_round_half_away(ty), _round_half_away(tx), :c]
    else:
      yd, xd = (ty - np.floor(ty)).astype(F)[:, None], (tx - np.floor(tx)).astype(F)[:, None]
      yf, yc, xf, xc = (np.floor(ty).astype(np.int64), np.ceil(ty).astype(np.int64), np.floor(tx).astype(np.int64), np.ceil(tx).astype(np.int64))
      ul, ur, dl, dr = texture[yf, xf, :c], texture[yf, xc, :c], texture[yc, xf, :c], texture[yc, xc, :c]
      one = F(1)
      a = ((ul * (one - xd)).astype(F) * (one - yd)).astype(F)
      b = ((ur * xd).astype(F) * (one - yd)).astype(F)
      cc = ((dl * (one - xd)).astype(F) * yd).astype(F)
      d = ((dr * xd).astype(F) * yd).astype(F)
      image[ys, xs] = (((a + b).astype(F) + cc).astype(F) + d).astype(F)
    depth_buffer[ys, xs] = pd
  return image, depth_buffer


def get_normal_py(normal, tri_normal, triangles):
  """In place on normal f32 [nver,3]: the serial loop of :92-104."""
  tri = np.asarray(triangles, np.int32).reshape(-1, 3)
  for t in range(tri.shape[0]):
    for k in range(3):
      normal[tri[t, k]] = (normal[tri[t, k]] + tri_normal[t]).astype(F)
  return normal


def interpolate_py(triangle_buffer, barycentric_weight, triangles, attributes, out):
  """out[y,x,:] = w0*a[i0] + w1*a[i1] + w2*a[i2] (float32, that order) where triangle_buffer >= 0; in place on out f32 [h,w,k]."""
  tri = np.asarray(triangles, np.int32).reshape(-1, 3)
  a = np.asarray(attributes, F)
  ys, xs = np.nonzero(triangle_buffer >= 0)
  ids = tri[triangle_buffer[ys, xs]]
  bw = barycentric_weight[ys, xs].astype(F)
  s = ((bw[:, 0:1] * a[ids[:, 0]]).astype(F) + (bw[:, 1:2] * a[ids[:, 1]]).astype(F)).astype(F)
  out[ys, xs] = (s + (bw[:, 2:3] * a[ids[:, 2]]).astype(F)).astype(F)
  return out


# ---- the compiled reference ------------------------------------------------------------------------------------------------------------
have_compiled_reference = rr.have_compiled_reference
_P, _I = ctypes.c_void_p, ctypes.c_int


def _fn(name):
  fn = getattr(ctypes.CDLL(rr._REF), name)
  fn.restype = None
  return fn


def _p(a):
  assert a.flags.c_contiguous
  return _P(a.ctypes.data)


def rasterize_triangles_ref(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, h, w):
  vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
  tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
  _fn("_Z25_rasterize_triangles_corePfPiS_S0_S_iiii")(_p(vertices), _p(tri), _p(depth_buffer), _p(triangle_buffer), _p(barycentric_weight),
                                                      _I(vertices.shape[0]), _I(tri.shape[0]), _I(h), _I(w))
  return depth_buffer, triangle_buffer, barycentric_weight


def render_texture_ref(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, h, w, mapping_type, tex_nver=None):
  vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
  tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
  ttri = np.ascontiguousarray(tex_triangles, np.int32).reshape(-1, 3)
  tc = np.ascontiguousarray(tex_coords, F).reshape(-1, 3)
  texture = np.ascontiguousarray(texture, F)
  assert tc.shape[0] >= vertices.shape[0] and image.shape[2] <= texture.shape[2]
  _fn("_Z20_render_texture_corePfS_PiS_S_S0_S_iiiiiiiiii")(
      _p(image), _p(vertices), _p(tri), _p(texture), _p(tc), _p(ttri), _p(depth_buffer), _I(vertices.shape[0]),
      _I(tc.shape[0] if tex_nver is None else tex_nver), _I(tri.shape[0]), _I(h), _I(w), _I(image.shape[2]), _I(texture.shape[0]),
      _I(texture.shape[1]), _I(texture.shape[2]), _I(mapping_type))
  return image, depth_buffer


def get_normal_ref(normal, tri_normal, triangles):
  tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
  tn = np.ascontiguousarray(tri_normal, F)
  _fn("_Z16_get_normal_corePfS_Pii")(_p(normal), _p(tn), _p(tri), _I(tri.shape[0]))
  return normal


# ---- the fixture inputs that are not the mesh itself (seeded; the goldens hold what the compiled reference made of them) ---------------
def texture_inputs(nver, ntri, seed):
  """A 16 x 16 x 3 texture, tex_coords [nver,3] that reach past the texture on every side (the clamp is exercised) and tex_triangles that
  differ from the mesh's (x and y come through different index lists, :270-272)."""
  rng = np.random.default_rng(seed)
  texture = rng.uniform(0, 1, size=(16, 16, 3)).astype(F)
  tex_coords = rng.uniform(-2, 18, size=(nver, 3)).astype(F)
  tex_triangles = rng.integers(0, nver, size=(ntri, 3)).astype(np.int32)
  return texture, tex_coords, tex_triangles


def normal_inputs(nver, ntri, seed):
  rng = np.random.default_rng(seed)
  return rng.normal(size=(nver, 3)).astype(F), rng.normal(size=(ntri, 3)).astype(F)


MESHES = {"m17": dict(seed=17, nlat=20, nlon=24, h=120, w=100), "m5": dict(seed=5, nlat=8, nlon=10, h=40, w=36)}
DEPTH_INIT = F(-999999.0)


def mesh(tag):
  kw = MESHES[tag]
  v, t, _ = rr.synthetic_mesh(**kw)
  return v, t, kw["h"], kw["w"]


def fresh_buffers(h, w, c=3):
  """depth, ids, weights, image as a caller of the reference prepares them (utils of the reference's family start ids at -1)."""
  return np.full((h, w), DEPTH_INIT, F), np.full((h, w), -1, np.int32), np.zeros((h, w, 3), F), np.zeros((h, w, c), F)

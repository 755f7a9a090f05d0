"""numpy restatement of FaceFitter.observe's two options (csrc/bfm_observe.hip: vp_bfmfit_observe_ex) and of
mesh_core.vertex_visibility (csrc/raster_dense.hip: vp_raster_vertex_visibility), written from the rules include/vp_hip.h states.
TEST INFRASTRUCTURE ONLY: it does not import the product.  Builds on tests/bfm_appearance_ref.py (geometry, bilinear) and on the plain
rasteriser of tests/mesh_core_ref.py.

  vertex_visibility  float32: visible = (z + tol >= min of the four depths around (x, y)); off the buffer or a NaN -> visible
  prefiltered        float64: the mean of k x k bilinear taps, k = min(ceil(a), 16), at (px + ((i + .5) / k - .5) a, py + ((j + .5) / k - .5) a),
                     each coordinate clamped to the photo; k = 1 for a <= 1
  observe_ex         bfm_appearance_ref.observe with either option; the depth raster from rasterize_triangles_py
  nose_model         the synthetic face model, triangles re-wound so that its normals face the camera, with a nose bump on the mean shape"""
import numpy as np

import bfm_appearance_ref as ar
import mesh_core_ref as mr
from oracle import bfm_ref as br

F = np.float32
DEPTH_CLEAR = F(-99999.0)
MAX_K = 16


def vertex_visibility(vertices, depth, tol):
  """vertices f32 [n,3], depth f32 [h,w] -> (visible u8 [n], margin [n] float64 = |z + tol - m|, inf where the buffer was not asked)."""
  v = np.asarray(vertices, F).reshape(-1, 3)
  d = np.asarray(depth, F)
  h, w = d.shape
  x, y, z = v[:, 0], v[:, 1], v[:, 2]
  with np.errstate(invalid="ignore"):
    asked = (x >= 0) & (x <= F(w - 1)) & (y >= 0) & (y <= F(h - 1)) & ~np.isnan(z)
  xs, ys = np.where(asked, x, F(0)), np.where(asked, y, F(0))
  x0 = np.minimum(np.floor(xs).astype(np.int64), w - 2)
  y0 = np.minimum(np.floor(ys).astype(np.int64), h - 2)
  m = np.fmin(np.fmin(d[y0, x0], d[y0, x0 + 1]), np.fmin(d[y0 + 1, x0], d[y0 + 1, x0 + 1]))
  lhs = (z + F(tol)).astype(F)
  with np.errstate(invalid="ignore"):
    vis = np.where(asked, lhs >= m, True)
    margin = np.where(asked, np.abs(lhs.astype(np.float64) - m.astype(np.float64)), np.inf)
  return vis.astype(np.uint8), margin


def filter_taps(a):
  return int(min(np.ceil(a), MAX_K)) if a > 1 else 1


def prefiltered(photo, px, py, a):
  """(values [n,3] float64, inside [n]): inside is the centre's; the taps are clamped to the photo."""
  H, W = photo.shape[:2]
  centre, inside = ar.bilinear(photo, px, py)
  k = filter_taps(a)
  if k == 1:
    return centre, inside
  px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
  cx, cy = np.where(inside, px, 0.0), np.where(inside, py, 0.0)
  off = ((np.arange(k) + 0.5) / k - 0.5) * a
  tx = np.clip(cx[:, None, None] + off[None, None, :], 0.0, W - 1.0) + np.zeros((1, k, 1))       # [n, j, i]
  ty = np.clip(cy[:, None, None] + off[None, :, None], 0.0, H - 1.0) + np.zeros((1, 1, k))
  taps = ar.bilinear(photo, tx.reshape(-1), ty.reshape(-1))[0].reshape(len(px), k * k, 3)       # one call: the photo is converted once
  return np.where(inside[:, None], taps.sum(axis=1) / (k * k), 0.0), inside


def rotation_of(coeff):
  """Compute_rotation_matrix of the row's angles IN THE ROW'S OWN DTYPE (float32 coefficients: float32 sines and cosines, as the
  reference and the product take them)."""
  return ar.rotation(np.asarray(coeff).reshape(257)[224:227])


def z_buffer(fm, coeff, R):
  """Projection_layer's z buffer value per vertex (utils/reconstruct_mesh.py:100-120): minus the camera-space depth, greater = nearer."""
  c = np.asarray(coeff, np.float64).reshape(257)
  shape = (np.asarray(fm.idBase, np.float64) @ c[:80] + np.asarray(fm.exBase, np.float64) @ c[80:144] + np.asarray(fm.meanshape, np.float64).reshape(-1))
  shape = shape.reshape(-1, 3) - np.asarray(fm.meanshape, np.float64).reshape(-1, 3).mean(axis=0, keepdims=True)
  return -(10.0 - (shape @ R + c[254:257])[:, 2])


def raster_vertices(fm, coeff, ss, R=None):
  """float32 [N,3] = (ss x, ss y, z_buffer), the products in float64."""
  c = np.asarray(coeff, np.float64).reshape(257)
  if R is None:
    R = rotation_of(coeff)
  _, proj = ar.geometry(fm, c, R)
  return np.concatenate([ss * proj, z_buffer(fm, c, R)[:, None]], axis=1).astype(F)


def depth_raster(fm, rv, ss):
  """(depth f32, triangle ids i32, weights f32) of the mesh drawn into a (224 ss)^2 buffer cleared to -99999 / -1."""
  side = 224 * ss
  depth, ids, bary = np.full((side, side), DEPTH_CLEAR, F), np.full((side, side), -1, np.int32), np.zeros((side, side, 3), F)
  tri = (np.asarray(fm.tri) - 1).astype(np.int32)
  mr.rasterize_triangles_py(rv, tri, depth, ids, bary, side, side)
  return depth, ids, bary


def observe_ex(fm, coeff, photo, affine, vertex_weights=None, R=None, visibility=False, prefilter=False, ss=2, tol=0.01):
  """One frame: (sh [N,9], weight [N], observed [N,3], visible u8 [N] or None, info) with info = dict(margin = |z + tol - m| per vertex,
  raster_vertices, depth) when visibility is on."""
  c = np.asarray(coeff, np.float64).reshape(257)
  if R is None:
    R = rotation_of(coeff)
  sh, weight, obs = ar.observe(fm, c, photo, affine, vertex_weights, R)
  a, bx, by = np.asarray(affine, np.float64)
  if prefilter:
    _, proj = ar.geometry(fm, c, R)
    obs, _ = prefiltered(photo, a * proj[:, 0] + bx, a * proj[:, 1] + by, a)
  visible, info = None, {}
  if visibility:
    rv = raster_vertices(fm, c, ss, R)
    depth, _, _ = depth_raster(fm, rv, ss)
    visible, margin = vertex_visibility(rv, depth, tol)
    weight = weight * visible.astype(np.float64)
    info = {"margin": margin, "raster_vertices": rv, "depth": depth}
  return sh, weight, obs, visible, info


def rewound(fm):
  """The same model with every triangle's last two corners swapped (its normals then point AT the camera: the synthetic model's own
  winding makes them point away) and point_buf rebuilt from the new list."""
  tri = np.asarray(fm.tri).copy()
  tri[:, [1, 2]] = tri[:, [2, 1]]
  n, nf = np.asarray(fm.meanshape).size // 3, tri.shape[0]
  point_buf = np.full((n, 8), nf + 1, np.int64)
  fill = np.zeros(n, np.int64)
  for f in range(nf):
    for v in tri[f] - 1:
      point_buf[v, fill[v]] = f + 1
      fill[v] += 1
  return br.FaceModel(meanshape=fm.meanshape, idBase=fm.idBase, exBase=fm.exBase, meantex=fm.meantex, texBase=fm.texBase, point_buf=point_buf,
                      tri=tri, keypoints=fm.keypoints)


def bump_height(fm):
  xyz = np.asarray(fm.meanshape, np.float64).reshape(-1, 3)
  return 0.8 * np.exp(-((xyz[:, 0] / 0.2) ** 2 + (xyz[:, 1] / 0.3) ** 2))


def plain_model(nlat=14, nlon=18):
  """The convex half-ellipsoid, re-wound."""
  return rewound(br.synthetic_facemodel(seed=3, smooth=True, nlat=nlat, nlon=nlon))


def nose_model(nlat=14, nlon=18):
  """plain_model with z += 0.8 exp(-((x / 0.2)^2 + (y / 0.3)^2)) on the mean shape; (model, bump height per vertex of the PLAIN shape)."""
  fm = plain_model(nlat, nlon)
  height = bump_height(fm)
  xyz = np.array(fm.meanshape, np.float64).reshape(-1, 3)
  xyz[:, 2] += height
  fm.meanshape = xyz.reshape(1, -1)
  return fm, height


POSE_T = (-0.02, 0.01, 0.05)         # chosen for the fixture conditions of tests/test_bfm_observe_host.py (no vertex near a threshold)


def pose_coeff(yaw, seed=None):
  """A row of coefficients: identity and expression at the mean, angles (0, yaw, 0), translation POSE_T; with a seed, texture and
  lighting drawn from it."""
  c = np.zeros(257, np.float32)
  c[225] = yaw
  c[254:257] = POSE_T
  if seed is not None:
    rng = np.random.default_rng(seed)
    c[144:224] = rng.normal(0, 1.0, 80)
    c[227:254] = rng.normal(0, 0.1, 27)
  return c


def two_plates():
  """Two plates in a 16 x 16 buffer whose depths are written by hand: a far plate (depth 1) on the pixels 3 .. 12 x 3 .. 12, a near plate
  (depth 5) on x 7 .. 12, y 5 .. 10 in front of it, every other pixel empty (-99999).  Four vertices belong to each plate (4 triangles),
  one per case of the rule.  Returns (vertices f32 [8,3], triangles i32 [4,3], depth f32 [16,16], expected u8 [8] at TWO_PLATES_TOL)."""
  depth = np.full((16, 16), DEPTH_CLEAR, F)
  depth[3:13, 3:13] = 1.0
  depth[5:11, 7:13] = 5.0
  nan = np.nan
  vertices = [(3.5, 3.5, 1.0),            # 0 far plate, on its own surface: visible
              (9.5, 7.5, 1.0),            # 1 far plate, all four centres on the near plate: HIDDEN
              (6.5, 7.5, 1.0),            # 2 far plate, on the occlusion edge (x 6 is far, x 7 near): the minimum is its own, visible
              (14.5, 14.25, 1.0),         # 3 far plate's height over empty pixels: visible
              (7.5, 5.5, 5.0),            # 4 near plate, on its own surface: visible
              (-0.5, 3.0, 5.0),           # 5 off the buffer: visible
              (nan, 3.0, 5.0),            # 6 a NaN: visible
              (10.25, 8.75, 4.75)]        # 7 behind the near plate by exactly TWO_PLATES_TOL: z + tol == m, visible (hidden at half of it)
  tri = [(0, 2, 1), (1, 2, 3), (4, 6, 5), (5, 6, 7)]
  return np.array(vertices, F), np.array(tri, np.int32), depth, np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)


TWO_PLATES_TOL = 0.25


def painted_photo(fm, coeff, extra=None, background=128.0):
  """The 224 x 224 uint8 photo (a = 1) of the model's own colours T(delta) L(gamma) at coeff, interpolated over the visible triangles
  (rasterize_triangles_py, interpolate_py); `extra` [N] is added to every channel of the vertex colours first (the painted occluder)."""
  c = np.asarray(coeff, np.float64).reshape(257)
  R = rotation_of(coeff)
  nr, _ = ar.geometry(fm, c, R)
  col = ar.face_color(fm, ar.sh_terms(nr), ar.coeff_to_p(c))
  if extra is not None:
    col = col + np.asarray(extra, np.float64)[:, None]
  _, ids, bary = depth_raster(fm, raster_vertices(fm, c, 1, R), 1)
  img = np.full((224, 224, 3), background, F)
  mr.interpolate_py(ids, bary, (np.asarray(fm.tri) - 1).astype(np.int32), col.astype(F), img)
  return np.clip(np.round(img), 0, 255).astype(np.uint8)


def smooth_field(h, w):
  """A smooth float64 RGB field [h,w,3] in 60 .. 200 (exactly integrable over a square is not needed: area_mean samples it densely)."""
  y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
  return np.stack([130 + 50 * np.sin(2 * np.pi * (0.7 * x + 0.4 * y) + 0.3 * c) + 20 * np.cos(2 * np.pi * (1.1 * y - 0.5 * x) + c) for c in range(3)], axis=2)


def checkerboard_photo(h, w, amplitude=40.0):
  """(photo uint8, the smooth field it was made of): the field plus a +-amplitude checkerboard of 1 px period."""
  field = smooth_field(h, w)
  y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
  board = np.where((x + y) % 2 == 0, amplitude, -amplitude)[:, :, None]
  return np.clip(np.round(field + board), 0, 255).astype(np.uint8), field


def area_mean(field, px, py, a, n=8):
  """The mean of the bilinearly interpolated float field over the a x a square around (px, py), by n x n midpoint samples per unit
  length of a (dense against the field's wavelength of hundreds of pixels)."""
  H, W = field.shape[:2]
  m = int(np.ceil(a)) * n
  total = np.zeros((len(px), 3))
  for j in range(m):
    for i in range(m):
      tx = np.clip(px + ((i + 0.5) / m - 0.5) * a, 0.0, W - 1.0)
      ty = np.clip(py + ((j + 0.5) / m - 0.5) * a, 0.0, H - 1.0)
      x0 = np.minimum(np.floor(tx).astype(np.int64), W - 2)
      y0 = np.minimum(np.floor(ty).astype(np.int64), H - 2)
      fx, fy = (tx - x0)[:, None], (ty - y0)[:, None]
      total += (1 - fy) * ((1 - fx) * field[y0, x0] + fx * field[y0, x0 + 1]) + fy * ((1 - fx) * field[y0 + 1, x0] + fx * field[y0 + 1, x0 + 1])
  return total / (m * m)


def facing(fm, coeff, R=None):
  """(n . R)_z per vertex."""
  c = np.asarray(coeff, np.float64).reshape(257)
  return ar.geometry(fm, c, rotation_of(coeff) if R is None else R)[0][:, 2]


def pixel_margin(rv, side):
  """The smallest distance of an x or y of the vertices on the buffer from a pixel boundary (an integer)."""
  on = (rv[:, 0] >= 0) & (rv[:, 0] <= side - 1) & (rv[:, 1] >= 0) & (rv[:, 1] <= side - 1)
  xy = rv[on][:, :2].astype(np.float64)
  return float(np.abs(xy - np.round(xy)).min()) if len(xy) else np.inf

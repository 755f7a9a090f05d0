"""Drop-in for the reference's `mesh_core_cython` module (utils/cython/mesh_core_cython.pyx:40-99) on the MI355X (libvp_hip.so):
the flat-shaded z-buffer rasteriser that turns BFMNet's reconstructed mesh into PixReferNet's conditioning image
(voicepuppet/pixrefer/infer_bfmvid.py:100-108; vp_render_colors), and the dense correspondence - per pixel the visible triangle,
its barycentric weights and the interpolated depth (vp_rasterize_triangles), the textured render (vp_render_texture), vertex
normals (vp_vertex_normals).

`render_colors_core`, `rasterize_triangles_core`, `render_texture_core` and `get_normal_core` keep the reference's positional
signatures and in-place convention.  numpy arguments are staged through HBM (the reference's calling convention); CUDA tensors are
processed where they lie.  `render_colors`, `rasterize_triangles`, `render_texture`, `interpolate` and `vertex_normals` are the
batched forms for a clip: F frames sharing one triangle list in ONE call.  `interpolate` has no counterpart in the reference's
module (its callers do that step in numpy): it turns the buffers into smooth colours, normal maps or vertex correspondences.
No CPU fallback.
"""
import weakref

import numpy as np
import torch

from .. import _lib
from .._handle import grow, ptr, stream


_workspaces = {}


def _workspace(nbytes, device):
  key = (device.index if device.index is not None else torch.cuda.current_device())
  ws = _workspaces[key] = grow(_workspaces.get(key), nbytes, device)
  return ws


def render_colors(image, face_mask, vertices, triangles, colors, depth_buffer):
  """Batched, device-resident form.  image u8 [F,h,w,c], face_mask u8 [F,h,w], vertices f32 [F,nver,3], triangles i32 [ntri,3],
  colors f32 [F,nver,c], depth_buffer f32 [F,h,w]; image / face_mask / depth_buffer are updated in place."""
  if not torch.cuda.is_available():
    raise RuntimeError("render_colors needs an MI355X (no CPU fallback)")
  F, h, w, c = image.shape
  nver = vertices.shape[1]
  ntri = triangles.shape[0]
  for t, dt in ((image, torch.uint8), (face_mask, torch.uint8), (vertices, torch.float32), (triangles, torch.int32),
                (colors, torch.float32), (depth_buffer, torch.float32)):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dt):
      raise ValueError("render_colors: arguments must be contiguous CUDA tensors of the reference's dtypes")
  if tuple(face_mask.shape) != (F, h, w) or tuple(depth_buffer.shape) != (F, h, w) or tuple(vertices.shape) != (F, nver, 3) \
      or tuple(colors.shape) != (F, nver, c) or triangles.shape[1] != 3:
    raise ValueError("render_colors: inconsistent shapes")
  L = _lib.lib()
  nbytes = L.vp_render_colors_workspace_bytes(F, h, w)
  ws = _workspace(nbytes, image.device)
  _lib.check(L.vp_render_colors(ptr(image), ptr(face_mask), ptr(vertices), ptr(triangles), ptr(colors), ptr(depth_buffer),
                                ntri, nver, h, w, c, F, ptr(ws), stream()), "vp_render_colors")
  return image, face_mask, depth_buffer


def render_colors_core(image, face_mask, vertices, triangles, colors, depth_buffer, ntri, h, w, c):
  """mesh_core_cython.render_colors_core(image, face_mask, vertices, triangles, colors, depth_buffer, ntri, h, w, c):
  flat uint8 image [h*w*c] and face_mask [h*w], flat float32 vertices [nver*3] / colors [nver*c] / depth_buffer [h*w],
  flat int32 triangles [ntri*3]; image, face_mask and depth_buffer are overwritten in place, nothing is returned."""
  host = isinstance(image, np.ndarray)
  if host:
    for a, dt in ((image, np.uint8), (face_mask, np.uint8), (vertices, np.float32), (triangles, np.int32), (colors, np.float32),
                  (depth_buffer, np.float32)):
      if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
        raise ValueError("render_colors_core: C-contiguous numpy arrays of the reference's dtypes expected")
    dev = torch.device("cuda", torch.cuda.current_device())
    t = [torch.from_numpy(a).to(dev) for a in (image, face_mask, vertices, triangles, colors, depth_buffer)]
  else:
    t = [image, face_mask, vertices, triangles, colors, depth_buffer]
  nver = t[2].numel() // 3
  if t[3].numel() < 3 * ntri or t[0].numel() != h * w * c or t[1].numel() != h * w or t[5].numel() != h * w or t[4].numel() != nver * c:
    raise ValueError("render_colors_core: buffer sizes do not match ntri / h / w / c")
  render_colors(t[0].view(1, h, w, c), t[1].view(1, h, w), t[2].view(1, nver, 3), t[3].view(-1)[:3 * ntri].view(ntri, 3),
                t[4].view(1, nver, c), t[5].view(1, h, w))
  if host:
    image[...] = t[0].cpu().numpy().reshape(image.shape)
    face_mask[...] = t[1].cpu().numpy().reshape(face_mask.shape)
    depth_buffer[...] = t[5].cpu().numpy().reshape(depth_buffer.shape)


def _check(what, tensors):
  if not torch.cuda.is_available():
    raise RuntimeError("%s needs an MI355X (no CPU fallback)" % what)
  for t, dt in tensors:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dt):
      raise ValueError("%s: arguments must be contiguous CUDA tensors of the reference's dtypes" % what)


def rasterize_triangles(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight):
  """Batched, device-resident _rasterize_triangles_core.  vertices f32 [F,nver,3], triangles i32 [ntri,3], depth_buffer f32 [F,h,w],
  triangle_buffer i32 [F,h,w], barycentric_weight f32 [F,h,w,3]; the three buffers are updated in place, for winning pixels only."""
  _check("rasterize_triangles", ((vertices, torch.float32), (triangles, torch.int32), (depth_buffer, torch.float32),
                                 (triangle_buffer, torch.int32), (barycentric_weight, torch.float32)))
  if vertices.dim() != 3 or depth_buffer.dim() != 3 or triangles.dim() != 2:
    raise ValueError("rasterize_triangles: inconsistent shapes")
  F, h, w = depth_buffer.shape
  nver, ntri = vertices.shape[1], triangles.shape[0]
  if tuple(vertices.shape) != (F, nver, 3) or triangles.shape[1] != 3 or tuple(triangle_buffer.shape) != (F, h, w) \
      or tuple(barycentric_weight.shape) != (F, h, w, 3):
    raise ValueError("rasterize_triangles: inconsistent shapes")
  L = _lib.lib()
  ws = _workspace(L.vp_rasterize_triangles_workspace_bytes(F, h, w), depth_buffer.device)
  _lib.check(L.vp_rasterize_triangles(ptr(vertices), ptr(triangles), ptr(depth_buffer), ptr(triangle_buffer), ptr(barycentric_weight),
                                      nver, ntri, h, w, F, ptr(ws), stream()), "vp_rasterize_triangles")
  return depth_buffer, triangle_buffer, barycentric_weight


def render_texture(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, tex_nver=None, mapping_type=0):
  """Batched, device-resident _render_texture_core.  image f32 [F,h,w,c], vertices f32 [F,nver,3], triangles i32 [ntri,3], texture f32
  [tex_h,tex_w,tex_c], tex_coords f32 [rows,3], tex_triangles i32 [ntri,3], depth_buffer f32 [F,h,w]; image and depth_buffer are updated
  in place.  The reference's indexing is kept as written (x through tex_triangles, y through triangles), which is why tex_coords needs
  max(nver, tex_nver) rows; tex_nver defaults to the rows of tex_coords.  mapping_type 0 is nearest, anything else bilinear."""
  _check("render_texture", ((image, torch.float32), (vertices, torch.float32), (triangles, torch.int32), (texture, torch.float32),
                            (tex_coords, torch.float32), (tex_triangles, torch.int32), (depth_buffer, torch.float32)))
  if image.dim() != 4 or vertices.dim() != 3 or texture.dim() != 3 or tex_coords.dim() != 2 or triangles.dim() != 2:
    raise ValueError("render_texture: inconsistent shapes")
  F, h, w, c = image.shape
  nver, ntri = vertices.shape[1], triangles.shape[0]
  tex_h, tex_w, tex_c = texture.shape
  rows = tex_coords.shape[0]
  tex_nver = rows if tex_nver is None else int(tex_nver)
  if tuple(vertices.shape) != (F, nver, 3) or triangles.shape[1] != 3 or tuple(tex_triangles.shape) != (ntri, 3) or tex_coords.shape[1] != 3 \
      or tuple(depth_buffer.shape) != (F, h, w):
    raise ValueError("render_texture: inconsistent shapes")
  if c > tex_c:
    raise ValueError("render_texture: c %d > tex_c %d" % (c, tex_c))
  if rows < max(nver, tex_nver):
    raise ValueError("render_texture: tex_coords has %d rows, max(nver, tex_nver) = %d are read" % (rows, max(nver, tex_nver)))
  L = _lib.lib()
  ws = _workspace(L.vp_render_texture_workspace_bytes(F, h, w), image.device)
  _lib.check(L.vp_render_texture(ptr(image), ptr(vertices), ptr(triangles), ptr(texture), ptr(tex_coords), ptr(tex_triangles), ptr(depth_buffer),
                                 nver, tex_nver, rows, ntri, h, w, c, tex_h, tex_w, tex_c, int(mapping_type), F, ptr(ws), stream()),
             "vp_render_texture")
  return image, depth_buffer


def interpolate(triangle_buffer, barycentric_weight, triangles, attributes, out=None):
  """out[f,y,x,:] = w0*a[i0] + w1*a[i1] + w2*a[i2] for the pixel's triangle and weights (float32, that order): triangle_buffer i32 [F,h,w],
  barycentric_weight f32 [F,h,w,3], triangles i32 [ntri,3], attributes f32 [F,nver,k] -> f32 [F,h,w,k].  Pixels whose triangle id is
  negative keep what `out` holds (zeros when it is not given)."""
  _check("interpolate", ((triangle_buffer, torch.int32), (barycentric_weight, torch.float32), (triangles, torch.int32),
                         (attributes, torch.float32)))
  if triangle_buffer.dim() != 3 or attributes.dim() != 3 or triangles.dim() != 2:
    raise ValueError("interpolate: inconsistent shapes")
  F, h, w = triangle_buffer.shape
  nver, k = attributes.shape[1], attributes.shape[2]
  if out is None:
    out = torch.zeros(F, h, w, k, dtype=torch.float32, device=attributes.device)
  _check("interpolate", ((out, torch.float32),))
  if tuple(barycentric_weight.shape) != (F, h, w, 3) or triangles.shape[1] != 3 or attributes.shape[0] != F or tuple(out.shape) != (F, h, w, k):
    raise ValueError("interpolate: inconsistent shapes")
  L = _lib.lib()
  _lib.check(L.vp_raster_interpolate(ptr(out), ptr(triangle_buffer), ptr(barycentric_weight), ptr(triangles), ptr(attributes), nver,
                                     triangles.shape[0], k, h, w, F, stream()), "vp_raster_interpolate")
  return out


def vertex_visibility(vertices, depth_buffer, tol=0.0, out=None):
  """Which vertices of the mesh `rasterize_triangles` drew lie in front of the depth buffer it left (vp_raster_vertex_visibility; no
  counterpart in the reference's module): vertices f32 [F,nver,3], depth_buffer f32 [F,h,w] (h, w >= 2) -> u8 [F,nver].  A vertex is
  visible when z + tol >= the minimum of the four depths around (x, y), in float32; a vertex off the buffer or with a NaN is visible.
  tol >= 0, in the units of z."""
  _check("vertex_visibility", ((vertices, torch.float32), (depth_buffer, torch.float32)))
  if vertices.dim() != 3 or depth_buffer.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] != depth_buffer.shape[0]:
    raise ValueError("vertex_visibility: inconsistent shapes")
  F, h, w = depth_buffer.shape
  nver = vertices.shape[1]
  if out is None:
    out = torch.empty(F, nver, dtype=torch.uint8, device=vertices.device)
  _check("vertex_visibility", ((out, torch.uint8),))
  if tuple(out.shape) != (F, nver):
    raise ValueError("vertex_visibility: inconsistent shapes")
  _lib.check(_lib.lib().vp_raster_vertex_visibility(ptr(vertices), ptr(depth_buffer), ptr(out), nver, h, w, F, float(tol), stream()),
             "vp_raster_vertex_visibility")
  return out


_adjacencies = {}     # id(triangle tensor) -> (weak reference to it, its version, nver, adjacency); tensors compare elementwise, hence the id


def vertex_adjacency(triangles, nver):
  """The vertex -> (triangle, corner) adjacency vertex_normals sums through: a function of the triangle list alone, built on the device
  once per triangle tensor (and again when the tensor was written to, or for another nver)."""
  _check("vertex_adjacency", ((triangles, torch.int32),))
  if triangles.dim() != 2 or triangles.shape[1] != 3:
    raise ValueError("vertex_adjacency: triangles must be [ntri,3]")
  key = id(triangles)
  hit = _adjacencies.get(key)
  if hit is not None and hit[0]() is triangles and hit[1] == triangles._version and hit[2] == nver:
    return hit[3]
  L = _lib.lib()
  ntri = triangles.shape[0]
  nbytes = L.vp_vertex_adjacency_bytes(nver, ntri)
  if nbytes == 0:
    raise ValueError("vertex_adjacency: nver %d / ntri %d out of range" % (nver, ntri))
  adj = torch.empty(nbytes, dtype=torch.uint8, device=triangles.device)
  _lib.check(L.vp_vertex_adjacency_build(ptr(triangles), nver, ntri, ptr(adj), nbytes, stream()), "vp_vertex_adjacency_build")
  _adjacencies[key] = (weakref.ref(triangles, lambda _, key=key: _adjacencies.pop(key, None)), triangles._version, nver, adj)
  return adj


def vertex_normals(normal, tri_normal, triangles):
  """Batched, device-resident _get_normal_core: normal f32 [F,nver,3] += tri_normal f32 [F,ntri,3] of the incident triangles of triangles
  i32 [ntri,3], in the serial loop's order (ascending triangle, then corner; a repeated index adds twice).  In place."""
  _check("vertex_normals", ((normal, torch.float32), (tri_normal, torch.float32), (triangles, torch.int32)))
  if normal.dim() != 3 or tri_normal.dim() != 3 or triangles.dim() != 2:
    raise ValueError("vertex_normals: inconsistent shapes")
  F, nver, _ = normal.shape
  ntri = triangles.shape[0]
  if normal.shape[2] != 3 or tuple(tri_normal.shape) != (F, ntri, 3) or triangles.shape[1] != 3:
    raise ValueError("vertex_normals: inconsistent shapes")
  adj = vertex_adjacency(triangles, nver)
  _lib.check(_lib.lib().vp_vertex_normals(ptr(normal), ptr(tri_normal), ptr(adj), nver, ntri, F, stream()), "vp_vertex_normals")
  return normal


def _stage(what, arrays):
  """(host?, tensors): numpy arrays of the reference's dtypes go to the current device, CUDA tensors pass."""
  host = isinstance(arrays[0][0], np.ndarray)
  if not host:
    return False, [a for a, _ in arrays]
  for a, dt in arrays:
    if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
      raise ValueError("%s: C-contiguous numpy arrays of the reference's dtypes expected" % what)
  if not torch.cuda.is_available():
    raise RuntimeError("%s needs an MI355X (no CPU fallback)" % what)
  dev = torch.device("cuda", torch.cuda.current_device())
  return True, [torch.from_numpy(a).to(dev) for a, _ in arrays]


def _back(array, tensor):
  array[...] = tensor.cpu().numpy().reshape(array.shape)


def rasterize_triangles_core(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, nver, ntri, h, w):
  """mesh_core_cython.rasterize_triangles_core(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, nver, ntri, h, w):
  float32 vertices [nver,3], int32 triangles [ntri,3], float32 depth_buffer [h,w], int32 triangle_buffer [h,w], float32
  barycentric_weight [h,w,3] (the .pyx declares it 2-D; any C-contiguous layout of h*w*3 values is taken); the three buffers are
  overwritten in place, nothing is returned."""
  host, t = _stage("rasterize_triangles_core", ((vertices, np.float32), (triangles, np.int32), (depth_buffer, np.float32),
                                                (triangle_buffer, np.int32), (barycentric_weight, np.float32)))
  if t[0].numel() != nver * 3 or t[1].numel() < 3 * ntri or t[2].numel() != h * w or t[3].numel() != h * w or t[4].numel() != h * w * 3:
    raise ValueError("rasterize_triangles_core: buffer sizes do not match nver / ntri / h / w")
  rasterize_triangles(t[0].view(1, nver, 3), t[1].view(-1)[:3 * ntri].view(ntri, 3), t[2].view(1, h, w), t[3].view(1, h, w),
                      t[4].view(1, h, w, 3))
  if host:
    _back(depth_buffer, t[2])
    _back(triangle_buffer, t[3])
    _back(barycentric_weight, t[4])


def render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, nver, tex_nver, ntri, h, w, c,
                        tex_h, tex_w, tex_c, mapping_type):
  """mesh_core_cython.render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, nver, tex_nver,
  ntri, h, w, c, tex_h, tex_w, tex_c, mapping_type): float32 image [h,w,c], vertices [nver,3], texture [tex_h,tex_w,tex_c], tex_coords
  [rows,3], depth_buffer [h,w], int32 triangles / tex_triangles [ntri,3]; image and depth_buffer are overwritten in place."""
  host, t = _stage("render_texture_core", ((image, np.float32), (vertices, np.float32), (triangles, np.int32), (texture, np.float32),
                                           (tex_coords, np.float32), (tex_triangles, np.int32), (depth_buffer, np.float32)))
  if t[0].numel() != h * w * c or t[1].numel() != nver * 3 or t[2].numel() < 3 * ntri or t[3].numel() != tex_h * tex_w * tex_c \
      or t[4].numel() % 3 or t[5].numel() < 3 * ntri or t[6].numel() != h * w:
    raise ValueError("render_texture_core: buffer sizes do not match the integer arguments")
  render_texture(t[0].view(1, h, w, c), t[1].view(1, nver, 3), t[2].view(-1)[:3 * ntri].view(ntri, 3), t[3].view(tex_h, tex_w, tex_c),
                 t[4].view(-1, 3), t[5].view(-1)[:3 * ntri].view(ntri, 3), t[6].view(1, h, w), tex_nver=tex_nver, mapping_type=mapping_type)
  if host:
    _back(image, t[0])
    _back(depth_buffer, t[6])


def get_normal_core(normal, tri_normal, triangles, ntri):
  """mesh_core_cython.get_normal_core(normal, tri_normal, triangles, ntri): float32 normal [nver,3] += float32 tri_normal [ntri,3] of the
  incident triangles of int32 triangles [ntri,3], in place."""
  host, t = _stage("get_normal_core", ((normal, np.float32), (tri_normal, np.float32), (triangles, np.int32)))
  if t[0].numel() % 3 or t[1].numel() < 3 * ntri or t[2].numel() < 3 * ntri:
    raise ValueError("get_normal_core: buffer sizes do not match ntri")
  nver = t[0].numel() // 3
  # the caller's own [ntri,3] tensor where possible: the adjacency is cached per triangle tensor
  tri = t[2] if tuple(t[2].shape) == (ntri, 3) else t[2].view(-1)[:3 * ntri].view(ntri, 3)
  vertex_normals(t[0].view(1, nver, 3), t[1].view(-1)[:3 * ntri].view(1, ntri, 3), tri)
  if host:
    _back(normal, t[0])

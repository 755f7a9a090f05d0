"""Captures tests/golden/mesh_core_dense.npz from the COMPILED reference (oracle/_ref/libmesh_core_ref.so, `make -C oracle`): for the two
synthetic meshes of tests/mesh_core_ref.py the depth / triangle-id / barycentric buffers of _rasterize_triangles_core, the texture render
of _render_texture_core in both mapping modes and the vertex normals of _get_normal_core onto a non-zero start, with the seeded inputs
they were made from.  Arrays only.  Run from the repository root in the build container: python tests/golden/make_mesh_core_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_core_ref as mr  # noqa: E402


def main():
  assert mr.have_compiled_reference(), "make -C oracle first"
  out = {}
  for n, tag in enumerate(mr.MESHES):
    v, t, h, w = mr.mesh(tag)
    nver, ntri = v.shape[0], t.shape[0]
    depth, ids, bary, _ = mr.fresh_buffers(h, w)
    mr.rasterize_triangles_ref(v, t, depth, ids, bary, h, w)
    texture, tex_coords, tex_triangles = mr.texture_inputs(nver, ntri, seed=100 + n)
    normal0, tri_normal = mr.normal_inputs(nver, ntri, seed=200 + n)
    out.update({tag + "_vertices": v, tag + "_triangles": t, tag + "_depth": depth, tag + "_ids": ids, tag + "_weights": bary,
                tag + "_texture": texture, tag + "_tex_coords": tex_coords, tag + "_tex_triangles": tex_triangles,
                tag + "_normal0": normal0, tag + "_tri_normal": tri_normal,
                tag + "_normal": mr.get_normal_ref(normal0.copy(), tri_normal, t)})
    for mode in (0, 1):
      d, _, _, image = mr.fresh_buffers(h, w)
      mr.render_texture_ref(image, v, t, texture, tex_coords, tex_triangles, d, h, w, mode)
      out["%s_tex%d_image" % (tag, mode)] = image
      out["%s_tex%d_depth" % (tag, mode)] = d
  path = os.path.join(HERE, "mesh_core_dense.npz")
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
  main()

"""Device time of the dense rasteriser (voicepuppet_amd.utils.mesh_core.rasterize_triangles, libvp_hip.so vp_rasterize_triangles) on one
GPU, next to the flat-shaded vp_render_colors on the same mesh in the same run: writes profiles/mesh_core_dense.json.

  mesh      oracle/raster_ref.synthetic_mesh(seed=0, nlat=189, nlon=189, extra=False) at 224 x 224: 35,721 vertices / 71,064 triangles (the
            BFM front model has 35,709 / about 70 k); frame f is the mesh shifted by a pixel or two with its depth scaled
  stages    for F in {1, 64} frames: HIP events on an otherwise idle stream, warm, median and p90 of --reps, around
              clear            the three fills that reset depth / ids / weights (part of every figure below)
              render_colors    clear of its buffers + vp_render_colors
              rasterize        clear + vp_rasterize_triangles
              texture_nearest  clear + vp_render_texture, mapping_type 0, 256 x 256 x 3 texture
              texture_bilinear the same with mapping_type 1
              interpolate      vp_raster_interpolate of 3 attributes through the buffers
              normals          vp_vertex_normals with the adjacency built (adjacency_build: the one-off build)
  check     frame 0 of the 64-frame run equals the reference's compiled mesh_core.cpp bit for bit when oracle/_ref is built, else null
Usage: python scripts/mesh_core_latency.py [--reps 50] [--out profiles/mesh_core_dense.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = 224


def timed(fn, reps):
  import torch
  st, ms = torch.cuda.current_stream(), []
  for r in range(reps + 10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    if r >= 10:
      ms.append(e0.elapsed_time(e1))
  return {"device_ms_median": float(np.median(ms)), "device_ms_p90": float(np.percentile(ms, 90))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=50)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_core_dense.json"))
  a = ap.parse_args()
  import torch
  import mesh_core_ref as mr
  from oracle import raster_ref as rr
  from voicepuppet_amd.utils import mesh_core
  h = w = SIZE
  v0, tri, c0 = rr.synthetic_mesh(seed=0, nlat=189, nlon=189, h=h, w=w, extra=False)
  nver, ntri = v0.shape[0], tri.shape[0]
  rng = np.random.default_rng(0)
  texture = torch.from_numpy(rng.uniform(0, 1, size=(256, 256, 3)).astype(np.float32)).cuda()
  tex_coords = torch.from_numpy(rng.uniform(0, 255, size=(nver, 3)).astype(np.float32)).cuda()
  T = torch.from_numpy(tri).cuda()
  stages, check = [], None
  for F in (1, 64):
    vs = np.repeat(v0[None], F, 0)
    vs[:, :, :2] += rng.normal(0, 1.5, size=(F, 1, 2)).astype(np.float32)
    vs[:, :, 2] *= (1 + 0.01 * np.arange(F, dtype=np.float32))[:, None]
    V = torch.from_numpy(vs).cuda()
    C = torch.from_numpy(np.repeat(c0[None], F, 0)).cuda()
    image8 = torch.zeros(F, h, w, 3, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(F, h, w, dtype=torch.uint8, device="cuda")
    depth = torch.empty(F, h, w, dtype=torch.float32, device="cuda")
    ids = torch.empty(F, h, w, dtype=torch.int32, device="cuda")
    bary = torch.empty(F, h, w, 3, dtype=torch.float32, device="cuda")
    image = torch.empty(F, h, w, 3, dtype=torch.float32, device="cuda")
    normal = torch.zeros(F, nver, 3, dtype=torch.float32, device="cuda")
    tri_normal = torch.from_numpy(rng.normal(size=(F, ntri, 3)).astype(np.float32)).cuda()

    def clear():
      depth.fill_(float(mr.DEPTH_INIT))
      ids.fill_(-1)
      bary.zero_()

    def colors():
      depth.fill_(float(mr.DEPTH_INIT))
      image8.zero_()
      mask.zero_()
      mesh_core.render_colors(image8, mask, V, T, C, depth)

    def rasterize():
      clear()
      mesh_core.rasterize_triangles(V, T, depth, ids, bary)

    def textured(mode):
      depth.fill_(float(mr.DEPTH_INIT))
      image.zero_()
      mesh_core.render_texture(image, V, T, texture, tex_coords, T, depth, mapping_type=mode)

    row = {"frames": F, "size": SIZE, "vertices": nver, "triangles": ntri,
           "clear": timed(clear, a.reps),
           "render_colors": timed(colors, a.reps),
           "rasterize": timed(rasterize, a.reps),
           "texture_nearest": timed(lambda: textured(0), a.reps),
           "texture_bilinear": timed(lambda: textured(1), a.reps)}
    rasterize()
    row["coverage"] = float((ids >= 0).float().mean())
    row["interpolate"] = timed(lambda: mesh_core.interpolate(ids, bary, T, V, out=image), a.reps)
    if F == 1:
      fresh = T.clone()                                       # a tensor the cache has not seen: every call builds
      row["adjacency_build"] = timed(lambda: (fresh.add_(0), mesh_core.vertex_adjacency(fresh, nver)), a.reps)
    mesh_core.vertex_adjacency(T, nver)
    row["normals"] = timed(lambda: mesh_core.vertex_normals(normal, tri_normal, T), a.reps)
    stages.append(row)
    if F == 64 and mr.have_compiled_reference():
      d, i, b, _ = mr.fresh_buffers(h, w)
      mr.rasterize_triangles_ref(vs[0], tri, d, i, b, h, w)
      check = bool(np.array_equal(i, ids[0].cpu().numpy()) and np.array_equal(d.view(np.uint32), depth[0].cpu().numpy().view(np.uint32))
                   and np.array_equal(b.view(np.uint32), bary[0].cpu().numpy().view(np.uint32)))
  res = {"metric": "mesh_core_dense",
         "parent_commit": subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None,
         "device": torch.cuda.get_device_name(0), "reps": a.reps, "stages": stages, "frame0_bit_exact_vs_compiled_reference": check}
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()

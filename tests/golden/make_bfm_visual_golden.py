"""Regenerates tests/golden/bfm_visual.npz (run in the build container only, like make_golden.py: it imports the REFERENCE's own
utils/reconstruct_mesh.py from /root/reference, pure numpy, and rasterises with the reference's compiled mesh_core.cpp, oracle/_ref,
`make -C oracle`).

  python tests/golden/make_bfm_visual_golden.py

Contents, for oracle.bfm_ref.synthetic_facemodel(seed) on its default 14 x 18 grid: the seed and the model checksum (as bfm_recon.npz);
real [1,12,257], pred [1,12,64], seq_len; for the 12 real frames and the 12 frames with the predicted expression spliced in
(utils/bfm_visual.py:148), `Reconstruction`'s seven outputs per frame, the float32 vertices and colours of the montage's packing
(bfm_visual.py:100-112, view 0) and of infer_bfmnet.py:212-216 (view 1, scale 3), and the 24 rasterised 224 x 224 tiles.

cv2 is not installed here, so plot_bfm_coeff_seq itself cannot run: its placement lines (:125-128) are restated by
tests/bfm_visual_ref.py on top of these reference-made tiles.  The fixture holds data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
MODEL_SEED, SEQ_SEED, FRAMES = 11, 23, 12


def main():
  from oracle import bfm_ref as br
  from oracle import raster_ref as rr
  import bfm_visual_ref as vr
  sys.path.insert(0, os.path.join(REF, "utils"))
  import reconstruct_mesh as rm                        # the reference module itself (numpy only)
  assert rr.have_compiled_reference(), "run `make -C oracle` first"
  fm = br.synthetic_facemodel(MODEL_SEED)
  real, pred = vr.synthetic_sequences(FRAMES, SEQ_SEED)
  d = {"model_seed": MODEL_SEED, "seq_seed": SEQ_SEED, "real": real, "pred": pred, "seq_len": np.array([FRAMES], np.int32)}
  d["model_checksum"] = np.array([fm.idBase.sum(), fm.exBase.sum(), fm.texBase.sum(), fm.meanshape.sum(), fm.meantex.sum(),
                                  float(fm.tri.sum()), float(fm.point_buf.sum()), float(fm.keypoints.sum())])
  # bfm_visual.py:148 (the id_coeff=None branch), written out: the reference's own concatenate
  spliced = np.concatenate([real[:, :, :80], pred[:, :, :], real[:, :, 144:]], axis=2)
  tri = (fm.tri - 1).reshape(-1).astype(np.int32).copy()
  for tag, seq in (("real", real), ("pred", spliced)):
    outs = {n: [] for n in vr.NAMES}
    v0, v1, cols, tiles = [], [], [], []
    for i in range(FRAMES):
      res = rm.Reconstruction(seq[0, i:i + 1, ...], fm)                         # bfm_visual.py:97-98
      for n, r in zip(vr.NAMES, res):
        outs[n].append(np.array(r[0]))
      face_shape, _, face_color, face_projection, z_buffer = res[:5]
      # bfm_visual.py:100-115
      shape = np.squeeze(np.concatenate([face_projection, z_buffer], axis=2), (0))
      color = np.clip(np.squeeze(face_color, (0)), 0, 255).astype(np.int32)
      vertices = shape.reshape(-1).astype(np.float32).copy()
      colors = color.reshape(-1).astype(np.float32).copy()
      tiles.append(rr.render_colors_ref(vertices, tri, colors, 224, 224)[0])
      v0.append(vertices.reshape(-1, 3)); cols.append(colors.reshape(-1, 3))
      # infer_bfmnet.py:212-222 (on a copy: the reference scales the returned face_shape in place)
      shape = np.squeeze(face_shape.copy(), (0))
      shape[:, :2] = 112 - shape[:, :2] * 112
      shape *= 3
      v1.append(shape.reshape(-1).astype(np.float32).copy().reshape(-1, 3))
    for n in vr.NAMES:
      d["%s_%s" % (tag, n)] = np.stack(outs[n])
    d[tag + "_vertices_view0"], d[tag + "_vertices_view1"], d[tag + "_colors"] = np.stack(v0), np.stack(v1), np.stack(cols)
    d[tag + "_tiles"] = np.stack(tiles)
  path = os.path.join(HERE, "bfm_visual.npz")
  np.savez_compressed(path, **d)
  print(path, os.path.getsize(path), "bytes")
  assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
  main()

"""Cost of BFMNet's visual evaluation on one GPU (voicepuppet_amd.bfmnet.visual, ClipRenderer.render_view): writes profiles/mesh_sheet.json.

  sheet   device time of one MeshSheet.render for a 30-frame clip (30 + 30 tiles of 224 x 224: reconstruction, raster, the two sheet
          launches, the landmark distance) and of MeshSheet.jpeg (the sheet's four strips through the device encoder, lengths read back)
  clip    device time of a 200-frame view-1 clip at 672 x 672, scale 3, one shared texture, in batches of 8 (infer_bfmnet.py's loop
          without the files)
HIP events on the current stream, warm, median of 20 repetitions after 5 warm-up ones.  The face model is the synthetic one at the BFM's
size (35709 vertices, oracle.bfm_ref.synthetic_facemodel(smooth=True)) unless --mat names a BFM_model_front.mat.  No threshold is set.
Usage: python scripts/mesh_sheet_latency.py [--mat BFM/BFM_model_front.mat] [--out profiles/mesh_sheet.json]
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


def timed(fn, rounds=25, warm=5):
  import torch
  st = torch.cuda.current_stream()
  ms = []
  for i in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    if i >= warm:
      ms.append(e0.elapsed_time(e1))
  return {"ms_median": float(np.median(ms)), "ms_p90": float(np.percentile(ms, 90)), "repetitions": len(ms)}


def face_model(mat):
  from oracle import bfm_ref as br
  if mat:
    from scipy.io import loadmat
    m = loadmat(mat)
    return br.FaceModel(m["meanshape"], m["idBase"], m["exBase"], m["meantex"], m["texBase"], m["point_buf"], m["tri"],
                        np.squeeze(m["keypoints"]).astype(np.int32) - 1), os.path.basename(mat)
  return br.synthetic_facemodel(0, nlat=189, nlon=189, smooth=True), "synthetic 189 x 189 grid (35721 vertices)"


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--mat", default=None)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sheet.json"))
  a = ap.parse_args()
  import torch
  import bfm_visual_ref as vr
  from voicepuppet_amd.bfmnet.visual import MeshSheet
  from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer
  fm, name = face_model(a.mat)
  ms = MeshSheet(fm)
  real, pred = vr.synthetic_sequences(30, 1)
  real_d, pred_d = torch.from_numpy(real).cuda(), torch.from_numpy(pred).cuda()
  rec = {"metric": "mesh_sheet", "device": torch.cuda.get_device_name(0), "face_model": name, "vertices": ms.model.nver, "triangles": ms.model.ntri,
         "commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None,
         "timing": "hip events, median of 20 warm repetitions"}
  rec["sheet_render_30_plus_30_tiles"] = timed(lambda: ms.render([30], real_d, pred_d))
  rec["sheet_jpeg"] = dict(timed(lambda: ms.jpeg()), bytes=len(ms.jpeg()))
  renderer = ClipRenderer(ms.model, 672, 672)
  clip = torch.from_numpy(np.tile(real[0, :1], (200, 1))).cuda()
  clip[:, 80:144] = torch.from_numpy(np.tile(pred[0], (7, 1))[:200]).cuda()

  def run_clip():
    for i0 in range(0, 200, 8):
      renderer.render_view(clip[i0:i0 + 8], view=1, scale=3, shared_texture=True)
  rec["clip_200_frames_672_view1_batches_of_8"] = timed(run_clip)
  line = json.dumps(rec, indent=1)
  print(line)
  out = os.path.abspath(a.out)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

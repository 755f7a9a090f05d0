"""What moving one conditioned frame between generator batch rows and plans changes: the yardstick of tests/test_gpu_puppet_group.py.

The same 512 x 512 conditioned frame (random inputs / fg_inputs / targets, saved random generator weights) runs at row 0 of a frame_batch 1
plan and at rows 0 and 3 of a frame_batch 4 plan (the other rows hold other frames; per-sample batch norm).  Records max |d| of the float
`Outputs` and of the uint8 frames over the three pairs, as one JSON line.  It uses nothing but infer_bfmvid.load_generator and the engine's
forward / fetch, so it runs unchanged on the commit before stream groups for frames: run it THERE and pass that commit's hash.
Usage: python scripts/puppet_group_parity.py --commit <hash> [--out profiles/puppet_group_parity.json]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--commit", required=True)
  ap.add_argument("--frames", type=int, default=3)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import torch
  from voicepuppet_amd.pixrefer import infer_bfmvid as ib
  cfg = os.path.join(ROOT, "config", "params.yml")
  out = os.path.abspath(a.out) if a.out else None
  os.chdir(tempfile.mkdtemp())
  gen = ib.load_generator(cfg, 4, 512)[0]
  os.makedirs("ckpt_pixrefer")
  np.savez(ib.PIX_CKPT + ".npz", **gen.engine.get_params(0))
  ib._GENERATORS.clear()
  e1, e4 = ib.load_generator(cfg, 1, 512)[0].engine, ib.load_generator(cfg, 4, 512)[0].engine
  rng = np.random.default_rng(0)

  def rand(n, c):
    return torch.from_numpy(rng.uniform(size=(n, 512, 512, c)).astype(np.float32)).cuda()

  def run(eng, x, f, t, row):
    eng.forward(x, f, t)
    return eng.fetch("Outputs")[row].cpu().numpy(), eng.fetch("Outputs_u8")[row].cpu().numpy()

  fmax, umax, rel = 0.0, 0, 0.0
  for _ in range(a.frames):
    x, f, t = rand(4, 6), rand(4, 3), rand(4, 3)
    ref = run(e1, x[:1].contiguous(), f[:1].contiguous(), t[:1].contiguous(), 0)
    at0 = run(e4, x, f, t, 0)
    perm = [3, 1, 2, 0]
    at3 = run(e4, x[perm].contiguous(), f[perm].contiguous(), t[perm].contiguous(), 3)
    for p, q in ((ref, at0), (ref, at3), (at0, at3)):
      fmax = max(fmax, float(np.abs(p[0] - q[0]).max()))
      umax = max(umax, int(np.abs(p[1].astype(np.int32) - q[1].astype(np.int32)).max()))
      rel = max(rel, float(np.linalg.norm((p[0] - q[0]).ravel()) / np.linalg.norm(p[0].ravel())))
  line = json.dumps({"metric": "generator_batch_row_sensitivity", "commit": a.commit, "device": torch.cuda.get_device_name(0),
                     "frames": a.frames, "outputs_max_abs": fmax, "outputs_rel_l2_max": rel, "u8_max_abs": umax})
  print(line)
  if out:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
      fh.write(line + "\n")


if __name__ == "__main__":
  main()

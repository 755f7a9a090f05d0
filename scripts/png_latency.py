"""Cost of one summary step's image summaries (voicepuppet_amd.png, libvp_hip.so vp_png_*) on one GPU: writes profiles/png_encode.json.

  device    device time of the fifteen 512 x 512 encodes of a summary step (five vp_png_encode calls of three frames each, float32 sources
            as the training step holds them: a 6-channel input read at channels 3:6 and 0:3, three 3-channel tensors), HIP events around
            the ten launches on an otherwise idle stream, warm, median and p90 of --reps; then the wall time of the copy of the used bytes
  host      the path it replaces, in the same run on the same machine: the float32 device-to-host copy of the same fifteen images (47 MB),
            the float -> uint8 conversion and PIL's save(..., 'PNG') of each, on one core as the reference's summary op does it; wall time,
            median of --host_reps, at PIL's default compress_level and at 1
  sizes     the bytes of both paths per summary
The images: the fixture panel of tests/golden/jpeg_frames.npz as inputs and targets, a smoothed copy of it as outputs, a soft disc as
alphas - the flat and photographic content the summaries are made of - different per frame by a shift.
Usage: python scripts/png_latency.py [--reps 50] [--host_reps 5] [--out profiles/png_encode.json]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, K = 512, 3


def sources():
  """the five float32 tensors [K, S, S, P] of a summary step and the (tensor index, channel offset) of each summary"""
  panel = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_frames.npz"))["sample22_panel"].astype(np.float32) / 255.0
  frames = np.stack([np.roll(panel, 37 * i, axis=1) for i in range(K)])
  blur = frames.copy()
  for ax in (1, 2):
    blur = (np.roll(blur, 1, ax) + 2 * blur + np.roll(blur, -1, ax)) / 4
  y, x = np.mgrid[0:S, 0:S]
  disc = np.clip((200.0 - np.hypot(x - 256, y - 280)) / 12.0, 0, 1).astype(np.float32)
  alphas = np.stack([np.repeat(np.roll(disc, 11 * i, axis=1)[..., None], 3, -1) for i in range(K)])
  inputs = np.concatenate([blur[:, ::-1], frames], -1)            # channels 0:3 and 3:6
  tensors = [np.ascontiguousarray(t, np.float32) for t in (inputs, frames[:, :, ::-1].copy(), blur, alphas)]
  plan = (("inputs1", 0, 3), ("targets", 1, 0), ("outputs", 2, 0), ("alphas", 3, 0), ("inputs0", 0, 0))
  return tensors, plan


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=50)
  ap.add_argument("--host_reps", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.json"))
  a = ap.parse_args()
  import torch
  from PIL import Image
  import png_ref
  from voicepuppet_amd.png import PngEncoder
  tensors, plan = sources()
  dev = [torch.from_numpy(t).to("cuda") for t in tensors]
  enc = PngEncoder(K, S, S, channels=3)
  st = torch.cuda.current_stream()

  def enqueue():
    return [enc.encode(dev[i], channel_offset=off) for _, i, off in plan]

  ms, copy_ms = [], []
  for r in range(a.reps + 10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    pending = enqueue()
    e1.record(st)
    e1.synchronize()
    t = time.perf_counter()
    files = [f for rows, n in pending for f in enc.to_host(rows, n)]
    if r >= 10:
      ms.append(e0.elapsed_time(e1))
      copy_ms.append(1000.0 * (time.perf_counter() - t))
  # what the device wrote is what the restatement says, and PIL reads the images back
  want = [png_ref.to_u8(tensors[i][k][..., off:off + 3]) for _, i, off in plan for k in range(K)]
  assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), w) for f, w in zip(files, want))
  assert files[0] == png_ref.encode(want[0])

  def host_path(level):
    t = time.perf_counter()
    out = []
    for _, i, off in plan:
      x = dev[i][..., off:off + 3].cpu().numpy()                  # the float32 copy a fetch of the summary's tensor makes
      for k in range(K):
        buf = io.BytesIO()
        Image.fromarray(png_ref.to_u8(x[k])).save(buf, "PNG", **({} if level is None else {"compress_level": level}))
        out.append(buf.getvalue())
    return 1000.0 * (time.perf_counter() - t), out
  host = {}
  for level in (None, 1):
    runs = [host_path(level) for _ in range(a.host_reps)]
    host["default" if level is None else "level_%d" % level] = {"wall_ms_median": float(np.median([r[0] for r in runs])),
                                                               "wall_ms_min": float(min(r[0] for r in runs)),
                                                               "bytes": sum(len(f) for f in runs[0][1])}
  res = {"metric": "png_encode",
         "parent_commit": subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None,
         "images": "%d x %d x %d x 3 float32 (five summaries of three)" % (len(plan) * K, S, S), "reps": a.reps,
         "rows_per_strip": enc.rows_per_strip,
         "device": {"name": torch.cuda.get_device_name(0), "launches": 2 * len(plan), "device_ms_median": float(np.median(ms)),
                    "device_ms_p90": float(np.percentile(ms, 90)), "used_bytes_copy_wall_ms_median": float(np.median(copy_ms)),
                    "bytes": sum(len(f) for f in files), "float32_bytes_not_copied": len(plan) * K * S * S * 3 * 4},
         "host_float32_copy_and_pil": host,
         "per_summary_bytes": {name: {"device": sum(len(f) for f in files[j * K:(j + 1) * K])} for j, (name, _, _) in enumerate(plan)}}
  res["device_over_host_default"] = res["device"]["device_ms_median"] / host["default"]["wall_ms_median"]
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()

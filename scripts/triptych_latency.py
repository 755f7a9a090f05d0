"""Device time of the training-triptych stages (voicepuppet_amd.triptych, libvp_hip.so vp_triptych_*) on one GPU: writes
profiles/triptych.json.

  stages    for T in {1, 64} frames and S in {256, 512}: HIP events on an otherwise idle stream, warm, median and p90 of --reps, around
              fill        vp_triptych_fill_holes alone (stage a; the masks are rasterised discs with a mouth hole, two rounds)
              mask_chain  vp_triptych_mask without the fill (stages b-d: four launches)
              matte       vp_triptych_build with an alpha matte (stages e and g: the compose launch alone)
              build       vp_triptych_build (stages a-f: six launches)
            and for the worst case of the fill, the one-pixel spiral corridor of tests/test_triptych_host.py, open to the border (the
            outside walks a turn or two per round)
  jpeg      the fidelity of the device-encoded triptych at quality 95 (cv2.imwrite's default, which write() uses) against the host encoder
            of the same format: PSNR of each decoded file against the raw triptych, device minus host, in dB
The frames are the fixture content of the JPEG tests (a ramp with noise); sides and positions differ per frame.
Usage: python scripts/triptych_latency.py [--reps 50] [--out profiles/triptych.json]
"""
import argparse
import io
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FACE = 224


def scene(T, S, rng):
  yy, xx = np.mgrid[0:FACE, 0:FACE]
  masks, renders = [], []
  for t in range(T):
    m = ((yy - 112) ** 2 / 95.0 ** 2 + (xx - 112 - t % 7) ** 2 / 75.0 ** 2 <= 1).astype(np.uint8)
    m[(yy - 150) ** 2 / 10.0 ** 2 + (xx - 112) ** 2 / 25.0 ** 2 <= 1] = 0                   # the mouth hole the fill closes
    masks.append(m * 255)
    renders.append((np.stack([xx, yy, (xx + yy) // 2], -1) * m[..., None]).astype(np.uint8))
  ys, xs = np.mgrid[0:S, 0:S]
  base = np.stack([xs * 255 // (S - 1), ys * 255 // (S - 1), ((xs + ys) * 5) % 256], -1)
  frames = np.stack([(base + rng.integers(-20, 20, base.shape)).clip(0, 255).astype(np.uint8) for _ in range(min(T, 4))])
  frames = frames[np.arange(T) % frames.shape[0]]
  sides = [int(S * 0.7) + (t % 9) for t in range(T)]
  geometry = np.array([[s, (S - s) // 2 - t % 5, (S - s) // 2 + t % 3] for t, s in enumerate(sides)])
  alpha = np.stack([m_[..., 0] for m_ in frames])
  return frames, np.stack(renders), np.stack(masks), geometry, alpha


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


def psnr(a, b):
  d = a.astype(np.float64) - b.astype(np.float64)
  return float(10.0 * np.log10(255.0 ** 2 / np.mean(d * d)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=50)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triptych.json"))
  a = ap.parse_args()
  import torch
  from PIL import Image
  import test_triptych_host as host
  import triptych_ref as tr
  from voicepuppet_amd.jpeg import host_jpeg
  from voicepuppet_amd.triptych import TriptychBuilder, fill_holes
  rng = np.random.default_rng(0)
  stages, fidelity = [], None
  for S in (256, 512):
    for T in (1, 64):
      frames, render, mask, geometry, alpha = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in scene(T, S, rng))
      b = TriptychBuilder(S, T)
      out = torch.zeros(T, S, 3 * S, 3, dtype=torch.uint8, device="cuda")
      row = {"frames": T, "size": S,
             "fill": timed(lambda: fill_holes(mask), a.reps),
             "mask_chain": timed(lambda: b.mask(mask, geometry, fill=False), a.reps),
             "matte": timed(lambda: b.build(frames, render, None, geometry, alpha=alpha, out=out), a.reps),
             "build": timed(lambda: b.build(frames, render, mask, geometry, out=out), a.reps)}
      trip, status = b.build(frames, render, mask, geometry, out=out)
      assert not status.any()
      # what was timed is what the restatement says (frame 0)
      want, _ = tr.triptych(frames[0].cpu().numpy(), render[0].cpu().numpy(), mask[0].cpu().numpy(), geometry[0].cpu().numpy())
      assert np.array_equal(trip[0].cpu().numpy(), want)
      stages.append(row)
      if S == 256 and T == 64:
        files = b.encode(trip[:8], 95)
        raw = trip[:8].cpu().numpy()
        dec = lambda data: np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))  # noqa: E731
        diffs = [psnr(dec(files[i]), raw[i]) - psnr(dec(host_jpeg(raw[i], 95)), raw[i]) for i in range(8)]
        fidelity = {"quality": 95, "frames": 8, "size": "256 x 768", "device_minus_host_psnr_db": diffs, "worst_db": min(diffs),
                    "bound_db": -0.18}
  corridor, turns = host.spiral(open_to_border=True)       # open: the outside has to walk the whole corridor, a turn or two per round
  sp = torch.from_numpy(corridor).cuda()[None]
  spiral = dict(timed(lambda: fill_holes(sp), a.reps), turns=turns, size=int(corridor.shape[0]))
  res = {"metric": "triptych",
         "parent_commit": subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None,
         "device": torch.cuda.get_device_name(0), "reps": a.reps, "stages": stages, "fill_spiral_worst_case": spiral, "jpeg_fidelity": fidelity}
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == "__main__":
  main()

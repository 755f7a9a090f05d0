"""Cost of the device JPEG encoder (voicepuppet_amd.jpeg, libvp_hip.so vp_jpeg_*) on one GPU: writes profiles/jpeg_encode.json.

  quality   per fixture of tests/golden/jpeg_frames.npz (+ sample22_256): PSNR and size of the float64 restatement (tests/jpeg_ref.py) and
            of PIL (quality=75, subsampling=2, restart_marker_rows=1) on the CPU: where the test margins come from
  encode    device time of vp_jpeg_encode for 1, 8 and 64 frames of 512 x 512 (HIP events around the two launches, warm, median of 50; the
            frames cycle through the fixture panel, a noise frame and a flat frame), the bytes read and written
  host      wall time PIL takes for the same 64 frames on the thread pool infer_streams.py uses (min(8, cpus - 1) workers)
  push      one 64-talker PuppetStreamGroup push (frame_batch 32, f32 trunk, one frame per slot) with and without jpeg_quality: device span
            by the method of scripts/puppet_group_latency.py, medians of --pushes pushes
Usage: python scripts/jpeg_latency.py [--pushes 30] [--no_push] [--out profiles/jpeg_encode.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def fixtures():
  z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_frames.npz"))
  fx = {k: z[k] for k in z.files}
  fx["sample22_256"] = np.load(os.path.join(ROOT, "tests", "golden", "sample22_256.npz"))["frame"]
  return fx


def pil_bytes(frame):
  from PIL import Image
  buf = io.BytesIO()
  Image.fromarray(frame).save(buf, "JPEG", quality=75, subsampling=2, restart_marker_rows=1)
  return buf.getvalue()


def quality():
  import jpeg_ref as jr
  from PIL import Image
  rows = []
  for name, f in fixtures().items():
    ours, pil = jr.encode(f, 75)[1], pil_bytes(f)
    po, pp = (jr.psnr(np.asarray(Image.open(io.BytesIO(b))), f) for b in (ours, pil))
    rows.append({"fixture": name, "shape": list(f.shape), "restatement_bytes": len(ours), "pil_bytes": len(pil), "restatement_psnr_db": round(po, 3),
                 "pil_psnr_db": round(pp, 3), "psnr_minus_pil_db": round(po - pp, 3), "size_over_pil": round(len(ours) / len(pil), 4)})
  return {"fixtures": rows, "worst_psnr_deficit_db": round(max(-r["psnr_minus_pil_db"] for r in rows), 3),
          "worst_size_over_pil": max(r["size_over_pil"] for r in rows)}


def encode_times():
  import torch
  from voicepuppet_amd.jpeg import JpegEncoder
  fx = fixtures()
  rng = np.random.default_rng(5)
  kinds = [fx["sample22_panel"], rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), np.full((512, 512, 3), 77, np.uint8)]
  frames = np.stack([kinds[i % 3] for i in range(64)])
  dev = torch.from_numpy(frames).to("cuda")
  enc = JpegEncoder(512, 512, 64)
  out = torch.empty(64, enc.capacity, dtype=torch.uint8, device="cuda")
  lengths = torch.empty(64, dtype=torch.int32, device="cuda")
  st = torch.cuda.current_stream()
  rows = []
  for n in (1, 8, 64):
    ms = []
    for i in range(60):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record(st)
      enc.encode(dev[:n], out, lengths)
      e1.record(st)
      e1.synchronize()
      if i >= 10:
        ms.append(e0.elapsed_time(e1))
    written = int(lengths[:n].sum())
    rows.append({"frames": n, "device_ms_median": float(np.median(ms)), "device_ms_p90": float(np.percentile(ms, 90)), "bytes_read": n * 512 * 512 * 3,
                 "bytes_written": written, "frames_per_second": n * 1000.0 / float(np.median(ms))})
  # the host pool of infer_streams.py on the same frames
  from concurrent.futures import ThreadPoolExecutor
  workers = max(1, min(8, (os.cpu_count() or 2) - 1))
  pool = ThreadPoolExecutor(max_workers=workers)
  walls = []
  for i in range(6):
    t = time.perf_counter()
    list(pool.map(pil_bytes, frames))
    walls.append(1000.0 * (time.perf_counter() - t))
  t = time.perf_counter()
  for f in frames[:16]:
    pil_bytes(f)
  one_core = 1000.0 * (time.perf_counter() - t) / 16
  pool.shutdown()
  host = {"frames": 64, "workers": workers, "wall_ms_median": float(np.median(walls[1:])), "one_core_ms_per_frame": one_core,
          "raw_bytes_to_host": 64 * 512 * 512 * 3}
  return rows, host


def push_times(pushes):
  import torch
  import puppet_group_latency as pg
  from voicepuppet_amd.stream import PuppetStreamGroup
  S, nb = 64, 32
  image, photos = pg.assets(S)
  rows = []
  for q in (None, 75):
    g = PuppetStreamGroup(pg.CFG, S, frame_batch=nb, max_chunk_frames=1, dtype="f32", jpeg_quality=q)
    for s in range(S):
      g.attach(s, image, photos[s])
    rng = np.random.default_rng(0)
    st = torch.cuda.current_stream()
    ms, warm = [], 5
    for i in range(pushes + 60):
      if len(ms) >= pushes:
        break
      k = g.audio.ready({s: 640 for s in range(S)})
      ears = {s: np.full((k[s], 1), 0.005, np.float32) for s in range(S) if k[s]}
      pcm = (0.3 * rng.standard_normal((S, 640))).astype(np.float32)
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record(st)
      g.push({s: pcm[s] for s in range(S)}, ears=ears)
      e1.record(st)
      e1.synchronize()
      if list(k) != [1] * S:
        continue
      if warm > 0:
        warm -= 1
        continue
      ms.append(e0.elapsed_time(e1))
    sizes = None
    if q is not None:
      files = g.last_jpeg()
      sizes = float(np.mean([len(b) for v in files.values() for _, b in v]))
    rows.append({"slots": S, "frame_batch": nb, "jpeg_quality": q, "pushes": len(ms), "device_ms_median": float(np.median(ms)),
                 "device_ms_p90": float(np.percentile(ms, 90)), "mean_file_bytes": sizes})
    del g
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--pushes", type=int, default=30)
  ap.add_argument("--no_push", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.json"))
  a = ap.parse_args()
  out = os.path.abspath(a.out)
  import torch
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  rec = {"metric": "jpeg_encode", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)), "parent_commit": commit,
         "quality": quality()}
  rec["encode"], rec["host_pil_pool"] = encode_times()
  if not a.no_push:
    rec["push"] = push_times(a.pushes)
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

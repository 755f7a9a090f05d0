"""Cost of reading a Motion-JPEG AVI clip on the device (voicepuppet_amd.avi_read.AviReader) on one GPU: writes profiles/avi_read.json.

The clip: 64 frames of 512 x 512 written with AviWriter from PIL-encoded frames, 4:2:2 and 4:2:0 alternating (quality 90, Huffman
tables kept), cycling through the fixture panel of tests/golden/jpeg_frames.npz, a noise frame and a flat frame as
scripts/jpeg_latency.py's do.  Three paths alternate in one process, so that all see the same clocks, caches and allocator state:

  first_sight   AviReader.read(0, 64) with an empty entry-point index: the device index scan runs in front of the entropy kernel
  from_index    the same read with the index of an earlier read
  pil           what the reader replaces: PIL decoding the same 64 chunks on the host, one pinned H2D copy of the frames

read() is timed with HIP events on the stream (recorded in front of the call and behind its last copy; the call's host work - one
readinto, 64 header parses, the packing - lies between them, as it does for a caller) and with the wall clock; pil with the wall clock
up to the end of its copy.  Median and p90 of --reps warm calls after --warm.  No threshold is asserted.
Usage: python scripts/avi_read_latency.py [--reps 20] [--warm 5] [--dir DIR] [--out profiles/avi_read.json]
"""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, SIDE = 64, 512


def write_clip(path):
  from PIL import Image
  from voicepuppet_amd.avi import AviWriter, host_segment
  z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_frames.npz"))
  rng = np.random.default_rng(5)
  panel = z["sample22_panel"]
  kinds = [panel[:SIDE, :SIDE], rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8), np.full((SIDE, SIDE, 3), 77, np.uint8)]
  jpegs = []
  for i in range(FRAMES):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(kinds[i % 3])).save(b, "JPEG", quality=90, subsampling=1 if i % 2 == 0 else 2)
    jpegs.append(b.getvalue())
  w = AviWriter(path, SIDE, SIDE)
  w.append(*host_segment(jpegs, np.zeros(16000 * FRAMES // 25, np.float32)))
  w.close()
  return jpegs


def stats(ms):
  return {"median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warm", type=int, default=5)
  ap.add_argument("--dir", default=None)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avi_read.json"))
  a = ap.parse_args()
  import torch
  from PIL import Image
  from voicepuppet_amd.avi_read import AviReader
  d = tempfile.mkdtemp(prefix="avi_read_", dir=a.dir)
  try:
    path = os.path.join(d, "clip.avi")
    jpegs = write_clip(path)
    reader = AviReader(path, batch=FRAMES)
    assert reader.frames == FRAMES and reader.check_index() == []
    out = torch.empty(FRAMES, SIDE, SIDE, 3, dtype=torch.uint8, device="cuda")
    pinned = torch.empty(FRAMES, SIDE, SIDE, 3, dtype=torch.uint8).pin_memory()
    st = torch.cuda.current_stream()
    dec = reader._decoder(False)
    want = np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
    ms = {k: {"event": [], "wall": []} for k in ("first_sight", "from_index")}
    pil_ms, lanes = [], {}
    for i in range(a.warm + a.reps):
      for name in ("first_sight", "from_index", "pil"):
        torch.cuda.synchronize()
        if name == "pil":
          t = time.perf_counter()
          for k, j in enumerate(jpegs):
            pinned[k] = torch.from_numpy(np.asarray(Image.open(io.BytesIO(j)).convert("RGB")))
          out.copy_(pinned, non_blocking=True)
          st.synchronize()
          if i >= a.warm:
            pil_ms.append(1000.0 * (time.perf_counter() - t))
          continue
        dec.harvest()
        if name == "first_sight":
          dec.index.clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record(st)
        reader.read(0, FRAMES, out=out)
        e1.record(st)
        e1.synchronize()
        wall = 1000.0 * (time.perf_counter() - t)
        lanes[name] = reader.last_segments
        if i >= a.warm:
          ms[name]["event"].append(e0.elapsed_time(e1))
          ms[name]["wall"].append(wall)
      if i == 0:
        assert np.array_equal(out.cpu().numpy(), want) and reader.fallbacks == 0
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    rec = {"metric": "avi_read", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)), "parent_commit": commit,
           "reps": a.reps, "warm": a.warm, "frames": FRAMES, "size": [SIDE, SIDE], "clip_bytes": os.path.getsize(path),
           "frame_bytes": {"min": min(map(len, jpegs)), "max": max(map(len, jpegs))}, "scan_chunk_bytes": reader.scan_chunk_bytes,
           "lanes_per_frame": {k: sorted(set(v)) for k, v in lanes.items()},
           "read": {k: {"hip_events": stats(v["event"]), "wall": stats(v["wall"])} for k, v in ms.items()},
           "pil_decode_plus_h2d": {"wall": stats(pil_ms)}}
  finally:
    shutil.rmtree(d, ignore_errors=True)
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

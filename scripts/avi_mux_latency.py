"""Cost of the device AVI muxer (voicepuppet_amd.avi, libvp_hip.so vp_avimux_*) on one GPU: writes profiles/avi_mux.json.

For 1, 8 and 64 talkers, two pushes each: `steady` (one 512 x 512 frame and 40 ms of audio per talker) and `finish` (13 frames per talker,
no audio: a clip's lookahead flushed).  The frames cycle through the fixture panel of tests/golden/jpeg_frames.npz, a noise frame and a
flat frame, as scripts/jpeg_latency.py's do.

  device   HIP events around vp_jpeg_encode (launches of at most 64 frames, as a stream group encodes) and around vp_avimux_segment of the
           same rows, warm, median and p90 of --reps calls after --warm; the bytes the segment call writes
  host     wall time from the end of the push (both calls enqueued) to bytes on disk, two paths alternating in the same process:
             avi   AviMuxer.to_host + one AviWriter.append per talker (PuppetStreamGroup.write_avi)
             jpg   JpegEncoder.to_host + one file per frame (PuppetStreamGroup.last_jpeg and the launchers' write loop: the path
                   before the muxer existed)
           written to --dir (a tmpfs path keeps the disk out of the number; the default is the system's temporary directory)
No threshold is asserted: the record says whether the segment call costs less than the encode it follows.
Usage: python scripts/avi_mux_latency.py [--reps 50] [--warm 10] [--dir DIR] [--out profiles/avi_mux.json]
"""
import argparse
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


def frames_u8(n):
  z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_frames.npz"))
  rng = np.random.default_rng(5)
  kinds = [z["sample22_panel"], rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), np.full((512, 512, 3), 77, np.uint8)]
  return np.stack([kinds[i % 3] for i in range(n)])


def stats(ms):
  return {"median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def measure(S, per_talker, samples, reps, warm, out_dir):
  import torch
  from voicepuppet_amd.avi import AviMuxer, AviWriter
  from voicepuppet_amd.jpeg import JpegEncoder
  K, nb = S * per_talker, 64
  dev = torch.from_numpy(frames_u8(K)).to("cuda")
  enc = JpegEncoder(512, 512, min(nb, K))
  mux = AviMuxer(K, enc.capacity, S, max(1, S * samples))
  data = torch.empty(K, enc.capacity, dtype=torch.uint8, device="cuda")
  lengths = torch.empty(K, dtype=torch.int32, device="cuda")
  slot = torch.arange(S, dtype=torch.int32, device="cuda").repeat_interleave(per_talker).contiguous()
  rng = np.random.default_rng(0)
  pcm = torch.from_numpy((0.3 * rng.standard_normal(S * samples)).astype(np.float32)).to("cuda") if samples else None
  counts = torch.full((S,), samples, dtype=torch.int32, device="cuda")
  offsets = (torch.arange(S, dtype=torch.int32, device="cuda") * samples).contiguous()
  blob = torch.empty(mux.call_capacity(K, enc.capacity, S * samples), dtype=torch.uint8, device="cuda")
  st = torch.cuda.current_stream()

  def push():
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    ev[0].record(st)
    for i0 in range(0, K, nb):
      n = min(nb, K - i0)
      enc.encode(dev[i0:i0 + n], data[i0:i0 + n], lengths[i0:i0 + n])
    ev[1].record(st)
    seg = mux.segment(data, lengths, slot, pcm, offsets if samples else None, counts if samples else None, out=blob)
    ev[2].record(st)
    return seg, ev

  enc_ms, mux_ms, avi_ms, jpg_ms, used = [], [], [], [], 0
  writers = [AviWriter(os.path.join(out_dir, "t%d.avi" % s), 512, 512) for s in range(S)]
  for i in range(warm + reps):
    for path in ("avi", "jpg"):                    # alternating: both see the same clocks, caches and allocator state
      seg, ev = push()
      t = time.perf_counter()
      if path == "avi":
        for s, (segment, entries) in mux.to_host(seg, dev).items():
          writers[s].append(segment, entries)
          writers[s]._f.flush()
        wall = avi_ms
      else:
        files = enc.to_host(data, lengths, dev)
        for r, f in enumerate(files):
          with open(os.path.join(out_dir, "%d_%d.jpg" % (r // per_talker, r % per_talker)), "wb") as fh:
            fh.write(f)
        wall = jpg_ms
      dt = 1000.0 * (time.perf_counter() - t)
      ev[2].synchronize()
      if i >= warm:
        wall.append(dt)
        if path == "avi":
          enc_ms.append(ev[0].elapsed_time(ev[1]))
          mux_ms.append(ev[1].elapsed_time(ev[2]))
  used = int(seg.blob[4:8].cpu().numpy().view("<u4")[0])
  for w in writers:
    w.close()
  return {"talkers": S, "frames_per_talker": per_talker, "samples_per_talker": samples, "blob_bytes_used": used,
          "device": {"jpeg_encode": stats(enc_ms), "avi_segment": stats(mux_ms)},
          "host_to_disk": {"write_avi": stats(avi_ms), "last_jpeg_and_files": stats(jpg_ms)}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=50)
  ap.add_argument("--warm", type=int, default=10)
  ap.add_argument("--dir", default=None)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avi_mux.json"))
  a = ap.parse_args()
  import torch
  commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
  rec = {"metric": "avi_mux", "device": torch.cuda.get_device_name(0), "host_cpus_used": len(os.sched_getaffinity(0)), "parent_commit": commit,
         "reps": a.reps, "warm": a.warm, "runs": []}
  for S in (1, 8, 64):
    for name, per_talker, samples in (("steady", 1, 640), ("finish", 13, 0)):
      d = tempfile.mkdtemp(prefix="avi_mux_", dir=a.dir)
      try:
        rec["runs"].append({"push": name, **measure(S, per_talker, samples, a.reps, a.warm, d)})
      finally:
        shutil.rmtree(d, ignore_errors=True)
  line = json.dumps(rec, indent=1)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()

#!/usr/bin/env python
"""Headline benchmark: PixReferNet G+D training step, frames/s at 256x256, bf16, GLOBAL batch 32 (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--scaling strong|weak] [--dump-outputs DIR] [--full]

One process per GPU.  With N > 1 and no WORLD_SIZE in the environment this script itself starts the N ranks
(`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD process, before anything here has touched
the GPU) and relays rank 0's JSON line; under torch.distributed.run it is a rank (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* from the environment), over RCCL.

A step = forward (G, composite, 3xD, VGG trunk on 2N, all losses) + both backward passes + all-reduce of the G/D gradient
arenas + Adam(D) + Adam(G) on synthetic inputs already resident in HBM.
  --scaling strong (default): the global batch stays 32, each rank runs 32/N samples;
  --scaling weak: every rank runs 32 samples.
Rank 0 prints ONE JSON line.  A plain run does only what the line's headline needs: set-up, the warm-up steps, the timed
steps, --dump-outputs, the line.  --full then measures everything else, after the timed steps, into the same line (the --no-*
options leave single legs of it out), among others
  roofline      the dominant kernel class, timed live with HIP events on the launch stream (with `kernels`, `long_region`),
  other_scaling (N > 1) the other --scaling mode; `distributed.buckets`: per-bucket timing of the gradient exchange,
  f32           (N = 1) the same step on the float32 path - the path that meets the 1e-3 pixel tolerance,
  cpu_baseline  (N = 1) CPU restatements of the same step on the host cores: the numpy port (oracle/pixrefer_ref.py) and
                a torch-CPU float32 (oneDNN) restatement as the TF-CPU proxy (oracle/pixrefer_torch.py), bounded samples,
and the strong-scaling ceiling, the PCIe-inclusive rate, the BFMNet training step and the other BASELINE workloads.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BF16_MFMA_PEAK = 2500.0   # TFLOP/s dense (MI355X_MICROARCH.md)
F32_MFMA_PEAK = 157.3
HBM_PEAK = 8000.0         # GB/s
GFLOP_PER_FRAME_256 = 163.02


def parse_args(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--gpus", type=int, default=1)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
  ap.add_argument("--global-batch", type=int, default=32, help="strong scaling: samples per step over all ranks")
  ap.add_argument("--batch", type=int, default=32, help="weak scaling: samples per step per rank")
  ap.add_argument("--height", type=int, default=256)
  ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
  ap.add_argument("--full", action="store_true",
                  help="after the timed steps, also measure the sub-records (per-kernel roofline, f32 path, other configurations, "
                       "CPU baselines, ...); the --no-* options below leave single ones out")
  ap.add_argument("--no-cpu-baseline", action="store_true")
  ap.add_argument("--no-profile", action="store_true")
  ap.add_argument("--no-f32", action="store_true")
  ap.add_argument("--no-scaling-ceiling", action="store_true", help="skip the step at global_batch / 8 frames (strong_scaling_ceiling)")
  ap.add_argument("--no-other-scaling", action="store_true")
  ap.add_argument("--no-input-pipeline", action="store_true")
  ap.add_argument("--no-bfmnet-train", action="store_true", help="skip the BFMNet training-step sub-record (SURVEY.md 8f-4)")
  ap.add_argument("--no-secondary", action="store_true", help="skip the other BASELINE workloads (h512_bs2, h512_bs8, bs8_256, config3 sub-records)")
  ap.add_argument("--tune", action="append", default=[], metavar="KEY=INT", help="vp_tune knob for experiments (repeatable)")
  ap.add_argument("--grad-dtype", default="auto", choices=["auto", "f32", "bf16"],
                  help="N > 1: transport type of the gradient all-reduce (f32 master either way); auto = the compute dtype")
  ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                  help="write what the last timed step computed (losses, generator outputs, updated weights) to DIR/<name>.npy")
  args = ap.parse_args(argv)
  if args.steps < 1 or args.warmup < 0:
    ap.error("--steps must be >= 1 and --warmup >= 0")
  return args


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def launch_ranks(args):
  """Parent of an N-rank run: has not initialised the GPU (importing torch does not), starts the ranks as a child process
  and exits with its code."""
  cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
         "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
  env = dict(os.environ)
  env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
  env.setdefault("OMP_NUM_THREADS", "8")
  return subprocess.call(cmd, env=env)


def pmc_traffic(name):
  """HBM bytes per launch of a kernel class from the newest committed rocprofv3 PMC summary (FETCH_SIZE and WRITE_SIZE in
  separate runs of this same command, folded by scripts/pmc_summary.py; FETCH_SIZE doubled per MI355X_MICROARCH.md 'HBM');
  launch-weighted over the template variants of the class; None when not collected."""
  paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))
  if not paths:
    return None, None
  rows = [r for r in json.load(open(paths[-1])) if r.get("class") == name]
  n = sum(r["launches"] for r in rows)
  src = "replayed from the committed rocprofv3 PMC summary profiles/%s (separate --pmc passes of this command; NOT measured in this run)" % os.path.basename(paths[-1])
  return (sum(r["hbm_bytes_per_launch"] * r["launches"] for r in rows) / n if n else None), src


def pmc_mfma_busy(name):
  """Matrix-pipe busy fraction of a kernel class from the newest committed counter summary (profiles/r*_pmc_mfma_busy.json, written by
  scripts/pmc_mix.sh: SQ_VALU_MFMA_BUSY_CYCLES against the kernel's GPU-active cycles, a separate --pmc pass of this command), time-weighted
  over the template variants of the class; None when not collected.  Replayed, NOT measured in this run."""
  paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_mfma_busy.json")))
  if not paths:
    return None, None
  rows = [r for r in json.load(open(paths[-1])).values() if r.get("class") == name and r.get("ms")]
  t = sum(r["ms"] for r in rows)
  return (sum(r["mfma_busy"] * r["ms"] for r in rows) / t if t else None), os.path.basename(paths[-1])


def synth_batch(n, h, seed, device):
  """U[0,1) box-blurred 5x5; soft-disc matte; fg = targets * masks packing."""
  import torch
  g = torch.Generator(device="cpu").manual_seed(seed)

  def img(c):
    x = torch.rand(n, c, h, h, generator=g)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="replicate"), 5, 1)
    return x.permute(0, 2, 3, 1).contiguous()
  yy, xx = torch.meshgrid(torch.arange(h), torch.arange(h), indexing="ij")
  r = ((yy - h / 2) ** 2 + (xx - h / 2) ** 2).float().sqrt()
  disc = ((0.35 * h + 4 - r) / 8).clamp(0, 1)
  masks = disc[None, :, :, None].expand(n, h, h, 3).contiguous()
  inputs, targets, ex_t = img(6), img(3), img(3)
  fg = torch.cat([ex_t * masks, targets * masks], dim=-1)
  return [t.to(device) for t in (inputs, fg, targets, masks)]


DUMP_BUDGET_BYTES = 64 << 20
# elements kept per array; a larger array is replaced by a fixed seeded sample of its flattened elements (same indices every run)
DUMP_CAP = {"Outputs": 8 << 20, "params_g": 4 << 20, "params_d": 2 << 20}


def dump_outputs(eng, out_dir):
  """What a caller of train_step holds after the last timed step: the step's losses (float64), the generator output of its forward pass
  (Outputs, [N, H, H, 3] float32) and the generator / discriminator weights after its Adam updates (float32), as out_dir/<name>.npy."""
  import numpy as np
  import torch
  torch.cuda.synchronize()
  arrays = {k: np.array([v], np.float64) for k, v in eng.losses().items()}
  for name, t in (("Outputs", eng.fetch("Outputs")), ("params_g", eng.params_g), ("params_d", eng.params_d)):
    a = t.float().cpu().numpy()
    if a.size > DUMP_CAP[name]:
      idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_CAP[name], replace=False))
      a = a.reshape(-1)[idx]
    arrays[name] = a
  total = sum(a.nbytes for a in arrays.values())
  assert total <= DUMP_BUDGET_BYTES, total
  os.makedirs(out_dir, exist_ok=True)
  for k, a in arrays.items():
    np.save(os.path.join(out_dir, k + ".npy"), a)
  return {"dir": out_dir, "arrays": {k: list(a.shape) for k, a in arrays.items()}, "bytes": total}


# ---- CPU restatements (rank 0, N = 1 only; the oracle is the thing timed here, never the GPU path) ---------------------
def _cpu_model():
  try:
    for line in open("/proc/cpuinfo"):
      if line.startswith("model name"):
        return line.split(":", 1)[1].strip()
  except OSError:
    pass
  return "unknown"


def _timed_steps(step, n, warm, steps, cap_s):
  """`warm` untimed calls, then up to `steps` timed ones (stops early once `cap_s` seconds of timed work are spent, but never
  before one step)."""
  for _ in range(warm):
    step()
  per, t0 = [], time.time()
  while len(per) < steps:
    t1 = time.perf_counter()
    step()
    per.append(time.perf_counter() - t1)
    if time.time() - t0 > cap_s:
      break
  dt = time.time() - t0
  per.sort()
  med = per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2])
  # frames_per_s = the MEDIAN step (a shared host's outliers do not move it); the mean and the best step beside it
  return {"frames_per_s": n / med, "frames_per_s_mean": n * len(per) / dt, "frames_per_s_best_step": n / per[0],
          "step_s_min_median_max": [round(per[0], 4), round(med, 4), round(per[-1], 4)],
          "steps": len(per), "warmup": warm, "batch": n, "seconds": round(dt, 2)}


def usable_cores():
  """Cores this process may really use: the affinity mask and the cgroup CPU quota, not the machine's core count (a 256-thread
  pool on a container limited to a few cores runs two orders of magnitude slower than a matched one)."""
  n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
  try:
    quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
    if quota != "max":
      n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
  except (OSError, ValueError):
    pass
  return max(1, n)


def cpu_baseline(h, ngf=64, ndf=64, cap_s=20.0):
  import numpy as np
  import torch
  from oracle import pixrefer_ref as ref
  from oracle.pixrefer_torch import TorchGraph
  cores = usable_cores()
  torch.set_num_threads(min(cores, 64))      # oneDNN convolutions of this size stop scaling (and start thrashing) beyond that
  rng = np.random.default_rng(0)

  def batch(n):
    return [rng.uniform(size=(n, h, h, c)).astype(np.float32) for c in (6, 6, 3, 3)]
  out = {}
  p = ref.init_params(ngf, ndf, seed=0, dtype=np.float32)
  b2 = batch(2)
  st = ref.TrainState({k: v.copy() for k, v in p.items()}, ngf, ndf)
  out["numpy_port_bs2"] = _timed_steps(lambda: st.step(*b2), 2, 1, 3, cap_s)
  tg = TorchGraph(p, ngf, ndf, torch.float32)
  out["torch_cpu_bs2"] = _timed_steps(lambda: tg.step(*b2), 2, 2, 12, cap_s)     # >= 10 timed steps: the quoted baseline
  b32 = batch(32)
  tg = TorchGraph(p, ngf, ndf, torch.float32)
  out["torch_cpu_bs32"] = _timed_steps(lambda: tg.step(*b32), 32, 1, 3, 2 * cap_s)
  best = max(out, key=lambda k: out[k]["frames_per_s"])
  return {"value": out[best]["frames_per_s"], "unit": "frames/s", "cores": cores, "torch_threads": min(cores, 64), "machine_cores": os.cpu_count(), "kind": "port", "cpu_model": _cpu_model(),
          "label": "CPU restatement (TF-CPU proxy): TensorFlow exists on neither box",
          "sample": "full G+D steps (fwd + both bwd + TF-Adam x2) at %dx%d, ngf=ndf=%d, float32, %d threads: numpy port "
                    "(oracle/pixrefer_ref.py) at the reference's batch 2, torch-CPU/oneDNN restatement (oracle/pixrefer_torch.py) "
                    "at batch 2 (12 timed steps) and 32, each after warm-up; per run the MEDIAN step is quoted (min / median / max in `runs`); "
                    "value = the fastest of them (%s)" % (h, h, ngf, cores, best),
          "runs": out}


def cpu_baseline_bfmnet_train(w, ex, vm, ears, mfccs, coeff, seq):
  """ONE step of the float64 torch restatement of BFMNet.build_train_op (oracle/bfmnet_train_torch.py) on the host cores."""
  import numpy as np
  import torch
  from oracle import bfmnet_train_torch as bt
  torch.set_num_threads(min(usable_cores(), 64))
  model = {"idBase": np.zeros((ex.shape[0], 80)), "exBase": ex, "meanshape": np.zeros(ex.shape[0]), "vmask": vm.reshape(-1)}
  t0 = time.perf_counter()
  bt.train_step(w, None, ears, mfccs, coeff, seq, {}, model)
  s = time.perf_counter() - t0
  return {"value": len(seq) / s, "unit": "clips/s", "cores": usable_cores(), "kind": "port",
          "sample": "1 step of the float64 torch-CPU restatement at the same batch (%.1f s)" % s}


def bfmnet_train_record(device, with_cpu, steps=30, batch=4, frames=24, nver=35709):
  """SURVEY.md 8f-4 beside the headline: one BFMNet build_train_op step at the reference's batch (train_bfmnet.py:46: 4 clips of 24
  frames, 35709-vertex face model, dropout on), replayed from its hipGraph; the CPU leg is ONE step of the float64 torch restatement
  (oracle/bfmnet_train_torch.py) on the host cores."""
  import numpy as np
  import torch
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.bfmnet.train_engine import BFMNetTrainEngine
  rng = np.random.default_rng(0)
  vm = np.ones((nver, 3), np.float32)
  vm[rng.choice(nver, nver // 20, replace=False)] = 10
  ex = rng.normal(0, 0.05, (3 * nver, 64)).astype(np.float32)
  eng = BFMNetTrainEngine(batch, frames, {"exBase": ex, "vmask": vm.reshape(-1)})
  w = random_variables(0)
  eng.load_params(w)
  ears = torch.rand(batch, frames, 1, device=device)
  mfccs = torch.randn(batch, 5 * frames, 80, device=device)
  coeff = torch.randn(batch, frames, 257, device=device) * 0.5
  seq = [frames] * batch
  for _ in range(5):
    eng.train_step_graphed(ears, mfccs, coeff, seq, 0.25)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    eng.train_step_graphed(ears, mfccs, coeff, seq, 0.25)
  torch.cuda.synchronize()
  ms = (time.perf_counter() - t0) / steps * 1e3
  rec = {"metric": "BFMNet training step clips/sec", "value": batch / ms * 1e3, "unit": "clips/s", "ms_per_step": ms, "steps": steps, "dtype": "f32",
         "config": {"workload": "BFMNet build_train_op: fwd + vertex-space loss + bwd + clip + Adam, hipGraph replay", "batch": batch,
                    "frames": frames, "vertices": nver, "dropout": True}}
  if with_cpu:
    rec["cpu_baseline"] = cpu_baseline_bfmnet_train(w, ex, vm, ears.cpu().numpy(), mfccs.cpu().numpy(), coeff.cpu().numpy(), seq)
  return rec


# ---- one measured configuration on this rank -----------------------------------------------------------------------------
STEP_ROOFLINE_MS_BS32_256 = {"bf16": 2.65, "f32": 33.6}      # mixed per-layer roofline of the whole step (HBM 6.3 TB/s)


# --tune keys that select the step executor's schedule of the benchmark plan: "streams" (vp_pixrefer_desc::streams: 1 = everything on
# the caller's stream, no executor streams), "overlap" / "d_backward_fork" / "d_beside_vgg" (vp_pixrefer_set_option)
SCHEDULE_KEYS = ("streams", "overlap", "d_backward_fork", "d_beside_vgg", "vgg_real_fork", "bwd_sums_in_epilogue")
SCHEDULE = {}


def make_engine(per_gpu, height, dtype):
  from voicepuppet_amd.engine import PixReferEngine
  eng = PixReferEngine(per_gpu, height, 64, 64, dtype=dtype, training=True, streams=SCHEDULE.get("streams", 0))
  for k in ("overlap", "d_backward_fork", "d_beside_vgg", "vgg_real_fork", "bwd_sums_in_epilogue"):
    if k in SCHEDULE:
      eng.set_option(k, SCHEDULE[k])
  return eng


def run_config(per_gpu, height, dtype, steps, warmup, rank, world, device, group, profile, grad_dtype="f32", dump_dir=None,
               exchange_timing=True):
  import torch
  import torch.distributed as dist
  eng = make_engine(per_gpu, height, dtype)
  eng.grad_transport = grad_dtype
  eng.load_params(eng.random_params(seed=0))   # the reference's initialisers, identical on every rank
  batch = synth_batch(per_gpu, height, 1000 + rank, device)
  lr = 3e-4

  def sync():
    if world > 1:
      dist.barrier(group=group)
    torch.cuda.synchronize()

  # rank liveness: a peer that dies inside a collective leaves this rank's streams spinning; the watchdog ends the process non-zero
  from voicepuppet_amd.parallel import StepWatchdog
  dog = StepWatchdog(rank=rank, device=device.index if hasattr(device, "index") else None) if world > 1 else None

  def step():
    eng.train_step(*batch, lr=lr, group=group)

  def beat():
    # one event behind a whole phase (warm-up, timed loop), recorded OUTSIDE the timed region: the single-GPU loop carries no such
    # host work, so the multi-GPU loop must not either; a phase lasts seconds, the watchdog's horizon is minutes
    if dog is not None:
      ev = torch.cuda.Event()
      ev.record()
      dog.beat(ev)

  beat()          # armed from the start: a peer that dies during rendezvous / warm-up must not leave this rank in sync() for ever
  for _ in range(warmup):
    step()
  beat()
  sync()
  t0 = time.perf_counter()
  for _ in range(steps):
    step()
  sync()
  dt = time.perf_counter() - t0
  beat()
  if world > 1:
    tmax = torch.tensor([dt], device=device, dtype=torch.float64)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX, group=group)
    dt = float(tmax.item())
  ms = dt / steps * 1e3
  res = {"ms_per_step": ms, "frames_per_s": per_gpu * world * steps / dt, "per_gpu_batch": per_gpu,
         "global_batch": per_gpu * world,
         "step_tflops": GFLOP_PER_FRAME_256 * 1e9 * (height / 256) ** 2 * per_gpu * world / (ms * 1e-3) / 1e12}
  if dump_dir is not None and rank == 0:
    # before any later step below moves the weights
    res["dumped"] = dump_outputs(eng, dump_dir)
  if world == 1 and profile:
    # the same step over a five times longer region (outside the judged one): the driver's 20-step region is 0.15 s, below the resolution
    # of the changes EXPERIMENTS.md discusses
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(5 * steps):
      step()
    torch.cuda.synchronize()
    res["long_region"] = {"steps": 5 * steps, "ms_per_step": (time.perf_counter() - t1) / (5 * steps) * 1e3}
  if world > 1 and exchange_timing:
    # where the exchange's time goes (outside the timed region): HIP events on the communication stream around every bucket of two
    # more steps; every rank runs them (they are collectives), rank 0 reports the second one
    ex = eng._exchange
    ex.timing = True
    for _ in range(2):
      step()
    sync()
    res["buckets"] = ex.bucket_ms()
    ex.timing = False
  if dog is not None:
    dog.close()
  if profile and rank == 0:
    # per-kernel launch durations, HIP events on the launch stream, over a few extra steps (outside the timed region)
    eng.profile(True)
    eng.train_step(*batch, lr=lr, group=None)       # one untimed step in the profiling (single-stream) schedule: its first pass can carry a
    torch.cuda.synchronize()                        # one-off stall (seen: one 1.7 ms launch of a 0.33 ms kernel) that would reorder the classes
    eng.profile_collect()
    psteps = 3
    for _ in range(psteps):
      eng.train_step(*batch, lr=lr, group=None)
    torch.cuda.synchronize()
    recs = eng.profile_collect()
    eng.profile(False)
    recs.sort(key=lambda r: -r["ms"])
    res["kernels"] = [{"name": r["name"], "calls_per_step": r["calls"] / psteps, "ms_per_step": r["ms"] / psteps,
                       "tflops": r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["ms"] > 0 else 0.0} for r in recs]
    res["conv_launches_per_step"] = sum(r["calls"] for r in recs) / psteps      # conv-family launches only (the timed ones)
    top = recs[0]
    peak = BF16_MFMA_PEAK if dtype == "bf16" else F32_MFMA_PEAK
    ach = top["flops"] / (top["ms"] * 1e-3) / 1e12
    traffic, traffic_src = pmc_traffic(top["name"]) if dtype == "bf16" else (None, None)
    busy, busy_src = pmc_mfma_busy(top["name"]) if dtype == "bf16" else (None, None)
    # the whole step against its mixed per-layer roofline, scaled to this rank's batch and image size
    step_roof_ms = STEP_ROOFLINE_MS_BS32_256[dtype] * per_gpu / 32.0 * (height / 256.0) ** 2
    res["roofline"] = {"kernel": top["name"], "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                       "frac": ach / peak, "traffic": traffic, "traffic_source": traffic_src,
                       "mfma_busy": busy, "mfma_busy_source": busy_src,
                       "step_roofline_ms": step_roof_ms, "step_frac": step_roof_ms / ms,
                       "avg_launch_ms": top["ms"] / top["calls"], "launches_per_step": top["calls"] / psteps,
                       "algorithmic_bytes_per_launch": top["bytes"] / top["calls"],
                       "algorithmic_flops_per_launch": top["flops"] / top["calls"]}
  if world > 1:
    dist.barrier(group=group)
  # the plan and its HIP streams go NOW, not when the collector finds the engine: a later leg's engine would share the runtime's hardware
  # queues with this one's streams (EXPERIMENTS.md 0.8: the 4-frame step then measures 2.8 - 4.6 ms instead of 2.15)
  torch.cuda.synchronize()
  eng.close()
  del eng, step
  import gc
  gc.collect()
  torch.cuda.empty_cache()
  return res


def run_with_input_pipeline(per_gpu, height, dtype, steps, warmup, device):
  """The same step fed through the on-device input pipeline (voicepuppet_amd/generator/device_pipeline.py): every step's batch
  starts as uint8 triptych frames in pinned HOST memory, crosses PCIe (2 * 9 * S * S bytes per sample) on a side stream and is
  cropped / resized / packed by vp_pixrefer_pack_frames, overlapped with the previous step.  This is the PCIe-inclusive rate
  SURVEY.md 8d asks for next to the resident-input headline; it is never `value`."""
  import numpy as np
  import torch
  from voicepuppet_amd.engine import PixReferEngine
  from voicepuppet_amd.generator.device_pipeline import FramePrefetcher
  eng = PixReferEngine(per_gpu, height, 64, 64, dtype=dtype, training=True)
  eng.load_params(eng.random_params(seed=0))
  rng = np.random.default_rng(0)
  S = height
  pin = lambda a: torch.from_numpy(a).pin_memory()       # decoded frames wait in pinned host memory, as a decoder thread would leave them
  pool = [(pin(rng.integers(0, 256, (per_gpu, S, 3 * S, 3)).astype(np.uint8)), pin(rng.integers(0, 256, (per_gpu, S, 3 * S, 3)).astype(np.uint8)),
           pin(np.tile(np.array([[[3, 5, S - 8], [0, 2, S - 4]]], np.int32), (per_gpu, 1, 1)))) for _ in range(4)]

  def source():
    k = 0
    while True:
      yield pool[k % len(pool)]
      k += 1
  eng.use_streams(3)      # the prefetcher's stream is the fourth busy one (include/vp_hip.h vp_pixrefer_use_streams)
  pf = FramePrefetcher(source(), per_gpu, S)
  for _ in range(warmup):
    eng.train_step(*pf.next(), lr=3e-4)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    eng.train_step(*pf.next(), lr=3e-4)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  eng.close()
  del eng, pf
  import gc
  gc.collect()
  torch.cuda.empty_cache()
  return {"value": per_gpu * steps / dt, "unit": "frames/s", "ms_per_step": dt / steps * 1e3,
          "host_to_device_bytes_per_step": int(per_gpu * (2 * 9 * S * S + 24)),
          "what": "uint8 frames in pinned host memory -> PCIe -> vp_pixrefer_pack_frames -> G+D step, copies and packing overlapped with the previous step"}


def secondary_records(device, steps, rank, world, group):
  """The other BASELINE.json workloads inside the driver-run line: few steps each, every one with `ms_per_step`,
  `step_frac` against the SURVEY.md 8d step roofline scaled to its batch and image size, and its dominant kernel class from the live
  HIP-event pass.  h512_bs2 = the reference's own training configuration (train_pixrefer.py:36-43); h512_bs8 = BASELINE config 4's
  per-GPU share; bs8_256 = BASELINE config 2; config3 = log-mel + BFMNet on 64 x 1 s (BASELINE config 3)."""
  import numpy as np
  import torch
  out = {}
  for key, n, h in (("bs8_256", 8, 256), ("h512_bs2", 2, 512), ("h512_bs8", 8, 512)):
    r = run_config(n, h, "bf16", max(10, steps), 5, rank, world, device, group, True)
    roof = r.get("roofline") or {}
    out[key] = {"workload": "G+D step bf16, batch %d, %dx%d" % (n, h, h), "ms_per_step": r["ms_per_step"], "frames_per_s": r["frames_per_s"],
                "step_tflops": r["step_tflops"], "step_roofline_ms": roof.get("step_roofline_ms"), "step_frac": roof.get("step_frac"),
                "dominant_class": {k: roof.get(k) for k in ("kernel", "achieved", "peak", "frac", "avg_launch_ms", "launches_per_step")}}
  # BASELINE config 3: log-mel (one launch, HBM / launch bound) + BFMNet inference (float32 MFMA) on 64 clips of 1 s
  from voicepuppet_amd.audio import BFMNetEngine, LogMel
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  B, T = 64, 25
  samples = 128 * (5 * T - 1) + 512                                   # infer_bfmvid.py:166: exactly 5 log-mel rows per video frame
  g = torch.Generator(device="cpu").manual_seed(0)
  tt = torch.arange(samples, dtype=torch.float32) / 16000.0
  sweep = 0.3 * torch.sin(2 * np.pi * (100.0 * tt + 0.5 * (4000.0 - 100.0) / tt[-1] * tt * tt))     # noise + 100 -> 4000 Hz sweep
  pcm = (0.1 * torch.randn(B, samples, generator=g) + sweep).clamp(-1, 1).to(device)
  lm, net = LogMel(B, samples), BFMNetEngine(B, T)
  net.load_params(random_variables(0))
  ears, seq = torch.full((B, T, 1), 0.3, device=device), [T] * B

  def timed(fn, warm, k):
    for _ in range(warm):
      fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
      fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3
  ms_lm = timed(lambda: lm(pcm), 3, 20)
  mf = lm(pcm)
  ms_net = timed(lambda: net.forward(ears, mf, seq), 3, 10)
  gflop = 10.64 * B                                                   # 10.61 MfccNet + 0.03 head per 1 s clip
  out["config3"] = {"workload": "log-mel -> BFMNet f32, 64 clips x 1 s", "ms_per_step": ms_lm + ms_net, "logmel_ms": ms_lm, "bfmnet_ms": ms_net,
                    "audio_seconds_per_s": B / (ms_lm + ms_net) * 1e3,
                    "bfmnet": {"bound": "mfma", "achieved": gflop / ms_net, "peak": F32_MFMA_PEAK, "unit": "TFLOP/s", "frac": gflop / ms_net / F32_MFMA_PEAK},
                    "logmel": {"bound": "hbm", "achieved": 4.0 * (pcm.numel() + mf.numel()) / ms_lm / 1e6, "peak": 8000.0, "unit": "GB/s",
                               "frac": 4.0 * (pcm.numel() + mf.numel()) / ms_lm / 1e6 / 8000.0, "note": "one 35 us launch: launch-bound, no MFMA roofline claimed"},
                    "step_frac": gflop / ms_net / F32_MFMA_PEAK}
  del lm, net
  torch.cuda.empty_cache()
  return out


def per_gpu_batch(args, scaling, world):
  if scaling == "weak":
    return args.batch
  if args.global_batch % world:
    raise SystemExit("strong scaling: global batch %d is not divisible by %d ranks" % (args.global_batch, world))
  return args.global_batch // world


def main():
  args = parse_args()
  if "WORLD_SIZE" not in os.environ:
    if args.gpus > 1:
      sys.exit(launch_ranks(args))
    world, rank, local = 1, 0, 0
  else:
    world, rank, local = int(os.environ["WORLD_SIZE"]), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
      sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d\n" % (args.gpus, world))
      sys.exit(2)

  import torch
  import torch.distributed as dist
  torch.cuda.set_device(local)
  device = torch.device("cuda", local)
  group = None
  if world > 1:
    from voicepuppet_amd.parallel import init_distributed
    group = init_distributed("nccl", device_id=device)       # collective timeout + async error handling: a dead peer ends every rank non-zero
    assert dist.get_world_size() == args.gpus

  grad_dtype = args.dtype if args.grad_dtype == "auto" else args.grad_dtype
  dist_info = None
  if world > 1:
    # proof of the run's shape for the scaling record: ranks, the device each one drives, the collective library
    mine = {"rank": rank, "local_rank": local, "device": torch.cuda.current_device(), "name": torch.cuda.get_device_name(local),
            "pci_bus_id": getattr(torch.cuda.get_device_properties(local), "pci_bus_id", None)}
    gathered = [None] * world
    dist.all_gather_object(gathered, mine, group=group)
    try:
      rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:
      rccl = None
    dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "rccl_version": rccl, "ranks": gathered,
                 "grad_transport": grad_dtype, "gradient_bytes_per_step_per_rank": int((35158852 + 2769601) * (2 if grad_dtype == "bf16" else 4))}
  if args.tune:
    from voicepuppet_amd import _lib
    for kv in args.tune:
      k, v = kv.split("=")
      if k in SCHEDULE_KEYS:            # per-plan schedule (vp_pixrefer_desc fields / vp_pixrefer_set_option), not a library knob
        SCHEDULE[k] = int(v)
      else:
        _lib.check(_lib.lib().vp_tune(k.encode(), int(v)), "vp_tune " + kv)
  main_res = run_config(per_gpu_batch(args, args.scaling, world), args.height, args.dtype, args.steps, args.warmup,
                        rank, world, device, group, args.full and not args.no_profile, grad_dtype, dump_dir=args.dump_outputs,
                        exchange_timing=args.full)
  # everything below measures the sub-records of --full: a plain run ends at its headline
  other = None
  if args.full and world > 1 and not args.no_other_scaling:
    mode = "weak" if args.scaling == "strong" else "strong"
    other = run_config(per_gpu_batch(args, mode, world), args.height, args.dtype, args.steps, args.warmup,
                       rank, world, device, group, False, grad_dtype)
    other["scaling"] = mode
  f32 = None
  if args.full and world == 1 and args.dtype == "bf16" and not args.no_f32:
    r = run_config(per_gpu_batch(args, args.scaling, world), args.height, "f32", max(3, args.steps // 4), 2,
                   rank, world, device, group, not args.no_profile)
    f32 = {"ms_per_step": r["ms_per_step"], "value": r["frames_per_s"], "unit": "frames/s", "step_tflops": r["step_tflops"],
           "roofline": r.get("roofline"), "tolerance": "generator pixels <= 1e-3 rel-L2 vs the float64 oracle (tests/test_gpu_step.py)"}

  # What strong scaling of the global batch can reach at 8 GPUs before any communication: the single-GPU step at the per-GPU share
  # (global batch / 8 frames), measured here so that a SCALE record explains itself
  ceiling = None
  if args.full and world == 1 and not args.no_scaling_ceiling and args.scaling == "strong" and args.global_batch % 8 == 0:
    share = args.global_batch // 8
    # two engines, the faster one counts (the record is an upper bound by definition).  Until the end of round 6 this leg now and then
    # measured 2.8 - 4.6 ms instead of 2.15: its engine's HIP streams were created while streams of earlier legs' engines existed and got
    # the runtime's leftover hardware queues; the executor's streams are process-wide now (include/vp_hip.h vp_reserve_streams,
    # EXPERIMENTS.md 0.8 of round 6) and every engine of a process measures alike
    runs = [run_config(share, args.height, args.dtype, max(10, args.steps), 5, rank, world, device, group, False)["ms_per_step"] for _ in range(2)]
    ceiling = {"per_gpu_batch_at_8_gpus": share, "ms_per_step_at_that_batch": min(runs), "ms_per_step_of_each_engine": runs,
               "ceiling_8_gpus": main_res["ms_per_step"] / min(runs),
               "note": "single-GPU step time at the 8-GPU share of the global batch (the faster of two engines), no gradient exchange: an upper bound of value(8 GPUs) / value(1 GPU)"}

  pcie = None
  if args.full and world == 1 and not args.no_input_pipeline:
    pcie = run_with_input_pipeline(per_gpu_batch(args, args.scaling, world), args.height, args.dtype, max(5, args.steps // 2), 3, device)

  f4 = None
  if args.full and world == 1 and not args.no_bfmnet_train:
    f4 = bfmnet_train_record(device, not args.no_cpu_baseline)

  secondary = None
  if args.full and world == 1 and not args.no_secondary and args.dtype == "bf16":
    secondary = secondary_records(device, min(args.steps, 10), rank, world, group)

  if rank == 0:
    n, h = main_res["per_gpu_batch"], args.height
    out = {"metric": "PixReferNet G+D step frames/sec @256x256 bs=32", "value": main_res["frames_per_s"], "unit": "frames/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": main_res["ms_per_step"],
           "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": "PixReferNet G+D training step (G + 3xD + VGG16-conv3_3 perceptual + TF-Adam x2), "
                                  "%dx%d, ngf=ndf=64, global batch %d = %d per GPU" % (h, h, n * world, n),
                      "global_batch": n * world, "per_gpu_batch": n, "parallelism": "dp%d" % world},
           "roofline": main_res.get("roofline"), "kernels": main_res.get("kernels"),
           "conv_launches_per_step": main_res.get("conv_launches_per_step"), "step_tflops": main_res["step_tflops"]}
    if main_res.get("long_region"):
      out["long_region"] = main_res["long_region"]
    if main_res.get("dumped"):
      out["dumped_outputs"] = main_res["dumped"]
    if dist_info is not None:
      dist_info["buckets"] = main_res.get("buckets")
      out["distributed"] = dist_info
    if other is not None:
      out["other_scaling"] = other
    if ceiling is not None:
      out["strong_scaling_ceiling"] = ceiling
    if f32 is not None:
      out["f32"] = f32
    if pcie is not None:
      out["with_input_pipeline"] = pcie
    if f4 is not None:
      out["bfmnet_train"] = f4
    if secondary is not None:
      out.update(secondary)           # h512_bs2, h512_bs8, bs8_256, config3: top-level keys of the line
    if args.full and not args.no_cpu_baseline and world == 1:
      out["cpu_baseline"] = cpu_baseline(args.height)
    print(json.dumps(out), flush=True)
  if world > 1:
    dist.barrier(group=group)
    dist.destroy_process_group()


if __name__ == "__main__":
  main()

"""CPU tests of the host side: config surface, data layout, session shim, LR schedule, driver arithmetic of
infer_bfmvid.py, and that libvp_hip.so loads and exports every symbol include/vp_hip.h declares."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "params.yml")


def test_config_surface_matches_reference_keys():
  from voicepuppet_amd.config.configure import YParams
  p = YParams(CFG, "default")
  # keys of the reference config/params.yml:1-31
  for k in ("train_dataset_path", "eval_dataset_path", "root_path", "train_by_eval", "sample_file", "model_dir", "mel",
            "frame_rate", "training"):
    assert k in p
  assert p.mel == {"sample_rate": 16000, "num_mel_bins": 80, "win_length": 512, "fft_length": 512, "hop_step": 128}
  assert p.frame_rate == 25 and p.training["decay_steps"] == 1000
  assert set(p.sample_file) == {"landmark_name", "wav_name", "bfmcoeff_name"}
  p.add_hparam("ngf", 64)
  with pytest.raises(ValueError):
    p.add_hparam("ngf", 32)
  p.batch_size = 2            # plain attribute assignment, as the reference scripts do
  assert p.batch_size == 2 and "batch_size" in p


def test_pixrefernet_hparams_and_lr_schedule():
  from voicepuppet_amd.pixrefer.pixrefer import PixReferNet, TRAIN_KEYS, INFER_KEYS
  net = PixReferNet(CFG)
  p = net.params
  assert (p.ngf, p.ndf, p.l1_weight, p.gan_weight, p.separable_conv) == (64, 64, 500.0, 1.0, False)   # pixrefer.py:24-37
  assert p.training["learning_rate"] == 0.0003 and p.training["beta1"] == 0.5 and p.training["decay_rate"] == 0.999
  p.batch_size = 2
  p.add_hparam("is_training", False)
  net.set_params(p)
  net.global_step = 999
  assert net.current_lr() == pytest.approx(3e-4)
  net.global_step = 1000      # == 500 iterations: global_step advances twice per iteration
  assert net.current_lr() == pytest.approx(3e-4 * 0.999)
  assert set(TRAIN_KEYS) >= {"Train_op", "Gen_loss_GAN", "Gen_loss_L1", "Discrim_loss", "Lr", "Global_step", "Outputs", "Alphas"}
  assert INFER_KEYS == ["Inputs", "FGInputs", "Targets", "Outputs", "Alphas", "Outputs_FG"]


def test_datagenerator_params_and_driver_arithmetic():
  from voicepuppet_amd.generator.generator import DataGenerator
  from voicepuppet_amd.pixrefer.infer_bfmvid import prepare_pcm, splice_coeff
  g = DataGenerator(CFG)
  g.set_params(g.params)
  assert (g.sample_rate, g.hop_step, g.win_length, g.frame_wav_scale, g.frame_mfcc_scale) == (16000, 128, 512, 640.0, 5)
  pcm = np.ones(16000, np.float32)            # 1 s -> pad_len = int(1 + 16000/640) = 26 (infer_bfmvid.py:162)
  sl, pad_len = prepare_pcm(pcm, g)
  assert pad_len == 26 and sl.shape == (1, 128 * (26 * 5 - 1) + 512)
  assert np.all(sl[0, :16000] == 1) and np.all(sl[0, 16000:] == 0)
  base = np.arange(257, dtype=np.float32)[None]
  seq = splice_coeff(base, np.full((1, 4, 64), -1, np.float32))
  assert seq.shape == (1, 4, 257) and np.all(seq[0, :, :80] == base[0, :80]) and np.all(seq[0, :, 80:144] == -1)
  assert np.all(seq[0, 2, 144:] == base[0, 144:])
  g2 = DataGenerator(CFG)
  lm = np.zeros((1, 136))
  lm[0, [72, 78]] = [0, 4]; lm[0, [75, 83]] = [1, -1]; lm[0, [77, 81]] = [1, -1]
  lm[0, [84, 90]] = [0, 4]; lm[0, [87, 95]] = [1, -1]; lm[0, [89, 93]] = [1, -1]
  assert g2.ear_compute(lm)[0, 0] == pytest.approx(1.0)      # (2+2)/4 per eye


def test_pixrefer_sample_packing_layout():
  """generator.py:1006-1019: inputs = (example 3dface, current 3dface); fg_inputs = (example tgt*mask, current tgt*mask)."""
  from voicepuppet_amd.generator.generator import pack_sample
  S = 4
  rng = np.random.default_rng(0)
  ex, cur = rng.uniform(size=(S, 3 * S, 3)).astype(np.float32), rng.uniform(size=(S, 3 * S, 3)).astype(np.float32)
  inputs, fg, tgt, msk = pack_sample(ex, cur, S)
  np.testing.assert_array_equal(inputs[..., 0:3], ex[:, S:2 * S])
  np.testing.assert_array_equal(inputs[..., 3:6], cur[:, S:2 * S])
  np.testing.assert_array_equal(fg[..., 0:3], ex[:, :S] * ex[:, 2 * S:])
  np.testing.assert_array_equal(fg[..., 3:6], cur[:, :S] * cur[:, 2 * S:])
  np.testing.assert_array_equal(tgt, cur[:, :S])
  np.testing.assert_array_equal(msk, cur[:, 2 * S:])


def test_dataset_iterator_and_session_shim():
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  from voicepuppet_amd.runtime import IteratorNext, Node, Session
  g = PixReferDataGenerator(CFG)
  p = g.params
  p.batch_size, p.img_size = 3, 32
  it = g.get_dataset().make_one_shot_iterator()
  nodes = it.get_next()
  assert [n.shape for n in nodes] == [(3, 32, 32, 6), (3, 32, 32, 6), (3, 32, 32, 3), (3, 32, 32, 3)]
  assert all(isinstance(n, IteratorNext) for n in nodes)
  b = it.next_batch()
  assert [x.shape for x in b] == [n.shape for n in nodes] and all(x.dtype == np.float32 for x in b)
  assert 0 <= b[2].min() and b[2].max() <= 1

  class Owner(object):
    calls = 0
    def execute(self, names, feeds):
      Owner.calls += 1
      return {n: len(n) for n in names}
  o = Owner()
  sess = Session()
  assert sess.run([Node(o, "ab"), Node(o, "abcd")]) == [2, 4] and Owner.calls == 1     # one execution per run
  assert sess.run(Node(o, "xyz")) == 3


def test_library_exports_every_declared_symbol():
  from voicepuppet_amd import _lib
  lib = _lib.lib()
  header = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  declared = sorted(set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", header)))
  assert len(declared) > 25
  for name in declared:
    assert hasattr(lib, name), "libvp_hip.so does not export %s" % name
  assert set(declared) == set(_lib.exported_symbols()), set(declared) ^ set(_lib.exported_symbols())
  assert lib.vp_version() >= 100
  # manifests are host-side queries: usable without a GPU
  d = _lib.PixReferDesc(1, 256, 64, 64, 1, 1, 500.0, 1.0, 0)
  assert [lib.vp_pixrefer_param_count(ctypes.byref(d), w) for w in range(3)] == [35158852, 2769601, 1735488]
  assert lib.vp_pixrefer_workspace_bytes(ctypes.byref(d)) > 0
  bad = _lib.PixReferDesc(1, 100, 64, 64, 1, 1, 500.0, 1.0, 0)
  assert lib.vp_pixrefer_workspace_bytes(ctypes.byref(bad)) == 0                        # height must be a multiple of 256
  assert lib.vp_bfmnet_param_count() > 7_000_000


def test_every_descriptor_size_query_has_its_layout_check():
  """_lib.lib() compares vp_X_desc_size() with the ctypes structure of _lib.DESC_SIZE_QUERIES (include/vp_hip.h, "ABI rule"): every such
  query the binding knows has its line there, and every structure but vp_pixrefer_desc, which predates the field, starts with the
  struct_bytes the library checks per call."""
  from voicepuppet_amd import _lib
  queries = [s for s in _lib.exported_symbols() if re.fullmatch(r"vp_\w+_desc_size", s)]
  assert len(queries) >= 10
  assert set(queries) == set(_lib.DESC_SIZE_QUERIES), set(queries) ^ set(_lib.DESC_SIZE_QUERIES)
  for query, struct in _lib.DESC_SIZE_QUERIES.items():
    assert issubclass(struct, ctypes.Structure), query
    if query != "vp_pixrefer_desc_size":
      assert struct._fields_[0][0] == "struct_bytes", query


def test_workspace_view_aliases_the_bytes_and_refuses_what_lies_outside():
  """_handle.workspace_view is a function of a uint8 tensor and an address: on a 64-byte CPU tensor an int16 [2, 3] view at offset 8 is
  bytes 8..19; a view that starts in front of the tensor or ends behind it raises, one that ends at its last byte does not."""
  import torch
  from voicepuppet_amd._handle import workspace_view
  ws = torch.zeros(64, dtype=torch.uint8)
  base = ws.data_ptr()
  v = workspace_view(ws, base + 8, (2, 3), torch.int16)
  assert v.dtype == torch.int16 and tuple(v.shape) == (2, 3)
  v.copy_(torch.tensor([[0x0102, 0x0304, 0x0506], [0x0708, 0x090a, 0x0b0c]], dtype=torch.int16))
  got = ws.numpy()
  assert got[8:20].tolist() == [2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11] and not got[:8].any() and not got[20:].any()
  with pytest.raises(ValueError):
    workspace_view(ws, base - 1, (2, 3), torch.int16)
  with pytest.raises(ValueError):
    workspace_view(ws, base + 53, (2, 3), torch.int16)          # 53 + 12 = 65: one byte behind the end
  with pytest.raises(ValueError):
    workspace_view(ws, base + 62, (1, 3), torch.uint8)
  last = workspace_view(ws, base + 52, (2, 3), torch.int16)     # ends exactly at byte 64
  last.fill_(-1)
  assert (ws.numpy()[52:] == 255).all() and not ws.numpy()[20:52].any()
  assert tuple(workspace_view(ws, base + 60, (4,), torch.uint8).shape) == (4,)


def test_missing_config_exits_with_status_zero(tmp_path):
  """train_pixrefer.py:24-32: logger.error + exit(0)."""
  from voicepuppet_amd.pixrefer import train_pixrefer
  with pytest.raises(SystemExit) as e:
    train_pixrefer.main(["--config_path", str(tmp_path / "nope.yml")])
  assert e.value.code == 0
  with pytest.raises(SystemExit) as e:
    train_pixrefer.main([])
  assert e.value.code == 0


def test_angle_sequence_follows_render_face_state_machine():
  # infer_bfmvid.py:76-90: +0.005 per frame on all three angles, direction flips once |angle_y| passes 0.03
  from voicepuppet_amd.pixrefer.infer_bfmvid import angle_sequence
  a = angle_sequence(40)
  assert a.shape == (40, 3) and a.dtype == np.float32
  assert np.array_equal(a[:, 0], a[:, 1]) and np.array_equal(a[:, 1], a[:, 2])
  d = np.diff(np.concatenate([[0.0], a[:, 1]]))
  assert np.allclose(np.abs(d), 0.005, atol=1e-6)
  assert a[:, 1].max() < 0.0401 and a[:, 1].min() > -0.0401 and (d < 0).any() and (d[20:] > 0).any()


def test_product_path_never_imports_the_oracle():
  """oracle/ is test infrastructure: the package and the launchers must not import it, bench.py only inside its cpu_baseline*() legs."""
  import ast
  import glob
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

  def oracle_imports(path):
    tree = ast.parse(open(path).read())
    hits = []
    for node in ast.walk(tree):
      if isinstance(node, ast.Import) and any(a.name.split(".")[0] == "oracle" for a in node.names):
        hits.append(node.lineno)
      if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "oracle":
        hits.append(node.lineno)
    return tree, hits

  files = glob.glob(os.path.join(root, "voicepuppet_amd", "**", "*.py"), recursive=True) + \
      glob.glob(os.path.join(root, "voicepuppet", "**", "*.py"), recursive=True)
  assert files
  for f in files:
    assert not oracle_imports(f)[1], f
  tree, hits = oracle_imports(os.path.join(root, "bench.py"))
  fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("cpu_baseline")]
  assert hits and all(any(fn.lineno <= h <= fn.end_lineno for fn in fns) for h in hits), hits


def test_pmc_kernel_classifier():
  import os
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
  import pmc_summary as p
  assert p.classify("_ZN2vp16igemm_dma_kernelIDF16bLi2ELi4ELi4ELi4ELb1ELb0EEEvNS_9IgemmArgsE") == "igemm_dma_bf16_128x256"
  assert p.classify("_ZN2vp15igemm_ws_kernelIDF16bLi2ELi4ELi8ELi4ELi4ELb0EEEvNS_9IgemmArgsE") == "igemm_ws_bf16_256x256"
  assert p.classify("_ZN2vp12wgrad_kernelIDF16bLi2ELi2ELi4ELi4ELi2ELb1EEEvNS_9WgradArgsE") == "wgrad_bf16_128x128"
  assert p.classify("void vp::conv_cin8_kernel<3>(vp::IgemmArgs, int, int)") == "cin8_bf16_64x16"
  assert p.classify("vp::adam_tf_kernel(vp::AdamArgs)") is None
  assert p.classify("_ZN2vp19igemm_patch3_kernelIDF16bLi2ELi4ELi8ELi2ELi8ELi16ELb0ELi4EEEvNS_9IgemmArgsE") == "patch3_bf16_256x128"
  assert p.classify("_ZN2vp19igemm_patch2_kernelIDF16bLi2ELi4ELi2ELi4ELi16ELi16ELb0ELi4ELb0EEEvNS_9IgemmArgsE") == "patch2_bf16_64x256"
  assert p.classify("void vp::wgrad_tr_kernel<4, 2, 4, 4, 3, true, true>(vp::WgradArgs)") == "wgrad_tr_exact_bf16_256x128"
  assert p.classify("void vp::wgrad_tr_kernel<4, 2, 4, 4, 3, true, false>(vp::WgradArgs)") == "wgrad_tr_fast_bf16_256x128"
  assert p.classify("void vp::wgrad_tr_kernel<4, 2, 2, 4, 3, false, false>(vp::WgradArgs)") == "wgrad_tr_bf16_128x128"


def test_bench_launches_n_ranks_as_a_child_before_touching_the_gpu(monkeypatch):
  """`python bench.py --gpus 4` with no WORLD_SIZE: the parent builds a torch.distributed.run command for 4 ranks on
  127.0.0.1 and relays the child's exit code; a rank whose WORLD_SIZE disagrees with --gpus refuses to run."""
  import importlib
  import subprocess
  import bench
  importlib.reload(bench)
  seen = {}

  def fake_call(cmd, env=None):
    seen["cmd"], seen["env"] = cmd, env
    return 7
  monkeypatch.setattr(subprocess, "call", fake_call)
  monkeypatch.delenv("WORLD_SIZE", raising=False)
  monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
  with pytest.raises(SystemExit) as e:
    bench.main()
  assert e.value.code == 7
  cmd = seen["cmd"]
  assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
  assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
  assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
  monkeypatch.setenv("WORLD_SIZE", "2")
  with pytest.raises(SystemExit) as e:
    bench.main()
  assert e.value.code == 2
  a = bench.parse_args(["--gpus", "8"])
  assert a.scaling == "strong" and bench.per_gpu_batch(a, "strong", 8) == 4 and bench.per_gpu_batch(a, "weak", 8) == 32
  with pytest.raises(SystemExit):
    bench.per_gpu_batch(bench.parse_args(["--global-batch", "30"]), "strong", 8)


def test_clip_sharding_and_the_config5_launcher(tmp_path, monkeypatch):
  """BASELINE config 5 (8 clips over 8 GPUs): clips are dealt round-robin, every clip has exactly one owner, and the launcher
  starts one child per rank with RANK / LOCAL_RANK / WORLD_SIZE set (no collective anywhere on this path)."""
  from voicepuppet_amd.parallel import shard_round_robin
  from voicepuppet_amd.pixrefer import infer_clips
  for n, w in ((8, 8), (11, 4), (3, 8), (0, 2)):
    owners = [shard_round_robin(n, r, w) for r in range(w)]
    assert sorted(i for o in owners for i in o) == list(range(n))
    assert max(len(o) for o in owners) - min(len(o) for o in owners) <= 1
  with pytest.raises(ValueError):
    shard_round_robin(4, 4, 4)
  lst = tmp_path / "clips.txt"
  lst.write_text("a.jpg a.wav\n# comment\nb.jpg b.wav b.npz\n\n")
  assert infer_clips.read_clip_list(str(lst)) == [("a.jpg", "a.wav"), ("b.jpg", "b.wav", "b.npz")]
  lst.write_text("only_one_field\n")
  with pytest.raises(ValueError):
    infer_clips.read_clip_list(str(lst))

  class Opts:
    config_path, frame_batch, out_root = CFG, 4, "o"
  cmds = infer_clips.rank_commands(Opts, "clips.txt", 8)
  assert len(cmds) == 8
  for r, (argv, env) in enumerate(cmds):
    assert env["RANK"] == env["LOCAL_RANK"] == str(r) and env["WORLD_SIZE"] == "8"
    assert argv[1:3] == ["-m", "voicepuppet_amd.pixrefer.infer_clips"] and argv[-1] == "clips.txt" and "--gpus" in argv


_VALIDATE_SNIPPET = r"""
import ctypes, sys
sys.path.insert(0, %r)
from voicepuppet_amd import _lib
L = _lib.lib()
bad = 0
# (batch, height, ngf, ndf, dtype, training, per_sample_bn): BASELINE.json configs 1, 2, 4 (per GPU), 5 and two corner cases
for cfg in [(1, 256, 64, 64, 0, 0, 0), (32, 256, 64, 64, 1, 1, 0), (8, 512, 64, 64, 1, 1, 0), (25, 256, 64, 64, 1, 0, 1), (2, 256, 8, 8, 0, 1, 0), (3, 512, 16, 32, 1, 1, 0)]:
  d = _lib.PixReferDesc(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], 500.0, 1.0, cfg[6])
  rc = L.vp_pixrefer_validate_plan(ctypes.byref(d))
  ws = L.vp_pixrefer_workspace_bytes(ctypes.byref(d))
  n = sum(L.vp_pixrefer_param_count(ctypes.byref(d), w) for w in range(3))
  print(cfg, rc, ws, n, L.vp_last_error().decode() if rc else "")
  bad += rc != 0 or ws == 0 or n == 0
# descriptors the planner must refuse (no out-of-bounds plan is ever built for them)
for cfg in [(0, 256, 64, 64, 1, 1, 0), (4, 200, 64, 64, 1, 1, 0), (4, 256, 128, 64, 1, 1, 0), (4, 256, 64, 48, 1, 1, 0), (2000, 256, 64, 64, 1, 0, 1)]:
  d = _lib.PixReferDesc(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], 500.0, 1.0, cfg[6])
  rc = L.vp_pixrefer_validate_plan(ctypes.byref(d))
  print("refused", cfg, rc)
  bad += rc != -1
sys.exit(1 if bad else 0)
"""


def _run_validate(env_extra):
  import subprocess
  env = dict(os.environ)
  env.update(env_extra)
  return subprocess.run([sys.executable, "-c", _VALIDATE_SNIPPET % ROOT], env=env, capture_output=True, text=True, timeout=600)


def test_plan_validation_every_baseline_config():
  """vp_pixrefer_validate_plan (host-only: no GPU call) on the descriptors of every BASELINE.json config."""
  r = _run_validate({})
  assert r.returncode == 0, r.stdout + r.stderr


def test_host_layer_under_sanitizers():
  """The `make host-asan` build of the host / C-ABI layer (AddressSanitizer + UBSan, kernels reduced to launch stubs) plans and
  validates the same descriptors: a heap overrun or UB in the planner fails here, on the CPU (GPU sanitizers do not exist on this pool)."""
  import shutil, subprocess
  csrc = os.path.join(ROOT, "voicepuppet_amd", "csrc")
  if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", csrc, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  so = os.path.join(ROOT, "voicepuppet_amd", "libvp_host_asan.so")
  rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
  assert os.path.exists(rt), rt
  r = _run_validate({"VP_LIB": so, "LD_PRELOAD": rt, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99", "UBSAN_OPTIONS": "halt_on_error=1:exitcode=98"})
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def _integration_stub():
  """The host part of the ctypes binding INTEGRATION.md section B documents (the fenced block marked '[binding-stub: host part]')."""
  import re
  doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
  m = re.search(r"```python\n(# \[binding-stub: host part\]\n.*?)```", doc, re.S)
  assert m, "INTEGRATION.md: the host part of the binding stub is gone"
  return m.group(1)


def _asan_env():
  import shutil, subprocess
  csrc = os.path.join(ROOT, "voicepuppet_amd", "csrc")
  if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", csrc, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  so = os.path.join(ROOT, "voicepuppet_amd", "libvp_host_asan.so")
  rt = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
  assert os.path.exists(rt), rt
  env = dict(os.environ)
  # PYTHONMALLOC=malloc: ctypes structures come from malloc (not from pymalloc's arenas), so ASan puts a red zone behind each one
  env.update({"VP_LIB": so, "LD_PRELOAD": rt, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=99", "UBSAN_OPTIONS": "halt_on_error=1:exitcode=98",
              "PYTHONMALLOC": "malloc"})
  return env


def test_integration_stub_executes_under_asan():
  """Row b3 of SURVEY.md section 8: the reference-side binding INTEGRATION.md shows is EXECUTED, as written, against the sanitizer build
  of the host layer (declarations, load-time layout check, vp_pixrefer_param_count / _workspace_bytes / _validate_plan).  A descriptor
  that drifts from include/vp_hip.h (round 5 grew the struct 36 -> 48 bytes and left the documented stub behind: VERDICT r5) fails
  here twice over: the stub's own vp_pixrefer_desc_size() check, and AddressSanitizer on the over-read."""
  import subprocess
  env = _asan_env()
  stub = _integration_stub()
  code = stub + "\nassert ws_bytes > 0 and all(c > 0 for c in counts), (ws_bytes, counts)\nprint('stub ok', ctypes.sizeof(Desc), counts, ws_bytes)\n"
  r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "stub ok 48" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
  # the declarations agree with the product binding and with the header's field list
  import re
  from voicepuppet_amd import _lib
  fields = re.findall(r'\("(\w+)", ctypes\.c_(\w+)\)', stub[stub.index("class Desc"):stub.index("lib.vp_pixrefer_desc_size")])
  assert fields == [(n, t.__name__[2:]) for n, t in _lib.PixReferDesc._fields_], fields
  hdr = open(os.path.join(ROOT, "include", "vp_hip.h")).read()
  body = hdr[hdr.index("typedef struct vp_pixrefer_desc {"):hdr.index("} vp_pixrefer_desc;")]
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  hfields = [n for decl in re.findall(r"\b(?:int|float)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
  assert hfields == [n for n, _ in fields], (hfields, fields)
  # the test has teeth: the 9-field struct of rounds 1-4 (what INTEGRATION.md still showed after round 5), pushed past the size check,
  # is caught by AddressSanitizer as a heap over-read inside the library
  old = stub.replace('                ("streams", ctypes.c_int), ("d_backward_fork", ctypes.c_int), ("d_beside_vgg", ctypes.c_int)]', "                ]")
  old = old.replace("if lib.vp_pixrefer_desc_size() != ctypes.sizeof(Desc):", "if False:")
  assert old != stub and "if False:" in old
  r2 = subprocess.run([sys.executable, "-c", old], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r2.returncode != 0 and "heap-buffer-overflow" in r2.stderr, (r2.returncode, r2.stderr[-2000:])
  # ... and by the stub's own check when it is left in
  r3 = subprocess.run([sys.executable, "-c", old.replace("if False:", "if lib.vp_pixrefer_desc_size() != ctypes.sizeof(Desc):")], env=env, cwd=ROOT,
                      capture_output=True, text=True, timeout=600)
  assert r3.returncode != 0 and "library 48 bytes, binding 36" in r3.stderr, r3.stderr[-2000:]


def test_product_library_reads_no_environment_switches():
  """Kernel selection and the executor's schedule are arguments (vp_pixrefer_desc, vp_pixrefer_set_option, vp_tune), not environment
  variables read once per process: no getenv in the library sources."""
  import glob
  import re
  root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voicepuppet_amd", "csrc")
  hits = []
  for f in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
    for i, line in enumerate(open(f), 1):
      if re.search(r"\bgetenv\s*\(", line):
        hits.append("%s:%d" % (os.path.basename(f), i))
  assert not hits, hits

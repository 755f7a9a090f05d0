"""Users of the device frame metrics on the GPU.  voicepuppet_amd/pixrefer/compare_frames.py on two directories of PIL-written JPEGs
reproduces the numpy restatement (tests/frame_metrics_ref.py) applied to PIL's decodes of the same files.  The held-out evaluation of the
training launcher (voicepuppet_amd/pixrefer/heldout.py) leaves a training run bit-identical, and what it logs is the restatement applied
to the generator output of the existing inference forward."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_metrics_ref as fr  # noqa: E402
from test_frame_metrics_host import _image, _jpeg, _pil_rgb  # noqa: E402

pytestmark = pytest.mark.gpu


def test_compare_frames_reproduces_the_restatement_on_pil_decodes(tmp_path, capsys):
  """quality 95 against quality 50 of the same 48 x 64 images; frame 2 of B is progressive, which the device decoder refuses: PIL's
  decode is uploaded for it; the frames themselves never come back to the host"""
  from voicepuppet_amd.pixrefer import compare_frames as cf
  from PIL import Image
  da, db = tmp_path / "q95", tmp_path / "q50"
  da.mkdir(); db.mkdir()
  n = 4
  for i in range(n):
    img = _image(64, 48, 80 + i)
    assert img.shape == (48, 64, 3)
    (da / ("%d.jpg" % i)).write_bytes(_jpeg(img, 95))
    if i == 2:
      Image.fromarray(img).save(str(db / "2.jpg"), "JPEG", quality=50, progressive=True)
    else:
      (db / ("%d.jpg" % i)).write_bytes(_jpeg(img, 50))
  out = str(tmp_path / "metrics.json")
  res = cf.main([str(da), str(db), "--out", out])
  want = np.stack([fr.metrics(_pil_rgb(str(da / ("%d.jpg" % i))), _pil_rgb(str(db / ("%d.jpg" % i)))) for i in range(n)])
  got = np.array([[f[k] for k in cf.COLUMNS] for f in res["frames"]])
  print(np.abs(got - want).max(0))
  assert [f["index"] for f in res["frames"]] == list(range(n))
  assert np.all(np.abs(got[:, :2] - want[:, :2]) <= np.spacing(want[:, :2]))
  assert np.abs(got[:, 2:] - want[:, 2:]).max() <= 1e-9
  assert 5 < want[:, 2].min() < 60 and 0 < want[:, 3].min() < 1            # the two qualities differ: no trivial comparison
  s = res["summary"]
  assert s["frames"] == n and s["PSNR"]["worst"] == int(np.argmin(want[:, 2])) and abs(s["SSIM"]["mean"] - want[:, 3].mean()) <= 1e-9
  with open(out) as f:
    assert json.load(f)["summary"] == s
  assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("frame ")]) == n


# ---- held-out evaluation ---------------------------------------------------------------------------------------------------------------
S, K, STEPS = 256, 2, 3                     # the mini size of the training tests: 256 x 256, ngf = ndf = 8, float32


def _eval_list(root):
  """a dataset list of one folder with three 256 x 768 triptychs"""
  folder = root / "clip"
  folder.mkdir()
  for i in range(3):
    (folder / ("%d.jpg" % i)).write_bytes(_jpeg(_image(3 * S, S, 90 + i), 90))
  lst = root / "eval.txt"
  lst.write_text("%s|3\n" % folder)
  return str(lst)


def _train(lst):
  """STEPS training steps on one fixed batch from one seed; lst: evaluate after every step (eval_step = 1), None: never"""
  import torch
  from oracle import pixrefer_ref as ref
  from voicepuppet_amd.engine import PixReferEngine
  from voicepuppet_amd.pixrefer.heldout import HeldOutEval
  eng = PixReferEngine(1, S, 8, 8, dtype="f32", training=True)
  eng.load_params(ref.init_params(8, 8, seed=0, dtype=np.float32))
  rng = np.random.default_rng(1)
  batch = [torch.tensor(rng.uniform(size=(1, S, S, c)).astype(np.float32), device="cuda") for c in (6, 6, 3, 3)]
  ev = HeldOutEval(eng, lst, frames=K) if lst else None
  losses, logged = [], []
  for _ in range(STEPS):
    eng.train_step(*batch, lr=3e-4)
    losses.append(eng.tensor("losses").clone())
    if ev is not None:
      ev.run()
      logged.append(ev.last.clone())
  torch.cuda.synchronize()
  state = {"params_g": eng.params_g, "params_d": eng.params_d, "m_g": eng.adam["g"][0], "v_g": eng.adam["g"][1], "m_d": eng.adam["d"][0],
           "v_d": eng.adam["d"][1], "losses": torch.stack(losses), "grads_g": eng.grads_g}
  return eng, ev, {k: v.cpu().numpy().copy() for k, v in state.items()}, logged


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
  lst = _eval_list(tmp_path_factory.mktemp("heldout"))
  plain = _train(None)
  plain[0].close()
  return lst, plain[2], _train(lst)


def test_held_out_evaluation_leaves_training_bit_identical(runs):
  _, plain, (eng, ev, state, logged) = runs
  assert eng.t_g == STEPS and eng.t_d == STEPS and len(logged) == STEPS
  for k in plain:
    assert plain[k].tobytes() == state[k].tobytes(), k
  assert np.abs(state["params_g"]).max() > 0 and np.abs(state["m_g"]).max() > 0 and np.isfinite(state["losses"]).all()
  assert not np.array_equal(logged[0].cpu().numpy(), logged[-1].cpu().numpy())          # it saw the weights move


def test_held_out_numbers_equal_the_restatement_on_the_inference_forward(runs):
  from oracle.input_pack_ref import pack_frames_ref
  from voicepuppet_amd.engine import PixReferEngine
  from voicepuppet_amd.pixrefer import heldout
  lst, _, (eng, ev, _, logged) = runs
  got = ev.read()
  assert got["frames"] == K and ev.crop == ((S - 243) // 2, (S - 243) // 2, 243) == heldout.centre_crop(S, 0.9)
  # the inputs: frames 0 and 1 of the list with frame 0 as example, cropped at the centre, packed as the host pipeline packs them
  folder = os.path.dirname(lst) + "/clip"
  frames = [np.ascontiguousarray(_pil_rgb("%s/%d.jpg" % (folder, i))[:, :, ::-1]) for i in range(K)]
  for j in range(K):
    want = pack_frames_ref(frames[0], frames[j], np.array([ev.crop, ev.crop], np.int32), S)
    for t, w in zip((ev.inputs, ev.fg_inputs, ev.targets), want):
      assert float(np.abs(t[j].cpu().numpy() - w).max()) < 2e-6
  # the numbers: an inference engine of the test's own with the trained weights, its Outputs against the targets through the restatement
  e2 = PixReferEngine(K, S, 8, 8, dtype="f32", training=False, per_sample_bn=True)
  e2.load_params(eng.get_params(0))
  e2.forward(ev.inputs, ev.fg_inputs, ev.targets)
  out, tg = e2.fetch("Outputs").cpu().numpy(), ev.targets.cpu().numpy()
  want = fr.batch(fr.map_f32(out, 255.0, 0.0), fr.map_f32(tg, 255.0, 0.0)).mean(0)
  print(got, want)
  assert abs(got["L1"] - want[0]) <= 1e-9 and abs(got["PSNR"] - want[2]) <= 1e-9 and abs(got["SSIM"] - want[3]) <= 1e-9
  assert np.abs(logged[-1].cpu().numpy() - want).max() <= 1e-9
  # --device_jpeg_decode: the same frames through JpegDecoder, byte for byte
  paths = ["%s/%d.jpg" % (folder, i) for i in range(3)]
  a, b = heldout.load_frames(paths, S), heldout.load_frames(paths, S, device_jpeg_decode=True)
  assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and int(a.max()) > 0
  e2.close()


def test_train_cli_logs_held_out_metrics(runs, tmp_path, monkeypatch, capsys):
  """train_pixrefer.py --eval_list: 50 steps reach the first step that prints the losses; the held-out line is printed next to them"""
  from voicepuppet_amd.pixrefer import train_pixrefer
  cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "params.yml")
  monkeypatch.chdir(tmp_path)
  os.makedirs("config")
  train_pixrefer.main(["--config_path", cfg, "--steps", "50", "--batch_size", "1", "--img_size", str(S), "--eval_list", runs[0],
                       "--eval_step", "25", "--eval_frames", str(K)])
  text = capsys.readouterr().out
  assert "gen_loss_L1=" in text and "held-out (%d frames): PSNR=" % K in text and "SSIM=" in text

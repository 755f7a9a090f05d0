"""The training summaries (voicepuppet_amd/pixrefer/summaries.py) on a mini training plan: the event file's scalars, tags and images, the
images against the restatement of the float -> uint8 rule on the step's own tensors; and train_pixrefer.py with and without --tensorboard."""
import glob
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
from test_tb_events_host import parse_event, records  # noqa: E402

pytestmark = pytest.mark.gpu

S = 256                                       # the smallest image the generator's eight stride-2 encoders take
NAMES = ("inputs1", "targets", "outputs", "alphas", "inputs0")


def decode(data):
  from PIL import Image
  im = Image.open(io.BytesIO(data))
  im.load()
  return np.asarray(im)


def test_one_step_writes_three_scalars_and_ten_images(tmp_path):
  import torch
  from oracle import pixrefer_ref as ref
  from voicepuppet_amd.engine import PixReferEngine
  from voicepuppet_amd.pixrefer.summaries import TrainSummaries
  eng = PixReferEngine(2, S, 8, 8, dtype="f32", training=True)
  eng.load_params(ref.init_params(8, 8, seed=0, dtype=np.float32))
  rng = np.random.default_rng(1)
  batch = [torch.tensor(rng.uniform(size=(2, S, S, c)).astype(np.float32), device="cuda") for c in (6, 6, 3, 3)]
  batch[2][0, :4, :4] = torch.tensor([-0.1, 0.0, 1.0, 1.2], device="cuda")[:, None, None]       # targets outside [0, 1] saturate
  tb = TrainSummaries(str(tmp_path / "log"), 2, S)
  eng.train_step(*batch, lr=3e-4)
  pending = tb.enqueue(eng)
  tb.write(2, (1.5, 0.25, 0.125), pending)
  tb.close()
  want = {"inputs1": batch[0][..., 3:6], "targets": batch[2], "outputs": eng.fetch("Outputs"), "alphas": eng.fetch("Alphas"),
          "inputs0": batch[0][..., 0:3]}
  want = {k: png_ref.to_u8(v.cpu().numpy()) for k, v in want.items()}
  eng.close()
  files = glob.glob(str(tmp_path / "log" / "events.out.tfevents.*"))
  assert len(files) == 1
  evs = [parse_event(r) for r in records(open(files[0], "rb").read())]
  assert len(evs) == 2 and evs[0]["file_version"] == "brain.Event:2" and evs[1]["step"] == 2
  values = evs[1]["summary"]
  assert [(v["tag"], v["simple_value"]) for v in values[:3]] == [("discriminator_loss", 1.5), ("generator_loss_GAN", 0.25),
                                                                 ("generator_loss_L1", 0.125)]
  assert [v["tag"] for v in values[3:]] == ["%s_summary/%s/image/%d" % (n, n, i) for n in NAMES for i in range(2)]
  for v in values[3:]:
    name, i = v["tag"].split("/")[1], int(v["tag"].rsplit("/", 1)[1])
    h, w, cs, data = v["image"]
    assert (h, w, cs) == (S, S, 3)
    assert np.array_equal(decode(data), want[name][i]), v["tag"]
    assert data == png_ref.encode(want[name][i]), v["tag"]
  assert want["targets"][0, :4, 0, 0].tolist() == [0, 0, 255, 255]
  assert len({bytes(v["image"][3]) for v in values[3:]}) == 10               # ten different pictures


def test_train_cli_writes_an_event_file_only_with_the_flag(tmp_path, monkeypatch, capsys):
  """50 steps reach global_step 100, the first summary step"""
  from voicepuppet_amd.pixrefer import train_pixrefer
  cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "params.yml")
  for flag in ([], ["--tensorboard"]):
    run = tmp_path / ("with" if flag else "without")
    os.makedirs(run / "config")
    monkeypatch.chdir(run)
    train_pixrefer.main(["--config_path", cfg, "--steps", "50", "--batch_size", "1", "--img_size", str(S)] + flag)
    assert "gen_loss_L1=" in capsys.readouterr().out
    assert os.path.exists(run / "log" / "summary_pixrefer" / "outputs_100.png")
    files = glob.glob(str(run / "log" / "summary_pixrefer" / "events.out.tfevents.*"))
    if not flag:
      assert files == [] and not glob.glob(str(run / "**" / "*tfevents*"), recursive=True)
      continue
    assert len(files) == 1
    evs = [parse_event(r) for r in records(open(files[0], "rb").read())]
    assert [e.get("step") for e in evs] == [None, 100]
    values = evs[1]["summary"]
    assert [v["tag"] for v in values] == ["discriminator_loss", "generator_loss_GAN", "generator_loss_L1"] + \
        ["%s_summary/%s/image/0" % (n, n) for n in NAMES]
    assert all(np.isfinite(v["simple_value"]) for v in values[:3])
    for v in values[3:]:
      assert v["image"][:3] == (S, S, 3) and decode(v["image"][3]).shape == (S, S, 3)

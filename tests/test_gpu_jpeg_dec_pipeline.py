"""The device JPEG decoder inside the training input pipeline (PixReferDataGenerator.get_device_dataset with amd.device_jpeg_decode,
FramePrefetcher's compressed-source mode): the batches of the PIL path bit for bit (the decoder equals libjpeg byte for byte:
tests/test_jpeg_dec_host.py), later epochs from the cached index, a refused file decoded by PIL into its row, a corrupt file fatal."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_dec_host import _image, _pil  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = os.path.join(ROOT, "config", "params.yml")
S, N = 64, 2


def _folders(tmp_path, grey=None):
  """two folders of three S x 3S triptychs and the two-line list file"""
  from PIL import Image
  lines = []
  for d in range(2):
    folder = tmp_path / ("clip%d" % d)
    folder.mkdir()
    for i in range(3):
      img = _image(3 * S, S, 70 + 3 * d + i)
      if grey == (d, i):
        Image.fromarray(img[..., 0]).save(str(folder / ("%d.jpg" % i)), "JPEG")
      else:
        (folder / ("%d.jpg" % i)).write_bytes(_pil(img, quality=90))
    lines.append("%s|3\n" % folder)
  (tmp_path / "train.txt").write_text("".join(lines))
  return str(tmp_path / "train.txt")


def _iterator(list_file, on):
  from voicepuppet_amd.generator.generator import PixReferDataGenerator
  g = PixReferDataGenerator(CFG)
  p = g.params
  p.dataset_path = list_file
  p.batch_size = N
  p.img_size = S
  p.shuffle_bufsize = 1
  amd = dict(p.get('amd') or {})
  amd['device_jpeg_decode'] = on
  p.amd = amd
  g.set_params(p)
  assert g.device_jpeg_decode == on and g.data_list is not None
  return g.get_device_dataset().make_one_shot_iterator()


def _batches(list_file, on, count):
  import torch
  random.seed(5)
  it = _iterator(list_file, on)
  out, segs = [], []
  for _ in range(count):
    b = it.next_batch()
    torch.cuda.synchronize()
    out.append([t.cpu().numpy().copy() for t in b])
    segs.append(list(it._pf.segments_used))
  return out, segs, it


def test_batches_equal_the_host_decode_and_later_epochs_use_the_index(tmp_path):
  import torch
  lst = _folders(tmp_path)
  off, segs_off, _ = _batches(lst, False, 9)
  on, segs, it = _batches(lst, True, 9)
  for a, b in zip(off, on):
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  assert all(s == [] for s in segs_off)
  # an epoch is 6 samples = 3 batches; a batch's entries are harvested three fills later and the prefetcher fills two batches ahead:
  # the first epoch decodes one lane per file, the last batches asked for run from the index, one lane per MCU row (S / 16 = 4)
  assert segs[0] == [1] * (2 * N)
  assert segs[-1] == [S // 16] * (2 * N), segs
  dec = it._pf.decoder
  dec.harvest()
  assert len(dec.index) == 6 and all(v.shape == (S // 16, 4) for v in dec.index.values())
  from voicepuppet_amd.jpeg_dec import JpegDecoder
  dec.save_index(str(tmp_path / "idx.npz"))
  other = JpegDecoder(2, S, 3 * S)
  other.load_index(str(tmp_path / "idx.npz"))
  assert sorted(other.index) == sorted(dec.index) and all(np.array_equal(other.index[k], dec.index[k]) for k in dec.index)
  paths = sorted(k[0] for k in dec.index)[:2]
  _, st = other.decode(paths)
  assert st.cpu().tolist() == [0, 0] and other.last_segments == [S // 16] * 2
  torch.cuda.synchronize()


def test_a_refused_file_is_decoded_by_pil_into_its_row(tmp_path):
  lst = _folders(tmp_path, grey=(1, 2))
  off, _, _ = _batches(lst, False, 3)
  on, segs, _ = _batches(lst, True, 3)
  for a, b in zip(off, on):
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  flat = [s for batch in segs for s in batch]
  assert 0 in flat and 1 in flat                    # the grey file came decoded, the others as files


def test_a_corrupt_file_is_fatal_and_named(tmp_path):
  import torch
  lst = _folders(tmp_path)
  bad = tmp_path / "clip0" / "1.jpg"
  data = bad.read_bytes()
  bad.write_bytes(data[:len(data) // 2])            # cut in the middle of its scan: the header parses, the lane runs out of data
  random.seed(5)
  it = _iterator(lst, True)
  with pytest.raises(RuntimeError, match="1.jpg"):
    for _ in range(12):
      it.next_batch()
  torch.cuda.synchronize()

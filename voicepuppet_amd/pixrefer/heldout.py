"""Held-out evaluation for the PixReferNet training launcher (train_pixrefer.py --eval_list): the first K triptychs of a dataset list,
cropped at the centre, through the generator's inference forward with the current training weights, compared with their targets on the
device (voicepuppet_amd.metrics.FrameMetrics, vp_frame_metrics_f32).  The reference has no evaluation at all.

The training engine is only READ: run() copies its generator arena into an inference engine of this object's own (own workspace, own
weights, per-sample batch-norm statistics as build_inference_op uses), so no gradient, optimiser slot, counter or activation buffer of
the training step is touched.  run() only enqueues on the current stream; read() is the host wait.
"""
import os

import numpy as np
import torch

from .. import _lib
from ..engine import PixReferEngine
from ..generator.device_pipeline import DeviceFramePacker
from ..metrics import FrameMetrics, L1, PSNR, SSIM


def centre_crop(img_size, crop_ratio):
  """(rx, ry, rsize) of the deterministic crop: the middle of the range draw_crop draws rsize from, centred"""
  rsize = (int(img_size * crop_ratio) + img_size) // 2
  return (img_size - rsize) // 2, (img_size - rsize) // 2, rsize


def first_pairs(list_path, frames):
  """the first `frames` (example .jpg, current .jpg) of a dataset list of 'folder|count' lines: frame i of a folder with the folder's
  frame 0 as its example (the training generator draws the example at random; here nothing is random)"""
  pairs = []
  with open(list_path) as f:
    for line in f:
      if not line.strip():
        continue
      folder, count = line.strip().split('|')
      for i in range(int(count)):
        if len(pairs) == frames:
          return pairs
        pairs.append((os.path.join(folder, '0.jpg'), os.path.join(folder, '{}.jpg'.format(i))))
  return pairs


def load_frames(paths, img_size, device_jpeg_decode=False):
  """.jpg triptychs -> uint8 [n, S, 3S, 3] BGR device tensor (what cv2.imread returns and vp_pixrefer_pack_frames takes); with
  device_jpeg_decode through JpegDecoder, PIL's decode uploaded for a file it refuses"""
  from PIL import Image
  S = img_size
  out = torch.zeros(len(paths), S, 3 * S, 3, dtype=torch.uint8, device="cuda")

  def pil(path):
    img = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    if img.shape != (S, 3 * S, 3):
      raise ValueError("%s is %s, not the %d x %d triptych of img_size %d" % (path, img.shape[:2], S, 3 * S, S))
    return torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1]))
  items = [None] * len(paths)
  if device_jpeg_decode:
    from .. import jpeg_dec
    for k, p in enumerate(paths):
      with open(p, "rb") as fh:
        data = fh.read()
      info = jpeg_dec.parse(data, S, 3 * S)
      if not info.refused and (info.height, info.width) == (S, 3 * S):
        items[k] = (data, info, None, None, p)
    if any(it is not None for it in items):
      dec = jpeg_dec.JpegDecoder(len(paths), S, 3 * S, bgr=True, max_file_bytes=max(1 << 22, max(len(it[0]) for it in items if it)))
      status = torch.zeros(len(paths), dtype=torch.int32, device="cuda")
      dec.decode_into(items, out, out.stride(1), out.stride(0), status, raise_bad=False)
      for k in np.nonzero(status.cpu().numpy())[0]:
        items[k] = None                                 # corrupt for the device decoder: libjpeg's word counts
  for k, p in enumerate(paths):
    if items[k] is None:
      out[k].copy_(pil(p))
  return out


class HeldOutEval:
  """run() -> device float64 [4] (mean L1, MSE, PSNR, SSIM over the K frames, values in [0, 255]); read() -> {'L1', 'PSNR', 'SSIM',
  'frames'} of the last run as Python floats."""

  def __init__(self, train_engine, eval_list, frames=8, crop_ratio=0.9, device_jpeg_decode=False):
    d = train_engine.desc
    S = int(d.height)
    pairs = first_pairs(eval_list, int(frames))
    if not pairs:
      raise ValueError("eval_list %s names no frames" % eval_list)
    K = self.frames = len(pairs)
    self.train_engine = train_engine
    self.crop = centre_crop(S, crop_ratio)
    ex = load_frames([p[0] for p in pairs], S, device_jpeg_decode)
    cur = load_frames([p[1] for p in pairs], S, device_jpeg_decode)
    crops = torch.tensor([[self.crop, self.crop]] * K, dtype=torch.int32, device="cuda")
    self.packer = DeviceFramePacker(K, S)
    self.inputs, self.fg_inputs, self.targets, _ = self.packer(ex, cur, crops)       # the held-out set is fixed: packed once
    self.engine = PixReferEngine(K, S, int(d.ngf), int(d.ndf), dtype="bf16" if d.dtype == _lib.VP_BF16 else "f32", training=False,
                                 per_sample_bn=True)
    if self.engine.params_g.numel() != train_engine.params_g.numel():
      raise RuntimeError("the inference plan's generator arena differs from the training plan's")
    self.metrics = FrameMetrics(K, S, S)
    self.rows = torch.zeros(K, 4, dtype=torch.float64, device="cuda")
    self.last = None

  def run(self):
    self.engine.params_g.copy_(self.train_engine.params_g)       # a read of the training weights, in stream order behind their update
    self.engine.params_changed()
    self.engine.forward(self.inputs, self.fg_inputs, self.targets)
    out = self.engine.fetch("Outputs")                             # deprocessed, [0, 1], like the targets
    self.metrics.compare(out, self.targets, value_range=(0, 1), out=self.rows)
    self.last = self.rows.mean(0)
    return self.last

  def read(self):
    m = self.last.cpu().numpy()
    return {"L1": float(m[L1]), "PSNR": float(m[PSNR]), "SSIM": float(m[SSIM]), "frames": self.frames}

"""Visual evaluation of BFMNet on the MI355X: the reference's mesh montage (utils/bfm_visual.py plot_bfm_coeff_seq, :88-154, what
voicepuppet/bfmnet/train_bfmnet.py:138 writes at every evaluation step) and a number in image units to go with it.

The montage is a 9 x 10 sheet of 224 x 224 tiles: up to 30 frames of the first sequence of the batch, the real coefficients from row 0,
the predicted expression spliced into them from row 3; rows 6-8 are never written (the reference sizes the sheet for three blocks and
fills two: kept).  Every tile is Reconstruction (reconstruct_mesh.py:172-194) of one frame, rasterised (mesh_core.cpp:169-231): here one
reconstruction launch chain and one raster launch for all tiles (ClipRenderer.render_view), one launch per block to lay them onto the
sheet (vp_sheet_tile_u8), one for the landmark distance (vp_landmark_distance), and a baseline JPEG encode of the sheet on the device.

LMD: per frame, the mean Euclidean distance between the 68 projected landmarks (facemodel.keypoints) of the real and the predicted
frame, in pixels of the 224 image, over all 68 and over landmarks 48..67 (the mouth).

Channel order.  The reference swaps every tile (cvtColor, :125) and hands the sheet to cv2.imwrite, which reads it as BGR (:154): the
FILE's RGB is big_img[..., ::-1], the rasteriser's order before the swap.  MeshSheet's sheet is that array (what is encoded);
MeshSheet(swap_rb=True) gives the reference's in-memory big_img instead.

No CPU fallback: without a GPU MeshSheet raises.  sheet_cells, splice_predicted and clip_time are plain arithmetic and need none.
"""
import os
import re

import numpy as np

BLOCK_X, BLOCK_Y, IMG_SIZE = 10, 9, 224          # bfm_visual.py:90-92
MAX_TIME = 30                                    # :133-136
REAL_ROW, PRED_ROW = 0, 3                        # :145, :152
JPEG_QUALITY = 95                                # cv2.imwrite's default
STRIP_W = 560                                    # the device encoder's frames are at most 832 wide: the sheet goes through it as 4 strips


def clip_time(seq_len):
  """bfm_visual.py:133-136: the first sequence of the batch, trimmed to 30 frames."""
  return min(int(seq_len[0]), MAX_TIME)


def sheet_cells(time, h_index, cols=BLOCK_X):
  """bfm_visual.py:127-128: (row, column) of frame i = (i // cols + h_index, i % cols), i.e. cell h_index * cols + i."""
  return [((h_index * cols + i) // cols, (h_index * cols + i) % cols) for i in range(int(time))]


def splice_predicted(real, pred, id_coeff=None, texture_coeff=None):
  """bfm_visual.py:147-150: the predicted expression [B,T,64] inside the real sequence [B,T,257]; with id_coeff [1,1,80] AND texture_coeff
  [1,1,80] those replace the real identity and texture (pose, lighting and translation, 224:, stay the real ones).  numpy in, numpy
  out; device tensors in, device tensor out."""
  if isinstance(real, np.ndarray):
    cat, tile = (lambda parts: np.concatenate(parts, axis=2)), (lambda a: np.tile(np.asarray(a), (1, real.shape[1], 1)))
  else:
    import torch
    cat = lambda parts: torch.cat([p.to(real.dtype) for p in parts], dim=2)
    tile = lambda a: torch.as_tensor(a, device=real.device).repeat(1, real.shape[1], 1)
  if id_coeff is None or texture_coeff is None:
    return cat([real[:, :, :80], pred, real[:, :, 144:]])
  return cat([tile(id_coeff), pred, tile(texture_coeff), real[:, :, 224:]])


def sheet_tile(tiles, sheet, first_cell=0, swap_rb=False):
  """vp_sheet_tile_u8: tile i of `tiles` uint8 [n,h,w,3] to cell first_cell + i of `sheet` uint8 [rows*h, cols*w, 3] (device tensors,
  contiguous), on the current stream.  A cell outside the sheet raises before anything is enqueued."""
  import torch
  from .. import _lib
  from .._handle import ptr, stream
  n, h, w = (int(v) for v in tiles.shape[:3])
  for t in (tiles, sheet):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == (4 if t is tiles else 3) and t.shape[-1] == 3):
      raise ValueError("sheet_tile: contiguous uint8 device tensors, tiles [n,h,w,3] and sheet [rows*h, cols*w, 3]")
  if sheet.shape[0] % h or sheet.shape[1] % w:
    raise ValueError("sheet_tile: a sheet of %d x %d is no whole number of %d x %d tiles" % (sheet.shape[0], sheet.shape[1], h, w))
  _lib.check(_lib.lib().vp_sheet_tile_u8(ptr(tiles), n, h, w, ptr(sheet), int(sheet.shape[0]) // h, int(sheet.shape[1]) // w, int(first_cell),
                                         1 if swap_rb else 0, stream()), "vp_sheet_tile_u8")
  return sheet


def landmark_distance(proj_a, proj_b, keypoints):
  """vp_landmark_distance: float64 [F,2] device = per frame the mean distance over the 68 landmarks and over landmarks 48..67, between
  proj_a and proj_b float64 [F,N,2] (device, contiguous); keypoints int32 [68] device."""
  import torch
  from .. import _lib
  from .._handle import ptr, stream
  F, N = int(proj_a.shape[0]), int(proj_a.shape[1])
  for t in (proj_a, proj_b):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (F, N, 2)):
      raise ValueError("landmark_distance: contiguous float64 device projections [F,N,2] of one shape")
  if not (keypoints.is_cuda and keypoints.dtype == torch.int32 and keypoints.is_contiguous() and keypoints.numel() == 68):
    raise ValueError("landmark_distance: keypoints int32 [68] on the device")
  out = torch.empty(F, 2, dtype=torch.float64, device=proj_a.device)
  _lib.check(_lib.lib().vp_landmark_distance(ptr(proj_a), ptr(proj_b), ptr(keypoints), F, N, ptr(out), stream()), "vp_landmark_distance")
  return out


def _assemble_strips(header, files, sheet_w):
  """One baseline JPEG of width sheet_w from the device encoder's files of its equally wide vertical strips.  The encoder closes every
  MCU row of a frame with a restart marker (jpeg.py), so a strip's MCU row is a restart interval of strip_w / 16 MCUs: the wide image with
  the same restart interval is, per MCU row, the strips' intervals left to right, the markers renumbered modulo 8."""
  at = header.index(b"\xff\xc0\x00\x11\x08")
  head = header[:at + 7] + bytes([sheet_w >> 8, sheet_w & 255]) + header[at + 9:]
  rows = []
  for f in files:
    assert f[:len(header)] == header and f[-2:] == b"\xff\xd9"
    rows.append(re.split(b"\xff[\xd0-\xd7]", f[len(header):-2]))      # entropy-coded bytes never hold FF D0..D7 (byte stuffing)
  n = len(rows[0])
  assert all(len(r) == n for r in rows)
  out, k = [head], 0
  for r in range(n):
    for strip in rows:
      if k:
        out.append(bytes([0xff, 0xd0 + ((k - 1) & 7)]))
      out.append(strip[r])
      k += 1
  out.append(b"\xff\xd9")
  return b"".join(out)


class MeshSheet:
  """render(seq_len, real, pred[, id_coeff, texture_coeff]) -> (sheet uint8 [2016, 2240, 3] device, lmd float64 [time, 2] device);
  jpeg() -> the sheet of the last render as the bytes of a .jpg file (quality 95, 4:2:0), encoded on the device."""

  def __init__(self, facemodel, swap_rb=False):
    import torch
    from ..utils.reconstruct_mesh import ClipRenderer
    if not torch.cuda.is_available():
      raise RuntimeError("MeshSheet needs an MI355X (no CPU fallback)")
    self.renderer = facemodel if isinstance(facemodel, ClipRenderer) else ClipRenderer(facemodel, IMG_SIZE, IMG_SIZE)
    if (self.renderer.h, self.renderer.w) != (IMG_SIZE, IMG_SIZE):
      raise ValueError("MeshSheet: the tiles are %d x %d" % (IMG_SIZE, IMG_SIZE))
    self.model = self.renderer.model
    kp = np.asarray(self.model.keypoints).reshape(-1)
    if kp.size != 68 or kp.min() < 0 or kp.max() >= self.model.nver:
      raise ValueError("MeshSheet: facemodel.keypoints must be 68 vertex indices (0-based)")
    self.keypoints = torch.from_numpy(kp.astype(np.int32)).to(self.model.device)
    self.swap_rb = bool(swap_rb)
    self.sheet = torch.zeros(BLOCK_Y * IMG_SIZE, BLOCK_X * IMG_SIZE, 3, dtype=torch.uint8, device=self.model.device)
    self._encoder = None

  def _coeff(self, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(self.model.device, torch.float32)

  def render(self, seq_len, real, pred, id_coeff=None, texture_coeff=None):
    import torch
    time = clip_time(seq_len.cpu().numpy() if torch.is_tensor(seq_len) else seq_len)
    real, pred = self._coeff(real), self._coeff(pred)
    if real.dim() != 3 or real.shape[2] != 257 or pred.dim() != 3 or pred.shape[2] != 64 or pred.shape[:2] != real.shape[:2]:
      raise ValueError("MeshSheet.render: real [B,T,257] and pred [B,T,64]")
    if not 1 <= time <= real.shape[1]:
      raise ValueError("MeshSheet.render: seq_len[0] %d outside 1 .. %d frames" % (time, real.shape[1]))
    if id_coeff is not None and texture_coeff is not None:
      id_coeff, texture_coeff = self._coeff(id_coeff).reshape(1, 1, 80), self._coeff(texture_coeff).reshape(1, 1, 80)
    spliced = splice_predicted(real[:1, :time], pred[:1, :time], id_coeff, texture_coeff)
    coeff = torch.cat([real[0, :time], spliced[0]], dim=0).contiguous()               # [2 * time, 257]: real tiles, then predicted
    # per-frame textures: what a Reconstruction call per frame gives (the real sequence's texture coefficients vary over a clip)
    tiles, _, o = self.renderer.render_view(coeff, view=0, shared_texture=False, full=True)
    self.sheet.zero_()                                                                # no stale tiles of a longer clip before
    for block, row in ((tiles[:time], REAL_ROW), (tiles[time:], PRED_ROW)):
      sheet_tile(block, self.sheet, row * BLOCK_X, self.swap_rb)
    proj = o["face_projection"]
    return self.sheet, landmark_distance(proj[:time], proj[time:], self.keypoints)

  def jpeg(self, rgb=None):
    """The .jpg file of `rgb` (default: the sheet) at quality 95.  The sheet is wider than a frame of the device encoder (832): its four
    560-wide strips are the encoder's frames, and the file is put together from their restart intervals (_assemble_strips).  A strip the
    encoder refuses (a row over its slot) sends the whole sheet through the host encoder, as JpegEncoder.to_host does for a frame."""
    from ..jpeg import JpegEncoder, host_jpeg
    rgb = self.sheet if rgb is None else rgb
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    n = W // STRIP_W
    if self._encoder is None:
      self._encoder = JpegEncoder(H, STRIP_W, n, quality=JPEG_QUALITY)
    strips = rgb.view(H, n, STRIP_W, 3).permute(1, 0, 2, 3).contiguous()
    data, lengths = self._encoder.encode(strips)
    if int(lengths.min()) < 0:
      return host_jpeg(rgb.cpu().numpy(), JPEG_QUALITY)
    return _assemble_strips(self._encoder.header(), self._encoder.to_host(data, lengths), W)


def plot_bfm_coeff_seq(save_dir, facemodel, step, seq_len, real_bfm_coeff_seq, bfm_coeff_seq, id_coeff=None, texture_coeff=None):
  """bfm_visual.py:88-154, same arguments (numpy arrays or device tensors; `facemodel` the reference's BFM object, or a MeshSheet that is
  kept between calls): writes <save_dir>/bfmnet_<step>.jpg and returns (mean LMD, mean mouth LMD) in pixels over the frames shown."""
  ms = facemodel if isinstance(facemodel, MeshSheet) else MeshSheet(facemodel)
  if ms.swap_rb:
    raise ValueError("plot_bfm_coeff_seq: the file is encoded from the unswapped sheet (MeshSheet(swap_rb=False))")
  _, lmd = ms.render(seq_len, real_bfm_coeff_seq, bfm_coeff_seq, id_coeff, texture_coeff)
  data = ms.jpeg()
  with open(os.path.join(save_dir, 'bfmnet_{}.jpg'.format(step)), 'wb') as fh:
    fh.write(data)
  mean = lmd.mean(dim=0).cpu().numpy()
  return float(mean[0]), float(mean[1])

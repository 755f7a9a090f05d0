"""Alpha mattes for clips in front of a plain backdrop, on the device (libvp_hip.so: vp_keymatte_*, csrc/key_matte.hip): a colour model of
the backdrop fitted to the frames' border (top band and upper sides), a soft key on the distance from it, one guided-filter pass with the
frame's luma as the guide.  include/vp_hip.h defines every number; tests/key_matte_ref.py restates it in numpy.

In place of the matte that step 6 of the reference's datasets/make_data_from_GRID.py takes from its segmentation and matting networks,
for a head and shoulders in front of a studio backdrop only.  It is a key, not a matting network: on a cluttered background it is the
wrong tool, and report() says so (status, kept, residual_rms).  The defaults below come from synthetic scenes and are untuned on real
footage.

foreground() (vp_key_foreground) returns the subject's own colours on the matte's soft edge, with the backdrop's share taken out by the
same model; voicepuppet_amd.matte_clean.MatteCleaner is the clean-up stage for the matte itself.

fit, matte and foreground only enqueue on the current stream; report() and spill() are the host reads.
"""
import ctypes
import os

import torch

from . import _lib
from ._handle import Handle, ptr, rgb_frames, stream, u8_plane

MODEL_DOUBLES = _lib.KEYMATTE_MODEL_DOUBLES
# the model record's fields (include/vp_hip.h): 9 plane numbers, 6 of the inverse covariance, then these
N, KEPT, RESIDUAL_RMS, STATUS = 15, 16, 17, 18
STATUS_TEXT = {0: "fitted", 1: "degenerate: too few samples or no spread in x and y; the backdrop is taken as one colour"}


def keymatte_desc(max_frames, max_height, max_width, max_radius=16):
  return _lib.KeyMatteDesc(ctypes.sizeof(_lib.KeyMatteDesc), int(max_frames), int(max_height), int(max_width), int(max_radius))


def default_band(height):
  return max(2, int(height) // 16)


def spill_of(model, height, width):
  """See KeyMatte.spill; model: the record as a host array (Python floats round as the kernel's float64 does)."""
  x, y = float(int(width) // 2), float(int(height) // 2)
  v = [(float(model[3 * c]) + float(model[3 * c + 1]) * x) + float(model[3 * c + 2]) * y for c in range(3)]
  k = max(range(3), key=lambda c: (v[c], -c))
  lead = v[k] - max(v[c] for c in range(3) if c != k)
  return {"channel": k, "lead": lead, "active": lead >= 16.0}


class KeyMatte(Handle):
  """fit(frames) then matte(frames) for device uint8 RGB tensors [n, H, W, 3], n <= max_frames, 16 <= H <= max_height, 16 <= W <= max_width.
  Strided views are taken as they are when a pixel's three values and a row's pixels are adjacent (a padded JpegDecoder output).  With
  max_radius > 0 the workspace holds two float64 planes: 16 bytes per pixel of max_frames x max_height x max_width."""

  def __init__(self, max_frames, max_height, max_width, max_radius=16):
    if not torch.cuda.is_available():
      raise RuntimeError("KeyMatte needs an MI355X (no CPU fallback)")
    self._open("keymatte", keymatte_desc(max_frames, max_height, max_width, max_radius), invalid="invalid key matte descriptor")
    self.max_frames, self.max_height, self.max_width, self.max_radius = int(max_frames), int(max_height), int(max_width), int(max_radius)
    self._png = None

  def fit(self, frames, band=None, side_rows=None, trim=16.0, sigma_min=2.0):
    """The backdrop model from the border of `frames` (all of them in one call): band rows at the top and band columns at both sides of
    the first side_rows rows; defaults max(2, H // 16) and H // 2.  Two passes, the second over the samples within `trim` (a squared
    distance in standard deviations) of the first.  Returns self."""
    pitch, stride, n, H, W = rgb_frames(frames, "fit")
    rc = self.L.vp_keymatte_fit(self.h, ptr(frames), pitch, stride, n, H, W, 0 if band is None else int(band),
                                0 if side_rows is None else int(side_rows), float(trim), float(sigma_min), stream())
    _lib.check(rc, "vp_keymatte_fit")
    return self

  def model(self):
    """A copy of the model record: device float64 [MODEL_DOUBLES]."""
    out = torch.empty(MODEL_DOUBLES, dtype=torch.float64, device="cuda")
    _lib.check(self.L.vp_keymatte_get_model(self.h, ptr(out), stream()), "vp_keymatte_get_model")
    return out

  def set_model(self, t):
    """Installs a model record (what model() returned, for these frames' size)."""
    if t.dtype != torch.float64 or tuple(t.shape) != (MODEL_DOUBLES,):
      raise ValueError("set_model: a float64 tensor [%d]" % MODEL_DOUBLES)
    t = t.cuda().contiguous()
    _lib.check(self.L.vp_keymatte_set_model(self.h, ptr(t), stream()), "vp_keymatte_set_model")
    return self

  def report(self):
    """{'status', 'N', 'kept', 'residual_rms'} of the model: the one host read.  status 0 is a fit; kept is the share of border samples
    the second pass kept; residual_rms the backdrop's spread about its planes in grey levels."""
    m = self.model().cpu().numpy()
    return {"status": int(m[STATUS]), "N": int(m[N]), "kept": float(m[KEPT]), "residual_rms": float(m[RESIDUAL_RMS])}

  def matte(self, frames, lo=4.0, hi=10.0, radius=4, eps=25.0, out=None, raw=None):
    """-> device uint8 [n, H, W]: 0 on the backdrop, 255 on the subject.  lo, hi: the key's ramp in standard deviations of the backdrop;
    radius, eps: the guided filter's window and regulariser (grey levels squared); radius 0 returns the raw key.  out, raw: contiguous
    device uint8 [>= n, H, W] to write the matte and the raw key into."""
    pitch, stride, n, H, W = rgb_frames(frames, "matte")
    if out is None:
      out = torch.empty(max(n, 1), H, W, dtype=torch.uint8, device="cuda")
    for name, t in (("out", out), ("raw", raw)):
      if t is not None:
        u8_plane(t, "matte", name, n, H, W)
    rc = self.L.vp_keymatte_apply(self.h, ptr(frames), pitch, stride, n, H, W, float(lo), float(hi), int(radius), float(eps), ptr(raw), ptr(out),
                                  stream())
    _lib.check(rc, "vp_keymatte_apply")
    return out[:n]

  def foreground(self, frames, matte, despill=0.0, out=None):
    """-> device uint8 [n, H, W, 3]: the subject's own colours, F of I = a F + (1 - a) B with the model's planes as B: per channel
    b + (I - b) * 255 / m, the frame's colours where the matte is 255 and 0 where it is 0.  What frame x matte then carries on the soft
    edge is the subject's colour, not a fringe of the backdrop's.  despill (0 .. 1) also pulls the backdrop's key channel down to the
    mean of the other two where it exceeds it - only when that channel leads by 16 grey levels at the frame's centre; spill() says
    whether it does.  matte: contiguous device uint8 [n, H, W] (KeyMatte's own or a cleaned one); out: contiguous [>= n, H, W, 3]."""
    pitch, stride, n, H, W = rgb_frames(frames, "foreground")
    u8_plane(matte, "foreground", "matte", n, H, W, exact=True)
    if out is None:
      out = torch.empty(max(n, 1), H, W, 3, dtype=torch.uint8, device="cuda")
    else:
      u8_plane(out, "foreground", "out", n, H, W, channels=3)
    rc = self.L.vp_key_foreground(self.h, ptr(frames), pitch, stride, n, H, W, ptr(matte), float(despill), ptr(out), stream())
    _lib.check(rc, "vp_key_foreground")
    return out[:n]

  def spill(self, height, width):
    """{'channel', 'lead', 'active'}: the backdrop's largest channel at the centre of a height x width frame, its lead over the larger of
    the other two in grey levels, and whether foreground's despill acts (lead >= 16).  A host read of the model."""
    return spill_of(self.model().cpu().numpy(), height, width)

  def tensor(self, name):
    """'moments': int64 [2, 21], pass 1 and pass 2 of the last fit; 'model': float64 [MODEL_DOUBLES].  Views of the workspace."""
    return self._tensor(name, torch.int64, 2) if name == "moments" else self._tensor(name, torch.float64, 1)

  def write_png(self, matte, dir, first_index):
    """matte [n, H, W] -> <first_index + i>.png in `dir`, one grey channel (PngEncoder); returns the paths."""
    from .png import PngEncoder
    n, H, W = (int(v) for v in matte.shape)
    if self._png is None or (self._png.height, self._png.width) != (H, W) or self._png.max_frames < n:
      self._png = PngEncoder(max(n, 1), H, W, channels=1)
    paths = []
    for i, data in enumerate(self._png.files(matte.contiguous())):
      paths.append(os.path.join(dir, "%d.png" % (first_index + i)))
      with open(paths[-1], "wb") as f:
        f.write(data)
    return paths

"""Numpy restatement of the triptych stages (include/vp_hip.h, "PixReferNet training triptychs"; csrc/triptych.hip), written from the
definitions there: float32 where the kernels are float32 (numpy rounds every float32 product and sum on its own), int64 for the blur, a
plain breadth-first flood fill from the border.  tests/test_gpu_triptych.py compares the device with these functions byte for byte;
tests/test_triptych_host.py pins them against scipy and a float64 Gaussian."""
from collections import deque

import numpy as np

TAPS, RADIUS = 21, 10
STATUS_OK, STATUS_SMALL, STATUS_LARGE, STATUS_OUTSIDE = 0, 1, 2, 3


def fill_holes(mask):
  """scipy.ndimage.binary_fill_holes(mask > 0) with the default structuring element, as uint8 0 / 1: a zero pixel stays zero only if a
  4-connected path of zero pixels joins it to the image border."""
  free = np.asarray(mask) == 0
  h, w = free.shape
  outside = np.zeros((h, w), bool)
  todo = deque()
  for y in range(h):
    for x in range(w):
      if (y in (0, h - 1) or x in (0, w - 1)) and free[y, x]:
        outside[y, x] = True
        todo.append((y, x))
  while todo:
    y, x = todo.popleft()
    for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
      if 0 <= ny < h and 0 <= nx < w and free[ny, nx] and not outside[ny, nx]:
        outside[ny, nx] = True
        todo.append((ny, nx))
  return (~outside).astype(np.uint8)


def linear_table(src, dst):
  """(index [dst] int, c0 [dst] float32, c1 [dst] float32): f = (d + 0.5) * (src / dst) - 0.5 in float64, clamped at both ends."""
  d = np.arange(dst, dtype=np.float64)
  f = (d + 0.5) * (float(src) / float(dst)) - 0.5
  s = np.floor(f)
  frac = f - s
  low, high = s < 0, s >= src - 1
  s = np.where(low, 0, np.where(high, src - 1, s)).astype(np.int64)
  frac = np.where(low | high, 0.0, frac)
  return s, (1.0 - frac).astype(np.float32), frac.astype(np.float32)


def resize_mask(mask01, side):
  """The 0 / 1 mask as float32, src x src -> side x side: horizontal pass, then vertical pass, each v0 * c0 + v1 * c1 in float32."""
  m = (np.asarray(mask01) > 0).astype(np.float32)
  src = m.shape[0]
  assert m.shape == (src, src)
  s, c0, c1 = linear_table(src, side)
  s1 = np.minimum(s + 1, src - 1)
  hor = m[:, s] * c0[None, :] + m[:, s1] * c1[None, :]
  out = hor[s, :] * c0[:, None] + hor[s1, :] * c1[:, None]
  assert out.dtype == np.float32
  return out


def erode5(m):
  """Minimum over the 5 x 5 window centred on the pixel; pixels outside the image take no part."""
  h, w = m.shape
  out = np.empty_like(m)
  for y in range(h):
    rows = m[max(y - 2, 0):y + 3]
    col_min = rows.min(axis=0)
    for x in range(w):
      out[y, x] = col_min[max(x - 2, 0):x + 3].min()
  return out


def blur_taps():
  k = np.arange(TAPS, dtype=np.float64)
  g = np.exp(-((k - RADIUS) ** 2) / 32.0)
  g = g / g.sum()
  q = np.floor(65536.0 * g + 0.5).astype(np.int64)
  q[RADIUS] += 65536 - q.sum()
  return q


def reflect101(i, n):
  return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def blur(u):
  """The integer Gaussian on uint8 [h, w] (h, w >= 11): taps of blur_taps, REFLECT_101, (v + 2^31) >> 32."""
  u = np.asarray(u)
  assert u.dtype == np.uint8 and min(u.shape) >= RADIUS + 1
  q = blur_taps()
  h, w = u.shape
  x = np.arange(w)
  y = np.arange(h)
  hor = np.zeros((h, w), np.int64)
  for k in range(TAPS):
    hor += q[k] * u[:, reflect101(x + k - RADIUS, w)].astype(np.int64)
  assert hor.max() < 2 ** 31
  ver = np.zeros((h, w), np.int64)
  for k in range(TAPS):
    ver += q[k] * hor[reflect101(y + k - RADIUS, h), :]
  return ((ver + 2 ** 31) >> 32).astype(np.uint8)


def mask_chain(mask01, side):
  """Stages b-d: uint8 [side, side]."""
  m = erode5(resize_mask(mask01, side))
  return blur((m * np.float32(255)).astype(np.uint8))


def geometry_status(side, y0, x0, size, max_side):
  if side < RADIUS + 1:
    return STATUS_SMALL
  if side > max_side:
    return STATUS_LARGE
  if y0 < 0 or x0 < 0 or y0 + side > size or x0 + side > size:
    return STATUS_OUTSIDE
  return STATUS_OK


def paste_render(render, side, y0, x0, size):
  """The render behind the channel swap and OpenCV's uint8 bilinear (oracle/cv_resize_ref.py), on a black size x size canvas."""
  from oracle import cv_resize_ref as cr
  canvas = np.zeros((size, size, 3), np.uint8)
  canvas[y0:y0 + side, x0:x0 + side] = cr.resize_linear_u8(np.ascontiguousarray(render[:, :, ::-1]), (side, side))
  return canvas


def triptych(frame, render, face_mask, geometry, max_side=None, alpha=None):
  """One frame: (uint8 [S, 3S, 3] or None, status)."""
  S = frame.shape[0]
  side, y0, x0 = (int(v) for v in geometry)
  status = geometry_status(side, y0, x0, S, S if max_side is None else max_side)
  if status:
    return None, status
  face = paste_render(render, side, y0, x0, S)
  out = np.zeros((S, 3 * S, 3), np.uint8)
  out[:, :S] = frame
  if alpha is not None:
    out[:, S:2 * S] = face
    out[:, 2 * S:] = alpha[:, :, None]
    return out, status
  u = mask_chain(fill_holes(face_mask), side)
  m = np.zeros((S, S), np.float32)
  m[y0:y0 + side, x0:x0 + side] = u.astype(np.float32) / np.float32(255)
  on = (m > 0).astype(np.float32)
  result = frame * (1 - m[:, :, None]) + face * m[:, :, None]
  result = result * on[:, :, None]
  assert result.dtype == np.float32
  out[:, S:2 * S] = result.astype(np.uint8)
  out[:, 2 * S:] = (m[:, :, None] * np.float32(255)).astype(np.uint8)
  return out, status


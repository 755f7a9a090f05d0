"""4:2:2 (components 2x1, 1x1, 1x1) on top of tests/jpeg_dec_ref.py: the definition the device decoder's third layout (sampling 3,
include/vp_hip.h) is tested against.  jpeg_dec_ref is imported as it is; this file adds what it does not know:

  the geometry      an MCU of 16 x 8 pixels, mcux = ceil(W / 16), mcuy = ceil(H / 8), a chroma component of ceil(W / 2) x H samples
  the block order   four blocks per MCU in scan order Y0 (left), Y1 (right), Cb, Cr
  the up-sampling   libjpeg's h2v1 "fancy" triangle filter along the row: out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] +
                    c[i+1] + 2) >> 2, the edge sample replicated at the border of the component's own samples; nothing down the column

jpeg_dec_ref.parse and decode_segment know two block sequences by name, so the header walk and the segment loop are restated here for any
sequence (COMP_OF); on a 4:2:0 file they give what jpeg_dec_ref gives, which tests/test_jpeg_dec_422_host.py checks.  Dequantisation, the
inverse DCT and the colour conversion are jpeg_dec_ref's.

Test infrastructure only: nothing under voicepuppet_amd/ imports it.
"""
import numpy as np

import jpeg_dec_ref as dr
from jpeg_ref import ZIGZAG

COMP_OF = {1: (0, 1, 2), 2: (0, 0, 0, 0, 1, 2), 3: (0, 0, 1, 2)}       # sampling -> component of every block of an MCU
MCU_SIZE = {1: (8, 8), 2: (16, 16), 3: (8, 16)}                        # sampling -> (height, width) of an MCU in pixels
_SAMPLING = {((1, 1), (1, 1), (1, 1)): 1, ((2, 2), (1, 1), (1, 1)): 2, ((2, 1), (1, 1), (1, 1)): 3}


def parse(data):
  """jpeg_dec_ref.parse for the three layouts: the same dictionary, with sampling 3 for a 4:2:2 file."""
  data = bytes(data)
  # the sampling factors of the frame header, read here; jpeg_dec_ref.parse then sees the file with (1x1, 1x1, 1x1) in their place, which
  # moves no byte, and the geometry is set from the true factors afterwards
  p, sof = 2, None
  while p + 4 <= len(data) and data[p] == 0xff:
    if data[p + 1] == 0xff:
      p += 1
      continue
    if data[p + 1] == 0xc0:
      sof = p + 4
      break
    if data[p + 1] == 0xda:
      break
    p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
  if sof is None or data[sof + 5] != 3:
    return dr.parse(data)                       # (its refusals)
  samp = tuple((data[sof + 7 + 3 * i] >> 4, data[sof + 7 + 3 * i] & 15) for i in range(3))
  if samp not in _SAMPLING:
    raise dr.Refused("sampling %s" % (samp,))
  plain = bytearray(data)
  for i in range(3):
    plain[sof + 7 + 3 * i] = 0x11
  info = dr.parse(bytes(plain))
  s = _SAMPLING[samp]
  H, W = info["size"]
  info["sampling"] = s
  info["comps"] = [(c[0],) + samp[i] + (c[3],) for i, c in enumerate(info["comps"])]
  info["mcuy"], info["mcux"] = -(-H // MCU_SIZE[s][0]), -(-W // MCU_SIZE[s][1])
  info["bpm"] = len(COMP_OF[s])
  return info


def _bits(data, start):
  """the de-stuffed bytes from `start` to the next marker (or the end), and the file offset of each (one more: where the data ended)"""
  raw, where, i = bytearray(), [], start
  while i < len(data):
    if data[i] == 0xff:
      if i + 1 < len(data) and data[i + 1] == 0:
        raw.append(0xff)
        where.append(i)
        i += 2
        continue
      break
    raw.append(data[i])
    where.append(i)
    i += 1
  where.append(i)
  return raw, where


def decode_segment(data, info, seg, out, entries=None):
  """jpeg_dec_ref.decode_segment for any block sequence: one segment (byte, bit, preds, first MCU, MCU count) into out [blocks, 64]
  (zig-zag); entries {mcu row: (byte, bit, preds)} at every MCU-row start."""
  byte, bit, pred, mcu0, count = seg
  pred = list(pred)
  dec = {k: dr._decoder_table(*v) for k, v in info["huff"].items()}
  comp_of, bpm, mcux = COMP_OF[info["sampling"]], info["bpm"], info["mcux"]
  raw, where = _bits(data, byte)
  pos = bit

  def take(n):
    nonlocal pos
    if pos + n > 8 * len(raw):
      raise dr.Corrupt("out of data")
    v = 0
    for _ in range(n):
      v = (v << 1) | ((raw[pos >> 3] >> (7 - (pos & 7))) & 1)
      pos += 1
    return v

  def symbol(t):
    code = 0
    for length in range(1, 17):
      code = (code << 1) | take(1)
      if (length, code) in t:
        return t[(length, code)]
    raise dr.Corrupt("invalid code")

  def extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1

  for mcu in range(mcu0, mcu0 + count):
    if info["dri"] and mcu > mcu0 and mcu % info["dri"] == 0:
      m = where[-1]
      if not (m + 1 < len(data) and data[m] == 0xff and 0xd0 <= data[m + 1] <= 0xd7):
        raise dr.Corrupt("no restart marker")
      raw, where = _bits(data, m + 2)
      pos, pred = 0, [0, 0, 0]
    if entries is not None and mcu % mcux == 0:
      entries[mcu // mcux] = (where[pos >> 3], pos & 7, tuple(dr._wrap16(v) for v in pred))
    for j in range(bpm):
      c = comp_of[j]
      _, td, ta = info["tables"][c]
      blk = out[mcu * bpm + j]
      blk[:] = 0
      s = symbol(dec[(0, td)])
      if s > 15:
        raise dr.Corrupt("DC category %d" % s)
      pred[c] += extend(take(s), s)
      blk[0] = dr._wrap16(pred[c])
      k = 1
      while k < 64:
        rs = symbol(dec[(1, ta)])
        r, s = rs >> 4, rs & 15
        if s == 0:
          if r == 15:
            k += 16
            continue
          break
        k += r
        if k > 63:
          raise dr.Corrupt("k > 63")
        blk[k] = extend(take(s), s)
        k += 1
      if k > 64:
        raise dr.Corrupt("k > 63")


def entropy_decode(data, info=None, segs=None):
  """-> (int16 [blocks, 64] zig-zag in scan order, entries {mcu row: (byte, bit, preds)})"""
  data = bytes(data)
  info = info or parse(data)
  out = np.zeros((info["mcux"] * info["mcuy"] * info["bpm"], 64), np.int16)
  entries = {}
  for seg in (segs if segs is not None else dr.segments(info)):
    decode_segment(data, info, seg, out, entries)
  return out, entries


def planes(info, coef):
  """coef: int16 [blocks, 64] zig-zag, scan order -> [Y, Cb, Cr] padded uint8 planes (4:2:2: Y is 8 mcuy x 16 mcux, chroma 8 mcuy x 8 mcux)"""
  if info["sampling"] != 3:
    return dr.planes(info, coef)
  nat = np.zeros_like(coef)
  nat[:, ZIGZAG] = coef
  mx, my = info["mcux"], info["mcuy"]
  c = nat.reshape(my, mx, 4, 64)
  q = [info["quant"][info["tables"][comp][0]] for comp in range(3)]
  y = dr.idct_blocks(c[:, :, :2].reshape(-1, 64), q[0]).reshape(my, mx, 2, 8, 8)        # block j of MCU (mx, my) is luma block (2 mx + j, my)
  out = [y.transpose(0, 3, 1, 2, 4).reshape(my * 8, mx * 16)]
  for comp in (1, 2):
    px = dr.idct_blocks(c[:, :, 1 + comp].reshape(-1, 64), q[comp]).reshape(my, mx, 8, 8)
    out.append(px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
  return out


def h2v1_upsample(p, h, w):
  """p: padded uint8 chroma plane, (h, w) the component's own size -> int32 [h, 2 w]"""
  c = p[:h, :w].astype(np.int32)
  last = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
  nxt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
  out = np.empty((h, 2 * w), np.int32)
  out[:, 0::2] = (3 * c + last + 1) >> 2
  out[:, 1::2] = (3 * c + nxt + 2) >> 2
  return out


def pixels(info, pl):
  if info["sampling"] != 3:
    return dr.pixels(info, pl)
  H, W = info["size"]
  cb, cr = (h2v1_upsample(p, H, -(-W // 2))[:, :W] for p in pl[1:])
  return dr.ycc_to_rgb(pl[0][:H, :W], cb, cr)


def decode(data):
  info = parse(data)
  coef, _ = entropy_decode(data, info)
  return pixels(info, planes(info, coef))

"""Baseline JPEG decoder in numpy integers: the definition the device decoder (csrc/jpeg_dec.hip, vp_jpegdec_*) is tested against.

Written from ITU T.81 (Annex B: markers, Annex F.2: Huffman decoding) and the published arithmetic of libjpeg's default decode path, which
is what PIL runs: dequantise, the "islow" inverse DCT (13-bit constants, two passes, range limit), "fancy" triangle up-sampling of 4:2:0
chroma (3:1 vertically then 3:1 horizontally, +8 / +7 rounding alternating, the edge sample replicated at the border of the component's own
ceil(W / 2) x ceil(H / 2) samples), the 16-bit fixed-point YCbCr -> RGB conversion.  Every step is int32 arithmetic (wrapping, which only
streams no encoder writes can reach), so a device implementation can equal it byte for byte.

  parse(data)                 dimensions, sampling, tables, DRI, the offset of the entropy-coded data, the restart marker positions
  segments(info)              the scan as segments (byte, bit, (pred Y, Cb, Cr), first MCU, MCU count): one per restart interval, else one.
                              A segment may be any MCU range: a restart boundary inside it is crossed at its marker
  entropy_decode(data, info)  -> int16 [blocks, 64] in scan order, zig-zag inside a block (tests/jpeg_ref.py's order), the entry point
                              recorded at every MCU row, symbol statistics
  planes(info, coef)          padded uint8 Y / Cb / Cr planes
  pixels(info, planes)        uint8 [H, W, 3] RGB
  decode(data)                all of it

Test infrastructure only: nothing under voicepuppet_amd/ imports it.
"""
import numpy as np

from jpeg_ref import ZIGZAG

LOOKUP_BITS = 9          # the device's first-level look-up; a longer code goes through the maxcode walk


class Refused(ValueError):
  pass


class Corrupt(ValueError):
  pass


def parse(data):
  data = bytes(data)
  if data[:2] != b"\xff\xd8":
    raise Refused("no SOI")
  info = {"quant": {}, "huff": {}, "dri": 0, "bytes": len(data)}
  p = 2
  while True:
    if p + 4 > len(data):
      raise Refused("truncated header")
    if data[p] != 0xff:
      raise Refused("no marker at %d" % p)
    m = data[p + 1]
    if m == 0xff:
      p += 1
      continue
    n = int.from_bytes(data[p + 2:p + 4], "big")
    body = data[p + 4:p + 2 + n]
    if p + 2 + n > len(data):
      raise Refused("truncated header")
    if m == 0xdb:
      q = 0
      while q < len(body):
        if body[q] >> 4:
          raise Refused("16-bit quantisation table")
        t = np.zeros(64, np.int32)
        t[ZIGZAG] = np.frombuffer(body[q + 1:q + 65], np.uint8)
        info["quant"][body[q] & 15] = t          # row-major
        q += 65
    elif m == 0xc4:
      q = 0
      while q < len(body):
        bits = list(body[q + 1:q + 17])
        info["huff"][(body[q] >> 4, body[q] & 15)] = (bits, list(body[q + 17:q + 17 + sum(bits)]))
        q += 17 + sum(bits)
    elif m == 0xc0:
      if body[0] != 8:
        raise Refused("%d-bit samples" % body[0])
      info["size"] = (int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"))
      if body[5] != 3:
        raise Refused("%d components" % body[5])
      comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)]
      samp = [(h, v) for _, h, v, _ in comps]
      if samp == [(2, 2), (1, 1), (1, 1)]:
        info["sampling"] = 2
      elif samp == [(1, 1), (1, 1), (1, 1)]:
        info["sampling"] = 1
      else:
        raise Refused("sampling %s" % samp)
      info["comps"] = comps
    elif m in (0xc1, 0xc2, 0xc3, 0xc5, 0xc6, 0xc7, 0xc9, 0xca, 0xcb, 0xcd, 0xce, 0xcf):
      raise Refused("SOF%d" % (m - 0xc0))
    elif m == 0xdd:
      info["dri"] = int.from_bytes(body, "big")
    elif m == 0xda:
      if "size" not in info:
        raise Refused("SOS before SOF")
      if body[0] != 3:
        raise Refused("scan of %d components" % body[0])
      sel = {body[1 + 2 * i]: (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(3)}
      info["tables"] = [(tq,) + sel[cid] for cid, _, _, tq in info["comps"]]       # per component: (Tq, Td, Ta)
      p += 2 + n
      break
    p += 2 + n
  info["scan"] = p
  H, W = info["size"]
  s = 8 * info["sampling"]
  info["mcux"], info["mcuy"] = -(-W // s), -(-H // s)
  info["bpm"] = 6 if info["sampling"] == 2 else 3
  rst = []
  i = p
  while i + 1 < len(data):                     # the plain loop the product's vectorised scan is compared with
    if data[i] == 0xff:
      if 0xd0 <= data[i + 1] <= 0xd7:
        rst.append(i)
      elif data[i + 1] != 0:
        break
      i += 2
    else:
      i += 1
  info["rst"] = rst
  return info


def segments(info):
  n = info["mcux"] * info["mcuy"]
  if not info["dri"]:
    return [(info["scan"], 0, (0, 0, 0), 0, n)]
  starts = [info["scan"]] + [r + 2 for r in info["rst"]]
  if len(starts) < -(-n // info["dri"]):
    raise Corrupt("restart markers missing")
  return [(starts[i], 0, (0, 0, 0), i * info["dri"], min(info["dri"], n - i * info["dri"])) for i in range(min(len(starts), -(-n // info["dri"])))]


def _decoder_table(bits, vals):
  """code -> symbol by (length, code)"""
  table, code, k = {}, 0, 0
  for length in range(1, 17):
    for _ in range(bits[length - 1]):
      table[(length, code)] = vals[k]
      code += 1
      k += 1
    code <<= 1
  return table


def _wrap16(v):
  return ((v + 32768) & 65535) - 32768


def decode_segment(data, info, seg, out, entries=None, stats=None):
  """Decodes one segment into out [blocks, 64] (zig-zag order).  entries: {mcu row: (byte, bit, preds)} recorded at every MCU-row start."""
  byte, bit, pred, mcu0, count = seg
  pred = list(pred)
  raw, where, nbits, acc, pos = bytearray(), [], 0, 0, 0

  def load(start, first_bit):
    """de-stuffed bits from byte `start` to the next marker (or the end), with the file offset of every data byte"""
    nonlocal nbits, acc, pos
    del raw[:], where[:]
    i = start
    while i < len(data):
      b = data[i]
      if b == 0xff:
        if i + 1 < len(data) and data[i + 1] == 0:
          raw.append(0xff)
          where.append(i)
          i += 2
          if stats is not None:
            stats["stuffed"] += 1
          continue
        break
      raw.append(b)
      where.append(i)
      i += 1
    where.append(i)
    nbits, acc, pos = 8 * len(raw), int.from_bytes(bytes(raw), "big") if raw else 0, first_bit

  load(byte, bit)

  def take(n):
    nonlocal pos
    if n == 0:
      return 0
    if pos + n > nbits:
      raise Corrupt("out of data")
    v = (acc >> (nbits - pos - n)) & ((1 << n) - 1)
    pos += n
    return v

  dec = {k: _decoder_table(*v) for k, v in info["huff"].items()}

  def symbol(t):
    nonlocal pos
    code = 0
    for length in range(1, 17):
      code = (code << 1) | take(1)
      if (length, code) in t:
        if stats is not None and length > LOOKUP_BITS:
          stats["long"] += 1
        return t[(length, code)]
    raise Corrupt("invalid code")

  def extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1

  bpm, mcux = info["bpm"], info["mcux"]
  comp_of = (0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2)
  for mcu in range(mcu0, mcu0 + count):
    if info["dri"] and mcu > mcu0 and mcu % info["dri"] == 0:       # a restart inside the segment: the marker, predictors zero
      m = where[-1]
      if not (m + 1 < len(data) and data[m] == 0xff and 0xd0 <= data[m + 1] <= 0xd7):
        raise Corrupt("no restart marker")
      load(m + 2, 0)
      pred = [0, 0, 0]
    if entries is not None and mcu % mcux == 0:
      entries[mcu // mcux] = (where[pos >> 3], pos & 7, tuple(_wrap16(v) for v in pred))
    for j in range(bpm):
      c = comp_of[j]
      _, td, ta = info["tables"][c]
      blk = out[mcu * bpm + j]
      blk[:] = 0
      s = symbol(dec[(0, td)])
      if s > 15:
        raise Corrupt("DC category %d" % s)
      pred[c] += extend(take(s), s)
      blk[0] = _wrap16(pred[c])
      k = 1
      t = dec[(1, ta)]
      while k < 64:
        rs = symbol(t)
        r, s = rs >> 4, rs & 15
        if s == 0:
          if r == 15:
            k += 16
            if stats is not None:
              stats["zrl"] += 1
            continue
          if stats is not None:
            stats["eob"] += 1
          break
        k += r
        if k > 63:
          raise Corrupt("k > 63")
        blk[k] = extend(take(s), s)
        k += 1
      else:
        if stats is not None and k == 64:
          stats["no_eob"] += 1
      if k > 64:
        raise Corrupt("k > 63")


def entropy_decode(data, info=None, segs=None):
  """-> (int16 [blocks, 64] zig-zag, entries {mcu row: (byte, bit, preds)}, stats)"""
  data = bytes(data)
  info = info or parse(data)
  out = np.zeros((info["mcux"] * info["mcuy"] * info["bpm"], 64), np.int16)
  entries, stats = {}, {"zrl": 0, "eob": 0, "no_eob": 0, "stuffed": 0, "long": 0}
  for seg in (segs if segs is not None else segments(info)):
    decode_segment(data, info, seg, out, entries, stats)
  return out, entries, stats


def entry_segments(info, entries):
  return [entries[r] + (r * info["mcux"], info["mcux"]) for r in range(info["mcuy"])]


# ---- pixels ------------------------------------------------------------------------------------------------------------------------------
_C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
          f2562=20995, f3072=25172)


def _idct_pass(x, shift):
  """x: int32 [..., 8] along the last axis -> the islow 8-point inverse pass, descaled by `shift` (int32, wrapping)."""
  i = [x[..., k] for k in range(8)]
  z1 = (i[2] + i[6]) * _C["f0541"]
  tmp2 = z1 + i[6] * (-_C["f1847"])
  tmp3 = z1 + i[2] * _C["f0765"]
  tmp0 = (i[0] + i[4]) << 13
  tmp1 = (i[0] - i[4]) << 13
  t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
  tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
  z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
  z5 = (z3 + z4) * _C["f1175"]
  tmp0, tmp1, tmp2, tmp3 = tmp0 * _C["f0298"], tmp1 * _C["f2053"], tmp2 * _C["f3072"], tmp3 * _C["f1501"]
  z1, z2 = z1 * (-_C["f0899"]), z2 * (-_C["f2562"])
  z3, z4 = z3 * (-_C["f1961"]) + z5, z4 * (-_C["f0390"]) + z5
  tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
  r = 1 << (shift - 1)
  o = [t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3]
  return np.stack([(v + r) >> shift for v in o], axis=-1)


def idct_blocks(coef_rowmajor, q):
  """int16 [n, 64] row-major, q int32 [64] row-major -> uint8 [n, 8, 8]"""
  with np.errstate(over="ignore"):
    x = (coef_rowmajor.astype(np.int32) * q.astype(np.int32)).reshape(-1, 8, 8)
    ws = _idct_pass(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)       # pass 1 down the columns
    px = _idct_pass(ws, 18)                                              # pass 2 along the rows
    return np.clip(px + 128, 0, 255).astype(np.uint8)


def planes(info, coef):
  """coef: int16 [blocks, 64] zig-zag, scan order -> [Y, Cb, Cr] padded uint8 planes"""
  nat = np.zeros_like(coef)
  nat[:, ZIGZAG] = coef
  mx, my, bpm, s = info["mcux"], info["mcuy"], info["bpm"], info["sampling"]
  c = nat.reshape(my, mx, bpm, 64)
  out = []
  for comp in range(3):
    q = info["quant"][info["tables"][comp][0]]
    if comp == 0 and s == 2:
      px = idct_blocks(c[:, :, :4].reshape(-1, 64), q).reshape(my, mx, 2, 2, 8, 8)
      out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16))
    else:
      j = comp if s == 1 else 3 + comp
      px = idct_blocks(c[:, :, j].reshape(-1, 64), q).reshape(my, mx, 8, 8)
      out.append(px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
  return out


def fancy_upsample(p, h, w):
  """p: padded uint8 chroma plane, (h, w) the component's own size -> int32 [2 h, 2 w]"""
  c = p[:h, :w].astype(np.int32)
  up = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
  rows = np.empty((2 * h, w), np.int32)
  rows[0::2] = 3 * c + up[0]
  rows[1::2] = 3 * c + up[1]
  last = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
  nxt = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
  out = np.empty((2 * h, 2 * w), np.int32)
  out[:, 0::2] = (3 * rows + last + 8) >> 4
  out[:, 1::2] = (3 * rows + nxt + 7) >> 4
  return out


def ycc_to_rgb(y, cb, cr):
  y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
  r = y + ((91881 * cr + 32768) >> 16)
  g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  b = y + ((116130 * cb + 32768) >> 16)
  return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(info, pl):
  H, W = info["size"]
  if info["sampling"] == 2:
    ch, cw = -(-H // 2), -(-W // 2)
    cb, cr = (fancy_upsample(p, ch, cw)[:H, :W] for p in pl[1:])
  else:
    cb, cr = pl[1][:H, :W], pl[2][:H, :W]
  return ycc_to_rgb(pl[0][:H, :W], cb, cr)


def decode(data):
  info = parse(data)
  coef, _, _ = entropy_decode(data, info)
  return pixels(info, planes(info, coef))

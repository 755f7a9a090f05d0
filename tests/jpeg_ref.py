"""Baseline JPEG encoder in numpy float64: the definition the device encoder (csrc/jpeg_enc.hip, vp_jpeg_*) is tested against.

Written from ITU T.81 (Annex A: DCT and zig-zag, Annex B: markers, Annex F: entropy coding, Annex K: the example quantisation and
Huffman tables) and the JFIF 1.01 colour equations.  The stream: SOI, APP0, DQT x 2, SOF0 (4:2:0), DHT x 4, DRI (one MCU row), SOS,
entropy-coded intervals separated by RSTn, EOI.

  colour        full-range YCbCr from the uint8 RGB frame, not rounded; chroma = mean of each 2 x 2; level shift 128
  DCT           8 x 8 type II with the JPEG normalisation
  quantisation  Annex K tables scaled by libjpeg's quality rule; quotient rounded to nearest, ties away from zero
  coefficients  int16 [H/16, 6 * W/16, 64]: per MCU row the blocks in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU), each in zig-zag order

Test infrastructure only: nothing under voicepuppet_amd/ imports it.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Table K.1 / K.2 (row-major, not zig-zag)
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# T.81 Tables K.3 - K.6: BITS (codes per length 1..16) and HUFFVAL
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def quant_tables(quality):
  """(luminance [64], chrominance [64]) in row-major order: libjpeg's jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)."""
  quality = int(quality)
  if not 1 <= quality <= 100:
    raise ValueError("quality %d outside 1 .. 100" % quality)
  scale = 5000 // quality if quality < 50 else 200 - 2 * quality
  return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (Q_LUMA, Q_CHROMA))


def huffman_codes(bits, vals):
  """T.81 Annex C: {symbol: (code, length)} of a BITS / HUFFVAL pair."""
  assert sum(bits) == len(vals)
  table, code, k = {}, 0, 0
  for length in range(1, 17):
    for _ in range(bits[length - 1]):
      table[vals[k]] = (code, length)
      code += 1
      k += 1
    code <<= 1
  return table


_DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _blocks(plane):
  """[h, w] -> [h/8, w/8, 8, 8]"""
  h, w = plane.shape
  return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def unquantised(rgb):
  """uint8 [H, W, 3] -> float64 DCT coefficients [H/16, 6 * W/16, 64] in scan order, zig-zag inside a block (before quantisation)."""
  rgb = np.asarray(rgb)
  assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
  H, W = rgb.shape[:2]
  if H % 16 or W % 16:
    raise ValueError("%d x %d: height and width must be multiples of 16" % (H, W))
  r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
  y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
  cb = -0.168736 * r - 0.331264 * g + 0.5 * b
  cr = 0.5 * r - 0.418688 * g - 0.081312 * b
  cb, cr = (c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3)) for c in (cb, cr))
  f = [np.einsum("ux,abxy,vy->abuv", _DCT, _blocks(p), _DCT).reshape(p.shape[0] // 8, p.shape[1] // 8, 64)[..., ZIGZAG] for p in (y, cb, cr)]
  R, M = H // 16, W // 16
  out = np.empty((R, M, 6, 64))
  yb = f[0].reshape(R, 2, M, 2, 64)
  for j in range(4):
    out[:, :, j] = yb[:, j >> 1, :, j & 1]
  out[:, :, 4], out[:, :, 5] = f[1], f[2]
  return out.reshape(R, M * 6, 64)


def quant_steps(quality, mcus):
  """The quantisation step of every position of unquantised()'s last two axes: [6 * mcus, 64]."""
  ql, qc = (t[ZIGZAG] for t in quant_tables(quality))
  return np.tile(np.stack([ql] * 4 + [qc] * 2), (mcus, 1))


def quantise(raw, quality):
  q = raw / quant_steps(quality, raw.shape[1] // 6)
  return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int16)       # nearest, ties away from zero


def coefficients(rgb, quality=75):
  return quantise(unquantised(rgb), quality)


def header(height, width, quality=75):
  ql, qc = quant_tables(quality)
  out = bytearray(b"\xff\xd8")
  out += b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
  for i, t in enumerate((ql, qc)):
    out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in t[ZIGZAG])
  out += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
  for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                            (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
    out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits) + bytes(vals)
  out += b"\xff\xdd\x00\x04" + (width // 16).to_bytes(2, "big")
  out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
  return bytes(out)


def _category(v):
  return int(abs(int(v))).bit_length()


def encode_interval(blocks, tables):
  """One restart interval: int16 [6 * mcus, 64] -> the stuffed, 1-padded bytes (T.81 F.1.2)."""
  (dc_l, ac_l), (dc_c, ac_c) = tables
  acc, nbits = 0, 0
  pred = [0, 0, 0]
  for j, blk in enumerate(blocks.tolist()):
    comp = (0, 0, 0, 0, 1, 2)[j % 6]
    dc_t, ac_t = (dc_l, ac_l) if comp == 0 else (dc_c, ac_c)
    diff = blk[0] - pred[comp]
    pred[comp] = blk[0]
    s = _category(diff)
    code, n = dc_t[s]
    acc, nbits = (acc << n) | code, nbits + n
    if s:
      acc, nbits = (acc << s) | ((diff if diff > 0 else diff - 1) & ((1 << s) - 1)), nbits + s
    run = 0
    for k in range(1, 64):
      v = blk[k]
      if v == 0:
        run += 1
        continue
      while run > 15:
        code, n = ac_t[0xf0]
        acc, nbits = (acc << n) | code, nbits + n
        run -= 16
      s = _category(v)
      code, n = ac_t[(run << 4) | s]
      acc, nbits = (acc << n) | code, nbits + n
      acc, nbits = (acc << s) | ((v if v > 0 else v - 1) & ((1 << s) - 1)), nbits + s
      run = 0
    if run:
      code, n = ac_t[0x00]
      acc, nbits = (acc << n) | code, nbits + n
  pad = -nbits % 8
  acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
  return acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00")


def entropy_encode(coef, height, width, quality=75):
  """int16 coefficients [H/16, 6 * W/16, 64] (coefficients()'s layout, from any source) -> the whole file."""
  coef = np.asarray(coef)
  assert coef.shape == (height // 16, 6 * (width // 16), 64), coef.shape
  tables = ((huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS)),
            (huffman_codes(DC_CHROMA_BITS, DC_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)))
  out = bytearray(header(height, width, quality))
  for i in range(coef.shape[0]):
    if i:
      out += bytes([0xff, 0xd0 + (i - 1) % 8])
    out += encode_interval(coef[i], tables)
  out += b"\xff\xd9"
  return bytes(out)


def encode(rgb, quality=75):
  """uint8 [H, W, 3] -> (int16 coefficients, file bytes)"""
  c = coefficients(rgb, quality)
  return c, entropy_encode(c, rgb.shape[0], rgb.shape[1], quality)


def near_boundary(raw, quality, eps=2.0 ** -8):
  """bool mask: the unquantised value lies within eps of a rounding boundary (k + 1/2) * Q."""
  q = quant_steps(quality, raw.shape[1] // 6)
  t = np.abs(raw) / q
  return np.abs(t - np.floor(t) - 0.5) * q <= eps


def psnr(a, b):
  d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
  return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def parse(data):
  """{'dri': restart interval, 'rst': number of RSTn markers in the scan, 'size': (H, W), 'segments': [(marker, payload)]}"""
  assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
  info = {"dri": None, "segments": []}
  p = 2
  while True:
    assert data[p] == 0xff, p
    m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
    body = data[p + 4:p + 2 + n]
    info["segments"].append((m, body))
    if m == 0xdd:
      info["dri"] = int.from_bytes(body, "big")
    if m == 0xc0:
      info["size"] = (int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"))
    p += 2 + n
    if m == 0xda:
      break
  scan = data[p:-2]
  info["rst"] = [scan[i + 1] - 0xd0 for i in range(len(scan) - 1) if scan[i] == 0xff and 0xd0 <= scan[i + 1] <= 0xd7]
  return info

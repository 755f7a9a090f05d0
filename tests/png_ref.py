"""The PNG files of vp_png_* (include/vp_hip.h, voicepuppet_amd/csrc/png_enc.hip), restated in numpy and plain Python.  This file is the
definition of the byte stream: the kernel follows it, tests/test_gpu_png.py asks for equal bytes.

File: signature, IHDR, IDAT(78 01), one IDAT per strip, IDAT(03 00, Adler-32), IEND.  Bit depth 8, colour type 0 / 2 / 6, no interlace.

Strip: rows_per_strip(width, channels) image rows (the last strip of a frame: what is left), filtered (filter byte + width * channels
bytes per row; the row above a strip's first row is the raw image row above it, zeros above row 0), then one deflate block:

  tokens    A maximal stretch of L equal bytes is one literal followed by its remaining L - 1 bytes cut into pieces of 258; a piece of
            3 .. 258 bytes is a run (a match of that length at distance 1), a last piece of 1 or 2 bytes is literals.  Stretches end at
            the end of the strip.
  codes     literal/length code over the token symbols and end-of-block, limit 15; code-length code over the code lengths sent (no
            repeat symbols 16 - 18), limit 7; one distance code of length 1.  huff_lengths() is the construction, tie-breaks included.
  coded     BFINAL 0, BTYPE 10, HLIT, HDIST = 0, HCLEN, the code-length code's lengths, the lengths of the literal/length symbols
            0 .. last used and of the one distance code, the tokens, end-of-block; then an empty stored block the way zlib's sync
            flush writes it: three zero bits, zero bits up to the byte boundary, 00 00 FF FF.
  stored    when the coded form is not shorter: 00 LEN NLEN, the filtered bytes (a strip is at most 65535 bytes: one block), then
            00 00 00 FF FF.

to_u8 is the float32 rule: (uint8) trunc(x * 255.5f), NaN and negatives 0, 255 from 255 / 255.5 up.
"""
import struct
import zlib

import numpy as np

MAX_ROWS = 16
LDS_BUDGET = 53248        # bytes of a workgroup's LDS for the raw rows (strip + the row above) and the filtered strip
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def rows_per_strip(width, channels):
  """The largest R <= 16 with (2 R + 1) * width * channels + R + 32 <= LDS_BUDGET; 0: the row is too wide for the encoder."""
  wc = width * channels
  return max(0, min(MAX_ROWS, (LDS_BUDGET - 32 - wc) // (2 * wc + 1)))


def to_u8(x):
  v = np.asarray(x, np.float32) * np.float32(255.5)
  with np.errstate(invalid="ignore"):
    out = np.where(v >= 255, 255, np.where(v > 0, v, 0))          # NaN fails both comparisons: 0
  return np.trunc(out).astype(np.uint8)


def _abs_signed_sum(res):
  r = res.astype(np.int64)
  return np.where(r < 128, r, 256 - r).sum(axis=-1)


def filtered_rows(img, filter=-1):
  """uint8 [H, W] or [H, W, C] -> uint8 [H, 1 + W * C]: the filter byte and the residuals of every row."""
  img = np.asarray(img)
  assert img.dtype == np.uint8
  if img.ndim == 2:
    img = img[..., None]
  H, W, C = img.shape
  raw = img.reshape(H, W * C).astype(np.int32)
  up = np.zeros_like(raw)
  up[1:] = raw[:-1]
  left = np.zeros_like(raw)
  left[:, C:] = raw[:, :-C]
  upleft = np.zeros_like(raw)
  upleft[:, C:] = up[:, :-C]
  p = left + up - upleft
  pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
  paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
  res = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - paeth]).astype(np.uint8)      # [5, H, W C], mod 256
  if filter < 0:
    choice = np.argmin(_abs_signed_sum(res), axis=0)               # argmin: the first (lowest) filter on a tie
  else:
    choice = np.full(H, int(filter))
  out = np.empty((H, 1 + W * C), np.uint8)
  out[:, 0] = choice
  out[:, 1:] = res[choice, np.arange(H)]
  return out


def _token_arrays(data):
  """data uint8 [N] -> (pos, run) of the tokens in order: run 0 for a literal of data[pos], else the run's length."""
  d = np.asarray(data, np.uint8)
  N = d.size
  brk = np.ones(N, bool)
  brk[1:] = d[1:] != d[:-1]
  starts = np.flatnonzero(brk)
  s = np.repeat(starts, np.diff(np.append(starts, N)))
  L = np.repeat(np.diff(np.append(starts, N)), np.diff(np.append(starts, N)))
  k = np.arange(N) - s
  j = k - 1
  piece = np.minimum(258, L - 1 - 258 * (j // 258))
  lit = (k == 0) | (piece < 3)
  run = (k > 0) & (piece >= 3) & (j % 258 == 0)
  pos = np.flatnonzero(lit | run)
  return pos, np.where(run[pos], piece[pos], 0)


def strip_tokens(data):
  """The token list of one strip: ('L', byte) and ('R', length)."""
  pos, run = _token_arrays(data)
  d = np.asarray(data, np.uint8)
  return [("R", int(r)) if r else ("L", int(d[p])) for p, r in zip(pos, run)]


def length_symbol(n):
  """run length 3 .. 258 -> (symbol, extra bits, extra value)"""
  n = np.asarray(n, np.int64)
  l = n - 3
  k = np.floor(np.log2(np.maximum(l, 1))).astype(np.int64)
  eb = np.where(l < 8, 0, k - 2)
  sym = np.where(l < 8, 257 + l, 261 + 4 * eb + ((l >> eb) & 3))
  sym = np.where(n == 258, 285, sym)
  eb = np.where(n == 258, 0, eb)
  return sym, eb, l & ((1 << eb) - 1)


def huff_lengths(freq, limit):
  """Code lengths of a length-limited Huffman code.

  1. The used symbols (freq > 0) are sorted by (freq, symbol), ascending.
  2. Huffman's algorithm with two queues: the sorted leaves and the internal nodes in the order they are made.  Each pick takes the
     leaf when there is one and either no internal node is waiting or the leaf's weight is <= that node's.
  3. count[d] = leaves at depth d, depths beyond `limit` counted at `limit`.
  4. While sum(count[d] << (limit - d)) exceeds 1 << limit: count[limit] -= 1; the largest d < limit with count[d] > 0 gives one
     leaf to d + 1 and takes one with it (count[d] -= 1, count[d + 1] += 2); the sum falls by one.
  5. The lengths are handed out along the sorted order: the first count[limit] symbols get `limit`, the next count[limit - 1] get
     limit - 1, and so on.
  One used symbol gets length 1."""
  used = sorted((int(f), s) for s, f in enumerate(freq) if f > 0)
  n = len(used)
  lens = [0] * len(freq)
  if n == 0:
    return lens
  if n == 1:
    lens[used[0][1]] = 1
    return lens
  w = [f for f, _ in used] + [0] * (n - 1)
  parent = [0] * (2 * n - 1)
  a, b = 0, n
  for node in range(n, 2 * n - 1):
    for _ in range(2):
      if a < n and (b >= node or w[a] <= w[b]):
        pick, a = a, a + 1
      else:
        pick, b = b, b + 1
      parent[pick] = node
      w[node] += w[pick]
  count = [0] * (limit + 1)
  for j in range(n):
    d, x = 0, j
    while x != 2 * n - 2:
      x, d = parent[x], d + 1
    count[min(d, limit)] += 1
  total = sum(count[d] << (limit - d) for d in range(1, limit + 1))
  while total > (1 << limit):
    count[limit] -= 1
    for d in range(limit - 1, 0, -1):
      if count[d]:
        count[d] -= 1
        count[d + 1] += 2
        break
    total -= 1
  j = 0
  for d in range(limit, 0, -1):
    for _ in range(count[d]):
      lens[used[j][1]] = d
      j += 1
  return lens


def canonical_codes(lens):
  """RFC 1951 3.2.2 -> the codes, bit-reversed (deflate sends Huffman codes from their most significant bit)."""
  maxl = max(lens) if len(lens) else 0
  count = [0] * (maxl + 2)
  for l in lens:
    if l:
      count[l] += 1
  nxt, code = [0] * (maxl + 2), 0
  for l in range(1, maxl + 1):
    code = (code + count[l - 1]) << 1
    nxt[l] = code
  out = [0] * len(lens)
  for s, l in enumerate(lens):
    if l:
      out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
      nxt[l] += 1
  return out


def _pack(vals, nbits):
  """LSB-first bit packing of (value, bit count) pairs -> (bytes zero-padded to a byte, bit length)."""
  vals, nbits = np.asarray(vals, np.uint64), np.asarray(nbits, np.int64)
  total = int(nbits.sum())
  idx = np.repeat(np.arange(vals.size), nbits)
  k = np.arange(total) - np.repeat(np.cumsum(nbits) - nbits, nbits)
  bits = ((vals[idx] >> k.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
  return np.packbits(bits, bitorder="little").tobytes(), total


def strip_deflate(data):
  """The filtered bytes of one strip -> (deflate bytes, stored flag)."""
  d = np.asarray(data, np.uint8).ravel()
  N = d.size
  assert 0 < N <= 65535
  stored = b"\x00" + struct.pack("<HH", N, N ^ 0xFFFF) + d.tobytes() + b"\x00\x00\x00\xff\xff"
  pos, run = _token_arrays(d)
  is_run = run > 0
  rsym, reb, rval = length_symbol(np.where(is_run, run, 3))
  sym = np.where(is_run, rsym, d[pos])
  freq = np.bincount(sym, minlength=286)
  freq[256] += 1
  ll_len = huff_lengths(freq.tolist(), 15)
  ll_code = canonical_codes(ll_len)
  n_ll = max(s for s in range(286) if ll_len[s]) + 1
  sent = ll_len[:n_ll] + [1]                                         # and the one distance code
  cl_freq = np.bincount(np.array(sent), minlength=19)
  cl_len = huff_lengths(cl_freq.tolist(), 7)
  cl_code = canonical_codes(cl_len)
  n_cl = max(4, max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1)
  vals = [0, 2, n_ll - 257, 0, n_cl - 4] + [cl_len[CL_ORDER[i]] for i in range(n_cl)] + [cl_code[l] for l in sent]
  nbits = [1, 2, 5, 5, 4] + [3] * n_cl + [cl_len[l] for l in sent]
  lens_a, codes_a = np.array(ll_len, np.int64), np.array(ll_code, np.int64)
  eb = np.where(is_run, reb, 0)
  tv = codes_a[sym] | (np.where(is_run, rval, 0) << lens_a[sym])      # the distance code (one 0 bit) sits above the extra bits
  tn = lens_a[sym] + eb + is_run
  vals = np.concatenate([np.array(vals, np.int64), tv, [ll_code[256], 0]])
  nbits = np.concatenate([np.array(nbits, np.int64), tn, [ll_len[256], 3]])
  body, _ = _pack(vals, nbits)
  coded = body + b"\x00\x00\xff\xff"
  return (coded, False) if len(coded) < len(stored) else (stored, True)


def chunk(kind, data):
  return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def adler32_combine(a1, b1, a2, b2, len2):
  return (a1 + a2 - 1) % 65521, (b1 + b2 + len2 * (a1 - 1)) % 65521


def adler32_pair(data):
  d = np.asarray(data, np.uint8).astype(np.int64).ravel()
  n = d.size
  return int(1 + d.sum()) % 65521, int(n + (d * (n - np.arange(n))).sum()) % 65521


def header(height, width, channels):
  return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, COLOUR_TYPE[channels], 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")


def encode_strips(img, filter=-1, rows_per_strip_=None):
  """-> (file bytes, [(chunk length, stored flag)] per strip)"""
  img = np.asarray(img)
  if img.ndim == 2:
    img = img[..., None]
  H, W, C = img.shape
  R = rows_per_strip_ or rows_per_strip(W, C)
  assert R >= 1
  rows = filtered_rows(img, filter)
  out, info = [header(H, W, C)], []
  a, b = 1, 0
  for y in range(0, H, R):
    part = rows[y:y + R].ravel()
    body, stored = strip_deflate(part)
    out.append(chunk(b"IDAT", body))
    info.append((12 + len(body), stored))
    a2, b2 = adler32_pair(part)
    a, b = adler32_combine(a, b, a2, b2, part.size)
  out.append(chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", (b << 16) | a)))
  out.append(chunk(b"IEND", b""))
  return b"".join(out), info


def encode(img_u8, filter=-1, rows_per_strip=None):
  return encode_strips(img_u8, filter, rows_per_strip)[0]


def frame_capacity(height, width, channels):
  """The largest file of these dimensions: every strip stored."""
  R = rows_per_strip(width, channels)
  row = 1 + width * channels
  n = 47 + 18 + 12
  for y in range(0, height, R):
    n += 12 + min(R, height - y) * row + 10
  return n


def parse_chunks(data):
  """-> [(kind, payload, crc)] after checking the signature; raises on a malformed file."""
  assert data[:8] == SIGNATURE
  at, out = 8, []
  while at < len(data):
    n, = struct.unpack(">I", data[at:at + 4])
    kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
    crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
    out.append((kind, payload, crc))
    at += 12 + n
  assert at == len(data)
  return out

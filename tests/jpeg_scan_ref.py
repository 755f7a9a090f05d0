"""The device index scan (csrc/jpeg_dec.hip: jpegdec_scan_kernel, vp_jpegdec_enable_scan) restated in plain Python: the same chunking, cold
start, void and drop-one-bit rules, rounds, counts and prefix sums, so that its entries, its verdict and its round count can be compared
with the device's int for int, and its entries with the serial decode of tests/jpeg_dec_ref.py.

A decoder state is (byte, bit, j, k): the file position of the next symbol in the form BitReader::where() gives it (the byte is never the
stuffed 0x00 of an 0xff 0x00 pair), the block-in-MCU and the zig-zag position (0: a DC symbol comes next).

  scan(data, chunk_bytes, max_rounds, lanes) -> Scan: ok, rounds, entries {row: (byte, bit, preds)} in jpeg_dec_ref's form, entries_int
                                                int32 [mcuy, 4] in the device's, and what the walk met (cold starts on a stuffed byte,
                                                long codes across a chunk end)
  oracle_by_rows(data, info)                  -> (coefficients, entries) of jpeg_dec_ref.decode_segment run row by row, each row from the
                                                entry the row before recorded: the serial decode at a cost linear in the file

Test infrastructure only: nothing under voicepuppet_amd/ imports it.
"""
import bisect

import numpy as np

import jpeg_dec_ref as dr

SCAN_LANES = 1024        # kScanLanes: chunks per sweep


class _Stream:
  """The file as every BitReader sees it: the data bytes (all but stuffed zeros), their file offsets, and the markers a reader stops at."""

  def __init__(self, data):
    a = np.frombuffer(data, np.uint8)
    n = len(a)
    stuffed = np.zeros(n, bool)
    stuffed[1:] = (a[1:] == 0) & (a[:-1] == 0xff)
    self.n = n
    self.raw_of = np.flatnonzero(~stuffed).tolist() + [n]                       # data byte number -> file offset
    self.count = np.concatenate([[0], np.cumsum(~stuffed)]).tolist()             # file offset -> data bytes in front of it
    self.ds = a[~stuffed].tobytes() + bytes(8)
    nxt = np.concatenate([a[1:], [1]])
    self.markers = np.flatnonzero((a == 0xff) & (nxt != 0)).tolist() + [n]      # an 0xff a reader does not pass (or the end)
    self.stuffed = stuffed

  def limit(self, byte):
    """data bits in front of the first marker at or behind `byte`"""
    return 8 * self.count[self.markers[bisect.bisect_left(self.markers, min(byte, self.n))]]

  def bits(self, at, n, limit):
    """n <= 16 bits from data bit `at`, zeros from `limit` on"""
    if at >= limit:
      return 0
    w = int.from_bytes(self.ds[at >> 3:(at >> 3) + 4], "big")
    v = (w >> (32 - n - (at & 7))) & ((1 << n) - 1)
    over = at + n - limit
    return v >> over << over if over > 0 else v

  def where(self, at, limit):
    return (self.raw_of[limit >> 3], 0) if at >= limit else (self.raw_of[at >> 3], at & 7)


def _lookup(bits, vals):
  """the next 16 bits -> (length << 8) | symbol, 0 where no code starts them"""
  t = [0] * 65536
  code, k = 0, 0
  for length in range(1, 17):
    for _ in range(bits[length - 1]):
      lo = code << (16 - length)
      t[lo:lo + (1 << (16 - length))] = [(length << 8) | vals[k]] * (1 << (16 - length))
      code += 1
      k += 1
    code <<= 1
  return t


def _extend(v, s):
  return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


class Scan:
  pass


class _Walker:
  def __init__(self, data, info):
    self.s = _Stream(data)
    self.info = info
    self.bpm = info["bpm"]
    self.comp_of = (0, 0, 0, 0, 1, 2) if self.bpm == 6 else (0, 1, 2)
    look = {k: _lookup(*v) for k, v in info["huff"].items()}
    self.dc = [look[(0, info["tables"][c][1])] for c in range(3)]
    self.ac = [look[(1, info["tables"][c][2])] for c in range(3)]
    self.memo = {}

  def walk(self, state, chunk_end):
    """decode(chunk, state) -> (exit state, [(byte, bit, j, component, DC difference) of every block that starts], the drop-one-bit rule
    was used, a code longer than 9 bits lies across chunk_end)"""
    key = (state, chunk_end)
    if key in self.memo:
      return self.memo[key]
    s, bpm = self.s, self.bpm
    byte, bit, j, k = state
    byte = min(byte, s.n)
    limit = s.limit(byte)
    at = 8 * s.count[byte] + bit
    blocks, err, straddle = [], False, False
    while True:
      here = s.where(at, limit)
      if here[0] >= chunk_end:
        break
      c = self.comp_of[j]
      e = (self.dc if k == 0 else self.ac)[c][s.bits(at, 16, limit)]
      bad = e == 0
      nxt, sym = at, 0
      if not bad:
        nxt, sym = at + (e >> 8), e & 255
        if k == 0:
          if sym > 15:
            bad = True
          else:
            diff = _extend(s.bits(nxt, sym, limit), sym)
            nxt += sym
        elif sym & 15:
          nxt += sym & 15
      if nxt > limit or (e == 0 and at + 16 > limit):       # void: the walk ends in front of this symbol
        break
      if not bad:
        if (e >> 8) > dr.LOOKUP_BITS and s.where(at + (e >> 8) - 1, limit)[0] >= chunk_end:
          straddle = True
        if k == 0:
          blocks.append((here[0], here[1], j, c, diff))
          k = 1
        elif sym & 15 == 0:
          if sym >> 4 == 15:
            k += 16
            bad = k > 64
          else:
            k = 64
        else:
          k += sym >> 4
          if k > 63:
            bad = True
          else:
            k += 1
      if bad:
        err = True
        at += 1
        k = 0
      else:
        at = nxt
        if k >= 64:
          k = 0
          j = 0 if j + 1 == bpm else j + 1
    out = (here + (j, k), blocks, err, straddle)
    self.memo[key] = out
    return out


def scan(data, chunk_bytes, max_rounds=1 << 30, lanes=SCAN_LANES, info=None):
  data = bytes(data)
  info = info or dr.parse(data)
  w = _Walker(data, info)
  start, n = info["scan"], len(data)
  bpm, mcux, mcuy = info["bpm"], info["mcux"], info["mcuy"]
  nchunks = -(-(n - start) // chunk_bytes)
  exit_ = [None] * nchunks
  r = Scan()
  r.chunks, r.sweeps, r.rounds, r.ok = nchunks, -(-nchunks // lanes), 0, True
  r.cold_on_stuffed = r.straddles = 0
  r.entries, failed = {}, False
  carry = [0, 0, 0, 0]                      # block index and predictors at the sweep's first chunk
  for base in range(0, nchunks, lanes):
    chunks = range(base, min(base + lanes, nchunks))
    end = {i: min(start + (i + 1) * chunk_bytes, n) for i in chunks}
    ins = {}
    for i in chunks:                        # cold pass
      if i == base:
        ins[i] = (start, 0, 0, 0) if base == 0 else exit_[i - 1]
      else:
        first = start + i * chunk_bytes
        on_stuffed = data[first] == 0 and data[first - 1] == 0xff
        r.cold_on_stuffed += on_stuffed
        ins[i] = (first + on_stuffed, 0, 0, 0)
      exit_[i] = w.walk(ins[i], end[i])[0]
    rounds = 0
    while True:                             # every lane reads its neighbour's state of the round before
      rounds += 1
      ins.update({i: exit_[i - 1] for i in chunks if i > base})
      new = {i: w.walk(ins[i], end[i])[0] for i in chunks if i > base}
      changed = any(new[i] != exit_[i] for i in new)
      for i in new:
        exit_[i] = new[i]
      if not changed or rounds >= max_rounds:
        break
    r.rounds = max(r.rounds, rounds)
    if changed:
      r.ok = False
      break
    at = list(carry)
    for i in chunks:                        # count, prefix sum and entries in one go: `at` is the running sum
      _, blocks, err, straddle = w.walk(ins[i], end[i])
      failed |= err
      r.straddles += straddle
      for byte, bit, j, c, diff in blocks:
        mcu = at[0] // bpm
        if at[0] - mcu * bpm != j:
          failed = True
        elif j == 0 and mcu % mcux == 0 and mcu // mcux < mcuy:
          r.entries[mcu // mcux] = (byte, bit, tuple(dr._wrap16(v) for v in at[1:]))
        at[0] += 1
        at[1 + c] += diff
    carry = at
  r.blocks = carry[0]
  r.ok = bool(r.ok and not failed and carry[0] == mcux * mcuy * bpm)
  r.entries_int = entries_int(r.entries, mcuy)
  return r


def entries_int(entries, mcuy):
  """{row: (byte, bit, preds)} -> int32 [mcuy, 4] as the device stores them (rows never met stay zero)"""
  out = np.zeros((mcuy, 4), np.int64)
  for row, (byte, bit, p) in entries.items():
    out[row] = (byte, bit, (p[0] & 0xffff) | ((p[1] & 0xffff) << 16), p[2] & 0xffff)
  return out.astype(np.uint32).view(np.int32)


def oracle_by_rows(data, info=None):
  """jpeg_dec_ref.decode_segment MCU row by MCU row: row r is decoded from the entry the decode of row r - 1 recorded when it went one
  MCU on, on the file cut a little behind (decode_segment's cost grows with the square of what it is given).  -> (int16 [blocks, 64],
  entries): what entropy_decode returns, by induction over the rows."""
  data = bytes(data)
  info = info or dr.parse(data)
  mcux, mcuy, bpm = info["mcux"], info["mcuy"], info["bpm"]
  total = mcux * mcuy
  out = np.zeros((total * bpm, 64), np.int16)
  entries = {}
  seg = (info["scan"], 0, (0, 0, 0))
  span = max(4096, 4 * (len(data) - info["scan"]) // mcuy)
  for row in range(mcuy):
    count = min(mcux + 1, total - row * mcux)            # one MCU into the next row: its entry is recorded
    cut = span
    while True:
      got = {}
      try:
        dr.decode_segment(data[:seg[0] + cut], info, seg + (row * mcux, count), out, got)
        break
      except dr.Corrupt:
        if seg[0] + cut >= len(data):
          raise
        cut *= 2
    entries[row] = got[row]
    if row + 1 < mcuy:
      seg = got[row + 1]
  return out, entries

"""JPEG decoding of training frames on the device (libvp_hip.so: vp_jpegdec_*, csrc/jpeg_dec.hip).

What the reference does per sample on the host (generator/generator.py:956-1019: two cv2.imread calls; loader.py: ImageLoader): here the
host only parses headers.  parse() accepts baseline 4:2:0 / 4:4:4 files (include/vp_hip.h; on request also 4:2:2 files and files
that leave their Huffman tables to T.81 Annex K.3, as Motion-JPEG frames do) and gives a refusal reason for the rest, finds the
restart markers with one numpy scan and packs the meta blob the kernels read.  JpegDecoder packs the metas and files of a batch into
one pinned buffer, copies it once and enqueues the decode; it never waits in decode_into.

Segments.  A file with restart markers is decoded one lane per interval, a file without them by one lane - and every decode records, per
MCU row, where the lane stood (`entries`).  Those records are the file's entry-point index: pure data, kept in a cache keyed by (path,
size, mtime); the next decode of the file runs one lane per MCU row.  save_index / load_index keep the cache in one .npz.

Index scan (JpegDecoder(scan_chunk_bytes=N), off by default).  The first decode of a file without restart markers then finds the entry
points on the device, in the same call and in front of the entropy kernel (vp_jpegdec_enable_scan, include/vp_hip.h): one workgroup per
file decodes chunks of N file bytes from guessed states and repeats "chunk i from the exit of chunk i - 1" until nothing changes.  A
file whose scan held is decoded one lane per MCU row at first sight; one whose scan did not hold (rounds exhausted, damaged data) by one
lane as before.  The entries recorded are the same either way, so the cache and the .npz are filled as before.
"""
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr, stream

LOOKUP_BITS = 9
META_BYTES = _lib.JPEGDEC_META_BYTES
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_SOF_OTHER = {0xc1: "extended sequential", 0xc2: "progressive", 0xc3: "lossless", 0xc5: "differential", 0xc6: "differential progressive",
              0xc7: "differential lossless", 0xc9: "arithmetic", 0xca: "arithmetic progressive", 0xcb: "arithmetic lossless",
              0xcd: "arithmetic differential", 0xce: "arithmetic differential progressive", 0xcf: "arithmetic differential lossless"}

# ITU T.81 Annex K.3: the BITS / HUFFVAL pairs a frame without DHT segments implies (Motion-JPEG in AVI), by (class, id): DC / AC,
# luminance / chrominance.  tests/test_jpeg_dec_422_host.py pins them to the DHT bodies PIL writes.
_K3_DC_VALS = bytes(range(12))
K3_HUFFMAN = {
    (0, 0): (bytes.fromhex("00010501010101010100000000000000"), _K3_DC_VALS),
    (0, 1): (bytes.fromhex("00030101010101010101010000000000"), _K3_DC_VALS),
    (1, 0): (bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex(
        "01020300041105122131410613516107227114328191a108" "2342b1c11552d1f02433627282090a161718191a25262728"
        "292a3435363738393a434445464748494a53545556575859" "5a636465666768696a737475767778797a83848586878889"
        "8a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6" "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2"
        "e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (1, 1): (bytes.fromhex("00020102040403040705040400010277"), bytes.fromhex(
        "000102031104052131061241510761711322328108144291" "a1b1c109233352f0156272d10a162434e125f11718191a26"
        "2728292a35363738393a434445464748494a535455565758" "595a636465666768696a737475767778797a828384858687"
        "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4" "b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9da"
        "e2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
}


class JpegInfo:
  """parse()'s result.  refused: None, or why the device decoder does not take the file (the other fields are then unset)."""
  refused = None

  def __init__(self, **kw):
    self.__dict__.update(kw)


@functools.lru_cache(maxsize=256)
def _huff_table(bits, vals):
  """BITS / HUFFVAL (bytes) -> the 1424 bytes of include/vp_hip.h's look-up form, or None for an impossible table.  Cached: the files of
  a dataset share a handful of tables, and building one is the costly part of parsing a header."""
  if sum(bits) > 256 or sum(bits) != len(vals):
    return None
  lut = np.zeros(512, np.uint16)
  maxcode = np.full(18, -1, np.int32)
  valoff = np.zeros(18, np.int32)
  v = np.zeros(256, np.uint8)
  v[:len(vals)] = np.frombuffer(vals, np.uint8)
  code, k = 0, 0
  for length in range(1, 17):
    n = bits[length - 1]
    if n:
      if code + n > 1 << length:
        return None
      valoff[length] = k - code
      maxcode[length] = code + n - 1
      if length <= LOOKUP_BITS:
        for i in range(n):
          lo = (code + i) << (LOOKUP_BITS - length)
          lut[lo:lo + (1 << (LOOKUP_BITS - length))] = (length << 8) | vals[k + i]
      code += n
      k += n
    code <<= 1
  return lut.tobytes() + maxcode.tobytes() + valoff.tobytes() + v.tobytes()


def parse(data, max_height=None, max_width=None, accept_422=False, default_huffman=False):
  """bytes of a .jpg -> JpegInfo: height, width, sampling (2: 4:2:0, 1: 4:4:4, 3: 4:2:2), mcux, mcuy, dri, scan (offset of the
  entropy-coded data), rst (offsets of the RSTn markers), tq / td / ta per component, segments int32 [n, 6] (one per restart interval,
  else one), tables (the quantisation and Huffman part of the meta blob).  .refused names the reason for a file outside the subset.
  accept_422: a (2x1, 1x1, 1x1) file is taken as sampling 3 (an MCU of 16 x 8 pixels) instead of refused.  default_huffman: a Huffman
  table the scan uses and the file does not define is the one of T.81 Annex K.3 (K3_HUFFMAN), as for the frames of a Motion-JPEG
  stream; a table the file defines always wins."""
  def no(why):
    r = JpegInfo()
    r.refused = why
    return r
  data = bytes(data)
  if data[:2] != b"\xff\xd8":
    return no("not a JPEG file (no SOI)")
  quant, huff, dri, sof, p = {}, {}, 0, None, 2
  while True:
    if p + 4 > len(data):
      return no("truncated header")
    if data[p] != 0xff:
      return no("no marker at byte %d" % p)
    m = data[p + 1]
    if m == 0xff:
      p += 1
      continue
    n = int.from_bytes(data[p + 2:p + 4], "big")
    if n < 2 or p + 2 + n > len(data):
      return no("truncated header")
    body = data[p + 4:p + 2 + n]
    if m in _SOF_OTHER:
      return no("%s (SOF%d): only baseline sequential Huffman files" % (_SOF_OTHER[m], m - 0xc0))
    if m == 0xdb:
      q = 0
      while q < len(body):
        if body[q] >> 4:
          return no("16-bit quantisation table")
        if (body[q] & 15) > 3 or q + 65 > len(body):
          return no("bad DQT segment")
        t = np.zeros(64, np.uint16)
        t[_ZIGZAG] = np.frombuffer(body[q + 1:q + 65], np.uint8)
        quant[body[q] & 15] = t
        q += 65
    elif m == 0xc4:
      q = 0
      while q < len(body):
        if q + 17 > len(body):
          return no("bad DHT segment")
        tc, th, bits = body[q] >> 4, body[q] & 15, bytes(body[q + 1:q + 17])
        vals = bytes(body[q + 17:q + 17 + sum(bits)])
        if tc > 1 or th > 1:
          return no("Huffman table %d / %d: baseline has two DC and two AC tables" % (tc, th))
        t = _huff_table(bits, vals)
        if t is None:
          return no("bad DHT segment")
        huff[(tc, th)] = t
        q += 17 + sum(bits)
    elif m == 0xc0:
      if len(body) < 6:
        return no("truncated header")
      if body[0] != 8:
        return no("%d-bit samples" % body[0])
      if body[5] != 3:
        return no("%d components (grey or CMYK): only three" % body[5])
      if len(body) < 15:
        return no("truncated header")
      comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)]
      samp = [(h, v) for _, h, v, _ in comps]
      if samp not in ([(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]) and not (accept_422 and samp == [(2, 1), (1, 1), (1, 1)]):
        return no("sampling %s: only 4:2:0 and 4:4:4" % "".join("%dx%d " % s for s in samp).strip())
      sof = (int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), 3 if samp[0] == (2, 1) else samp[0][0], comps)
    elif m == 0xdd:
      dri = int.from_bytes(body[:2], "big")
    elif m == 0xda:
      if sof is None:
        return no("SOS before SOF0")
      if len(body) < 1:
        return no("truncated header")
      if body[0] != 3 or len(body) < 10:
        return no("a scan of %d components: only one interleaved scan" % body[0])
      if tuple(body[7:10]) != (0, 63, 0):
        return no("not a sequential scan")
      sel = {body[1 + 2 * i]: (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(3)}
      p += 2 + n
      break
    p += 2 + n
  H, W, s, comps = sof
  if H < 1 or W < 1:
    return no("empty image")
  if (max_height is not None and H > max_height) or (max_width is not None and W > max_width):
    return no("oversize: %d x %d, up to %d x %d" % (W, H, max_width, max_height))
  try:
    tq, td, ta = [c[3] for c in comps], [sel[c[0]][0] for c in comps], [sel[c[0]][1] for c in comps]
  except KeyError:
    return no("the scan names a component the frame does not have")
  if default_huffman:
    for k in [(0, t) for t in td] + [(1, t) for t in ta]:
      if k not in huff and k in K3_HUFFMAN:
        huff[k] = _huff_table(*K3_HUFFMAN[k])
  if any(t not in quant for t in tq) or any((0, t) not in huff for t in td) or any((1, t) not in huff for t in ta):
    return no("a table the scan uses is missing")
  # restart markers: in entropy-coded data 0xff is followed only by 0x00 or RSTn; the first other follower ends the scan
  a = np.frombuffer(data, np.uint8)[p:]
  ff = np.flatnonzero(a[:-1] == 0xff)
  nxt = a[ff + 1]
  is_rst = (nxt & 0xf8) == 0xd0
  other = np.flatnonzero((nxt != 0) & ~is_rst)
  if other.size:
    ff, is_rst = ff[:other[0]], is_rst[:other[0]]
  rst = (ff[is_rst] + p).astype(np.int64)
  mcux, mcuy = -(-W // (8 if s == 1 else 16)), -(-H // (16 if s == 2 else 8))
  total = mcux * mcuy
  if dri:
    nseg = -(-total // dri)
    if len(rst) + 1 < nseg:           # a scan cut short or damaged: no lane would own the MCUs behind the last marker found
      return no("restart markers missing: %d found, %d intervals" % (len(rst), nseg))
    seg = np.zeros((nseg, 6), np.int32)
    seg[0, 0] = p
    seg[1:, 0] = rst[:nseg - 1] + 2
    seg[:, 4] = np.arange(nseg) * dri
    seg[:, 5] = np.minimum(dri, total - seg[:, 4])
  else:
    seg = np.array([[p, 0, 0, 0, 0, total]], np.int32)
  zero = bytes(1424)
  tables = b"".join(quant.get(i, np.zeros(64, np.uint16)).tobytes() for i in range(4)) + b"".join(huff.get(k, zero) for k in ((0, 0), (0, 1), (1, 0), (1, 1)))
  return JpegInfo(height=H, width=W, sampling=s, mcux=mcux, mcuy=mcuy, dri=dri, scan=p, rst=rst, tq=tq, td=td, ta=ta, segments=seg, tables=tables,
                  bytes=len(data))


def index_segments(info, entries):
  """entries int32 [mcuy, 4] (a decode's record of the file) -> the segment table of one lane per MCU row"""
  seg = np.zeros((info.mcuy, 6), np.int32)
  seg[:, :4] = entries[:info.mcuy]
  seg[:, 4] = np.arange(info.mcuy) * info.mcux
  seg[:, 5] = info.mcux
  return seg


def meta_blob(info, segments=None):
  seg = info.segments if segments is None else segments
  head = np.zeros(32, np.int32)
  head[:8] = (1, info.width, info.height, info.sampling, info.mcux, info.mcuy, info.dri, len(seg))
  return head.tobytes() + info.tables + np.ascontiguousarray(seg, np.int32).tobytes()


def _key(path):
  st = os.stat(path)
  return (os.path.abspath(path), st.st_size, st.st_mtime_ns)


class JpegDecoder(Handle):
  """decode(files) -> (uint8 [n, max_height, max_width, 3] device, status int32 [n] device), files being bytes or paths.  A path's decode
  feeds the index cache and uses it from its second decode on.  last_segments: the segment count of every file of the last call.  It is
  a read-only property and, with the index scan enabled, a lazy one: the count of a scanned file (its MCU rows, or 1) is the device's
  verdict, so reading it waits for that call's event, and it speaks of whatever call is the last when it is read.  Without the scan
  it is the list the host packed, as before.  Nothing on the training path reads it.
  scan_chunk_bytes: None, or the chunk size of the device index scan (a power of two, 32 .. 4096; 128 suits training triptychs);
  scan_max_rounds bounds its fixed-point rounds per sweep.  The default is 512, not the 32 first pencilled in: files of dense noise
  synchronise slowly (tests/test_jpeg_scan_host.py counts up to 209 rounds at 32-byte chunks, profiles/jpeg_scan.json), and a lane
  whose input did not change does not decode again, so late rounds cost little.  last_scan_rounds: the rounds per file of the last
  harvested call (0: not scanned).
  accept_422 / default_huffman: parse()'s flags for the files items() reads: 4:2:2 files and files without their Huffman tables are
  taken, not refused.  Both off by default."""

  RING = 3          # staging buffers: one stays untouched until two calls later (the prefetcher's contract for pinned memory)

  def __init__(self, max_files, max_height, max_width, bgr=True, max_file_bytes=1 << 22, max_segments_per_file=1 << 16,
               scan_chunk_bytes=None, scan_max_rounds=512, accept_422=False, default_huffman=False):
    if not torch.cuda.is_available():
      raise RuntimeError("JpegDecoder needs an MI355X (no CPU fallback)")
    desc = _lib.JpegDecDesc(ctypes.sizeof(_lib.JpegDecDesc), int(max_files), int(max_height), int(max_width), int(max_file_bytes),
                            int(max_segments_per_file), int(bool(bgr)))
    self._open("jpegdec", desc, invalid="invalid JPEG decoder descriptor")
    self.max_files, self.max_height, self.max_width, self.bgr = int(max_files), int(max_height), int(max_width), bool(bgr)
    self.accept_422, self.default_huffman = bool(accept_422), bool(default_huffman)
    self.scan_chunk_bytes, self.scan_max_rounds, self.scan_workspace = None, None, None
    if scan_chunk_bytes is not None:
      sws = self.L.vp_jpegdec_scan_workspace_bytes(ctypes.byref(self.desc), int(scan_chunk_bytes))
      if sws == 0:
        raise ValueError("invalid JPEG index scan setting: " + self.L.vp_last_error().decode())
      self.scan_workspace = torch.empty(sws, dtype=torch.uint8, device="cuda")
      _lib.check(self.L.vp_jpegdec_enable_scan(self.h, ptr(self.scan_workspace), sws, int(scan_chunk_bytes), int(scan_max_rounds)),
                 "vp_jpegdec_enable_scan")
      self.scan_chunk_bytes, self.scan_max_rounds = int(scan_chunk_bytes), int(scan_max_rounds)
    self.index = {}                 # (path, size, mtime_ns) -> int32 [mcuy, 4]
    self.last_scan_rounds = []
    self._last = ([], None)         # the last call's segment counts as packed, and (event, pinned scan_ok, MCU rows) with the scan
    self._ring = [None] * self.RING
    self._turn = 0
    self._pending = [None] * self.RING

  # ---- the index ----
  def save_index(self, path):
    self.harvest()
    keys = sorted(self.index)
    np.savez(path, paths=np.array([k[0] for k in keys], dtype=str), sizes=np.array([k[1] for k in keys], np.int64),
             mtimes=np.array([k[2] for k in keys], np.int64), rows=np.array([len(self.index[k]) for k in keys], np.int64),
             entries=np.concatenate([self.index[k] for k in keys]).astype(np.int32) if keys else np.zeros((0, 4), np.int32))

  def load_index(self, path):
    z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
    at = 0
    for p, s, m, r in zip(z["paths"], z["sizes"], z["mtimes"], z["rows"]):
      self.index[(str(p), int(s), int(m))] = z["entries"][at:at + int(r)].copy()
      at += int(r)

  @property
  def last_segments(self):
    segs, scan = self._last
    if scan is None:
      return segs
    event, ok, rows = scan
    event.synchronize()
    return [rows[i] if ok[i] else s for i, s in enumerate(segs)]

  def harvest(self, slot=None):
    """Reads the status and entries earlier decode_into calls left in pinned memory (of staging slot `slot`, or of all: waits for their
    events, long completed when a slot is refilled) -> the names of the files whose status was not 0.  Their entries are dropped, the
    others fill the index cache."""
    bad = []
    for k in (range(self.RING) if slot is None else [slot]):
      if self._pending[k] is None:
        continue
      event, status, entries, keys, rows, names, scan_rounds = self._pending[k]
      self._pending[k] = None
      event.synchronize()
      if scan_rounds is not None:
        self.last_scan_rounds = scan_rounds.numpy()[:len(keys)].tolist()
      st, en = status.numpy(), entries.numpy()
      for i, key in enumerate(keys):
        if names[i] is None:
          continue
        if st[i] != 0:
          bad.append(names[i])
        elif key is not None and key not in self.index:
          self.index[key] = en[i, :rows[i]].copy()
    return bad

  # ---- decoding ----
  def tensor(self, name):
    """'coefficients' int16 [max_files, blocks, 64], 'entries' int32 [max_files, rows, 4], 'planes' uint8 [max_files, 3, Hp, Wp]: views of
    the workspace, rows in the order of the last decode (chroma of a 4:2:0 file fills the top left quarter of its plane, chroma of a
    4:2:2 file the left half).  With the index scan 'scan_ok' and 'scan_rounds', int32 [max_files]."""
    if name in ("scan_ok", "scan_rounds"):          # the index scan's buffers lie in its own workspace
      return self._tensor(name, torch.int32, 1, self.scan_workspace)
    dtype = {"coefficients": torch.int16, "entries": torch.int32, "planes": torch.uint8}[name]
    return self._tensor(name, dtype, 4 if name == "planes" else 3)

  def _staging(self, slot, nbytes, keep=0):
    """The staging buffers of `slot`, grown to nbytes (the first `keep` bytes of the pinned one are carried over)."""
    ring = self._ring[slot]
    if ring is None or ring[0].numel() < nbytes:
      cap = max(nbytes, 1 << 16) * 3 // 2
      new = (torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device="cuda"),
             torch.empty(self.max_files, dtype=torch.int32).pin_memory(),
             torch.empty(self.tensor("entries").shape, dtype=torch.int32).pin_memory(),
             torch.empty(2, self.max_files, dtype=torch.int32).pin_memory())          # scan_ok, scan_rounds
      if keep:
        new[0].numpy()[:keep] = ring[0].numpy()[:keep]
      self._ring[slot] = ring = new
    return ring

  def stage(self, nbytes):
    """For a caller whose files lie in one span of a larger file (the chunks of an AVI clip): takes the next staging slot and returns
    (token, uint8 numpy view of its first nbytes of pinned memory).  The caller reads the span into the view, parses its files from it
    and hands pack() the token with items whose data is (offset in the span, length): the files then travel where they were read."""
    slot = self._turn
    self._turn = (self._turn + 1) % self.RING
    bad = self.harvest(slot)
    ring = self._staging(slot, int(nbytes) + 16)
    return (slot, int(nbytes), bad), ring[0].numpy()[:int(nbytes)]

  def pack(self, items, staged=None):
    """Host half of a decode.  items: [(bytes, JpegInfo, key or None, segments or None, name) or None (a gap: that row of the output is
    left alone)] -> what enqueue() takes: the per-file table and the metas and files in one pinned staging buffer (a ring of RING: a
    buffer stays untouched until two calls later).  Before it reuses a staging slot it reads the status and entries the decode RING
    calls ago left there.  staged: stage()'s token; the items' data are then (offset, length) pairs in the staged span, and only the
    metas are added behind it."""
    n = len(items)
    if not 1 <= n <= self.max_files:
      raise ValueError("decode: %d files, 1 .. %d" % (n, self.max_files))
    if staged is not None:
      return self._pack_staged(items, staged)
    slot = self._turn
    self._turn = (self._turn + 1) % self.RING
    bad = self.harvest(slot)                # of the call RING calls ago: its event has long completed
    table = (_lib.JpegDecFile * n)()
    parts, at, segments = [], 0, []
    for i, item in enumerate(items):
      if item is None:                      # a gap: n_segments 0, the caller fills the row
        segments.append(0)
        continue
      data, info, key, seg, _ = item
      if seg is None and key is not None and key in self.index and not info.dri:
        seg = index_segments(info, self.index[key])
      meta = meta_blob(info, seg)
      f = table[i]
      f.meta_offset, f.file_offset = at, at + len(meta)
      f.file_bytes, f.width, f.height, f.sampling, f.restart_interval = len(data), info.width, info.height, info.sampling, info.dri
      f.n_segments = len(info.segments if seg is None else seg)
      segments.append(int(f.n_segments))
      for c in range(3):
        f.tq[c], f.td[c], f.ta[c] = info.tq[c], info.td[c], info.ta[c]
      pad = -(len(meta) + len(data)) % 16
      parts += [meta, data, bytes(pad)]
      at += len(meta) + len(data) + pad
    ring = self._staging(slot, at)
    ring[0].numpy()[:at] = np.frombuffer(b"".join(parts), np.uint8)
    return slot, table, at, segments, items, bad

  def _pack_staged(self, items, staged):
    slot, span, bad = staged
    n = len(items)
    table = (_lib.JpegDecFile * n)()
    at0 = (span + 15) & ~15
    parts, at, segments = [], at0, []
    for i, item in enumerate(items):
      if item is None:
        segments.append(0)
        continue
      (offset, length), info, key, seg, _ = item
      if not (0 <= offset and 0 < length and offset + length <= span):
        raise ValueError("decode: file %d lies at %d .. %d of a staged span of %d bytes" % (i, offset, offset + length, span))
      if seg is None and key is not None and key in self.index and not info.dri:
        seg = index_segments(info, self.index[key])
      meta = meta_blob(info, seg)
      f = table[i]
      f.meta_offset, f.file_offset = at, offset
      f.file_bytes, f.width, f.height, f.sampling, f.restart_interval = length, info.width, info.height, info.sampling, info.dri
      f.n_segments = len(info.segments if seg is None else seg)
      segments.append(int(f.n_segments))
      for c in range(3):
        f.tq[c], f.td[c], f.ta[c] = info.tq[c], info.td[c], info.ta[c]
      pad = -len(meta) % 16
      parts += [meta, bytes(pad)]
      at += len(meta) + pad
    ring = self._staging(slot, at, keep=span)
    if at > at0:
      ring[0].numpy()[at0:at] = np.frombuffer(b"".join(parts), np.uint8)
    return slot, table, at, segments, items, bad

  def enqueue(self, packed, out, row_pitch, frame_stride, status, raise_bad=True):
    """Device half: one H2D copy of the staging buffer, vp_jpegdec_decode into out (device uint8 the caller owns), and the copies of status
    and entries back to pinned memory, all on the current stream; no wait."""
    slot, table, at, segments, items, bad = packed
    n = len(items)
    pinned, dev, st_host, en_host, scan_host = self._ring[slot]
    dev[:at].copy_(pinned[:at], non_blocking=True)
    _lib.check(self.L.vp_jpegdec_decode(self.h, ptr(dev), table, n, ptr(out), int(row_pitch), int(frame_stride), ptr(status), stream()),
               "vp_jpegdec_decode")
    st_host[:n].copy_(status[:n], non_blocking=True)
    en_host[:n].copy_(self.tensor("entries")[:n], non_blocking=True)
    scan = self.scan_chunk_bytes is not None
    if scan:
      scan_host[0, :n].copy_(self.tensor("scan_ok")[:n], non_blocking=True)
      scan_host[1, :n].copy_(self.tensor("scan_rounds")[:n], non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    rows = [it and it[1].mcuy for it in items]
    self._last = (segments, (event, scan_host[0].numpy(), rows) if scan else None)
    self._pending[slot] = (event, st_host, en_host, [it and it[2] for it in items], rows, [it and it[4] for it in items],
                           scan_host[1] if scan else None)
    if bad and raise_bad:
      raise RuntimeError("corrupt JPEG data in %s" % ", ".join(str(b) for b in bad))

  def decode_into(self, items, out, row_pitch, frame_stride, status, raise_bad=True):
    """pack() then enqueue().  A file's status is looked at RING calls later, when its staging slot is packed again, and only there: one
    with status != 0 then raises RuntimeError naming it (raise_bad).  The files of the last RING calls before a decoder is dropped are
    therefore never reported unless the caller ends with harvest(), which waits for them and returns the names."""
    self.enqueue(self.pack(items), out, row_pitch, frame_stride, status, raise_bad)

  def items(self, files, indexes=None):
    """bytes or paths -> decode_into's items (read and parsed; a file parse() refuses raises ValueError naming the reason)."""
    items = []
    for i, f in enumerate(files):
      key = None
      if isinstance(f, (bytes, bytearray, memoryview)):
        data, name = bytes(f), "file %d" % i
      else:
        key, name = _key(f), str(f)
        with open(f, "rb") as fh:
          data = fh.read()
      info = parse(data, self.max_height, self.max_width, self.accept_422, self.default_huffman)
      if info.refused:
        raise ValueError("%s: %s" % (name, info.refused))
      seg = index_segments(info, np.asarray(indexes[i], np.int32)) if indexes is not None and indexes[i] is not None else None
      items.append((data, info, key, seg, name))
    return items

  def decode(self, files, out=None, indexes=None):
    """files: bytes or paths.  indexes: per file None or int32 [mcuy, 4] entries to decode from (paths use the cache on their own).  A
    file parse() refuses raises ValueError naming the reason."""
    self.harvest()                          # this convenience call may wait: the index of every earlier call is used
    items = self.items(files, indexes)
    if out is None:
      out = torch.zeros(len(items), self.max_height, self.max_width, 3, dtype=torch.uint8, device="cuda")
    assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 4 and out.shape[0] >= len(items) and out.stride(3) == 1 and out.stride(2) == 3
    status = torch.empty(len(items), dtype=torch.int32, device="cuda")
    self.decode_into(items, out, out.stride(1), out.stride(0), status, raise_bad=False)
    return out[:len(items)], status

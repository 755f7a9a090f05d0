"""Stream ingest on the device (libvp_hip.so: vp_pcmin_*, csrc/pcm_in.hip): client PCM as it arrives - interleaved int16 or float32, 1 .. 8
channels, any common rate - to the mono float32 16 kHz signal AudioStreamGroup takes.

What WavLoader.get_data does for a whole file on the host (scale, mean over the channels, scipy.signal.resample_poly), chunk by chunk: the
concatenated output of a clip is the same bits however the pushes cut it, and it is WavLoader's signal up to float32 summation order
(exactly, for 16 kHz input).  push only enqueues; every count is host arithmetic (ready, samples_after).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr, slot_arrays, stream

COMMON_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000)     # a default for PcmIngest(rates=): at most 8 per handle
FORMATS = {"s16": (_lib.PCM_S16, np.int16), "f32": (_lib.PCM_F32, np.float32)}


def pcmin_desc(slots, rates, out_rate=16000, max_in_frames=1 << 20):
  rates = [int(r) for r in rates]
  if len(rates) > 8:
    raise ValueError("at most 8 rates per PcmIngest (%d given)" % len(rates))
  return _lib.PcmInDesc(ctypes.sizeof(_lib.PcmInDesc), int(slots), int(out_rate), int(max_in_frames), len(rates), (ctypes.c_int * 8)(*rates))


def ratio(in_rate, out_rate=16000):
  """(up, down, half, taps per phase) of resample_poly's default design for in_rate -> out_rate.  Host only."""
  v = [ctypes.c_int() for _ in range(4)]
  _lib.check(_lib.lib().vp_pcmin_ratio(int(in_rate), int(out_rate), *[ctypes.byref(x) for x in v]), "vp_pcmin_ratio")
  return tuple(x.value for x in v)


def bank(in_rate, out_rate=16000):
  """The filter h [2 half + 1] float32 the device's polyphase bank is cut from.  Host only."""
  half = ratio(in_rate, out_rate)[2]
  h = np.zeros(2 * half + 1, np.float32)
  _lib.check(_lib.lib().vp_pcmin_bank(int(in_rate), int(out_rate), h.ctypes.data_as(ctypes.c_void_p)), "vp_pcmin_bank")
  return h


def samples_after(in_rate, in_frames, finished=False, out_rate=16000):
  """Output samples a clip has emitted after in_frames input frames.  Host only."""
  n = int(_lib.lib().vp_pcmin_samples_after(int(in_rate), int(out_rate), int(in_frames), int(bool(finished))))
  if n < 0:
    raise ValueError(_lib.lib().vp_last_error().decode())
  return n


def read_wav(path):
  """A PCM .wav as stored, for push_raw: (rate, frames [n, channels] int16 or float32, "s16" or "f32")."""
  from scipy.io import wavfile
  rate, data = wavfile.read(path)
  fmt = {np.dtype(np.int16): "s16", np.dtype(np.float32): "f32"}.get(data.dtype)
  if fmt is None:
    raise ValueError("%s: %s samples; the ingest takes int16 and float32" % (path, data.dtype))
  return int(rate), np.ascontiguousarray(data.reshape(data.shape[0], -1)), fmt


class PcmIngest(Handle):
  """`slots` independent ingest sessions behind one handle.

  open_slot(slot, rate, channels=1, fmt="s16") starts (or restarts) a slot's clip.  push({slot: frames}, finish=()) -> (float32 device
  tensor with the slots' new 16 kHz samples packed in slot order, samples per slot): exactly the packed pcm and sizes of
  AudioStreamGroup.push_device_packed.  frames: an interleaved array [n, channels] or [n * channels] of the slot's sample type (numpy,
  or a torch tensor on either side).  Host chunks reach the device in one pinned copy."""

  def __init__(self, slots, rates=COMMON_RATES, out_rate=16000, max_in_frames=1 << 20):
    if not torch.cuda.is_available():
      raise RuntimeError("PcmIngest needs an MI355X (no CPU fallback)")
    self.slots, self.out_rate, self.max_in_frames = int(slots), int(out_rate), int(max_in_frames)
    self._open("pcmin", pcmin_desc(slots, rates, out_rate, max_in_frames), (stream(),), invalid="invalid ingest descriptor")
    self.fmt = [None] * self.slots        # per open slot: (channels, numpy sample type)

  def open_slot(self, slot, rate, channels=1, fmt="s16"):
    slot = int(slot)
    if not 0 <= slot < self.slots:
      raise IndexError("slot %d of %d" % (slot, self.slots))
    if fmt not in FORMATS:
      raise ValueError("fmt %r: one of %s" % (fmt, sorted(FORMATS)))
    code, dt = FORMATS[fmt]
    _lib.check(self.L.vp_pcmin_open_slot(self.h, slot, int(rate), int(channels), code, stream()), "vp_pcmin_open_slot")
    self.fmt[slot] = (int(channels), np.dtype(dt))

  def ready(self, frames_by_slot, finish=()):
    """Samples per slot (a list of `slots` counts) that a push of frames_by_slot ({slot: input frames} or a sequence) emits, the slots in
    `finish` ending their clips after them.  Host only.  (One launch: more than max_in_frames for a slot is refused; push splits.)"""
    n, fin = slot_arrays(self.slots, frames_by_slot, finish)
    k = (ctypes.c_longlong * self.slots)()
    if self.L.vp_pcmin_ready(self.h, n, fin, k) < 0:
      raise ValueError(self.L.vp_last_error().decode())
    return [int(v) for v in k]

  def _frames(self, slot, x):
    """One slot's chunk as a flat array / tensor of its sample type, and its frame count."""
    if self.fmt[slot] is None:
      raise ValueError("slot %d is not open" % slot)
    c, dt = self.fmt[slot]
    if torch.is_tensor(x):
      tdt = torch.int16 if dt == np.int16 else torch.float32
      if x.dtype != tdt:
        raise TypeError("slot %d takes %s samples, not %s" % (slot, dt, x.dtype))
      x = x.contiguous().reshape(-1)
      n = int(x.numel())
    else:
      x = np.asarray(x)
      if x.dtype != dt:
        raise TypeError("slot %d takes %s samples, not %s" % (slot, dt, x.dtype))
      x = np.ascontiguousarray(x).reshape(-1)
      n = int(x.size)
    if n % c:
      raise ValueError("slot %d: %d samples are no whole frames of %d channels" % (slot, n, c))
    return x, n // c

  def _push_once(self, chunks, frames, finish):
    """One vp_pcmin_push: chunks {slot: flat samples}, frames {slot: count}."""
    k = self.ready(frames, finish)
    order = [s for s in sorted(chunks) if frames[s]]
    offs, nbytes = {}, 0
    for s in order:
      nbytes = (nbytes + 15) & ~15
      offs[s] = nbytes
      nbytes += frames[s] * self.fmt[s][0] * self.fmt[s][1].itemsize
    raw = None
    if order:
      if all(not torch.is_tensor(chunks[s]) or not chunks[s].is_cuda for s in order):
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        for s in order:
          v = chunks[s].numpy() if torch.is_tensor(chunks[s]) else chunks[s]
          hv[offs[s]:offs[s] + v.nbytes] = v.view(np.uint8)
        raw = host.to("cuda", non_blocking=True)
      else:
        raw = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for s in order:
          v = chunks[s] if torch.is_tensor(chunks[s]) else torch.from_numpy(chunks[s])
          v = v.view(torch.uint8)
          raw[offs[s]:offs[s] + v.numel()].copy_(v, non_blocking=True)
    total = sum(k)
    out = torch.empty(total, dtype=torch.float32, device="cuda")
    n, fin = slot_arrays(self.slots, frames, finish)
    _lib.check(self.L.vp_pcmin_push(self.h, ptr(raw), n, fin, ptr(out if total else None), stream()), "vp_pcmin_push")
    return out, k

  def push(self, raw_by_slot, finish=()):
    finish = sorted(set(int(s) for s in finish))
    chunks, frames = {}, {}
    for s, x in raw_by_slot.items():
      s = int(s)
      if not 0 <= s < self.slots:
        raise IndexError("slot %d of %d" % (s, self.slots))
      chunks[s], frames[s] = self._frames(s, x)
    for s in finish:
      if not 0 <= s < self.slots:
        raise IndexError("slot %d of %d" % (s, self.slots))
    if all(n <= self.max_in_frames for n in frames.values()):
      return self._push_once(chunks, frames, finish)
    # a chunk longer than max_in_frames: several launches, each slot's pieces put back together in slot order
    pieces, done = {s: [] for s in range(self.slots)}, {s: 0 for s in chunks}
    while True:
      part = {s: min(frames[s] - done[s], self.max_in_frames) for s in chunks}
      last = all(done[s] + part[s] == frames[s] for s in chunks)
      sub = {s: chunks[s][done[s] * self.fmt[s][0]:(done[s] + part[s]) * self.fmt[s][0]] for s in chunks}
      out, k = self._push_once(sub, part, finish if last else ())
      o = 0
      for s in range(self.slots):
        if k[s]:
          pieces[s].append(out[o:o + k[s]])
        o += k[s]
      for s in chunks:
        done[s] += part[s]
      if last:
        break
    k = [sum(int(p.numel()) for p in pieces[s]) for s in range(self.slots)]
    flat = [p for s in range(self.slots) for p in pieces[s]]
    return (torch.cat(flat) if flat else torch.empty(0, dtype=torch.float32, device="cuda")), k

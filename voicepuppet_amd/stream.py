"""Streaming audio-to-face inference (libvp_hip.so: vp_bfmstream_*).

AudioStream takes PCM in chunks of any size and returns each video frame's 64 BFM coefficients as soon as the frame's receptive field
has arrived: the frames infer_bfmvid computes offline for the whole clip (same checkpoint, same ears), with the values of the offline
forward.  The lookahead is the receptive field's right side (right_frames video frames) plus the half frame the log-mel window reaches
past its hop; nothing is approximated.  push / finish never wait on the device (host data is staged through pinned memory).

PuppetStreamGroup puts the rest of infer_bfmvid behind an AudioStreamGroup, for many talkers at once: splice_coeff -> ClipRenderer (the
head-sway state carried across pushes) -> PixReferNet -> uint8 frames, conditioned on the same background and reference panels by global
frame index (libvp_hip.so: vp_puppet_*, vp_bfm_reconstruct_rows).  Its push only enqueues too: the sway state and every per-row table
are host arithmetic on frame counts.  PuppetStream is a group of one slot that hands out host arrays.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._handle import Handle, ptr, slot_arrays, stream
from ._lib import BfmStreamDesc, BfmStreamGroupDesc
from .audio import bfmnet_manifest, write_params

SAMPLES_PER_FRAME = 640          # 16 kHz / 25 frames per second (config/params.yml)


def stream_desc(max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
  return BfmStreamDesc(ctypes.sizeof(BfmStreamDesc), max_chunk_frames, num_mel_bins, {"f32": _lib.VP_F32, "bf16": _lib.VP_BF16}[dtype],
                       sample_rate, lower_hz, upper_hz)


def stream_context(desc):
  """(left_mel, right_mel, left_frames, right_frames, window_frames), derived by the library from MfccNet's layer table."""
  v = [ctypes.c_int() for _ in range(5)]
  _lib.check(_lib.lib().vp_bfmstream_context(ctypes.byref(desc), *[ctypes.byref(x) for x in v]), "vp_bfmstream_context")
  return tuple(x.value for x in v)


def load_bfmnet_params(path):
  """A BFMNet checkpoint as infer_bfmvid restores it: an .npz keyed by the TF variable names, or a TensorFlow checkpoint prefix."""
  if path.endswith('.npz'):
    z = np.load(path)
    return {k: z[k] for k in z.files}
  from .utils import tf_checkpoint
  return tf_checkpoint.read_checkpoint(path)


def _lookahead_ms(right_mel, sample_rate):
  return 1000.0 * (right_mel * 128 + (512 - 128)) / sample_rate


class AudioStream(Handle):
  """One streaming session of BFMNet inference.

  push(pcm) / finish() return [k, 64] f32 device tensors, k = ready(len(pcm)) / ready_finish(); finish zero-pads the clip the way
  prepare_pcm does (pad_len = 1 + N // 640 frames in all).  ears: [k, 1] per call, or None to draw np.random.rand(k, 1) / 100 (numpy's
  legacy generator: consecutive draws are the offline single draw of pad_len, so a seeded run gets infer_bfmvid's ears)."""

  def __init__(self, params=None, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
    if not torch.cuda.is_available():
      raise RuntimeError("AudioStream needs an MI355X (no CPU fallback)")
    ws = self._query("bfmstream", stream_desc(max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz), "invalid stream descriptor")
    self.left_mel, self.right_mel, self.left_frames, self.right_frames, self.window_frames = stream_context(self.desc)
    self.manifest = bfmnet_manifest()
    self.params = torch.zeros(self.L.vp_bfmnet_param_count(), dtype=torch.float32, device="cuda")
    self._create(ws, (ptr(self.params), stream()), zero=True)
    self.samples = 0
    if params is not None:
      self.load_params(load_bfmnet_params(params) if isinstance(params, str) else params)

  @property
  def lookahead_ms(self):
    """Audio that must arrive after a frame's own 40 ms before the frame is emitted: its right context in mel rows plus the part of
    the last mel window past its hop."""
    return _lookahead_ms(self.right_mel, self.desc.sample_rate)

  def load_params(self, params):
    write_params(self.params, self.manifest, params)
    _lib.check(self.L.vp_bfmstream_params_changed(self.h), "vp_bfmstream_params_changed")

  def ready(self, n_samples):
    return int(self.L.vp_bfmstream_ready(self.h, int(n_samples)))

  def ready_finish(self):
    return int(self.L.vp_bfmstream_ready_finish(self.h))

  @staticmethod
  def _to_device(x):
    """Host data -> device without a host wait: copied into a pinned block of torch's host allocator (which keeps the block until
    the asynchronous copy has run), then enqueued on the current stream."""
    if isinstance(x, np.ndarray):
      x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not x.is_cuda:
      x = x.pin_memory().to("cuda", non_blocking=True)
    return x.contiguous()

  def _ears(self, k, ears):
    if ears is None:
      ears = np.random.rand(k, 1).astype(np.float32) / 100
    ears = self._to_device(ears)
    assert ears.dtype == torch.float32 and ears.numel() == k, (tuple(ears.shape), k)
    return ears

  def push(self, pcm, ears=None):
    """pcm: 1-D f32 (numpy or tensor) -> coefficients [k, 64] of the frames that became exact.  Enqueues only: the returned
    tensor is ready when the current stream reaches it."""
    pcm = self._to_device(pcm)
    assert pcm.dtype == torch.float32 and pcm.dim() == 1
    n = pcm.numel()
    k = self.ready(n)
    out = torch.empty(k, 64, dtype=torch.float32, device="cuda")
    e = self._ears(k, ears) if k else None
    _lib.check(self.L.vp_bfmstream_push(self.h, ptr(pcm), n, ptr(e), ptr(out if k else None), stream()), "vp_bfmstream_push")
    self.samples += n
    return out

  def finish(self, ears=None):
    k = self.ready_finish()
    out = torch.empty(k, 64, dtype=torch.float32, device="cuda")
    e = self._ears(k, ears)
    _lib.check(self.L.vp_bfmstream_finish(self.h, ptr(e), ptr(out), stream()), "vp_bfmstream_finish")
    return out

  def reset(self):
    _lib.check(self.L.vp_bfmstream_reset(self.h, stream()), "vp_bfmstream_reset")
    self.samples = 0

  def mel_history(self):
    """The device mel history: [rows, num_mel_bins]; mel frame r of the clip sits at row r % rows while it is kept."""
    return self._tensor("mel", torch.float32, 2)


def group_desc(slots, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
  return BfmStreamGroupDesc(ctypes.sizeof(BfmStreamGroupDesc), slots, max_chunk_frames, num_mel_bins,
                            {"f32": _lib.VP_F32, "bf16": _lib.VP_BF16}[dtype], sample_rate, lower_hz, upper_hz)


class AudioStreamGroup(Handle):
  """`slots` independent AudioStream sessions behind one handle (libvp_hip.so: vp_bfmstream_group_*), for serving many talkers at once.

  One push advances any subset of the slots by any number of samples each and runs one kernel chain per round for all of them.  Every
  slot's coefficients are bit-identical to an AudioStream with the same max_chunk_frames and dtype fed the same chunks (finish: the
  chunk, then AudioStream.finish).  ears: {slot: [k, 1]} per push, or None to draw np.random.rand(k, 1) / 100 per slot in slot order."""

  def __init__(self, params=None, slots=1, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
    if not torch.cuda.is_available():
      raise RuntimeError("AudioStreamGroup needs an MI355X (no CPU fallback)")
    self.slots = int(slots)
    ws = self._query("bfmstream_group", group_desc(self.slots, max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz),
                     "invalid stream group descriptor")
    self.left_mel, self.right_mel, self.left_frames, self.right_frames, self.window_frames = stream_context(
        stream_desc(max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz))
    self.manifest = bfmnet_manifest()
    self.params = torch.zeros(self.L.vp_bfmnet_param_count(), dtype=torch.float32, device="cuda")
    self._create(ws, (ptr(self.params), stream()), zero=True)
    self.keep_pcm = False           # a PuppetStreamGroup that writes AVI: last_pcm is the packed device samples of the last push (or None)
    self.last_pcm = None
    if params is not None:
      self.load_params(load_bfmnet_params(params) if isinstance(params, str) else params)

  @property
  def lookahead_ms(self):
    """As AudioStream.lookahead_ms (the same for every slot)."""
    return _lookahead_ms(self.right_mel, self.desc.sample_rate)

  def load_params(self, params):
    write_params(self.params, self.manifest, params)
    _lib.check(self.L.vp_bfmstream_group_params_changed(self.h), "vp_bfmstream_group_params_changed")

  def ready(self, n_by_slot, finish_by_slot=()):
    """Frames per slot (a list of `slots` counts) that a push of n_by_slot ({slot: samples} or a sequence) new samples emits, the slots
    in finish_by_slot ending their clips after them.  Host only."""
    n, fin = slot_arrays(self.slots, n_by_slot, finish_by_slot)
    k = (ctypes.c_int * self.slots)()
    if self.L.vp_bfmstream_group_ready(self.h, n, fin, k) < 0:
      raise ValueError("bad ready query (negative count, or samples / finish for a finished slot)")
    return list(k)

  def push(self, pcm_by_slot, finish=(), ears=None):
    """{slot: 1-D f32 pcm (numpy or tensor)} -> {slot: coefficients [k, 64]} for every slot pushed or finished.  Enqueues only: the
    tensors are ready when the current stream reaches them."""
    out, k, sizes = self.push_packed(pcm_by_slot, finish, ears)
    res, row = {}, 0
    for s in range(self.slots):
      if s in sizes:
        res[s] = out[row:row + k[s]]
      row += k[s]
    return res

  def push_packed(self, pcm_by_slot, finish=(), ears=None):
    """push, returning (the packed coefficients [K, 64] in slot order, frames per slot, {slot pushed or finished: samples})."""
    slots = sorted(set(int(s) for s in pcm_by_slot) | set(int(s) for s in finish))
    for s in slots:
      if not 0 <= s < self.slots:
        raise IndexError("slot %d of %d" % (s, self.slots))
    chunks = {int(s): v for s, v in pcm_by_slot.items()}
    sizes = {s: (int(chunks[s].numel()) if torch.is_tensor(chunks[s]) else int(np.asarray(chunks[s]).size)) if s in chunks else 0 for s in slots}
    total = sum(sizes.values())
    if total == 0:
      pcm = None
    elif all(not (torch.is_tensor(chunks[s]) and chunks[s].is_cuda) for s in chunks):
      # host chunks: packed on the host, staged through pinned memory in one copy
      pcm = AudioStream._to_device(np.concatenate([np.asarray(chunks[s].numpy() if torch.is_tensor(chunks[s]) else chunks[s], dtype=np.float32).reshape(-1)
                                                   for s in slots if s in chunks]))
    else:
      pcm = torch.empty(total, dtype=torch.float32, device="cuda")
      o = 0
      for s in slots:
        if sizes[s]:
          pcm[o:o + sizes[s]].copy_(AudioStream._to_device(chunks[s]).reshape(-1))
          o += sizes[s]
    return self.push_device_packed(pcm, sizes, finish, ears)

  def push_device_packed(self, pcm, sizes, finish=(), ears=None):
    """push_packed for samples that are already packed on the device: pcm, a 1-D f32 device tensor with the slots' new samples in slot
    order (None when there are none; voicepuppet_amd.pcm.PcmIngest.push returns it so), sizes {slot: samples} (or a sequence of `slots`
    counts) of the slots pushed.  Nothing is copied."""
    sizes = {int(s): int(v) for s, v in (sizes.items() if isinstance(sizes, dict) else enumerate(sizes))}
    for s in finish:
      sizes.setdefault(int(s), 0)
    for s in sizes:
      if not 0 <= s < self.slots:
        raise IndexError("slot %d of %d" % (s, self.slots))
    total = sum(sizes.values())
    if total:
      if not (torch.is_tensor(pcm) and pcm.is_cuda and pcm.dtype == torch.float32 and pcm.is_contiguous() and pcm.numel() == total):
        raise ValueError("push_device_packed: a contiguous f32 device tensor of %d samples" % total)
    else:
      pcm = None
    if self.keep_pcm:
      self.last_pcm = pcm
    k = self.ready(sizes, finish)
    K = sum(k)
    out = torch.empty(K, 64, dtype=torch.float32, device="cuda")
    e = None
    if K:
      if ears is None:
        e = np.concatenate([np.random.rand(k[s], 1).astype(np.float32) / 100 for s in range(self.slots) if k[s]])
      else:
        e = np.concatenate([np.asarray(ears[s], dtype=np.float32).reshape(k[s], 1) for s in range(self.slots) if k[s]])
      e = AudioStream._to_device(e)
    n, fin = slot_arrays(self.slots, sizes, finish)
    _lib.check(self.L.vp_bfmstream_group_push(self.h, ptr(pcm), n, fin, ptr(e), ptr(out if K else None), stream()),
               "vp_bfmstream_group_push")
    return out, k, sizes

  def reset_slot(self, slot):
    """Slot `slot` starts a new clip; the other slots are untouched."""
    _lib.check(self.L.vp_bfmstream_group_reset_slot(self.h, int(slot), stream()), "vp_bfmstream_group_reset_slot")

  def mel_history(self):
    """The device mel rings: [slots, rows, num_mel_bins]."""
    return self._tensor("mel", torch.float32, 3)


class HeadSway:
  """infer_bfmvid.angle_sequence with its state carried: next(n) returns the angles of the next n frames, so consecutive calls
  concatenate to angle_sequence(total) (same float32 accumulation, same direction flips)."""

  def __init__(self, start=(0.0, 0.0, 0.0), shift=0.005):
    self.start, self.shift0 = start, shift
    self.reset()

  def reset(self):
    self.angles = np.array([self.start], dtype=np.float32)
    self.shift = self.shift0

  def next(self, n):
    angles, shift = self.angles, self.shift
    out = np.zeros((n, 3), np.float32)
    for i in range(n):
      angles[0][0] += shift
      angles[0][1] += shift
      angles[0][2] += shift
      if (angles[0][1] > 0.03 or angles[0][1] < -0.03):
        shift = -shift
      out[i] = angles[0]
    self.shift = shift
    return out


class PuppetRowPlan:
  """Host side of a PuppetStreamGroup push, a pure function of the frame counts: which slot, global frame index and head-sway angles
  every packed row of a push has.  Per slot the angles of consecutive pushes concatenate to infer_bfmvid.angle_sequence(total) and
  the indices to 0 .. total-1; reset_slot starts a slot's clip again.  No device involved."""

  def __init__(self, slots):
    self.slots = int(slots)
    self.sway = [HeadSway() for _ in range(self.slots)]
    self.frame = [0] * self.slots

  def reset_slot(self, slot):
    self.sway[slot].reset()
    self.frame[slot] = 0

  def rows(self, k_by_slot):
    """k_by_slot: `slots` frame counts -> (slot [K] int32, global frame index [K] int64, angles [K, 3] f32), rows packed in slot order."""
    assert len(k_by_slot) == self.slots
    slot, g, ang = [], [], []
    for s, k in enumerate(k_by_slot):
      k = int(k)
      if k:
        slot.append(np.full(k, s, np.int32))
        g.append(np.arange(self.frame[s], self.frame[s] + k, dtype=np.int64))
        ang.append(self.sway[s].next(k))
        self.frame[s] += k
    if not slot:
      return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
    return np.concatenate(slot), np.concatenate(g), np.concatenate(ang)


def launch_tables(slot, g, has_coeff, bg_row, frame_batch):
  """The device tables of one push from its rows (PuppetRowPlan.rows), host only.  has_coeff [slots] bool: the slots conditioned on
  their rendered face; bg_row [100]: row of the background bank for global frame index % 100, or -1.  Returns
    render [R, 4] int32   {slot, packed row, 0, 0} of the R rows that are rendered (vp_puppet_splice)
    tex_src [n] / tex_row [R] int32   one texture per slot present among them (vp_bfm_reconstruct_rows)
    cond [Kp, 4] int32    {slot, render row or -1, background row or -1, global frame index} for every row, padded with the last row to a
                          multiple of frame_batch (vp_puppet_condition; as infer_bfmvid pads a short last batch)"""
  K = int(slot.shape[0])
  rendered = np.flatnonzero(np.asarray(has_coeff, bool)[slot]) if K else np.zeros(0, np.int64)
  R = int(rendered.shape[0])
  render = np.zeros((R, 4), np.int32)
  render[:, 0], render[:, 1] = slot[rendered], rendered
  present, first = np.unique(slot[rendered], return_index=True)
  tex_src = first.astype(np.int32)
  tex_row = np.searchsorted(present, slot[rendered]).astype(np.int32)
  Kp = -(-K // frame_batch) * frame_batch
  cond = np.zeros((Kp, 4), np.int32)
  face = np.full(K, -1, np.int32)
  face[rendered] = np.arange(R, dtype=np.int32)
  cond[:K, 0], cond[:K, 1], cond[:K, 2], cond[:K, 3] = slot, face, np.asarray(bg_row, np.int32)[g % 100], g
  if K:
    cond[K:] = cond[K - 1]
  return render, tex_src, tex_row, cond


def puppet_desc(slots, frame_batch=8, img_size=512, face_size=224):
  return _lib.PuppetDesc(ctypes.sizeof(_lib.PuppetDesc), slots, frame_batch, img_size, face_size)


_BANKS = {}      # background banks by (directory, image size, the files and their modification times): decoded once per process


def background_bank(img_size):
  """The backgrounds that exist, as infer_bfmvid.background_target reads them: (uint8 device bank [n, H, H, 3] or None, bg_row [100] with
  the bank row of global frame index % 100 or -1).  background_target's float image is float32(u8) / 255.0 of the resized uint8 image, so
  the uint8 bank loses nothing (checked here, value for value)."""
  import os
  from .pixrefer import infer_bfmvid as ib
  names = ['background/{}.jpg'.format(j + 1) for j in range(100)]
  key = (os.path.abspath('background'), img_size, tuple(os.path.getmtime(f) if os.path.exists(f) else None for f in names))
  if key not in _BANKS:
    imgs, bg_row = [], np.full(100, -1, np.int32)
    for j in range(100):
      f = ib.background_target(j, img_size)
      if f is not None:
        u8 = np.rint(f * 255.0).astype(np.uint8)
        if not np.array_equal(u8.astype(np.float32) / 255.0, f):
          raise RuntimeError("%s: not float32(uint8) / 255.0" % names[j])
        bg_row[j] = len(imgs)
        imgs.append(u8)
    if len(_BANKS) >= 4:
      _BANKS.clear()
    _BANKS[key] = (torch.from_numpy(np.stack(imgs)).to("cuda") if imgs else None, bg_row)
  return _BANKS[key]


class PuppetStreamGroup(Handle):
  """Streaming infer_bfmvid for `slots` talkers behind one handle: one AudioStreamGroup, one generator plan (infer_bfmvid's cache, batch
  frame_batch, per-sample batch norm), one ClipRenderer; per slot a photo, its coefficients, a head-sway state and a frame counter.

  attach(slot, image, bfmcoeff): that talker's 512 x 1536 photo (RGB float in [0,1], as infer_bfmvid reads it) and coefficient npz
  (bfmcoeff, transform_params, center_x, center_y, ratio); without the npz (or without BFM/BFM_model_front.mat) the slot is conditioned
  on its reference 3-D face panel.  Restarts the slot's clip.
  push({slot: pcm}, finish=()) -> {slot: [(global frame index, uint8 [H, W, 3] RGB device tensor)]} for every slot pushed or finished.
  The frames of all slots that emitted run packed in slot order through splice, render, conditioning (libvp_hip.so: vp_puppet_*,
  vp_bfm_reconstruct_rows) and the generator in launches of frame_batch rows, a short last launch padded with the last row.  A push
  only enqueues: frame counts follow from sample counts, the per-row tables (slot, sway rotation, background, geometry) are computed
  on the host first and reach the device through pinned memory; the frames are views of one [K, H, W, 3] tensor (last_frames) that is
  ready when the current stream reaches it.

  jpeg_quality=Q (1 .. 100; None, the default: no encoder exists and push is what it is without the keyword): the group owns a
  voicepuppet_amd.jpeg.JpegEncoder of frame_batch frames, a push also enqueues the JPEG encode of last_frames in launches of at most
  frame_batch rows, and last_jpeg() -> {slot: [(global frame index, bytes of the .jpg file)]} for the frames of the last push (the one
  wait: the lengths, then the used part of the byte rows; the raw frames stay on the device).

  avi=True (with jpeg_quality): the group owns a voicepuppet_amd.avi.AviMuxer and a push also enqueues, behind its JPEG encodes, the
  AVI segments of the push: per slot the 16-bit PCM of the samples pushed and the frames emitted, as RIFF chunks.  last_avi() -> {slot:
  (segment bytes, index entries)} of the last push (AviMuxer.to_host: one wait).  record(slot, path) opens a voicepuppet_amd.avi.AviWriter
  for the slot, write_avi() appends last_avi() to the writers that are open, stop(slot) closes the slot's file and returns its paths;
  attach and reset_slot stop a recording.  Without the keyword nothing of this exists and a push is what it was."""

  def __init__(self, config_path, slots, frame_batch=8, max_chunk_frames=1, dtype="f32", img_size=512, jpeg_quality=None, ingest_rates=None,
               avi=False):
    import os
    from .pixrefer import infer_bfmvid as ib
    if not torch.cuda.is_available():
      raise RuntimeError("PuppetStreamGroup needs an MI355X (no CPU fallback)")
    self.ib = ib
    self.slots, self.nb, self.img_size = int(slots), int(frame_batch), int(img_size)
    ws = self._query("puppet", puppet_desc(self.slots, self.nb, self.img_size), "invalid puppet group descriptor")
    bfm_file = next((f for f in (ib.BFMNET_CKPT + '.index', ib.BFMNET_CKPT + '.npz') if os.path.exists(f)), None)
    if bfm_file is None:
      from .bfmnet.bfmnet import random_variables
      ib.logger.warning('%s not found: running with randomly initialised weights', ib.BFMNET_CKPT)
      bfm_params = random_variables()
    else:
      bfm_params = load_bfmnet_params(bfm_file[:-len('.index')] if bfm_file.endswith('.index') else bfm_file)
    self.audio = AudioStreamGroup(bfm_params, slots=self.slots, max_chunk_frames=max_chunk_frames, dtype=dtype)
    self.net = ib.load_generator(config_path, self.nb, self.img_size)[0]
    self.engine = self.net.engine
    self.renderer = ib.clip_renderer() if os.path.exists(os.path.join('BFM', 'BFM_model_front.mat')) else None
    self._create(ws, (stream(),))
    self.bank, self.bg_row = background_bank(self.img_size)
    _lib.check(self.L.vp_puppet_set_backgrounds(self.h, ptr(self.bank), 0 if self.bank is None else int(self.bank.shape[0])),
               "vp_puppet_set_backgrounds")
    nb, H = self.nb, self.img_size
    self.inputs = torch.empty([nb, H, H, 6], dtype=torch.float32, device="cuda")
    self.fg_inputs = torch.empty([nb, H, H, 3], dtype=torch.float32, device="cuda")
    self.targets = torch.empty([nb, H, H, 3], dtype=torch.float32, device="cuda")
    self.plan = PuppetRowPlan(self.slots)
    self.has_coeff = np.zeros(self.slots, bool)
    self.attached = np.zeros(self.slots, bool)
    self.last_frames = None
    self.keep_conditioning = False     # tests: keep every row's generator inputs and float Outputs of a push in last_conditioning
    self.last_conditioning = None
    self.jpeg = None
    self._jpeg_rows = None
    if jpeg_quality is not None:
      from .jpeg import JpegEncoder
      self.jpeg = JpegEncoder(self.img_size, self.img_size, self.nb, quality=jpeg_quality)
    self.avi = None
    self._avi_seg = None
    self._writers = {}
    if avi:
      if self.jpeg is None:
        raise ValueError("PuppetStreamGroup: avi=True needs jpeg_quality (the video chunks are the device encoder's files)")
      from .avi import AviMuxer
      # a finishing push flushes the lookahead and a catch-up push carries any number of samples: the ABI's limits, not a guess
      self.avi = AviMuxer(_lib.AVIMUX_MAX_FRAMES, self.jpeg.capacity, self.slots, 1 << 24, quality=jpeg_quality)
      self.audio.keep_pcm = True
    self.ingest = None
    self._ingest_fmt = {}
    if ingest_rates is not None:
      from .pcm import PcmIngest
      self.ingest = PcmIngest(self.slots, rates=ingest_rates, out_rate=self.audio.desc.sample_rate)

  def attach(self, slot, image, bfmcoeff=None, rate=16000, channels=1, fmt="s16"):
    """rate / channels / fmt: what push_raw will be given for this slot (groups created with ingest_rates; ignored otherwise)."""
    ib, H = self.ib, self.img_size
    slot = int(slot)
    if not 0 <= slot < self.slots:
      raise IndexError("slot %d of %d" % (slot, self.slots))
    image = np.asarray(image)
    face3d_refer = image[:, H:H * 2, :]
    fg_refer = image[:, :H, :] * image[:, H * 2:, :]
    refer_t = torch.as_tensor(np.ascontiguousarray(face3d_refer, dtype=np.float32)).to("cuda")
    fg_t = torch.as_tensor(np.ascontiguousarray(fg_refer, dtype=np.float32)).to("cuda")
    if tuple(refer_t.shape) != (H, H, 3) or tuple(fg_t.shape) != (H, H, 3):
      raise ValueError("attach: the photo must be %d x %d x 3 (three panels side by side)" % (H, 3 * H))
    coeff, side, y0, x0 = None, 0, 0, 0
    if bfmcoeff and self.renderer is not None:
      p = np.load(bfmcoeff) if isinstance(bfmcoeff, str) else bfmcoeff
      coeff = np.ascontiguousarray(np.asarray(p['bfmcoeff'], dtype=np.float32).reshape(257))
      side, y0, x0 = ib.paste_geometry(int(p['center_x']), int(p['center_y']), float(p['ratio']), p['transform_params'], self.desc.face_size)
    else:
      ib.logger.warning('BFM assets unavailable: conditioning every frame on the reference 3-D face panel')
    _lib.check(self.L.vp_puppet_attach(self.h, slot, ptr(refer_t), ptr(fg_t), coeff.ctypes.data_as(ctypes.c_void_p) if coeff is not None else None,
                                       int(side), int(y0), int(x0), stream()), "vp_puppet_attach")
    self.has_coeff[slot] = coeff is not None
    self.attached[slot] = True
    if self.ingest is not None:
      self._ingest_fmt[slot] = (int(rate), int(channels), fmt)
    self.reset_slot(slot)

  def reset_slot(self, slot):
    """Slot `slot` starts a new clip (audio session, head sway, frame counter, ingest filter state); its photo stays."""
    if int(slot) in self._writers:
      self.stop(slot)
    self.audio.reset_slot(slot)
    self.plan.reset_slot(int(slot))
    if self.ingest is not None and int(slot) in self._ingest_fmt:
      self.ingest.open_slot(int(slot), *self._ingest_fmt[int(slot)])

  def frame(self, slot):
    """Frames emitted so far in slot `slot`'s clip."""
    return self.plan.frame[int(slot)]

  @staticmethod
  def _upload(parts):
    """Host arrays -> device tensors in ONE pinned-memory copy (no host wait): a list of numpy arrays -> their device copies."""
    offs, n = [], 0
    for a in parts:
      n = (n + 15) & ~15
      offs.append(n)
      n += a.nbytes
    host = torch.empty(max(n, 16), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for a, o in zip(parts, offs):
      hv[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    dev = host.to("cuda", non_blocking=True)
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64}
    return [dev[o:o + a.nbytes].view(tdt[a.dtype]).view(a.shape) for a, o in zip(parts, offs)]

  def push(self, pcm_by_slot, finish=(), ears=None):
    for s in set(int(s) for s in pcm_by_slot) | set(int(s) for s in finish):
      if not (0 <= s < self.slots and self.attached[s]):
        raise ValueError("slot %d has no photo attached" % s)
    # host first: frame counts from sample counts, then every per-row quantity
    return self._frames(*self.audio.push_packed(pcm_by_slot, finish, ears))

  def push_raw(self, raw_by_slot, finish=(), ears=None):
    """push for client PCM as it arrives: {slot: interleaved int16 / float32 frames at the rate, channel count and format the slot was
    attached with} -> the same result.  The ingest (voicepuppet_amd.pcm.PcmIngest: convert, down-mix, resample to 16 kHz, on the device)
    and the push that exists are enqueued back to back; a slot in `finish` flushes its last samples and ends its clip in the same push."""
    if self.ingest is None:
      raise RuntimeError("push_raw: the group was created without ingest_rates")
    slots = set(int(s) for s in raw_by_slot) | set(int(s) for s in finish)
    for s in slots:
      if not (0 <= s < self.slots and self.attached[s]):
        raise ValueError("slot %d has no photo attached" % s)
    pcm, n = self.ingest.push(raw_by_slot, finish)
    return self._frames(*self.audio.push_device_packed(pcm, {s: n[s] for s in slots}, finish, ears))

  def _frames(self, coeff, k, sizes):
    """The frame half of a push: the packed coefficients of AudioStreamGroup.push_packed -> {slot: [(global frame index, frame)]}."""
    from .utils.reconstruct_mesh import Compute_rotation_matrix
    L, nb, H = self.L, self.nb, self.img_size
    slot, g, angles = self.plan.rows(k)
    K = int(slot.shape[0])
    res = {s: [] for s in sizes}
    self.last_frames, self.last_conditioning = None, None
    self._jpeg_rows = None
    self._avi_seg = None
    if K == 0:
      if self.avi is not None and self.audio.last_pcm is not None:      # audio without a frame yet (the lookahead): a segment all the same
        self._avi_segment(None, None, None, sizes)
      return res
    render, tex_src, tex_row, cond = launch_tables(slot, g, self.has_coeff, self.bg_row, nb)
    R = int(render.shape[0])
    faces = None
    if R:
      rot = Compute_rotation_matrix(angles[render[:, 1]])
      rot_d, render_d, tex_src_d, tex_row_d, cond_d = self._upload([rot, render, tex_src, tex_row, cond])
      spliced = torch.empty(R, 257, dtype=torch.float32, device="cuda")
      _lib.check(L.vp_puppet_splice(self.h, ptr(coeff), K, ptr(render_d), R, ptr(spliced), stream()), "vp_puppet_splice")
      faces, _ = self.renderer.render_rows(spliced, rot_d, tex_src_d, int(tex_src.shape[0]), tex_row_d)
    else:
      cond_d, = self._upload([cond])
    Kp = int(cond.shape[0])
    out = torch.empty(Kp, H, H, 3, dtype=torch.uint8, device="cuda")
    kept = [] if self.keep_conditioning else None
    eng = self.engine
    for i0 in range(0, Kp, nb):
      _lib.check(L.vp_puppet_condition(self.h, ptr(faces), R, ptr(cond_d[i0:i0 + nb]), nb, ptr(self.inputs), ptr(self.fg_inputs),
                                       ptr(self.targets), stream()), "vp_puppet_condition")
      eng.forward(self.inputs, self.fg_inputs, self.targets)
      _lib.check(L.vp_pixrefer_fetch(eng.h, eng.FETCH["Outputs_u8"], ptr(out[i0:i0 + nb]), stream()), "vp_pixrefer_fetch(Outputs_u8)")
      if kept is not None:
        n = min(nb, K - i0)
        kept.append([t[:n].clone() for t in (self.inputs, self.fg_inputs, self.targets, eng.fetch("Outputs"))])
    self.last_frames = out[:K]
    if self.jpeg is not None:
      # a finishing push flushes the lookahead: K has no small bound, the encoder's launches have (frame_batch rows)
      data = torch.empty(K, self.jpeg.capacity, dtype=torch.uint8, device="cuda")
      lengths = torch.empty(K, dtype=torch.int32, device="cuda")
      for i0 in range(0, K, nb):
        n = min(nb, K - i0)
        self.jpeg.encode(out[i0:i0 + n], data[i0:i0 + n], lengths[i0:i0 + n])
      self._jpeg_rows = (data, lengths, slot, g)
      if self.avi is not None:
        self._avi_segment(data, lengths, cond_d[:K, 0].contiguous(), sizes)
    if kept is not None:
      self.last_conditioning = {"slot": slot, "frame": g,
                                **{name: torch.cat([b[i] for b in kept]) for i, name in enumerate(("inputs", "fg_inputs", "targets", "Outputs"))}}
    for r in range(K):
      res[int(slot[r])].append((int(g[r]), out[r]))
    return res

  def last_jpeg(self):
    """{slot: [(global frame index, .jpg bytes)]} of the last push's frames (jpeg_quality groups); waits for them."""
    if self.jpeg is None:
      raise RuntimeError("last_jpeg: the group was created without jpeg_quality")
    if self._jpeg_rows is None:
      return {}
    data, lengths, slot, g = self._jpeg_rows
    files = self.jpeg.to_host(data, lengths, self.last_frames)
    res = {}
    for r, f in enumerate(files):
      res.setdefault(int(slot[r]), []).append((int(g[r]), f))
    return res

  def _avi_segment(self, data, lengths, slot_d, sizes):
    """Enqueues the AVI segments of this push: the JPEG rows (or none) and the samples AudioStreamGroup packed, in slot order."""
    pcm = self.audio.last_pcm
    counts = np.zeros(self.slots, np.int32)
    for s, n in sizes.items():
      counts[s] = n
    offsets = (np.cumsum(counts) - counts).astype(np.int32)
    self._avi_seg = self.avi.segment(data, lengths, slot_d, pcm, offsets, counts)

  def last_avi(self):
    """{slot: (the slot's chunks of the last push, their uint32 [n, 4] index entries)} (avi=True groups); waits for them."""
    if self.avi is None:
      raise RuntimeError("last_avi: the group was created without avi=True")
    if self._avi_seg is None:
      return {}
    return self.avi.to_host(self._avi_seg, self.last_frames)

  def record(self, slot, path, **writer_args):
    """Slot `slot`'s pushes from now on go to an AVI file at `path` (write_avi appends, stop closes); writer_args: AviWriter's keywords."""
    from .avi import AviWriter
    if self.avi is None:
      raise RuntimeError("record: the group was created without avi=True")
    slot = int(slot)
    if not 0 <= slot < self.slots:
      raise IndexError("slot %d of %d" % (slot, self.slots))
    if slot in self._writers:
      self.stop(slot)
    writer_args.setdefault("frame_us", 1000000 * SAMPLES_PER_FRAME // self.audio.desc.sample_rate)
    writer_args.setdefault("sample_rate", self.audio.desc.sample_rate)
    self._writers[slot] = AviWriter(path, self.img_size, self.img_size, **writer_args)

  def write_avi(self):
    """last_avi() appended to the writers that are open; returns it."""
    segs = self.last_avi()
    for s, (segment, entries) in segs.items():
      if s in self._writers:
        self._writers[s].append(segment, entries)
    return segs

  def stop(self, slot):
    """Closes slot `slot`'s recording; the paths of its files (more than one when it passed max_bytes), or None when none was open."""
    w = self._writers.pop(int(slot), None)
    if w is None:
      return None
    w.close()
    return w.paths

  def __del__(self):
    try:
      for s in list(getattr(self, "_writers", {})):
        self.stop(s)
    except Exception:
      pass
    Handle.__del__(self)


class PuppetStream:
  """Streaming infer_bfmvid for one talker: a PuppetStreamGroup of one slot.  push(pcm) / finish() -> [(global frame index, uint8 frame
  [H, W, 3] RGB, host array)] of the frames that became exact.  image / bfmcoeff: as PuppetStreamGroup.attach.  BFMNet / PixReferNet
  weights: the checkpoints infer_bfmvid restores (ckpt_bfmnet/bfmnet-65000, ckpt_pixrefer/pixrefernet-20000; TF prefix or .npz), the
  generator from infer_bfmvid's cache.  The group's push only enqueues; this class hands out host-readable frames, so it waits once, at
  the end of a push that emitted frames.  With jpeg_quality=Q the second element of every pair is the bytes of the frame's .jpg file,
  encoded on the device (PuppetStreamGroup), and no raw frame crosses to the host."""

  def __init__(self, config_path, image, bfmcoeff=None, frame_batch=8, max_chunk_frames=1, dtype="f32", img_size=512, jpeg_quality=None,
               pcm_format=None, avi=False):
    """pcm_format=(rate, channels, fmt): the stream also takes client PCM of that form through push_raw (PuppetStreamGroup.push_raw).
    avi=True (with jpeg_quality): as PuppetStreamGroup; record(path) / stop() hold the file, and every push and finish appends to it."""
    self.group = PuppetStreamGroup(config_path, 1, frame_batch=frame_batch, max_chunk_frames=max_chunk_frames, dtype=dtype, img_size=img_size,
                                   jpeg_quality=jpeg_quality, **({'ingest_rates': (pcm_format[0],)} if pcm_format else {}),
                                   **({'avi': True} if avi else {}))
    self.jpeg_quality = jpeg_quality
    self.group.attach(0, image, bfmcoeff, *(pcm_format or ()))
    self.audio = self.group.audio

  @property
  def frame(self):
    return self.group.frame(0)

  def reset(self):
    self.group.reset_slot(0)

  def push(self, pcm):
    return self._host(self.group.push({0: pcm}))

  def push_raw(self, raw):
    return self._host(self.group.push_raw({0: raw}))

  def finish(self):
    if self.group.ingest is not None:       # the resampler's last samples first: one push ends both
      return self._host(self.group.push_raw({}, finish=(0,)))
    return self._host(self.group.push({}, finish=(0,)))

  def record(self, path, **writer_args):
    self.group.record(0, path, **writer_args)

  def stop(self):
    return self.group.stop(0)

  def _host(self, res):
    if self.group._writers:
      self.group.write_avi()
    if not res[0]:
      return []
    if self.jpeg_quality is not None:      # the device's .jpg bytes in place of host arrays; no raw frame is copied
      return self.group.last_jpeg()[0]
    frames = self.group.last_frames.cpu().numpy()
    return [(g, frames[i]) for i, (g, _) in enumerate(res[0])]

"""Streaming audio-to-face inference (libvp_hip.so: vp_bfmstream_*).

AudioStream takes PCM in chunks of any size and returns each video frame's 64 BFM coefficients as soon as the frame's receptive field
has arrived: the frames infer_bfmvid computes offline for the whole clip (same checkpoint, same ears), with the values of the offline
forward.  The lookahead is the receptive field's right side (right_frames video frames) plus the half frame the log-mel window reaches
past its hop; nothing is approximated.  push / finish never wait on the device (host data is staged through pinned memory).

PuppetStream puts the rest of infer_bfmvid behind it: splice_coeff -> ClipRenderer (the head-sway state carried across pushes) ->
PixReferNet -> uint8 frames, conditioned on the same background and reference panels by global frame index.  It waits for each push's
coefficients (the splice and the sway state are host-side, as in infer_bfmvid).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import BfmStreamDesc, BfmStreamGroupDesc
from .audio import bfmnet_manifest

SAMPLES_PER_FRAME = 640          # 16 kHz / 25 frames per second (config/params.yml)


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


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


def _write_params(arena, manifest, params):
  """The named arrays of `params` into their places of the device parameter arena (names it does not hold are left as they are)."""
  host = arena.cpu().numpy()
  for name, off, shape in manifest:
    if name in params:
      v = np.asarray(params[name], dtype=np.float32)
      assert v.shape == shape, (name, v.shape, shape)
      host[off:off + v.size] = v.reshape(-1)
  arena.copy_(torch.from_numpy(host))


def _lookahead_ms(right_mel, sample_rate):
  return 1000.0 * (right_mel * 128 + (512 - 128)) / sample_rate


class AudioStream:
  """One streaming session of BFMNet inference.

  push(pcm) / finish() return [k, 64] f32 device tensors, k = ready(len(pcm)) / ready_finish(); finish zero-pads the clip the way
  prepare_pcm does (pad_len = 1 + N // 640 frames in all).  ears: [k, 1] per call, or None to draw np.random.rand(k, 1) / 100 (numpy's
  legacy generator: consecutive draws are the offline single draw of pad_len, so a seeded run gets infer_bfmvid's ears)."""

  def __init__(self, params=None, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
    if not torch.cuda.is_available():
      raise RuntimeError("AudioStream needs an MI355X (no CPU fallback)")
    self.L = _lib.lib()
    self.desc = stream_desc(max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz)
    d = ctypes.byref(self.desc)
    ws = self.L.vp_bfmstream_workspace_bytes(d)
    if ws == 0:
      raise ValueError("invalid stream descriptor")
    self.left_mel, self.right_mel, self.left_frames, self.right_frames, self.window_frames = stream_context(self.desc)
    self.manifest = bfmnet_manifest()
    self.params = torch.zeros(self.L.vp_bfmnet_param_count(), dtype=torch.float32, device="cuda")
    self.workspace = torch.zeros(ws, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    _lib.check(self.L.vp_bfmstream_create(d, _ptr(self.workspace), ws, _ptr(self.params), _stream(), ctypes.byref(h)), "vp_bfmstream_create")
    self.h = h
    self.samples = 0
    if params is not None:
      self.load_params(load_bfmnet_params(params) if isinstance(params, str) else params)

  @property
  def lookahead_ms(self):
    """Audio that must arrive after a frame's own 40 ms before the frame is emitted: its right context in mel rows plus the part of
    the last mel window past its hop."""
    return _lookahead_ms(self.right_mel, self.desc.sample_rate)

  def load_params(self, params):
    _write_params(self.params, self.manifest, params)
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
    _lib.check(self.L.vp_bfmstream_push(self.h, _ptr(pcm), n, _ptr(e), _ptr(out if k else None), _stream()), "vp_bfmstream_push")
    self.samples += n
    return out

  def finish(self, ears=None):
    k = self.ready_finish()
    out = torch.empty(k, 64, dtype=torch.float32, device="cuda")
    e = self._ears(k, ears)
    _lib.check(self.L.vp_bfmstream_finish(self.h, _ptr(e), _ptr(out), _stream()), "vp_bfmstream_finish")
    return out

  def reset(self):
    _lib.check(self.L.vp_bfmstream_reset(self.h, _stream()), "vp_bfmstream_reset")
    self.samples = 0

  def mel_history(self):
    """The device mel history: [rows, num_mel_bins]; mel frame r of the clip sits at row r % rows while it is kept."""
    p = ctypes.c_void_p()
    shp = (ctypes.c_int64 * 4)()
    _lib.check(self.L.vp_bfmstream_tensor(self.h, b"mel", ctypes.byref(p), shp), "vp_bfmstream_tensor")
    rows, nmel = int(shp[0]), int(shp[1])
    off = p.value - self.workspace.data_ptr()
    return self.workspace[off:off + 4 * rows * nmel].view(torch.float32).view(rows, nmel)

  def __del__(self):
    try:
      if getattr(self, "h", None):
        self.L.vp_bfmstream_destroy(self.h)
        self.h = None
    except Exception:
      pass


def group_desc(slots, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
  return BfmStreamGroupDesc(ctypes.sizeof(BfmStreamGroupDesc), slots, max_chunk_frames, num_mel_bins,
                            {"f32": _lib.VP_F32, "bf16": _lib.VP_BF16}[dtype], sample_rate, lower_hz, upper_hz)


class AudioStreamGroup:
  """`slots` independent AudioStream sessions behind one handle (libvp_hip.so: vp_bfmstream_group_*), for serving many talkers at once.

  One push advances any subset of the slots by any number of samples each and runs one kernel chain per round for all of them.  Every
  slot's coefficients are bit-identical to an AudioStream with the same max_chunk_frames and dtype fed the same chunks (finish: the
  chunk, then AudioStream.finish).  ears: {slot: [k, 1]} per push, or None to draw np.random.rand(k, 1) / 100 per slot in slot order."""

  def __init__(self, params=None, slots=1, max_chunk_frames=1, dtype="f32", num_mel_bins=80, sample_rate=16000, lower_hz=80.0, upper_hz=7600.0):
    if not torch.cuda.is_available():
      raise RuntimeError("AudioStreamGroup needs an MI355X (no CPU fallback)")
    self.L = _lib.lib()
    self.slots = int(slots)
    self.desc = group_desc(self.slots, max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz)
    d = ctypes.byref(self.desc)
    ws = self.L.vp_bfmstream_group_workspace_bytes(d)
    if ws == 0:
      raise ValueError("invalid stream group descriptor: " + self.L.vp_last_error().decode())
    self.left_mel, self.right_mel, self.left_frames, self.right_frames, self.window_frames = stream_context(
        stream_desc(max_chunk_frames, dtype, num_mel_bins, sample_rate, lower_hz, upper_hz))
    self.manifest = bfmnet_manifest()
    self.params = torch.zeros(self.L.vp_bfmnet_param_count(), dtype=torch.float32, device="cuda")
    self.workspace = torch.zeros(ws, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    _lib.check(self.L.vp_bfmstream_group_create(d, _ptr(self.workspace), ws, _ptr(self.params), _stream(), ctypes.byref(h)),
               "vp_bfmstream_group_create")
    self.h = h
    if params is not None:
      self.load_params(load_bfmnet_params(params) if isinstance(params, str) else params)

  @property
  def lookahead_ms(self):
    """As AudioStream.lookahead_ms (the same for every slot)."""
    return _lookahead_ms(self.right_mel, self.desc.sample_rate)

  def load_params(self, params):
    _write_params(self.params, self.manifest, params)
    _lib.check(self.L.vp_bfmstream_group_params_changed(self.h), "vp_bfmstream_group_params_changed")

  def _arrays(self, n_by_slot, finish_by_slot):
    n = (ctypes.c_longlong * self.slots)()
    fin = (ctypes.c_int * self.slots)()
    items = n_by_slot.items() if isinstance(n_by_slot, dict) else enumerate(n_by_slot or ())
    for s, v in items:
      n[int(s)] = int(v)
    for s in finish_by_slot or ():
      fin[int(s)] = 1
    return n, fin

  def ready(self, n_by_slot, finish_by_slot=()):
    """Frames per slot (a list of `slots` counts) that a push of n_by_slot ({slot: samples} or a sequence) new samples emits, the slots
    in finish_by_slot ending their clips after them.  Host only."""
    n, fin = self._arrays(n_by_slot, finish_by_slot)
    k = (ctypes.c_int * self.slots)()
    if self.L.vp_bfmstream_group_ready(self.h, n, fin, k) < 0:
      raise ValueError("bad ready query (negative count, or samples / finish for a finished slot)")
    return list(k)

  def push(self, pcm_by_slot, finish=(), ears=None):
    """{slot: 1-D f32 pcm (numpy or tensor)} -> {slot: coefficients [k, 64]} for every slot pushed or finished.  Enqueues only: the
    tensors are ready when the current stream reaches them."""
    slots = sorted(set(int(s) for s in pcm_by_slot) | set(int(s) for s in finish))
    for s in slots:
      if not 0 <= s < self.slots:
        raise IndexError("slot %d of %d" % (s, self.slots))
    chunks = {int(s): v for s, v in pcm_by_slot.items()}
    sizes = {s: (int(chunks[s].numel()) if torch.is_tensor(chunks[s]) else int(np.asarray(chunks[s]).size)) if s in chunks else 0 for s in slots}
    k = self.ready(sizes, finish)
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
    K = sum(k)
    out = torch.empty(K, 64, dtype=torch.float32, device="cuda")
    e = None
    if K:
      if ears is None:
        e = np.concatenate([np.random.rand(k[s], 1).astype(np.float32) / 100 for s in range(self.slots) if k[s]])
      else:
        e = np.concatenate([np.asarray(ears[s], dtype=np.float32).reshape(k[s], 1) for s in range(self.slots) if k[s]])
      e = AudioStream._to_device(e)
    n, fin = self._arrays(sizes, finish)
    _lib.check(self.L.vp_bfmstream_group_push(self.h, _ptr(pcm), n, fin, _ptr(e), _ptr(out if K else None), _stream()),
               "vp_bfmstream_group_push")
    res, row = {}, 0
    for s in range(self.slots):
      if s in sizes:
        res[s] = out[row:row + k[s]]
      row += k[s]
    return res

  def reset_slot(self, slot):
    """Slot `slot` starts a new clip; the other slots are untouched."""
    _lib.check(self.L.vp_bfmstream_group_reset_slot(self.h, int(slot), _stream()), "vp_bfmstream_group_reset_slot")

  def mel_history(self):
    """The device mel rings: [slots, rows, num_mel_bins]."""
    p = ctypes.c_void_p()
    shp = (ctypes.c_int64 * 4)()
    _lib.check(self.L.vp_bfmstream_group_tensor(self.h, b"mel", ctypes.byref(p), shp), "vp_bfmstream_group_tensor")
    S, rows, nmel = int(shp[0]), int(shp[1]), int(shp[2])
    off = p.value - self.workspace.data_ptr()
    return self.workspace[off:off + 4 * S * rows * nmel].view(torch.float32).view(S, rows, nmel)

  def __del__(self):
    try:
      if getattr(self, "h", None):
        self.L.vp_bfmstream_group_destroy(self.h)
        self.h = None
    except Exception:
      pass


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


class PuppetStream:
  """Streaming infer_bfmvid: push(pcm) / finish() -> [(global frame index, uint8 frame [H, W, 3] RGB)] of the frames that became
  exact.  image: the 512 x 1536 input (RGB float in [0,1], as infer_bfmvid reads it); bfmcoeff: the photo's coefficient npz
  (bfmcoeff, transform_params, center_x, center_y, ratio) - with it and BFM/BFM_model_front.mat every frame is conditioned on its
  rendered face, without them on the reference 3-D face panel.  BFMNet / PixReferNet weights: the checkpoints infer_bfmvid restores
  (ckpt_bfmnet/bfmnet-65000, ckpt_pixrefer/pixrefernet-20000; TF prefix or .npz), the generator from infer_bfmvid's cache."""

  def __init__(self, config_path, image, bfmcoeff=None, frame_batch=8, max_chunk_frames=1, dtype="f32", img_size=512):
    import os
    from .pixrefer import infer_bfmvid as ib
    from .runtime import Session
    self.ib = ib
    bfm_file = next((f for f in (ib.BFMNET_CKPT + '.index', ib.BFMNET_CKPT + '.npz') if os.path.exists(f)), None)
    if bfm_file is None:
      from .bfmnet.bfmnet import random_variables
      ib.logger.warning('%s not found: running with randomly initialised weights', ib.BFMNET_CKPT)
      bfm_params = random_variables()
    else:
      bfm_params = load_bfmnet_params(bfm_file[:-len('.index')] if bfm_file.endswith('.index') else bfm_file)
    self.audio = AudioStream(bfm_params, max_chunk_frames=max_chunk_frames, dtype=dtype)
    self.nb, self.img_size = frame_batch, img_size
    self.net, self.inputs_holder, self.fg_holder, self.targets_holder, self.nodes = ib.load_generator(config_path, frame_batch, img_size)
    self.sess = Session()
    self.photo = None
    if bfmcoeff and os.path.exists(os.path.join('BFM', 'BFM_model_front.mat')):
      self.photo = np.load(bfmcoeff)
      self.renderer = ib.clip_renderer()
    else:
      ib.logger.warning('BFM assets unavailable: conditioning every frame on the reference 3-D face panel')
    face3d_refer = image[:, 512:512 * 2, :]
    fg_refer = image[:, :512, :] * image[:, 512 * 2:, :]
    nb, H = frame_batch, img_size
    self.inputs = torch.zeros([nb, H, H, 6], dtype=torch.float32, device="cuda")
    self.fg_inputs = torch.zeros([nb, H, H, 3], dtype=torch.float32, device="cuda")
    self.targets = torch.full([nb, H, H, 3], 0.5, dtype=torch.float32, device="cuda")
    refer_t = torch.as_tensor(np.ascontiguousarray(face3d_refer, dtype=np.float32)).to("cuda")
    self.inputs[:, ..., 0:3] = refer_t
    self.fg_inputs[:, ..., 0:3] = torch.as_tensor(np.ascontiguousarray(fg_refer, dtype=np.float32)).to("cuda")
    if self.photo is None:
      self.inputs[:, ..., 3:6] = refer_t
    self.sway = HeadSway()
    self.frame = 0

  def reset(self):
    self.audio.reset()
    self.sway.reset()
    self.frame = 0

  def push(self, pcm):
    return self._frames(self.audio.push(pcm))

  def finish(self):
    return self._frames(self.audio.finish())

  def _frames(self, coeff):
    ib, H = self.ib, self.img_size
    k = int(coeff.shape[0])
    if k == 0:
      return []
    g0 = self.frame
    self.frame += k
    angles = self.sway.next(k)
    face3d = None
    if self.photo is not None:
      p = self.photo
      coeff_seq = ib.splice_coeff(p['bfmcoeff'].reshape(1, 257), coeff.cpu().numpy()[np.newaxis])[0]
      face3d = ib.render_faces(self.renderer, int(p['center_x']), int(p['center_y']), float(p['ratio']), coeff_seq, (H, H, 3),
                               p['transform_params'], on_device=True, angles=angles)
    out = []
    for i0 in range(0, k, self.nb):                    # batches of the generator plan, padded with the last frame as infer_bfmvid pads
      idx = [min(i0 + j, k - 1) for j in range(self.nb)]
      if face3d is not None:
        self.inputs[:, ..., 3:6] = face3d[idx].flip(-1).to(torch.float32) / 255.0
      for j, i in enumerate(idx):
        bg = ib.background_target(g0 + i, H)
        if bg is not None:
          self.targets[j] = torch.as_tensor(bg).to("cuda")
        else:
          self.targets[j] = 0.5
      frames = self.sess.run([self.nodes['Outputs_u8']],
                             feed_dict={self.inputs_holder: self.inputs, self.fg_holder: self.fg_inputs, self.targets_holder: self.targets})[0]
      out.extend((g0 + i0 + j, frames[j]) for j in range(self.nb) if i0 + j < k)
    return out

"""BFM coefficients from 68 landmarks, on the MI355X (libvp_hip.so: vp_bfmfit_*; csrc/bfm_fit.hip).

The reference obtains a photo's 257 coefficients and the `bfmcoeff.txt` rows BFMNet is trained on from FaceReconModel.pb, a frozen
TensorFlow 1 ResNet (voicepuppet/pixrefer/infer_bfmvid.py:47-74, datasets/make_data_from_GRID.py:193-214).  This module gets identity
(0:80), expression (80:144), angles (224:227) and translation (254:257) from a landmark file instead: it inverts `Reconstruction`
(utils/reconstruct_mesh.py:172-194) for the 68 landmarks that function returns.  Texture (144:224) and lighting (227:254) come from the
photo's pixels (`observe`, `fit_appearance`, `enroll(image=...)`; libvp_hip.so: vp_bfmfit_observe, vp_bfmfit_observe_ex, vp_bfmfit_appearance;
csrc/bfm_appear.hip, csrc/bfm_observe.hip),
with the geometry fixed at the landmark fit's; without a photo they stay at the caller's template, zeros by default, i.e. the mean albedo
under ambient light.

  E(p) = sum_k w_k |pi_k(p) - l_k|^2 + lam_id |alpha|^2 + lam_ex |beta|^2        p = [alpha(80) | beta(64) | angles(3) | t(3)]

minimised per frame by Levenberg-Marquardt in float64, one workgroup per frame (include/vp_hip.h states the rule).
`report` [frames,4] = (status, accepted iterations, final E, final |g|_inf); status 0 converged, 1 max_iters, 2 stalled, 3 non-finite input.

Appearance: p = [delta(80) | gamma(27)], r_vc = T_vc(delta) L_vc(gamma) - I_vc at the vertices, I the photo sampled at their projections,
  E(p) = (1/W) sum_v w_v sum_c r_vc^2 + lam_tex |delta|^2 + lam_gamma |gamma|^2,  W = 3 sum_v w_v,  w_v = mask_v max(0, (n_v . R)_z) inside
by the same rule with a relative stopping test (|g|_inf <= gtol E), as a fixed chain of `max_trials` launch pairs; report as above with
status 1 = max_trials used up, 3 = non-finite input or no visible vertex.  lam_tex = lam_gamma = 1 are untuned on real photos.

`FaceFitter.fit_sequence` is a FIXED SCHEDULE of block-coordinate descent for a clip of one person (per-frame fits, then identity steps
alternating with tracking fits), not a minimiser: it stops after `rounds` rounds whatever the cost does.

`FaceFitter.fit_clip` is the minimiser (vp_bfmfit_clip; csrc/bfm_clip.hip): one Levenberg-Marquardt solve, by the same rule, over a whole
clip's unknowns, alpha (80) and q_t = [beta_t | angles | t] (70) per frame t = 1 .. T:
  E = sum_t ( sum_k w_tk |pi_k(alpha, q_t) - l_tk|^2 + lam_id |alpha|^2 + lam_ex |beta_t|^2 )
    + sum_{t<T} ( s_ex |beta_t+1 - beta_t|^2 + s_ang |ang_t+1 - ang_t|^2 + s_t |t_t+1 - t_t|^2 ),      lam_smooth = (s_ex, s_ang, s_t)
With lam_smooth = (0, 0, 0), the default, E is the sum of the per-frame costs for a shared alpha (T lam_id |alpha|^2 in all, as the identity
step counts it); the coupling terms damp the frame-to-frame jitter a landmark detector leaves in the rows BFMNet's loss differences in
time.  Useful values of lam_smooth are UNTUNED on real landmark files.  A fixed chain of `max_trials` rounds of two launches (the frames'
150x150 systems at the trial point, one workgroup per frame; then one workgroup per clip: accept / reject on the SUM OF THE FRAMES'
DIFFERENCES, a block Cholesky sweep over the block-arrowhead matrix, the next trial point).  report [clips,4] = (status, accepted steps,
final E, final |g|_inf over all 80 + 70 T unknowns); status 1 = max_trials trial points used up.

The alignment helpers (`crop_alignment`, `preprocess_landmarks`) are plain numpy float64 and do no device work.  No CPU fallback for the fit.
"""
import ctypes

import numpy as np

from . import _lib
from ._handle import grow, ptr, stream

NP = 150
NA = 107                                                    # appearance unknowns: texture 80 | lighting 27
FREE_ID, FREE_EX, FREE_ANGLES, FREE_T = 1, 2, 4, 8
FREE = {"all": 15, "tracking": FREE_EX | FREE_ANGLES | FREE_T, "pose": FREE_ANGLES | FREE_T}


def _free_mask(free):
  if isinstance(free, str):
    if free not in FREE:
      raise ValueError("free must be one of %s or a bit mask 1 .. 15" % sorted(FREE))
    return FREE[free]
  free = int(free)
  if not 1 <= free <= 15:
    raise ValueError("free must be one of %s or a bit mask 1 .. 15" % sorted(FREE))
  return free


def five_points(lm):
  """The five points load_lm3d takes from 68 (utils/bfm_load_data.py:122-127): eye centres (means of the two corners), nose tip, mouth corners."""
  lm = np.asarray(lm, np.float64)
  idx = np.array([31, 37, 40, 43, 46, 49, 55]) - 1
  five = np.stack([lm[idx[0]], np.mean(lm[idx[[1, 2]]], 0), np.mean(lm[idx[[3, 4]]], 0), lm[idx[5]], lm[idx[6]]], axis=0)
  return five[[1, 2, 0, 3, 4]]


def _crop_box(landmarks_xy, img_h, img_w, ratio=1.3):
  """crop_expand_alignment's square (utils/utils.py:78-104): (xy [68,2], center_x, center_y, left, top, width)."""
  xy = np.array(landmarks_xy, np.float64).reshape(-1, 2)
  max_x, max_y = xy[:, 0].max(), xy[:, 1].max()
  min_x, min_y = xy[:, 0].min(), xy[:, 1].min()
  center_x = int(round((max_x + min_x) / 2))
  center_y = int(round((max_y + min_y) / 2))
  width = max_x - min_x
  height = width                                                                                  # :87-89
  if not width > 0:
    raise ValueError("crop_alignment: the landmarks have no extent in x")
  max_ratio = min([(img_h - center_y) / (height / 2), (img_w - center_x) / (width / 2), center_y / (height / 2), center_x / (width / 2)])
  if max_ratio < ratio:
    ratio = max_ratio
  width = int((max_x - min_x) * ratio)
  height = width
  if width < 1:
    raise ValueError("crop_alignment: the landmarks' centre lies outside the %d x %d image" % (img_w, img_h))
  left = int(round(center_x - width / 2))
  top = int(round(center_y - height / 2))
  return xy, center_x, center_y, left, top, width


def crop_alignment(landmarks_xy, img_h, img_w, out_img_size=224, ratio=1.3):
  """The landmark arithmetic of crop_expand_alignment (utils/utils.py:78-110): the square crop around the landmarks' bounding box, expanded
  by `ratio` (less where the image ends), resized to out_img_size.  landmarks_xy [68,2] image pixels -> (landmarks in the crop [68,2],
  center_x, center_y, ratio = out_img_size / crop width)."""
  xy, center_x, center_y, left, top, width = _crop_box(landmarks_xy, img_h, img_w, ratio)
  height = width
  out = np.stack([(xy[:, 0] - left) * out_img_size / width, (xy[:, 1] - top) * out_img_size / height], axis=1)
  return out, center_x, center_y, float(out_img_size) / width


def preprocess_landmarks(lm, lm3D, w0=224, h0=224):
  """The landmark half of Preprocess / POS / process_img (utils/bfm_load_data.py:148-212).  lm [68,2] in the w0 x h0 crop; lm3D the
  standard landmarks, [68,3] (BFM/similarity_Lm3D_all.mat's `lm`) or the five points load_lm3d returns.  The five points of both are
  load_lm3d's (:122-127).  Returns (lm_new [68,2]: all 68 in the 224 image the network would have seen, trans_params [5] =
  (w0, h0, 102 / s, t0 - w0/2, h0/2 - t1))."""
  lm, s, t0, t1, w, h = _similarity(lm, lm3D, w0, h0)
  flip = np.stack([lm[:, 0], h0 - 1 - lm[:, 1]], axis=1)                                          # :201
  new = np.stack([flip[:, 0] - t0 + w0 / 2, flip[:, 1] - t1 + h0 / 2], axis=1) / s * 102          # :179
  new = new - np.array([w / 2 - 112, h / 2 - 112]).reshape(1, 2)                                  # :191
  lm_new = np.stack([new[:, 0], 223 - new[:, 1]], axis=1)                                         # :209
  return lm_new, np.array([w0, h0, 102.0 / s, t0 - w0 / 2, h0 / 2 - t1], np.float64)


def _similarity(lm, lm3D, w0=224, h0=224):
  """POS (utils/bfm_load_data.py:148-170) on the five points and process_img's image size (:176-177): (lm [68,2], s, t0, t1, w, h)."""
  lm = np.asarray(lm, np.float64).reshape(68, 2)
  lm3D = np.asarray(lm3D, np.float64)
  x = five_points(lm3D) if lm3D.shape[0] == 68 else lm3D.reshape(5, 3)
  flip = np.stack([lm[:, 0], h0 - 1 - lm[:, 1]], axis=1)                                          # :201
  xp = five_points(flip)
  A = np.zeros([10, 8])                                                                           # POS :148-170
  A[0::2, 0:3] = x
  A[0::2, 3] = 1
  A[1::2, 4:7] = x
  A[1::2, 7] = 1
  k = np.linalg.lstsq(A, xp.reshape(10), rcond=None)[0]
  s = (np.linalg.norm(k[0:3]) + np.linalg.norm(k[4:7])) / 2
  t0, t1 = k[3], k[7]
  w = np.int32(w0 / s * 102)                                                                      # process_img :176-177
  h = np.int32(h0 / s * 102)
  return lm, s, t0, t1, w, h


def photo_affine(landmarks_xy, img_h, img_w, lm3D):
  """The inverse of preprocess_landmarks o crop_alignment as an affine map, float64: (a, bx, by) with photo (x, y) = (a u + bx, a v + by)
  for a point (u, v) of the 224 image the fit works in (face_projection's pixels).  One uniform scale: the crop is square and both resizes
  are isotropic.  Forward, from the two functions: c = (xy - (left, top)) 224 / width;  u = (c_x - t0 + 112) k - (w/2 - 112),
  v = 223 - ((223 - c_y - t1 + 112) k - (h/2 - 112)),  k = 102 / s (two y flips).  Solved for xy:
    a = width / (224 k);  bx = left + ((w/2 - 112) / k + t0 - 112) width / 224;  by = top + (335 - t1 - (111 + h/2) / k) width / 224."""
  xy, _, _, left, top, width = _crop_box(landmarks_xy, img_h, img_w)
  crop = np.stack([(xy[:, 0] - left) * 224 / width, (xy[:, 1] - top) * 224 / width], axis=1)
  _, s, t0, t1, w, h = _similarity(crop, lm3D)
  k = 102.0 / s
  g = width / 224.0
  return np.array([g / k, left + ((w / 2 - 112) / k + t0 - 112) * g, top + (335 - t1 - (111 + h / 2) / k) * g], np.float64)


def params_of(coeff):
  """[...,257] -> p [...,150]."""
  return np.concatenate([coeff[..., :144], coeff[..., 224:227], coeff[..., 254:257]], axis=-1)


class FaceFitter:
  """fit / fit_sequence / enroll against one face model.  `facemodel`: the reference's BFM object (utils/bfm_load_data.py:9-21) or a
  voicepuppet_amd.utils.reconstruct_mesh.DeviceFaceModel (reused as it is)."""

  def __init__(self, facemodel):
    import torch
    from .utils.reconstruct_mesh import DeviceFaceModel
    self.model = facemodel if isinstance(facemodel, DeviceFaceModel) else DeviceFaceModel(facemodel)
    kp = np.ascontiguousarray(np.asarray(self.model.keypoints).reshape(-1), np.int32)
    if kp.shape != (68,):
      raise ValueError("facemodel.keypoints must hold 68 vertex indices")
    self._kp = kp                                           # host array: the library checks it before it launches anything
    self._ws = None
    self._table_ready = False
    self.last_params = None                                 # float64 [frames,150] of the last call
    self._ws_obs = self._ws_app = self._ws_clip = None
    self._clip_table_ready = False
    self.last_appearance = None                             # float64 [frames,107] of the last fit_appearance
    self.last_appearance_report = None                      # enroll(image=...): fit_appearance's report [1,4]
    self.last_appearance_lams = None                        # (lam_tex, lam_gamma) of the last fit_appearance
    self._torch = torch

  def _workspace(self, frames):
    n = _lib.lib().vp_bfmfit_workspace_bytes(frames)
    ws = grow(self._ws, n, self.model.device)
    if ws is not self._ws:
      self._ws = ws
      self._table_ready = False                             # the gathered keypoint table lives at the head of the workspace
    return self._ws

  def _device(self, a, dtype, shape, what):
    torch = self._torch
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = t.to(device=self.model.device, dtype=dtype).contiguous()
    if tuple(t.shape) != tuple(shape):
      raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    return t

  def _weights(self, weights, T):
    if weights is None:
      return None, 0
    if not isinstance(weights, np.ndarray) and not self._torch.is_tensor(weights):
      weights = np.asarray(weights, np.float64)
    n = int(np.prod(tuple(weights.shape)))
    if n == 68:
      return self._device(weights, self._torch.float64, tuple(weights.shape), "weights").reshape(68), 0
    return self._device(weights, self._torch.float64, (T, 68), "weights"), 1

  def fit(self, landmarks, weights=None, init=None, free="all", lam_id=1.0, lam_ex=1.0, gtol=1e-6, max_iters=100, params=None):
    """landmarks [frames,68,2] pixels of the 224 image (float64; numpy or device); weights None, [68] or [frames,68]; init [frames,257]
    float32 start values and template (zeros by default).  Returns (coeff [frames,257] float32, report [frames,4] float64), device tensors;
    the call only enqueues.  `params` [frames,150] float64 device tensor: start from these float64 values instead of init's.  The float64
    solution is kept in `self.last_params`."""
    torch, dev = self._torch, self.model.device
    if not isinstance(landmarks, np.ndarray) and not torch.is_tensor(landmarks):
      landmarks = np.asarray(landmarks, np.float64)
    if landmarks.ndim == 2:
      landmarks = landmarks.reshape(1, 68, 2)
    T = int(landmarks.shape[0])
    if T < 1:
      raise ValueError("fit: at least one frame")
    lm = self._device(landmarks, torch.float64, (T, 68, 2), "landmarks")
    w, per_frame = self._weights(weights, T)
    tmpl = torch.zeros(T, 257, dtype=torch.float32, device=dev) if init is None else self._device(init, torch.float32, (T, 257), "init")
    params_in = params is not None
    p = self._device(params, torch.float64, (T, NP), "params").clone() if params_in else torch.empty(T, NP, dtype=torch.float64, device=dev)
    coeff = torch.empty(T, 257, dtype=torch.float32, device=dev)
    report = torch.empty(T, 4, dtype=torch.float64, device=dev)
    ws = self._workspace(T)
    P = ctypes.c_void_p
    _lib.check(_lib.lib().vp_bfmfit_fit(ctypes.byref(self.model.c), self._kp.ctypes.data_as(P), 1 if self._table_ready else 0, ptr(lm), ptr(w),
                                        per_frame, ptr(tmpl), ptr(p), 1 if params_in else 0, T, float(lam_id), float(lam_ex), float(gtol),
                                        int(max_iters), _free_mask(free), ptr(coeff), ptr(report), ptr(ws), ws.numel(), stream()), "vp_bfmfit_fit")
    self._table_ready = True
    self.last_params = p
    return coeff, report

  def identity_step(self, landmarks, params, coeff=None, weights=None, lam_id=1.0):
    """One Gauss-Newton step on the alpha all frames share (vp_bfmfit_identity_step), beta and pose fixed: `params` [frames,150] float64
    (and `coeff` [frames,257] float32, when given) get the new alpha in every row, in place.  Enqueues only."""
    torch = self._torch
    T = int(params.shape[0])
    lm = self._device(landmarks, torch.float64, (T, 68, 2), "landmarks")
    w, per_frame = self._weights(weights, T)
    for t, dt, shp in ((params, torch.float64, (T, NP)),) + (((coeff, torch.float32, (T, 257)),) if coeff is not None else ()):
      if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shp):
        raise ValueError("identity_step: contiguous device tensors params float64 [frames,150] / coeff float32 [frames,257]")
    ws = self._workspace(T)
    P = ctypes.c_void_p
    _lib.check(_lib.lib().vp_bfmfit_identity_step(ctypes.byref(self.model.c), self._kp.ctypes.data_as(P), 1 if self._table_ready else 0,
                                                  ptr(lm), ptr(w), per_frame, ptr(params), ptr(coeff), T, float(lam_id), ptr(ws), ws.numel(),
                                                  stream()), "vp_bfmfit_identity_step")
    self._table_ready = True
    return params

  def fit_sequence(self, landmarks, rounds=3, id_steps=3, weights=None, lam_id=1.0, lam_ex=1.0, gtol=1e-6, max_iters=100):
    """A clip of ONE person: a full fit of every frame from zeros; alpha <- the mean of the per-frame identities; then `rounds` times
    (`id_steps` identity steps, then a tracking fit of every frame from its previous values).  A fixed schedule, not a minimiser:
    block-coordinate descent converges slowly, and the cost may still be falling when it ends.  Returns (coeff, report) of the last
    tracking fit (of the first fit when rounds = 0); enqueues only."""
    torch = self._torch
    if not isinstance(landmarks, np.ndarray) and not torch.is_tensor(landmarks):
      landmarks = np.asarray(landmarks, np.float64)
    T = int(landmarks.shape[0])
    lm = self._device(landmarks, torch.float64, (T, 68, 2), "landmarks")
    if weights is not None and not isinstance(weights, np.ndarray) and not torch.is_tensor(weights):
      weights = np.asarray(weights, np.float64)
    kw = dict(weights=weights, lam_id=lam_id, lam_ex=lam_ex, gtol=gtol, max_iters=max_iters)
    coeff, report = self.fit(lm, free="all", **kw)
    p = self.last_params
    alpha = p[:, :80].mean(dim=0, keepdim=True)
    p[:, :80] = alpha
    coeff[:, :80] = alpha.to(torch.float32)
    for _ in range(int(rounds)):
      for _ in range(int(id_steps)):
        self.identity_step(lm, p, coeff, weights=weights, lam_id=lam_id)
      coeff, report = self.fit(lm, init=coeff, params=p, free="tracking", **kw)
      p = self.last_params
    return coeff, report

  def fit_clip(self, landmarks, clip_lengths=None, init=None, params=None, weights=None, lam_id=1.0, lam_ex=1.0, lam_smooth=(0, 0, 0), gtol=1e-6,
               max_trials=64):
    """The joint fit of whole clips (vp_bfmfit_clip; the module docstring states the energy): ONE identity per clip, expression and pose per
    frame, `lam_smooth` = (s_ex, s_ang, s_t) weighting the squared frame-to-frame differences of expression, angles and translation.  The
    weights default to 0 (no coupling); their useful values are UNTUNED on real landmark files.  landmarks [frames,68,2]; clip_lengths: the
    frame counts of the clips, in order (default: one clip); init [frames,257] float32 template; params [frames,150] float64 start values
    (a clip's alpha is its first row's).  Without `params` the start is what fit_sequence(rounds=0) gives each clip: a full fit of every
    frame from `init`, alpha set to the clip's mean.  Returns (coeff [frames,257] float32, report [clips,4] float64 = status, accepted
    steps, final E, final |g|_inf over all 80 + 70 T unknowns), device tensors; status 0 converged, 1 `max_trials` trial points used up,
    2 stalled, 3 non-finite input.  A fixed chain of `max_trials` rounds; the call only enqueues.  The float64 solution is kept in
    `self.last_params`."""
    torch, dev = self._torch, self.model.device
    if not isinstance(landmarks, np.ndarray) and not torch.is_tensor(landmarks):
      landmarks = np.asarray(landmarks, np.float64)
    F = int(landmarks.shape[0])
    if F < 1:
      raise ValueError("fit_clip: at least one frame")
    lengths = [F] if clip_lengths is None else [int(n) for n in clip_lengths]
    if not lengths or min(lengths) < 1 or sum(lengths) != F:
      raise ValueError("fit_clip: clip_lengths must be positive and add up to the %d frames" % F)
    smooth = np.asarray(lam_smooth, np.float64).reshape(-1)
    if smooth.shape != (3,) or not np.all(np.isfinite(smooth)) or np.any(smooth < 0):
      raise ValueError("fit_clip: lam_smooth must be three non-negative numbers (expression, angles, translation)")
    smooth = np.ascontiguousarray(smooth)
    offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lengths)]), np.int32)
    lm = self._device(landmarks, torch.float64, (F, 68, 2), "landmarks")
    if weights is not None and not isinstance(weights, np.ndarray) and not torch.is_tensor(weights):
      weights = np.asarray(weights, np.float64)
    w, per_frame = self._weights(weights, F)
    tmpl = torch.zeros(F, 257, dtype=torch.float32, device=dev) if init is None else self._device(init, torch.float32, (F, 257), "init")
    if params is not None:
      p = self._device(params, torch.float64, (F, NP), "params").clone()
    else:
      self.fit(lm, weights=weights, init=tmpl, free="all", lam_id=lam_id, lam_ex=lam_ex)
      p = self.last_params
      for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        p[a:b, :80] = p[a:b, :80].mean(dim=0, keepdim=True)
    coeff = torch.empty(F, 257, dtype=torch.float32, device=dev)
    report = torch.empty(len(lengths), 4, dtype=torch.float64, device=dev)
    n = _lib.lib().vp_bfmfit_clip_workspace_bytes(F, len(lengths))
    ws = grow(self._ws_clip, n, dev)
    if ws is not self._ws_clip:
      self._ws_clip = ws
      self._clip_table_ready = False                        # the gathered keypoint table lives at the head of this workspace too
    P = ctypes.c_void_p
    _lib.check(_lib.lib().vp_bfmfit_clip(ctypes.byref(self.model.c), self._kp.ctypes.data_as(P), 1 if self._clip_table_ready else 0, ptr(lm), ptr(w),
                                         per_frame, offsets.ctypes.data_as(P), len(lengths), ptr(tmpl), ptr(p), float(lam_id), float(lam_ex),
                                         smooth.ctypes.data_as(P), float(gtol), int(max_trials), ptr(coeff), ptr(report), ptr(ws), ws.numel(),
                                         stream()), "vp_bfmfit_clip")
    self._clip_table_ready = True
    self.last_params = p
    return coeff, report

  def _photo(self, photo, T):
    torch = self._torch
    t = torch.from_numpy(np.ascontiguousarray(photo)) if isinstance(photo, np.ndarray) else photo
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or (t.dim() == 4 and t.shape[0] not in (1, T)):
      raise ValueError("photo must be uint8 RGB [H,W,3] or [frames,H,W,3]")
    t = t.to(self.model.device).contiguous()
    return t, (1 if t.dim() == 3 else int(t.shape[0])), int(t.shape[-3]), int(t.shape[-2])

  def observe(self, coeff, photo, affine, vertex_weights=None, visibility=False, prefilter=False, raster_scale=2, depth_tol=0.01,
              return_visible=False):
    """What the photo shows at the vertices of Reconstruction(coeff) (vp_bfmfit_observe).  coeff [frames,257] float32; photo [H,W,3] (shared)
    or [frames,H,W,3] uint8 RGB; affine [3] or [frames,3] float64 (a, bx, by), 224-image pixels -> photo pixels (`photo_affine`);
    vertex_weights None or [N] float64 (a skin mask).  Returns device float64 (sh [frames,N,9], weight [frames,N], observed [frames,N,3]):
    the SH terms of the rotated normals, mask x max(0, (n . R)_z) x inside, and the bilinear samples.  The rotation matrices are made on
    the host from coeff's angles, as reconstruct_view makes them (a device coeff is read back for that); everything else only enqueues.
    Two options, both off by default (the call is then vp_bfmfit_observe, as it always was; with either on, vp_bfmfit_observe_ex):
      visibility  self-occlusion: the fitted mesh is rasterised into a depth buffer of (224 raster_scale)^2 pixels (raster_scale 1, 2 or 4)
                  and a vertex that lies more than depth_tol behind the surface drawn around it gets weight 0
                  (mesh_core.vertex_visibility states the rule).  depth_tol is in model units, decimetres: 0.01 = 1 mm is a default, not
                  a tuned value.
      prefilter   a frame whose a exceeds 1 is observed as the mean of k x k bilinear taps spread over the a x a photo pixels a pixel of
                  the 224 image covers, k = min(ceil(a), 16); frames with a <= 1 keep their single tap.
    return_visible: a fourth result, the 0 / 1 mask uint8 [frames,N] (needs visibility)."""
    torch, dev = self._torch, self.model.device
    from .utils.reconstruct_mesh import Compute_rotation_matrix
    c = (torch.from_numpy(np.ascontiguousarray(coeff, np.float32)) if isinstance(coeff, np.ndarray) else coeff).to(dev).contiguous()
    if c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != 257 or c.shape[0] < 1:
      raise ValueError("coeff must be float32 [frames,257]")
    T, N = int(c.shape[0]), self.model.nver
    angles = coeff[:, 224:227] if isinstance(coeff, np.ndarray) else c[:, 224:227].cpu().numpy()
    rot = torch.from_numpy(Compute_rotation_matrix(np.asarray(angles, np.float32))).to(dev)
    img, photo_frames, H, W = self._photo(photo, T)
    if not isinstance(affine, np.ndarray) and not torch.is_tensor(affine):
      affine = np.asarray(affine, np.float64)
    if affine.ndim == 1:
      affine = (torch.from_numpy(np.tile(affine, (T, 1))) if isinstance(affine, np.ndarray) else affine.reshape(1, 3).repeat(T, 1))
    aff = self._device(affine, torch.float64, (T, 3), "affine")
    vw = None if vertex_weights is None else self._device(vertex_weights, torch.float64, (N,), "vertex_weights")
    sh = torch.empty(T, N, 9, dtype=torch.float64, device=dev)
    weight = torch.empty(T, N, dtype=torch.float64, device=dev)
    observed = torch.empty(T, N, 3, dtype=torch.float64, device=dev)
    if return_visible and not visibility:
      raise ValueError("observe: return_visible needs visibility=True")
    if not (visibility or prefilter):
      n = _lib.lib().vp_bfmfit_observe_workspace_bytes(N, self.model.ntri, T)
      self._ws_obs = grow(self._ws_obs, n, dev)
      _lib.check(_lib.lib().vp_bfmfit_observe(ctypes.byref(self.model.c), ptr(c), ptr(rot), T, ptr(img), photo_frames, H, W, ptr(aff), ptr(vw),
                                              ptr(sh), ptr(weight), ptr(observed), ptr(self._ws_obs), self._ws_obs.numel(), stream()),
                 "vp_bfmfit_observe")
      return sh, weight, observed
    opts = _lib.BfmObserveOpts(ctypes.sizeof(_lib.BfmObserveOpts), 1 if visibility else 0, int(raster_scale), 1 if prefilter else 0, float(depth_tol))
    n = _lib.lib().vp_bfmfit_observe_ex_workspace_bytes(N, self.model.ntri, T, ctypes.byref(opts))
    if n == 0:
      raise ValueError("observe: %s" % _lib.lib().vp_last_error().decode())
    self._ws_obs = grow(self._ws_obs, n, dev)
    visible = torch.empty(T, N, dtype=torch.uint8, device=dev) if return_visible else None
    _lib.check(_lib.lib().vp_bfmfit_observe_ex(ctypes.byref(self.model.c), ptr(c), ptr(rot), T, ptr(img), photo_frames, H, W, ptr(aff), ptr(vw),
                                               ptr(sh), ptr(weight), ptr(observed), ptr(self._ws_obs), self._ws_obs.numel(), stream(),
                                               ctypes.byref(opts), ptr(visible)), "vp_bfmfit_observe_ex")
    return (sh, weight, observed, visible) if return_visible else (sh, weight, observed)

  def fit_appearance(self, coeff, photo=None, affine=None, observation=None, vertex_weights=None, init=None, params=None, lam_tex=1.0,
                     lam_gamma=1.0, gtol=1e-6, max_trials=32, _stages=3, visibility=False, prefilter=False):
    """Texture and lighting of coeff [frames,257] float32 (the landmark fit's output: its geometry is kept) from the photo's pixels
    (vp_bfmfit_appearance).  Either photo + affine (see `observe`; `visibility` and `prefilter` are passed on to it, with its defaults for
    raster_scale and depth_tol) or a ready observation = (sh, weight, observed).  init [frames,257]:
    start values of columns 144:224 and 227:254 (default: coeff's own); params [frames,107] float64: start from these instead.  Returns
    (coeff [frames,257] float32 with those columns fitted and every other column coeff's, report [frames,4] float64), device tensors; the
    float64 solution is kept in `self.last_appearance`.  A fixed chain of `max_trials` rounds; the call only enqueues.  `_stages` is for
    timing only (scripts/bfm_appearance_latency.py): 1 / 2 enqueue only the accumulate / only the step launches, and what is returned is then
    undefined."""
    torch, dev = self._torch, self.model.device
    if (observation is None) == (photo is None) or (photo is not None and affine is None):
      raise ValueError("fit_appearance: either photo and affine, or observation = (sh, weight, observed)")
    c = (torch.from_numpy(np.ascontiguousarray(coeff, np.float32)) if isinstance(coeff, np.ndarray) else coeff).to(dev).contiguous()
    if c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != 257 or c.shape[0] < 1:
      raise ValueError("coeff must be float32 [frames,257]")
    T, N = int(c.shape[0]), self.model.nver
    if observation is None:
      observation = self.observe(coeff, photo, affine, vertex_weights, visibility=visibility, prefilter=prefilter)
    sh, weight, observed = observation
    sh = self._device(sh, torch.float64, (T, N, 9), "sh")
    weight = self._device(weight, torch.float64, (T, N), "weight")
    observed = self._device(observed, torch.float64, (T, N, 3), "observed")
    tmpl = c
    if init is not None:
      start = self._device(init, torch.float32, (T, 257), "init")
      tmpl = c.clone()
      tmpl[:, 144:224], tmpl[:, 227:254] = start[:, 144:224], start[:, 227:254]
    params_in = params is not None
    p = self._device(params, torch.float64, (T, NA), "params").clone() if params_in else torch.empty(T, NA, dtype=torch.float64, device=dev)
    out = torch.empty(T, 257, dtype=torch.float32, device=dev)
    report = torch.empty(T, 4, dtype=torch.float64, device=dev)
    n = _lib.lib().vp_bfmfit_appearance_workspace_bytes(N, T)
    self._ws_app = grow(self._ws_app, n, dev)
    _lib.check(_lib.lib().vp_bfmfit_appearance(ctypes.byref(self.model.c), ptr(sh), ptr(weight), ptr(observed), ptr(tmpl), ptr(p),
                                               1 if params_in else 0, T, float(lam_tex), float(lam_gamma), float(gtol), int(max_trials),
                                               int(_stages), ptr(out), ptr(report), ptr(self._ws_app), self._ws_app.numel(), stream()),
               "vp_bfmfit_appearance")
    self.last_appearance, self.last_appearance_lams = p, (float(lam_tex), float(lam_gamma))
    return out, report

  def enroll(self, landmarks_xy, img_h, img_w, lm3D, image=None, lam_tex=1.0, lam_gamma=1.0, visibility=False, prefilter=False,
             **fit_args):
    """A photo's landmarks [68,2] (image pixels) -> the dictionary infer_bfmvid.py --bfmcoeff reads (np.savez(path, **d)): bfmcoeff [1,257]
    float32, transform_params [5], center_x, center_y, ratio.  crop_alignment, preprocess_landmarks and one full fit; the fit's report
    [1,4] (device) and the landmarks it was given [68,2] stay in `self.last_report` / `self.last_landmarks`.  With `image` ([img_h,img_w,3]
    uint8 RGB, numpy or device) texture and lighting are then fitted to it (`photo_affine`, `fit_appearance`; its report in
    `self.last_appearance_report`; `visibility` and `prefilter` are `observe`'s options, off by default); without, they stay zeros."""
    crop, center_x, center_y, ratio = crop_alignment(landmarks_xy, img_h, img_w)
    lm_new, trans_params = preprocess_landmarks(crop, lm3D)
    coeff, report = self.fit(lm_new.reshape(1, 68, 2), **fit_args)
    self.last_report, self.last_landmarks = report, lm_new
    if image is not None:
      if tuple(image.shape) != (img_h, img_w, 3):
        raise ValueError("enroll: image must be [img_h,img_w,3], got %s" % (tuple(image.shape),))
      coeff, self.last_appearance_report = self.fit_appearance(coeff, photo=image, affine=photo_affine(landmarks_xy, img_h, img_w, lm3D),
                                                               lam_tex=lam_tex, lam_gamma=lam_gamma, visibility=visibility,
                                                               prefilter=prefilter)
    return {"bfmcoeff": coeff.cpu().numpy().reshape(1, 257), "transform_params": trans_params, "center_x": center_x, "center_y": center_y,
            "ratio": ratio}

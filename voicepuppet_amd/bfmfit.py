"""BFM coefficients from 68 landmarks, on the MI355X (libvp_hip.so: vp_bfmfit_*; csrc/bfm_fit.hip).

The reference obtains a photo's 257 coefficients and the `bfmcoeff.txt` rows BFMNet is trained on from FaceReconModel.pb, a frozen
TensorFlow 1 ResNet (voicepuppet/pixrefer/infer_bfmvid.py:47-74, datasets/make_data_from_GRID.py:193-214).  This module gets identity
(0:80), expression (80:144), angles (224:227) and translation (254:257) from a landmark file instead: it inverts `Reconstruction`
(utils/reconstruct_mesh.py:172-194) for the 68 landmarks that function returns.  Texture (144:224) and lighting (227:254) are NOT fitted:
they stay at the caller's template, zeros by default, i.e. the mean albedo under ambient light.

  E(p) = sum_k w_k |pi_k(p) - l_k|^2 + lam_id |alpha|^2 + lam_ex |beta|^2        p = [alpha(80) | beta(64) | angles(3) | t(3)]

minimised per frame by Levenberg-Marquardt in float64, one workgroup per frame (include/vp_hip.h states the rule).
`report` [frames,4] = (status, accepted iterations, final E, final |g|_inf); status 0 converged, 1 max_iters, 2 stalled, 3 non-finite input.

`FaceFitter.fit_sequence` is a FIXED SCHEDULE of block-coordinate descent for a clip of one person (per-frame fits, then identity steps
alternating with tracking fits), not a minimiser: it stops after `rounds` rounds whatever the cost does.

The alignment helpers (`crop_alignment`, `preprocess_landmarks`) are plain numpy float64 and do no device work.  No CPU fallback for the fit.
"""
import ctypes

import numpy as np

from . import _lib

NP = 150
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


def crop_alignment(landmarks_xy, img_h, img_w, out_img_size=224, ratio=1.3):
  """The landmark arithmetic of crop_expand_alignment (utils/utils.py:78-110): the square crop around the landmarks' bounding box, expanded
  by `ratio` (less where the image ends), resized to out_img_size.  landmarks_xy [68,2] image pixels -> (landmarks in the crop [68,2],
  center_x, center_y, ratio = out_img_size / crop width)."""
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
  out = np.stack([(xy[:, 0] - left) * out_img_size / width, (xy[:, 1] - top) * out_img_size / height], axis=1)
  return out, center_x, center_y, float(out_img_size) / width


def preprocess_landmarks(lm, lm3D, w0=224, h0=224):
  """The landmark half of Preprocess / POS / process_img (utils/bfm_load_data.py:148-212).  lm [68,2] in the w0 x h0 crop; lm3D the
  standard landmarks, [68,3] (BFM/similarity_Lm3D_all.mat's `lm`) or the five points load_lm3d returns.  The five points of both are
  load_lm3d's (:122-127).  Returns (lm_new [68,2]: all 68 in the 224 image the network would have seen, trans_params [5] =
  (w0, h0, 102 / s, t0 - w0/2, h0/2 - t1))."""
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
  new = np.stack([flip[:, 0] - t0 + w0 / 2, flip[:, 1] - t1 + h0 / 2], axis=1) / s * 102          # :179
  new = new - np.array([w / 2 - 112, h / 2 - 112]).reshape(1, 2)                                  # :191
  lm_new = np.stack([new[:, 0], 223 - new[:, 1]], axis=1)                                         # :209
  return lm_new, np.array([w0, h0, 102.0 / s, t0 - w0 / 2, h0 / 2 - t1], np.float64)


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
    self._torch = torch

  def _workspace(self, frames):
    n = _lib.lib().vp_bfmfit_workspace_bytes(frames)
    if self._ws is None or self._ws.numel() < n:
      self._ws = self._torch.empty(n, dtype=self._torch.uint8, device=self.model.device)
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
    _lib.check(_lib.lib().vp_bfmfit_fit(ctypes.byref(self.model.c), self._kp.ctypes.data_as(P), 1 if self._table_ready else 0, P(lm.data_ptr()),
                                        P(w.data_ptr() if w is not None else 0), per_frame, P(tmpl.data_ptr()), P(p.data_ptr()), 1 if params_in else 0, T,
                                        float(lam_id), float(lam_ex), float(gtol), int(max_iters), _free_mask(free), P(coeff.data_ptr()),
                                        P(report.data_ptr()), P(ws.data_ptr()), ws.numel(), P(torch.cuda.current_stream().cuda_stream)),
               "vp_bfmfit_fit")
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
                                                  P(lm.data_ptr()), P(w.data_ptr() if w is not None else 0), per_frame, P(params.data_ptr()),
                                                  P(coeff.data_ptr() if coeff is not None else 0), T, float(lam_id), P(ws.data_ptr()), ws.numel(),
                                                  P(torch.cuda.current_stream().cuda_stream)), "vp_bfmfit_identity_step")
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

  def enroll(self, landmarks_xy, img_h, img_w, lm3D, **fit_args):
    """A photo's landmarks [68,2] (image pixels) -> the dictionary infer_bfmvid.py --bfmcoeff reads (np.savez(path, **d)): bfmcoeff [1,257]
    float32, transform_params [5], center_x, center_y, ratio.  crop_alignment, preprocess_landmarks and one full fit; the fit's report
    [1,4] (device) and the landmarks it was given [68,2] stay in `self.last_report` / `self.last_landmarks`."""
    crop, center_x, center_y, ratio = crop_alignment(landmarks_xy, img_h, img_w)
    lm_new, trans_params = preprocess_landmarks(crop, lm3D)
    coeff, report = self.fit(lm_new.reshape(1, 68, 2), **fit_args)
    self.last_report, self.last_landmarks = report, lm_new
    return {"bfmcoeff": coeff.cpu().numpy().reshape(1, 257), "transform_params": trans_params, "center_x": center_x, "center_y": center_y,
            "ratio": ratio}

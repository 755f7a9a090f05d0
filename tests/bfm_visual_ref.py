"""numpy float64 restatement of what voicepuppet_amd.bfmnet.visual and vp_bfm_reconstruct_view compute: `Reconstruction`
(utils/reconstruct_mesh.py:172-194) batched over frames, the two packings (view 0: utils/bfm_visual.py:100-112; view 1:
voicepuppet/bfmnet/infer_bfmnet.py:212-216), the montage of plot_bfm_coeff_seq (bfm_visual.py:88-152), its coefficient splice
(:147-150) and the 68-landmark distance.  TEST INFRASTRUCTURE ONLY.  PINNED: tests/golden/bfm_visual.npz holds what the reference's own
reconstruct_mesh.Reconstruction returned (tests/golden/make_bfm_visual_golden.py); tests/test_bfm_visual_host.py checks this file
against it."""
import numpy as np

from oracle import bfm_ref as br
from oracle import raster_ref as rr

NAMES = ["face_shape", "face_texture", "face_color", "face_projection", "z_buffer", "landmarks_2d", "translation"]
BLOCK_X, BLOCK_Y, IMG = 10, 9, 224


def reconstruction(coeff, fm, focal=1015.0, center=112.0):
  """Batched Reconstruction: coeff [T,257] -> dict of NAMES; face_shape is the UNROTATED shape, the rotation comes from coeff[:, 224:227]."""
  coeff = np.asarray(coeff)
  T = coeff.shape[0]
  idc, exc, texc, angles, gamma, trans = coeff[:, :80], coeff[:, 80:144], coeff[:, 144:224], coeff[:, 224:227], coeff[:, 227:254], coeff[:, 254:]
  shape = (idc @ fm.idBase.T + exc @ fm.exBase.T + fm.meanshape).reshape(T, -1, 3)                   # :21-25
  shape = shape - fm.meanshape.reshape(1, -1, 3).mean(axis=1, keepdims=True)                         # :27
  tex = (texc @ fm.texBase.T + fm.meantex).reshape(T, -1, 3)                                         # :59-60
  tri = (fm.tri - 1).astype(np.int32)
  pb = (fm.point_buf - 1).astype(np.int32)
  fn = np.cross(shape[:, tri[:, 0]] - shape[:, tri[:, 1]], shape[:, tri[:, 1]] - shape[:, tri[:, 2]])     # :43-46
  fn = np.concatenate([fn, np.zeros((T, 1, 3))], axis=1)
  vn = fn[:, pb].sum(axis=2)                                                                         # :50
  vn = vn / np.linalg.norm(vn, axis=2)[..., None]
  R = br.rotation_matrices(angles)                                                                   # :181
  vn_r = vn @ R                                                                                      # :182
  # Projection_layer (:100-120) on the unrotated shape: ONE rotation
  cam = (shape @ R + trans.reshape(T, 1, 3)) * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 10.0])
  aug = np.stack([focal * cam[..., 0] + center * cam[..., 2], focal * cam[..., 1] + center * cam[..., 2], cam[..., 2]], -1)
  proj = aug[..., :2] / aug[..., 2:3]
  zbuf = -aug[..., 2:3]
  proj = np.stack([proj[..., 0], 224 - proj[..., 1]], axis=2)                                        # :186
  g = gamma.reshape(T, 3, 9).astype(np.float64) + np.array([0.8, 0, 0, 0, 0, 0, 0, 0, 0])            # :133-135
  a0, a1, a2 = br.SH_A
  c0, c1, c2 = br.SH_C
  nx, ny, nz = vn_r[..., 0], vn_r[..., 1], vn_r[..., 2]
  Y = np.stack([np.full_like(nx, a0 * c0), -a1 * c1 * ny, a1 * c1 * nz, -a1 * c1 * nx, a2 * c2 * nx * ny, -a2 * c2 * ny * nz,
                a2 * c2 * 0.5 / np.sqrt(3.0) * (3 * np.square(nz) - 1), -a2 * c2 * nx * nz,
                a2 * c2 * 0.5 * (np.square(nx) - np.square(ny))], axis=2)                            # :145-155
  color = np.einsum("tnk,tck->tnc", Y, g) * tex                                                      # :159-165
  return {"face_shape": shape, "face_texture": tex, "face_color": color, "face_projection": proj, "z_buffer": zbuf,
          "landmarks_2d": proj[:, fm.keypoints], "translation": trans}


def pack_view(out, view, scale=3):
  """float32 vertices [T,N,3] and colours [T,N,3] as the two callers hand them to render_colors_core."""
  colors = np.clip(out["face_color"], 0, 255).astype(np.int32).astype(np.float32)
  if view == 0:
    return np.concatenate([out["face_projection"], out["z_buffer"]], axis=2).astype(np.float32), colors        # bfm_visual.py:100-112
  shape = out["face_shape"].copy()
  shape[..., :2] = 112 - shape[..., :2] * 112                                                        # infer_bfmnet.py:215
  shape *= scale                                                                                     # :216
  return shape.astype(np.float32), colors


def raster(vertices, colors, fm, size=IMG):
  """One frame through the compiled reference rasteriser when it is there, its pinned restatement otherwise (bit-identical:
  tests/test_raster.py)."""
  fn = rr.render_colors_ref if rr.have_compiled_reference() else rr.render_colors_py
  return fn(vertices, (fm.tri - 1).astype(np.int32), colors, size, size)[0]


def splice(real, pred, id_coeff=None, texture_coeff=None):
  """bfm_visual.py:147-150."""
  if id_coeff is None or texture_coeff is None:
    return np.concatenate([real[:, :, :80], pred[:, :, :], real[:, :, 144:]], axis=2)
  return np.concatenate([np.tile(id_coeff, (1, real.shape[1], 1)), pred[:, :, :], np.tile(texture_coeff, (1, real.shape[1], 1)), real[:, :, 224:]], axis=2)


def clip_time(seq_len):
  return 30 if seq_len[0] > 30 else int(seq_len[0])                                                  # :133-136


def place(big_img, tiles, h_index):
  """merge_seq's paste (:125-128) of already rasterised tiles: channel swap, then cell (i // 10 + h_index, i % 10)."""
  for i, tile in enumerate(tiles):
    big_img[(i // BLOCK_X + h_index) * IMG:(i // BLOCK_X + h_index + 1) * IMG, (i % BLOCK_X) * IMG:(i % BLOCK_X + 1) * IMG] = tile[..., ::-1]
  return big_img


def tiles_of(coeff, fm):
  v, c = pack_view(reconstruction(coeff, fm), 0)
  return np.stack([raster(v[i], c[i], fm) for i in range(v.shape[0])])


def montage(fm, seq_len, real, pred, id_coeff=None, texture_coeff=None, tiles=None):
  """plot_bfm_coeff_seq's big_img [2016,2240,3] (the array cv2.imwrite is handed: the .jpg file's RGB is big_img[..., ::-1]) and the
  landmark distance [time,2].  tiles: (real tiles, predicted tiles) already rasterised (the golden's), else they are drawn here."""
  time = clip_time(seq_len)
  spliced = splice(real, pred, id_coeff, texture_coeff)
  a, b = (tiles_of(real[0, :time], fm), tiles_of(spliced[0, :time], fm)) if tiles is None else tiles
  big = np.zeros((IMG * BLOCK_Y, IMG * BLOCK_X, 3), np.uint8)
  place(big, a[:time], 0)
  place(big, b[:time], 3)
  pa, pb = reconstruction(real[0, :time], fm)["face_projection"], reconstruction(spliced[0, :time], fm)["face_projection"]
  return big, lmd(pa, pb, fm.keypoints)


def lmd(proj_a, proj_b, keypoints):
  """[F,2]: mean Euclidean distance over the 68 landmarks, and over landmarks 48..67 (the mouth)."""
  kp = np.asarray(keypoints).astype(np.int64)
  d = np.sqrt(((proj_a[:, kp] - proj_b[:, kp]) ** 2).sum(axis=2))
  return np.stack([d.mean(axis=1), d[:, 48:].mean(axis=1)], axis=1)


def synthetic_sequences(frames, seed, batch=1):
  """real [batch,frames,257] like a training clip (identity and texture jitter from frame to frame, as FaceRecon's per-frame fits do;
  the pose drifts), pred [batch,frames,64], float32."""
  rng = np.random.default_rng(seed)
  real = np.stack([br.synthetic_coeffs(frames, seed + 1 + b)[0] for b in range(batch)])
  real[:, :, :80] += rng.normal(0, 0.05, size=(batch, frames, 80))
  real[:, :, 144:224] += rng.normal(0, 0.3, size=(batch, frames, 80))
  real[:, :, 224:227] += np.cumsum(rng.normal(0, 0.03, size=(batch, frames, 3)), axis=1)
  real[:, :, 254:] += rng.normal(0, 0.01, size=(batch, frames, 3))
  pred = real[:, :, 80:144] + rng.normal(0, 0.4, size=(batch, frames, 64))
  return real.astype(np.float32), pred.astype(np.float32)

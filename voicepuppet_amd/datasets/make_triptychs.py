#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""A PixReferNet training folder from a clip's frames and a 68-landmark file, on the MI355X:

    python voicepuppet/datasets/make_triptychs.py --clip_dir frames/ --landmarks frames/_landmark.txt --out_dir data/clip0 --list train.txt

In place of steps 5 and 6 of the reference's datasets/make_data_from_GRID.py (deep_video_portraits, :408-471; the layout of
deep_video_portraits_v2, :690-695), which need TensorFlow 1, MXNet, OpenCV and FaceReconModel.pb.

--clip_dir DIR     0.jpg, 1.jpg, ... (read with JpegDecoder; a file outside its subset is read with PIL)
--clip_avi FILE    instead of --clip_dir: a Motion-JPEG AVI file (voicepuppet_amd.avi_read.AviReader: its frames are decoded on the device, 4:2:2
                   and frames without Huffman tables included).  A PCM audio track is written to out_dir/audio.wav as stored, which is
                   step 2 of the reference's make_data_from_GRID.py (:110-141, ffmpeg there); the summary line gains
                   "avi: 75 frames 4:2:2, audio 44100 Hz x 2 -> audio.wav", or "no audio" for a clip without a PCM track
--landmarks FILE   one frame per line, 136 comma-separated values x0,y0,...,x67,y67 in pixels of those frames (the _landmark.txt of the
                   reference's step 3; any landmark model with the 68-point layout)
--out_dir DIR      gets <i>.jpg (S x 3S: frame | 3-D face on the frame | mask), bfmcoeff.txt (one row of 257 per frame), ear.txt
                   (ear_compute's formula, :96-102, on the landmark values as given)
--size S           the triptych's panel size; the (cropped) frames are resized to S x S with the OpenCV-exact uint8 bilinear.  Default: the
                   frames' own size, which must then be square
--crop X0 Y0 SIDE  the square of the frame to keep, before the resize (the landmarks follow)
--alpha_dir DIR    <i>.jpg or <i>.png mattes, S x S after the same crop and resize: step 6's layout (render on black | matte) instead of step 5's
                   (a matte that already has the panel's size, as --write_alpha writes it, is taken as it is)
--key_matte        step 6's layout with the matte computed here (voicepuppet_amd.matte.KeyMatte): a colour key against the backdrop, fitted
                   to the border of the clip's first frames, and one guided-filter pass.  For a head and shoulders in front of a PLAIN
                   backdrop only; it is no matting network.  Not together with --alpha_dir
--key_frames N     the backdrop model is fitted once, on the first N panel-size frames (default: one device batch)
--key_thresholds LO HI, --key_radius R, --key_eps E, --key_band B   KeyMatte's ramp (4 10), guided-filter window (4) and regulariser
                   (25), and the width of the border band (panel size // 16); the defaults are untuned on real footage
--write_alpha DIR  with --key_matte: gets the mattes as <i>.png, panel size, for inspection and for reuse as --alpha_dir
--clean_matte      cleans the matte of --key_matte or --alpha_dir before the build and before --write_alpha (voicepuppet_amd.matte_clean.
                   MatteCleaner): components of the matte that are not the subject (they neither leave through the bottom edge nor hold
                   one of the frame's 68 landmarks: speckle, a prop, the frame's edge) are removed with the haze around them, enclosed holes
                   in the subject are filled.  Component bookkeeping: it moves no edge
--clean_support S, --clean_core C, --clean_min_area A, --clean_max_hole A, --clean_grow G, --clean_keep all|anchored   MatteCleaner.clean's
                   parameters (32, 224, S * S // 1024, S * S // 256, 4, anchored); the defaults are untuned on real footage
--solve_matte      solves the matte of --key_matte or --alpha_dir (after --clean_matte) inside a trimap's unknown band
                   (voicepuppet_amd.matte_solve.MatteSolver): the trimap from an erosion and a dilation of the matte, then closed-form matting
                   on the frame's colours, step 6's trimap and matting network without the network.  It moves the matte's edge to where
                   the colours put it.  --alpha_dir with binary masks plus --solve_matte is the path for a CLUTTERED background, where
                   --key_matte is the wrong tool
--solve_erode E, --solve_dilate D, --solve_radius R, --solve_eps EPS, --solve_iters N, --solve_tol T   MatteSolver's squares (by panel size:
                   max(5, S // 19) and max(5, S // 29)), window radius (1), regulariser (1), iteration cap (512) and relative residual
                   (1e-6); the defaults are untuned on real footage
--key_foreground   the frame panel gets the subject's own colours instead of the frame's (KeyMatte.foreground): on the matte's soft edge
                   the frame is a mix of subject and backdrop, and frame x matte teaches the generator a fringe of backdrop colour.  With
                   --alpha_dir the backdrop model is fitted to the border of the first frames as with --key_matte.  Exact only where the
                   matte is; where the matte is 0 the panel is black
--key_despill S    with --key_foreground: 0 .. 1, how much of the backdrop's key channel is taken out of the subject (default 0; acts only
                   on a backdrop whose largest channel leads by 16 levels)
--bfmcoeff FILE    rows of 257 coefficients to use instead of fitting them (fit_landmarks.py --clip writes such a file)
--appearance first|none   first (default): texture and lighting are fitted to frame 0's pixels and shared by the clip; none: zeros
--appearance_visibility, --appearance_prefilter   that fit without self-occluded vertices / on area means of frame 0 (both off by default)
--frame_batch N    frames per device batch (default 32)
--list FILE        gets the line "out_dir|count" appended: the list train_pixrefer.py reads

The paste geometry is infer_bfmvid.paste_geometry for every frame, i.e. step 6's and inference's int(), not step 5's int(round()).  A frame
that cannot be built (TriptychBuilder's status) repeats the frame before it, as step 6 does; a clip whose first frame cannot be built is
refused.  Needs BFM/BFM_model_front.mat and BFM/similarity_Lm3D_all.mat, like fit_landmarks.py.  One line is printed: frames, statuses,
repeated frames, and the reprojection error in pixels of the 224 image as fit_landmarks.py prints it; with --key_matte also the share of
border samples the backdrop model kept and its residual, with a warning when the border was not a plain backdrop; with --clean_matte
also "clean: removed 3 components / 66 px, filled 1 hole / 26 px" over all frames, with a warning for frames in which no component held a
landmark or reached the bottom edge (they are left as they were); with --solve_matte also "solve: 1742 px unknown, 65 iterations,
residual 9e-7" (means over the clip), with a warning when a frame ended with a status bit set or at its iteration cap.  The order is
matte, clean, solve, foreground, build.

A one-frame run with --key_matte (a folder with 0.jpg and a one-line landmark file) is how an enrolment photo for infer_bfmvid.py and
PuppetStreamGroup.attach is made: out_dir/0.jpg is the [photo | render on black | matte] triptych they read."""
import logging
import math
import os
import sys
from optparse import OptionParser

import numpy as np

sys.path.append(os.getcwd())

logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
logger = logging.getLogger(__name__)


def ear_value(ps):
  """ear_compute (make_data_from_GRID.py:96-102) for one line of 136 values: the mean of the two eyes' aspect ratios, landmarks 36..41 and
  42..47 (0-based): (|p1 - p5| + |p2 - p4|) / |p0 - p3|."""
  def dist(a, b):
    return math.sqrt((ps[a] - ps[b]) ** 2 + (ps[a + 1] - ps[b + 1]) ** 2)
  ear1 = (dist(74, 82) + dist(76, 80)) / dist(72, 78)
  ear2 = (dist(86, 94) + dist(88, 92)) / dist(84, 90)
  return (ear1 + ear2) / 2


def count_frames(clip_dir):
  n = 0
  while os.path.exists(os.path.join(clip_dir, '%d.jpg' % n)):
    n += 1
  return n


def _pil_rgb(path):
  from PIL import Image
  return np.array(Image.open(path).convert('RGB'), np.uint8)


class FrameReader(object):
  """<i>.jpg of a folder -> uint8 RGB device tensors [n, S, S, 3], cropped and resized.  All files have the size of the first."""

  def __init__(self, clip_dir, batch, crop, size):
    import torch
    from PIL import Image
    from voicepuppet_amd.jpeg_dec import JpegDecoder
    self.torch, self.dir = torch, clip_dir
    with Image.open(os.path.join(clip_dir, '0.jpg')) as im:
      self.w, self.h = im.size
    self._set_panel(clip_dir, crop, size)
    self.decoder = JpegDecoder(batch, self.h, self.w, bgr=False)
    self.fallbacks = 0

  def _set_panel(self, clip_dir, crop, size):
    x0, y0, side = crop if crop is not None else (0, 0, self.h)
    if crop is None and self.h != self.w:
      raise ValueError('%s: the frames are %d x %d; --crop X0 Y0 SIDE must name a square' % (clip_dir, self.w, self.h))
    if x0 < 0 or y0 < 0 or side < 1 or x0 + side > self.w or y0 + side > self.h:
      raise ValueError('--crop %d %d %d does not lie inside the %d x %d frames' % (x0, y0, side, self.w, self.h))
    self.crop = (int(x0), int(y0), int(side))
    self.size = int(size) if size else int(side)

  def _decode(self, paths):
    torch = self.torch
    try:
      out, status = self.decoder.decode(paths)
      bad = np.flatnonzero(status.cpu().numpy() != 0).tolist()
    except ValueError as e:                                       # a file outside the decoder's subset (progressive, 4:4:4, another size...)
      logger.info('%s: read with PIL', e)
      out, bad = torch.zeros(len(paths), self.h, self.w, 3, dtype=torch.uint8, device='cuda'), list(range(len(paths)))
    for i in bad:
      img = _pil_rgb(paths[i])
      if img.shape != (self.h, self.w, 3):
        raise ValueError('%s is %d x %d, the clip\'s first frame %d x %d' % (paths[i], img.shape[1], img.shape[0], self.w, self.h))
      out[i] = torch.from_numpy(img).cuda()
      self.fallbacks += 1
    return out

  def fit_to_panel(self, frames):
    """[n, h, w, 3] device -> the crop, resized to S x S as cv2.resize(uint8) does."""
    from voicepuppet_amd.utils.cv_resize import resize_paste_u8
    x0, y0, side = self.crop
    frames = frames[:, y0:y0 + side, x0:x0 + side].contiguous()
    if side == self.size:
      return frames
    return resize_paste_u8(frames, self.size, self.size, (self.size, self.size), 0, 0)

  def read(self, first, n):
    return self.fit_to_panel(self._decode([os.path.join(self.dir, '%d.jpg' % i) for i in range(first, first + n)]))

  def landmarks_to_panel(self, lms):
    x0, y0, side = self.crop
    return (np.asarray(lms, np.float64) - np.array([x0, y0], np.float64)) * (float(self.size) / side)


class AviFrameReader(FrameReader):
  """The frames of a Motion-JPEG AVI file (AviReader) through FrameReader's crop and resize."""

  def __init__(self, avi_path, batch, crop, size):
    import torch
    from voicepuppet_amd.avi_read import AviReader
    self.torch, self.dir = torch, avi_path
    self.avi = AviReader(avi_path, batch=batch)
    self.w, self.h = self.avi.width, self.avi.height
    self._set_panel(avi_path, crop, size)
    self.fallbacks = 0

  def read(self, first, n):
    frames = self.avi.read(first, n)
    self.fallbacks = self.avi.fallbacks
    return self.fit_to_panel(frames)

  def extract_audio(self, out_dir):
    """The clip's PCM track to out_dir/audio.wav -> the summary line's words on the clip."""
    text = 'avi: %s' % self.avi.describe()
    if self.avi.audio_format is None:
      return text + ', no audio' + (' (%s)' % self.avi.audio_refused if self.avi.audio_refused else '')
    self.avi.write_wav(os.path.join(out_dir, 'audio.wav'))
    return text + ', audio %d Hz x %d -> audio.wav' % (self.avi.audio_rate, self.avi.audio_channels)


def read_alpha(reader, alpha_dir, first, n):
  """<i>.jpg / <i>.png mattes of the frames' size -> uint8 device [n, S, S] (PIL, grey), through the frames' crop and resize."""
  import torch
  planes = []
  for i in range(first, first + n):
    path = next((p for p in (os.path.join(alpha_dir, '%d.%s' % (i, e)) for e in ('png', 'jpg')) if os.path.exists(p)), None)
    if path is None:
      raise ValueError('%s: no %d.png or %d.jpg' % (alpha_dir, i, i))
    from PIL import Image
    a = np.array(Image.open(path).convert('L'), np.uint8)
    if a.shape != (reader.h, reader.w) and not (a.shape == (reader.size, reader.size) and (not planes or planes[0].shape == a.shape)):
      raise ValueError('%s is %d x %d, the frames %d x %d' % (path, a.shape[1], a.shape[0], reader.w, reader.h))
    planes.append(a)
  a = torch.from_numpy(np.stack(planes)).cuda()
  if planes[0].shape != (reader.h, reader.w):                     # panel-size mattes (--write_alpha): no crop, no resize
    return a
  return reader.fit_to_panel(a[..., None].expand(-1, -1, -1, 3))[..., 0].contiguous()


def parse_options(argv=None):
  p = OptionParser(usage='usage: %prog (--clip_dir DIR | --clip_avi FILE) --landmarks FILE --out_dir DIR [--size S] [--crop X0 Y0 SIDE] [--alpha_dir DIR] '
                         '[--key_matte [--write_alpha DIR]] [--clean_matte] [--solve_matte] [--key_foreground [--key_despill S]] [--bfmcoeff FILE] [--appearance first|none] [--frame_batch N] [--list FILE]')
  p.add_option('--clip_dir', type='string', dest='clip_dir', default=None, help='folder of 0.jpg, 1.jpg, ...')
  p.add_option('--clip_avi', type='string', dest='clip_avi', default=None,
               help='a Motion-JPEG AVI file instead of --clip_dir; its PCM track goes to out_dir/audio.wav')
  p.add_option('--landmarks', type='string', dest='landmarks', default=None, help='68 landmarks per frame, 136 comma-separated values per line')
  p.add_option('--out_dir', type='string', dest='out_dir', default=None, help='the dataset folder to write')
  p.add_option('--size', type='int', dest='size', default=None, help='panel size S (default: the frames\' own)')
  p.add_option('--crop', type='int', nargs=3, dest='crop', default=None, help='X0 Y0 SIDE: the square of each frame to keep')
  p.add_option('--alpha_dir', type='string', dest='alpha_dir', default=None, help='mattes <i>.png / <i>.jpg: step 6\'s layout')
  p.add_option('--bfmcoeff', type='string', dest='bfmcoeff', default=None, help='rows of 257 coefficients instead of a fit')
  p.add_option('--appearance', type='choice', choices=['first', 'none'], dest='appearance', default='first',
               help='first: texture and lighting fitted to frame 0 and shared; none: zeros')
  p.add_option('--appearance_visibility', action='store_true', dest='appearance_visibility', default=False,
               help='--appearance first: leave self-occluded vertices out of that fit (FaceFitter.observe)')
  p.add_option('--appearance_prefilter', action='store_true', dest='appearance_prefilter', default=False,
               help='--appearance first: area-average frame 0 where it is larger than the 224 image')
  p.add_option('--frame_batch', type='int', dest='frame_batch', default=32, help='frames per device batch')
  p.add_option('--list', type='string', dest='list', default=None, help='dataset list to append "out_dir|count" to')
  p.add_option('--rounds', type='int', dest='rounds', default=3, help='fit_sequence: rounds of (identity steps, tracking fit)')
  p.add_option('--id_steps', type='int', dest='id_steps', default=3, help='fit_sequence: identity steps per round')
  p.add_option('--joint', action='store_true', dest='joint', default=False,
               help='fit the clip with FaceFitter.fit_clip (one joint solve) instead of fit_sequence')
  p.add_option('--smooth', type='float', nargs=3, dest='smooth', default=None,
               help='--joint: EX ANG T, weights of the squared frame-to-frame differences of expression, angles and translation '
                    '(default 0 0 0; useful values are untuned on real landmark files)')
  p.add_option('--key_matte', action='store_true', dest='key_matte', default=False,
               help='step 6\'s layout with the matte keyed against a plain backdrop on the device (KeyMatte); not with --alpha_dir')
  p.add_option('--key_frames', type='int', dest='key_frames', default=None,
               help='--key_matte: fit the backdrop model on the first N frames (default: one device batch)')
  p.add_option('--key_thresholds', type='float', nargs=2, dest='key_thresholds', default=(4.0, 10.0),
               help='--key_matte: LO HI, the key\'s ramp in standard deviations of the backdrop (untuned on real footage)')
  p.add_option('--key_radius', type='int', dest='key_radius', default=4, help='--key_matte: guided-filter radius, 0 .. 16 (0: the raw key)')
  p.add_option('--key_eps', type='float', dest='key_eps', default=25.0, help='--key_matte: guided-filter regulariser, grey levels squared')
  p.add_option('--key_band', type='int', dest='key_band', default=None, help='--key_matte: width of the border band (default: size // 16)')
  p.add_option('--write_alpha', type='string', dest='write_alpha', default=None, help='--key_matte: folder that gets the mattes as <i>.png')
  p.add_option('--clean_matte', action='store_true', dest='clean_matte', default=False,
               help='clean the matte of --key_matte or --alpha_dir on the device (MatteCleaner): stray components out, enclosed holes filled')
  p.add_option('--clean_support', type='int', dest='clean_support', default=32, help='--clean_matte: components of matte >= S (1 .. 255)')
  p.add_option('--clean_core', type='int', dest='clean_core', default=224, help='--clean_matte: holes of matte < C (1 .. 255)')
  p.add_option('--clean_min_area', type='int', dest='clean_min_area', default=None, help='--clean_matte: smallest component kept (default S * S // 1024)')
  p.add_option('--clean_max_hole', type='int', dest='clean_max_hole', default=None, help='--clean_matte: largest hole filled, 0: none (default S * S // 256)')
  p.add_option('--clean_grow', type='int', dest='clean_grow', default=4, help='--clean_matte: width of the soft fringe kept around a component, 0 .. 16')
  p.add_option('--clean_keep', type='choice', choices=['all', 'anchored'], dest='clean_keep', default='anchored',
               help='--clean_matte: anchored keeps the components that reach the bottom edge or hold a landmark; all keeps every large one')
  p.add_option('--solve_matte', action='store_true', dest='solve_matte', default=False,
               help='solve the matte of --key_matte or --alpha_dir inside a trimap\'s band on the device (MatteSolver: closed-form matting); '
                    '--alpha_dir with binary masks plus --solve_matte is the path for cluttered backgrounds')
  p.add_option('--solve_erode', type='int', dest='solve_erode', default=None, help='--solve_matte: the trimap\'s erosion square, 1 .. 64 (default max(5, S // 19))')
  p.add_option('--solve_dilate', type='int', dest='solve_dilate', default=None, help='--solve_matte: the trimap\'s dilation square, 1 .. 64 (default max(5, S // 29))')
  p.add_option('--solve_radius', type='int', dest='solve_radius', default=1, help='--solve_matte: window radius of the matting Laplacian, 1 .. 3')
  p.add_option('--solve_eps', type='float', dest='solve_eps', default=1.0, help='--solve_matte: its regulariser in grey levels squared, above 0')
  p.add_option('--solve_iters', type='int', dest='solve_iters', default=512, help='--solve_matte: most conjugate-gradient iterations, 1 .. 1024')
  p.add_option('--solve_tol', type='float', dest='solve_tol', default=1e-6, help='--solve_matte: relative residual at which a frame stops, not negative')
  p.add_option('--key_foreground', action='store_true', dest='key_foreground', default=False,
               help='the frame panel gets the subject\'s colours without the backdrop\'s share (KeyMatte.foreground); needs a matte')
  p.add_option('--key_despill', type='float', dest='key_despill', default=0.0, help='--key_foreground: 0 .. 1 of the key channel\'s spill removed')
  opts, args = p.parse_args(argv)
  if opts.clip_dir and opts.clip_avi:
    p.error('--clip_dir and --clip_avi both name the clip: give one of the two')
  if opts.key_matte and opts.alpha_dir:
    p.error('--key_matte computes the matte that --alpha_dir reads: give one of the two')
  if opts.write_alpha and not opts.key_matte:
    p.error('--write_alpha writes the mattes of --key_matte')
  if (opts.clean_matte or opts.key_foreground) and not (opts.key_matte or opts.alpha_dir):
    p.error('--clean_matte and --key_foreground work on the matte of --key_matte or --alpha_dir')
  if opts.solve_matte and not (opts.key_matte or opts.alpha_dir):
    p.error('--solve_matte works on the matte of --key_matte or --alpha_dir')
  if ((opts.solve_erode is not None and not (1 <= opts.solve_erode <= 64)) or (opts.solve_dilate is not None and not (1 <= opts.solve_dilate <= 64))
      or not (1 <= opts.solve_radius <= 3) or not (0.0 < opts.solve_eps < float('inf')) or not (1 <= opts.solve_iters <= 1024)
      or not (0.0 <= opts.solve_tol < float('inf'))):
    p.error('--solve_erode and --solve_dilate 1 .. 64, --solve_radius 1 .. 3, --solve_eps above 0, --solve_iters 1 .. 1024, --solve_tol not negative')
  if (not (1 <= opts.clean_support <= 255) or not (1 <= opts.clean_core <= 255) or not (0 <= opts.clean_grow <= 16)
      or (opts.clean_min_area is not None and opts.clean_min_area < 0) or (opts.clean_max_hole is not None and opts.clean_max_hole < 0)):
    p.error('--clean_support and --clean_core 1 .. 255, --clean_grow 0 .. 16, --clean_min_area and --clean_max_hole not negative')
  if not (0.0 <= opts.key_despill <= 1.0):
    p.error('--key_despill 0 .. 1')
  lo, hi = opts.key_thresholds
  if not (0.0 <= lo < hi < float('inf')) or not (0 <= opts.key_radius <= 16) or not (0.0 < opts.key_eps < float('inf')):
    p.error('--key_thresholds LO HI with 0 <= LO < HI, --key_radius 0 .. 16, --key_eps above 0')
  return opts, args


def read_landmarks_for(path, frames_n, clip_dir):
  """-> (landmarks [frames_n, 68, 2] in pixels of the frames, the file's lines for them)."""
  from voicepuppet_amd.bfmnet.fit_landmarks import read_landmarks
  with open(path) as f:
    raw_lines = [line for line in f if line.strip()]
  lms = read_landmarks(path)
  if lms.shape[0] < frames_n:
    raise SystemExit('%s has %d lines for the %d frames of %s' % (path, lms.shape[0], frames_n, clip_dir))
  return lms[:frames_n], raw_lines[:frames_n]


def align_landmarks(lms, S, lm3D):
  """Alignment and paste geometry per frame (host, float64): datasets/make_data_from_GRID.py:193-214 and infer_bfmvid.py:83-86.
  -> (aligned landmarks, int64 [frames, 4] geometry)."""
  from voicepuppet_amd.bfmfit import crop_alignment, preprocess_landmarks
  from voicepuppet_amd.pixrefer.infer_bfmvid import paste_geometry
  aligned, geometry = [], []
  for lm in lms:
    crop, center_x, center_y, ratio = crop_alignment(lm, S, S)
    lm_new, trans_params = preprocess_landmarks(crop, lm3D)
    aligned.append(lm_new)
    geometry.append(paste_geometry(center_x, center_y, ratio, trans_params, 224))
  return np.stack(aligned), np.array(geometry, np.int64)


def choose_coefficients(opts, fitter, aligned, frames_n, reader, lms, lm3D):
  """--bfmcoeff, --joint or fit_sequence, then --appearance -> (coeff [frames_n, 257], the fit's report, the summary line's words on
  the appearance fit)."""
  import torch
  from voicepuppet_amd.bfmfit import photo_affine
  if opts.bfmcoeff:
    rows = np.loadtxt(opts.bfmcoeff, delimiter=',', dtype=np.float32, ndmin=2)
    if rows.shape[0] < frames_n or rows.shape[1] != 257:
      raise SystemExit('%s: %s, expected at least %d rows of 257' % (opts.bfmcoeff, rows.shape, frames_n))
    coeff, report = torch.from_numpy(rows[:frames_n]).cuda(), torch.zeros(frames_n, 4, dtype=torch.float64, device='cuda')
  elif opts.joint:
    coeff, clip_report = fitter.fit_clip(aligned, lam_smooth=opts.smooth or (0.0, 0.0, 0.0))
    report = clip_report.repeat(frames_n, 1)                # the clip's status in every frame's row of the summary line
  else:
    coeff, report = fitter.fit_sequence(aligned, rounds=opts.rounds, id_steps=opts.id_steps)
  extra = ''
  if opts.appearance == 'first':
    S = reader.size
    frame0 = reader.read(0, 1)[0]
    first, rep = fitter.fit_appearance(coeff[:1], photo=frame0, affine=photo_affine(lms[0], S, S, lm3D),
                                       visibility=opts.appearance_visibility, prefilter=opts.appearance_prefilter)
    coeff = coeff.clone()
    coeff[:, 144:224], coeff[:, 227:254] = first[:, 144:224], first[:, 227:254]
    extra = ', appearance status %d' % int(rep[0, 0].item())
  return coeff, report, extra


def matte_chain(opts, reader, batch, frames_n):
  """The MatteChain of --key_matte, --clean_matte, --solve_matte and --key_foreground; a stage that refuses its options ends the run in
  that option's name."""
  import torch
  from voicepuppet_amd.matte_chain import MatteChain
  chain = MatteChain(batch, reader.size, reader.size)
  if opts.key_matte or opts.key_foreground:
    key_n = min(opts.key_frames or batch, frames_n)
    if key_n < 1:
      raise SystemExit('--key_frames must be at least 1')
    try:
      chain.add_key(torch.cat([reader.read(first, min(batch, key_n - first)) for first in range(0, key_n, batch)]), matte=opts.key_matte,
                    lo=opts.key_thresholds[0], hi=opts.key_thresholds[1], radius=opts.key_radius, eps=opts.key_eps, band=opts.key_band)
    except (ValueError, RuntimeError) as e:
      raise SystemExit('%s: %s' % ('--key_matte' if opts.key_matte else '--key_foreground', e))
    if opts.write_alpha:
      os.makedirs(opts.write_alpha, exist_ok=True)
  if opts.clean_matte:
    chain.add_clean(support=opts.clean_support, core=opts.clean_core, min_area=opts.clean_min_area, max_hole=opts.clean_max_hole,
                    grow=opts.clean_grow, keep=opts.clean_keep)
  if opts.solve_matte:
    try:
      chain.add_solve(erode=opts.solve_erode, dilate=opts.solve_dilate, radius=opts.solve_radius, eps=opts.solve_eps, iters=opts.solve_iters,
                      tol=opts.solve_tol)
    except ValueError as e:
      raise SystemExit('--solve_matte: %s' % e)
  if opts.key_foreground:
    chain.add_foreground(despill=opts.key_despill)
  return chain


def write_lists(opts, coeff, raw_lines, frames_n):
  """out_dir/bfmcoeff.txt, out_dir/ear.txt and the line of --list."""
  np.savetxt(os.path.join(opts.out_dir, 'bfmcoeff.txt'), coeff.cpu().numpy(), delimiter=',', fmt='%.8g')
  with open(os.path.join(opts.out_dir, 'ear.txt'), 'w') as f:
    for line in raw_lines:
      f.write('{}\n'.format(ear_value([float(v) for v in line.strip().split(',')])))
  if opts.list:
    with open(opts.list, 'a') as f:
      f.write('%s|%d\n' % (opts.out_dir, frames_n))


def main(argv=None):
  opts, _ = parse_options(argv)
  if (opts.clip_dir is None and opts.clip_avi is None) or opts.landmarks is None or opts.out_dir is None:
    logger.error('Please check your parameters: --clip_dir (or --clip_avi), --landmarks and --out_dir are needed.')
    exit(0)
  from voicepuppet_amd.bfmnet.fit_landmarks import BFM_MAT, LM3D_MAT, _BFM, reprojection_error, summary_line
  if not (os.path.exists(BFM_MAT) and os.path.exists(LM3D_MAT)):
    logger.error('%s and %s are needed', BFM_MAT, LM3D_MAT)
    exit(0)
  if opts.frame_batch < 1:
    raise SystemExit('--frame_batch must be at least 1')
  import torch
  from scipy.io import loadmat
  from voicepuppet_amd.bfmfit import FaceFitter
  from voicepuppet_amd.triptych import STATUS, TriptychBuilder
  from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer

  clip = opts.clip_avi or opts.clip_dir
  if opts.clip_avi:
    from voicepuppet_amd.avi_read import AviReader
    try:
      frames_n = AviReader(opts.clip_avi).frames
    except (OSError, ValueError) as e:
      raise SystemExit(str(e))
    if frames_n < 1:
      raise SystemExit('%s: no video frame' % opts.clip_avi)
  else:
    frames_n = count_frames(opts.clip_dir)
    if frames_n < 1:
      raise SystemExit('%s: no 0.jpg' % opts.clip_dir)
  lms, raw_lines = read_landmarks_for(opts.landmarks, frames_n, clip)
  batch = min(opts.frame_batch, frames_n)
  try:
    reader = AviFrameReader(opts.clip_avi, batch, opts.crop, opts.size) if opts.clip_avi else FrameReader(opts.clip_dir, batch, opts.crop, opts.size)
  except ValueError as e:
    raise SystemExit(str(e))
  S = reader.size
  lms = reader.landmarks_to_panel(lms)
  fitter = FaceFitter(_BFM(loadmat(BFM_MAT)))
  lm3D = loadmat(LM3D_MAT)['lm']
  aligned, geometry = align_landmarks(lms, S, lm3D)
  coeff, report, extra = choose_coefficients(opts, fitter, aligned, frames_n, reader, lms, lm3D)

  os.makedirs(opts.out_dir, exist_ok=True)
  renderer = ClipRenderer(fitter.model)
  builder = TriptychBuilder(S, batch)
  status, repeated = [], []
  chain = matte_chain(opts, reader, batch, frames_n)
  anchors = torch.from_numpy(np.floor(lms).astype(np.int32)).cuda() if opts.clean_matte else None     # the panel landmarks' pixels
  try:
    for first in range(0, frames_n, batch):
      n = min(batch, frames_n - first)
      frames = reader.read(first, n)
      render, face_mask = renderer.render_view(coeff[first:first + n], view=0)
      alpha = read_alpha(reader, opts.alpha_dir, first, n) if opts.alpha_dir else None
      frames, alpha = chain.run(frames, alpha, anchors[first:first + n] if anchors is not None else None)
      if opts.write_alpha:
        chain.write_alpha(alpha, opts.write_alpha, first)
      trip, st = builder.build(frames, render, face_mask, geometry[first:first + n], alpha=alpha)
      repeated += builder.write(trip, st, opts.out_dir, first)
      status.append(st.cpu().numpy())
  except ValueError as e:
    raise SystemExit('%s: %s' % (clip, e))
  finally:
    chain.close()
  status = np.concatenate(status)

  write_lists(opts, coeff, raw_lines, frames_n)
  counts = ' '.join('%d:%d' % (s, int((status == s).sum())) for s in sorted(set(status.tolist())))
  for s in sorted(set(status.tolist()) - {0}):
    logger.warning('triptych status %d: %s', s, STATUS.get(s, '?'))
  text, warnings, fatal = chain.summary()
  for w in warnings:
    logger.warning('%s', w)
  if fatal:
    raise SystemExit(fatal)
  if opts.clip_avi:
    text += '; ' + reader.extract_audio(opts.out_dir)
  fit = summary_line(clip, report, reprojection_error(fitter, coeff, aligned))
  print('%s; triptych status %s, %d repeated, %d read with PIL%s' % (fit, counts, len(repeated), reader.fallbacks, extra + text))
  res = {'frames': frames_n, 'status': status, 'repeated': repeated, 'geometry': geometry}
  res.update(chain.reports())
  return res


if (__name__ == '__main__'):
  main()

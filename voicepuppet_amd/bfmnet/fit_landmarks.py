#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""BFM coefficients from a 68-landmark file (voicepuppet_amd.bfmfit.FaceFitter), in place of the reference's FaceReconModel.pb:

    python voicepuppet/bfmnet/fit_landmarks.py --photo landmarks.txt --size H W --out photo.npz
    python voicepuppet/bfmnet/fit_landmarks.py --photo landmarks.txt --image photo.jpg --out photo.npz
    python voicepuppet/bfmnet/fit_landmarks.py --clip landmarks.txt --size H W --out bfmcoeff.txt
    python voicepuppet/bfmnet/fit_landmarks.py --clip landmarks.txt --size H W --out bfmcoeff.txt --joint [--smooth EX ANG T]

--photo: the first line of the landmarks file is enrolled; photo.npz is what infer_bfmvid.py / infer_bfmnet.py take as --bfmcoeff
         (bfmcoeff [1,257], transform_params [5], center_x, center_y, ratio).  With --image (read with PIL as RGB; --size is then the
         image's own) texture and lighting (coefficients 144:224, 227:254) are fitted to the photo's pixels, with weights --lam_tex and
         --lam_gamma on their squared norms (defaults 1, untuned on real photos); without it they stay zeros.  --visibility leaves
         self-occluded vertices out of that fit and --prefilter area-averages a photo larger than the 224 image (FaceFitter.observe;
         both off by default).
--clip:  every line is a frame of ONE person; the frames are aligned one by one as the reference's data preparation does
         (datasets/make_data_from_GRID.py:193-214), fitted with FaceFitter.fit_sequence, and written as one row of 257 comma-separated
         values per frame: the bfmcoeff.txt that BFMCoeffLoader reads and train_bfmnet.py learns from.  With --joint the clip is fitted by
         FaceFitter.fit_clip instead: one Levenberg-Marquardt solve over the clip's identity and every frame's expression and pose, and
         --smooth EX ANG T weights the squared frame-to-frame differences of expression, angles and translation (default 0 0 0; useful
         values are untuned on real landmark files).  The line printed then holds the clip's status, accepted steps, E and |g|_inf.
A landmarks file has one frame per line: 136 comma-separated values x0,y0,...,x67,y67 in pixels of the H x W image (any landmark model
with the 68-point layout; the reference's README names dlib).  Needs BFM/BFM_model_front.mat and BFM/similarity_Lm3D_all.mat, as the
reference does.  --clip never fits texture and lighting (zeros: mean albedo, ambient light): BFMNet learns expression only.  One line
per clip is printed: frames, statuses, mean and worst reprojection error in pixels of the 224 image, and with --image the appearance fit's
status and the RMS colour residual in grey levels."""
import logging
import os
import sys
from optparse import OptionParser

import numpy as np

sys.path.append(os.getcwd())

logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
logger = logging.getLogger(__name__)

BFM_MAT = os.path.join('BFM', 'BFM_model_front.mat')
LM3D_MAT = os.path.join('BFM', 'similarity_Lm3D_all.mat')


class _BFM(object):
  """utils/bfm_load_data.py:9-21."""

  def __init__(self, model):
    for k in ('meanshape', 'idBase', 'exBase', 'meantex', 'texBase', 'point_buf', 'tri'):
      setattr(self, k, model[k])
    self.keypoints = np.squeeze(model['keypoints']).astype(np.int32) - 1


def read_landmarks(path):
  """[frames,68,2] float64 from lines of 136 comma-separated values."""
  rows = []
  with open(path) as f:
    for n, line in enumerate(f):
      if not line.strip():
        continue
      vals = [float(v) for v in line.strip().split(',')]
      if len(vals) != 136:
        raise ValueError('%s:%d: expected 136 comma-separated values (x0,y0,...,x67,y67), got %d' % (path, n + 1, len(vals)))
      rows.append(vals)
  if not rows:
    raise ValueError('%s: no landmarks' % path)
  return np.array(rows, np.float64).reshape(-1, 68, 2)


def reprojection_error(fitter, coeff, landmarks):
  """[frames,68] distances in pixels between the landmarks of Reconstruction(coeff) and the ones that were fitted (device)."""
  import torch
  from voicepuppet_amd.utils.reconstruct_mesh import reconstruct_view
  proj = reconstruct_view(coeff, fitter.model, full=True)['landmarks_2d']
  target = torch.from_numpy(np.ascontiguousarray(landmarks, np.float64)).to(proj.device)
  return torch.sqrt(((proj - target) ** 2).sum(dim=2))


def summary_line(name, report, err):
  status = report[:, 0].cpu().numpy().astype(np.int64)
  counts = ' '.join('%d:%d' % (s, int((status == s).sum())) for s in sorted(set(status.tolist())))
  return '%s: %d frames, status %s, reprojection mean %.3f px, worst %.3f px' % (name, status.shape[0], counts, float(err.mean()), float(err.max()))


def joint_summary_line(name, report, err):
  rep = report.cpu().numpy()[0]
  return '%s: %d frames, joint status %d, %d accepted steps, E %.6f, |g| %.3e, reprojection mean %.3f px, worst %.3f px' % (
      name, err.shape[0], int(rep[0]), int(rep[1]), rep[2], rep[3], float(err.mean()), float(err.max()))


def appearance_summary(fitter):
  """', appearance status S, colour RMS R grey levels': R^2 = the report's E without its two regularisation terms (the weighted mean of
  the squared colour residuals at the fitted point; the lambdas are read back from E's definition: E - lam |p|^2)."""
  rep = fitter.last_appearance_report.cpu().numpy()[0]
  p = fitter.last_appearance.cpu().numpy()[0]
  lam_tex, lam_gamma = fitter.last_appearance_lams
  data = rep[2] - lam_tex * float(np.sum(p[:80] ** 2)) - lam_gamma * float(np.sum(p[80:] ** 2))
  return ', appearance status %d, colour RMS %.2f grey levels' % (int(rep[0]), float(np.sqrt(max(data, 0.0))))


def parse_options(argv=None):
  cmd_parser = OptionParser(usage="usage: %prog (--photo LANDMARKS [--image PHOTO] | --clip LANDMARKS) [--size H W] --out FILE")
  cmd_parser.add_option('--photo', type="string", dest="photo", default=None, help='landmarks file; its first line is enrolled -> npz')
  cmd_parser.add_option('--clip', type="string", dest="clip", default=None, help='landmarks file of one person\'s clip -> bfmcoeff.txt')
  cmd_parser.add_option('--size', type="int", nargs=2, dest="size", default=None, help='image height and width in pixels (optional with --image)')
  cmd_parser.add_option('--image', type="string", dest="image", default=None, help='--photo: the photo itself; fits texture and lighting to it')
  cmd_parser.add_option('--lam_tex', type="float", dest="lam_tex", default=1.0, help='--image: weight of |texture coefficients|^2')
  cmd_parser.add_option('--lam_gamma', type="float", dest="lam_gamma", default=1.0, help='--image: weight of |lighting coefficients|^2')
  cmd_parser.add_option('--visibility', action="store_true", dest="visibility", default=False,
                        help='--image: drop self-occluded vertices (a depth raster of the fitted mesh) from the observation')
  cmd_parser.add_option('--prefilter', action="store_true", dest="prefilter", default=False,
                        help='--image: area-average the photo where it has more than one pixel per pixel of the 224 image')
  cmd_parser.add_option('--out', type="string", dest="out", default=None, help='output file')
  cmd_parser.add_option('--rounds', type="int", dest="rounds", default=3, help='--clip: rounds of (identity steps, tracking fit)')
  cmd_parser.add_option('--id_steps', type="int", dest="id_steps", default=3, help='--clip: identity steps per round')
  cmd_parser.add_option('--joint', action="store_true", dest="joint", default=False, help='--clip: one joint solve of the clip (FaceFitter.fit_clip)')
  cmd_parser.add_option('--smooth', type="float", nargs=3, dest="smooth", default=None,
                        help='--joint: weights of the squared frame-to-frame differences of expression, angles, translation (default 0 0 0)')
  cmd_parser.add_option('--max_trials', type="int", dest="max_trials", default=64, help='--joint: trial points of the joint solve')
  return cmd_parser.parse_args(argv)


def main(argv=None):
  opts, _ = parse_options(argv)
  if (opts.photo is None) == (opts.clip is None) or (opts.size is None and opts.image is None) or opts.out is None or (opts.image and opts.clip):
    logger.error('Please check your parameters: one of --photo / --clip, --size H W (or --photo with --image) and --out are needed.')
    exit(0)
  if not (os.path.exists(BFM_MAT) and os.path.exists(LM3D_MAT)):
    logger.error('%s and %s are needed', BFM_MAT, LM3D_MAT)
    exit(0)
  from scipy.io import loadmat
  from voicepuppet_amd.bfmfit import FaceFitter, crop_alignment, preprocess_landmarks
  fitter = FaceFitter(_BFM(loadmat(BFM_MAT)))
  lm3D = loadmat(LM3D_MAT)['lm']
  image = None
  if opts.image:
    from PIL import Image
    image = np.array(Image.open(opts.image).convert('RGB'), np.uint8)                     # (a writable copy)
    if opts.size is not None and tuple(opts.size) != image.shape[:2]:
      logger.error('--size %d %d does not match %s (%d x %d)', opts.size[0], opts.size[1], opts.image, image.shape[0], image.shape[1])
      exit(0)
  img_h, img_w = opts.size if image is None else image.shape[:2]
  if opts.photo:
    lms = read_landmarks(opts.photo)
    photo = fitter.enroll(lms[0], img_h, img_w, lm3D, image=image, lam_tex=opts.lam_tex, lam_gamma=opts.lam_gamma,
                          visibility=opts.visibility, prefilter=opts.prefilter)
    np.savez(opts.out, **photo)
    import torch
    coeff = torch.from_numpy(photo['bfmcoeff']).to(fitter.model.device)
    line = summary_line(opts.photo, fitter.last_report, reprojection_error(fitter, coeff, fitter.last_landmarks.reshape(1, 68, 2)))
    if image is not None:
      line += appearance_summary(fitter)
    print(line)
    return
  lms = read_landmarks(opts.clip)
  aligned = np.stack([preprocess_landmarks(crop_alignment(lm, img_h, img_w)[0], lm3D)[0] for lm in lms])
  if opts.smooth is not None and not opts.joint:
    logger.error('--smooth needs --joint')
    exit(0)
  if opts.joint:
    coeff, report = fitter.fit_clip(aligned, lam_smooth=opts.smooth or (0.0, 0.0, 0.0), max_trials=opts.max_trials)
    np.savetxt(opts.out, coeff.cpu().numpy(), delimiter=',', fmt='%.8g')
    print(joint_summary_line(opts.clip, report, reprojection_error(fitter, coeff, aligned)))
    return
  coeff, report = fitter.fit_sequence(aligned, rounds=opts.rounds, id_steps=opts.id_steps)
  np.savetxt(opts.out, coeff.cpu().numpy(), delimiter=',', fmt='%.8g')
  print(summary_line(opts.clip, report, reprojection_error(fitter, coeff, aligned)))


if (__name__ == '__main__'):
  main()

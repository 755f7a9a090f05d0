#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Audio -> talking mesh video, same CLI as the reference (voicepuppet/bfmnet/infer_bfmnet.py):

    python voicepuppet/bfmnet/infer_bfmnet.py --config_path config/params.yml <image> <audio.wav>

wav -> log-mel -> BFMNet -> 64 expression coefficients per video frame, spliced into the photo's 257 coefficients (:196-198) ->
`Reconstruction` of every frame (:209), packed as :212-216 (112 - x*112, 112 - y*112, z, all times 3) -> the rasteriser at 672 x 672
(:218-228) -> <output_dir>/<i>.jpg (-> ffmpeg mux when ffmpeg exists; --avi writes <output_dir>.avi without it).  No generator runs.

Reconstruction and rasteriser work on the device, --frame_batch frames per launch chain (voicepuppet_amd.utils.reconstruct_mesh.
ClipRenderer.render_view: vp_bfm_reconstruct_view view 1 + vp_render_colors).  They need BFM/BFM_model_front.mat and the photo's own
coefficients, which the reference takes from FaceReconModel.pb and the MXNet aligner (:73-118, :169-170; out of scope, as for
infer_bfmvid.py): pass them as `--bfmcoeff <npz with bfmcoeff[1,257]>`.  The image argument is what the reference fits those
coefficients to; it is accepted for the command line's sake and not read.  The options are infer_bfmvid.py's own.

Channel order: the reference swaps the raster (cvtColor, :230) and cv2.imwrite reads the result as BGR (:232): the file's RGB is the
rasteriser's order, which is what is encoded here.
"""
import logging
import os
import shutil
import subprocess
import sys

import numpy as np

sys.path.append(os.getcwd())

from voicepuppet_amd.bfmnet.bfmnet import BFMNet
from voicepuppet_amd.generator.generator import DataGenerator
from voicepuppet_amd.generator.loader import WavLoader
from voicepuppet_amd.pixrefer.infer_bfmvid import BFMNET_CKPT, clip_renderer, parse_options, prepare_pcm, restore_or_init, splice_coeff
from voicepuppet_amd.runtime import Session, convert_to_tensor
from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer

logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
logger = logging.getLogger(__name__)

IMG_SIZE, SCALE = 672, 3          # infer_bfmnet.py:216-218
BFM_MAT = os.path.join('BFM', 'BFM_model_front.mat')


def ears_sequence(pad_len):
  """infer_bfmnet.py:162-164: 0.2 over the first half of the clip, 0.9 over the rest."""
  ears = np.ones([1, pad_len, 1], dtype=np.float32) * 0.9
  for i in range(pad_len // 2):
    ears[0, i, 0] = 0.2
  return ears


def predict_coefficients(config_path, audio_file, bfmcoeff_file):
  """infer_bfmnet.py:146-198: the clip's [T,257] float32 coefficients (the photo's, with BFMNet's expression per frame spliced in), the
  16 kHz signal they were predicted from, and the generator whose constants time the frames."""
  ### Generator for inference setting
  infer_generator = DataGenerator(config_path)
  params = infer_generator.params
  params.batch_size = 1
  infer_generator.set_params(params)
  pcm = WavLoader(sr=infer_generator.sample_rate).get_data(audio_file)
  pcm_slice, pad_len = prepare_pcm(pcm, infer_generator)
  mfcc = infer_generator.extract_mfcc(pcm_slice)

  with Session() as sess:
    seq_len = convert_to_tensor(np.array([pad_len], dtype=np.int32))
    ears = convert_to_tensor(ears_sequence(pad_len))

    ### BFMNet setting
    bfmnet = BFMNet(config_path)
    params = bfmnet.params
    params.batch_size = 1
    bfmnet.set_params(params)
    infer_nodes = bfmnet.build_inference_op(ears, mfcc, seq_len)
    restore_or_init(bfmnet, BFMNET_CKPT)

    ### Run inference
    bfm_coeff_seq = sess.run(infer_nodes['BFMCoeffDecoder'])
  photo = np.load(bfmcoeff_file)
  coeff_seq = splice_coeff(photo['bfmcoeff'].reshape(1, 257), bfm_coeff_seq)[0]                     # :196-198
  return np.ascontiguousarray(coeff_seq, dtype=np.float32), pcm, infer_generator


def main(argv=None):
  opts, argv = parse_options(argv)
  avi = opts.avi or opts.avi_only
  if avi:
    opts.device_jpeg = True           # the video chunks are the device encoder's files

  if (opts.config_path is None):
    logger.error('Please check your parameters.')
    exit(0)
  config_path = opts.config_path
  if (not os.path.exists(config_path)):
    logger.error('config_path not exists')
    exit(0)

  image_file, audio_file = argv
  if not opts.bfmcoeff or not os.path.exists(BFM_MAT):
    logger.error('%s and --bfmcoeff <npz> are needed: there is no mesh to draw without them', BFM_MAT)
    exit(0)

  out_dir = opts.output_dir
  if not os.path.exists(out_dir):
    os.makedirs(out_dir)
  for file in os.listdir(out_dir):
    p = os.path.join(out_dir, file)
    shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)

  coeff_seq, pcm, infer_generator = predict_coefficients(config_path, audio_file, opts.bfmcoeff)
  import torch
  T = coeff_seq.shape[0]
  nb = max(1, min(opts.frame_batch, T))
  dev = torch.device('cuda', torch.cuda.current_device())
  renderer = ClipRenderer(clip_renderer().model, IMG_SIZE, IMG_SIZE)       # the face model's bases are on the device once per process
  coeff_d = torch.from_numpy(coeff_seq).to(dev)

  # The reference advances an `angles` variable per frame here (:202-207) that Reconstruction never reads: the pose of every frame is
  # the photo's own coeff[224:227].  No rotation is invented for it.

  from concurrent.futures import ThreadPoolExecutor
  from PIL import Image
  pool = ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1)))
  pending = []

  def write_jpg(arr_u8, path):
    Image.fromarray(arr_u8).save(path)

  def write_bytes(data, path):
    with open(path, 'wb') as fh:
      fh.write(data)
  encoder = muxer = writer = None
  if opts.device_jpeg:
    from voicepuppet_amd.jpeg import JpegEncoder
    encoder = JpegEncoder(IMG_SIZE, IMG_SIZE, nb, quality=75)
  if avi:
    from voicepuppet_amd.avi import AviMuxer, AviWriter
    spf = infer_generator.frame_wav_scale
    pcm_d = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.float32)).to(dev)
    n_pcm = int(pcm_d.numel())
    muxer = AviMuxer(nb, encoder.capacity, 1, max(n_pcm, 1), quality=75)
    writer = AviWriter(out_dir.rstrip('/') + '.avi', IMG_SIZE, IMG_SIZE, frame_us=int(round(1e6 * spf / infer_generator.sample_rate)),
                       sample_rate=infer_generator.sample_rate)
    slot0 = torch.zeros(nb, dtype=torch.int32, device=dev)
  try:
    for i0 in range(0, T, nb):
      n = min(nb, T - i0)
      # the photo's texture coefficients are constant over the clip: one texture per batch
      u8, _ = renderer.render_view(coeff_d[i0:i0 + n], view=1, scale=SCALE, shared_texture=True)
      if encoder is None:
        frames = u8.cpu().numpy()
        for k in range(n):
          pending.append(pool.submit(write_jpg, frames[k], os.path.join(out_dir, '{}.jpg'.format(i0 + k))))
        continue
      data, lengths = encoder.encode(u8)
      if muxer is not None:
        a = min(i0 * spf, n_pcm)
        b = n_pcm if i0 + n >= T else min((i0 + n) * spf, n_pcm)
        seg = muxer.segment(data, lengths, slot0[:n], pcm_d if n_pcm else None, [a], [b - a])
        for segment, entries in muxer.to_host(seg, u8).values():
          writer.append(segment, entries)
        if opts.avi_only:
          continue
      files = encoder.to_host(data, lengths, u8)
      for k in range(n):
        pending.append(pool.submit(write_bytes, files[k], os.path.join(out_dir, '{}.jpg'.format(i0 + k))))
    for f in pending:
      f.result()           # every frame is on disk (and any write error surfaces) before ffmpeg reads the directory
  finally:
    pool.shutdown()
    if writer is not None:
      writer.close()
  if writer is not None:
    logger.info('wrote %s', ', '.join(writer.paths))
  if opts.avi_only:
    return

  if shutil.which('ffmpeg'):
    # same command line as infer_bfmnet.py:234, as an argument vector (no shell: the audio path is user input)
    subprocess.call(['ffmpeg', '-i', os.path.join(out_dir, '%d.jpg'), '-i', audio_file, '-c:v', 'libx264', '-c:a', 'aac',
                     '-strict', 'experimental', '-y', out_dir.rstrip('/') + '.mp4'])
  else:
    logger.warning('ffmpeg not found: frames are in %s, no mp4 written', out_dir)


if (__name__ == '__main__'):
  main()

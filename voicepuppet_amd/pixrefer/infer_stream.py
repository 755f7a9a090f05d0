#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Streaming end-to-end inference: the infer_bfmvid command line plus --chunk_ms.

    python voicepuppet/pixrefer/infer_stream.py --config_path config/params.yml --chunk_ms 40 <image 1536x512> <audio.wav>

The wav is fed to voicepuppet_amd.stream.PuppetStream in chunks of chunk_ms milliseconds, as a live source would deliver it. Every
frame is written to output/<i>.jpg as soon as it is emitted, and the per-push latency is logged. At the end the clip is finished and
muxed as infer_bfmvid muxes it. --native_pcm pushes the wav as stored (its rate, channels, int16 or float32 samples; chunk_ms of source
frames per push) and leaves conversion, down-mix and resampling to the device (voicepuppet_amd.pcm) instead of WavLoader. --device_jpeg encodes the frames on the device (voicepuppet_amd.jpeg) and writes those bytes. Under the same np.random.seed the frames are infer_bfmvid's: same count, same ears, same conditioning
by global frame index, coefficients bit-identical or within 1e-5 of max|offline| (tests/test_gpu_stream_cli.py
states what that means in pixels).
"""
import logging
import math
import os
import shutil
import subprocess
import sys
import time
from optparse import OptionParser

import numpy as np

sys.path.append(os.getcwd())

from voicepuppet_amd.generator.generator import DataGenerator
from voicepuppet_amd.generator.loader import ImageLoader, WavLoader

logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(name)s - %(levelname)s - %(message)s')
logger = logging.getLogger(__name__)


def parse_options(argv=None):
  """(options, positional arguments) of the command line."""
  cmd_parser = OptionParser(usage="usage: %prog [options] --config_path <> image audio")
  cmd_parser.add_option('--config_path', type="string", dest="config_path", help='the config yaml file')
  cmd_parser.add_option('--frame_batch', type="int", dest="frame_batch", default=8, help='frames per device batch')
  cmd_parser.add_option('--bfmcoeff', type="string", dest="bfmcoeff", default=None,
                        help='npz with the photo\'s bfmcoeff [1,257], transform_params [5], center_x, center_y, ratio')
  cmd_parser.add_option('--output_dir', type="string", dest="output_dir", default='output', help='frame directory')
  cmd_parser.add_option('--chunk_ms', type="float", dest="chunk_ms", default=40.0, help='audio per push, milliseconds')
  cmd_parser.add_option('--device_jpeg', action="store_true", dest="device_jpeg", default=False,
                        help='encode the .jpg files on the device (quality 75) instead of PIL on the host pool')
  cmd_parser.add_option('--native_pcm', action="store_true", dest="native_pcm", default=False,
                        help='push the wav as it is (its rate, channels and sample type): converted and resampled on the device, chunk by chunk')
  cmd_parser.add_option('--avi', action="store_true", dest="avi", default=False,
                        help='also write <output_dir>.avi (Motion-JPEG + 16-bit PCM, built on the device; implies --device_jpeg)')
  cmd_parser.add_option('--avi_only', action="store_true", dest="avi_only", default=False,
                        help='--avi without the per-frame .jpg files and without the ffmpeg call')
  return cmd_parser.parse_args(argv)


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
  if not opts.chunk_ms > 0:
    logger.error('--chunk_ms must be positive')
    exit(0)

  image_file, audio_file = argv
  out_dir = opts.output_dir
  if not os.path.exists(out_dir):
    os.makedirs(out_dir)
  for file in os.listdir(out_dir):
    p = os.path.join(out_dir, file)
    shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)

  gen = DataGenerator(config_path)
  params = gen.params
  params.batch_size = 1
  gen.set_params(params)
  pcm_format = None
  if opts.native_pcm:
    from voicepuppet_amd.pcm import read_wav
    rate, pcm, fmt = read_wav(audio_file)                   # [frames, channels] as stored; chunk_ms of SOURCE frames per push
    pcm_format = (rate, pcm.shape[1], fmt)
  else:
    rate = gen.sample_rate
    pcm = WavLoader(sr=gen.sample_rate).get_data(audio_file).astype(np.float32)
  img = ImageLoader().get_data(image_file)[:, :, ::-1]      # RGB float in [0,1], 512 x 1536

  from voicepuppet_amd.stream import PuppetStream
  chunk = max(1, int(round(opts.chunk_ms * rate / 1000.0)))
  frame_ms = 1000.0 * gen.frame_wav_scale / gen.sample_rate
  # a window emits at most the frames one chunk completes (a catch-up push runs several windows)
  stream = PuppetStream(config_path, img, bfmcoeff=opts.bfmcoeff, frame_batch=opts.frame_batch,
                        max_chunk_frames=max(1, int(math.ceil(opts.chunk_ms / frame_ms))),
                        **({'jpeg_quality': 75} if opts.device_jpeg else {}), **({'pcm_format': pcm_format} if pcm_format else {}),
                        **({'avi': True} if avi else {}))
  if avi:
    stream.record(out_dir.rstrip('/') + '.avi', frame_us=int(round(1000.0 * frame_ms)))
  logger.info('streaming %d samples in chunks of %d (%.0f ms), lookahead %.0f ms', pcm.shape[0], chunk, opts.chunk_ms,
              stream.audio.lookahead_ms)

  from PIL import Image
  from concurrent.futures import ThreadPoolExecutor
  pool = ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1)))
  pending, lat = [], []

  def write_jpg(arr_u8, path):
    if opts.device_jpeg:               # the device's bytes: a plain file write
      with open(path, 'wb') as fh:
        fh.write(arr_u8)
      return
    Image.fromarray(arr_u8).save(path)

  def emit(frames):
    if opts.avi_only:                  # the frames are in the .avi (PuppetStream appends every push to the open recording)
      return
    for i, f in frames:
      pending.append(pool.submit(write_jpg, f, os.path.join(out_dir, '{}.jpg'.format(i))))

  try:
    for at in range(0, pcm.shape[0], chunk):
      t = time.perf_counter()
      frames = stream.push_raw(pcm[at:at + chunk]) if opts.native_pcm else stream.push(pcm[at:at + chunk])
      lat.append(1000.0 * (time.perf_counter() - t))
      emit(frames)
      logger.debug('push %d: %d frames, %.2f ms', len(lat), len(frames), lat[-1])
    t = time.perf_counter()
    emit(stream.finish())
    fin_ms = 1000.0 * (time.perf_counter() - t)
    for f in pending:
      f.result()
  finally:
    pool.shutdown()
  if lat:
    logger.info('%d pushes: latency median %.2f ms, max %.2f ms (frames included); finish %.2f ms; %d frames', len(lat),
                float(np.median(lat)), float(np.max(lat)), fin_ms, stream.frame)

  if avi:
    logger.info('wrote %s', ', '.join(stream.stop()))
  if opts.avi_only:
    return
  if shutil.which('ffmpeg'):
    # infer_bfmvid's mux (infer_bfmvid.py:245), as an argument vector
    subprocess.call(['ffmpeg', '-i', os.path.join(out_dir, '%d.jpg'), '-i', audio_file, '-c:v', 'libx264', '-c:a', 'aac',
                     '-strict', 'experimental', '-y', out_dir.rstrip('/') + '.mp4'])
  else:
    logger.warning('ffmpeg not found: frames are in %s/, no mp4 written', out_dir)


if (__name__ == '__main__'):
  main()

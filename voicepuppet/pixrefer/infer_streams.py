#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Launcher beside infer_stream.py for many talkers at once (a list file of `image audio.wav [photo.npz]` lines):
    python voicepuppet/pixrefer/infer_streams.py --config_path config/params.yml --chunk_ms 40 --output_dir output list.txt
The implementation lives in voicepuppet_amd/pixrefer/infer_streams.py."""
import os
import sys

sys.path.append(os.getcwd())

from voicepuppet_amd.pixrefer.infer_streams import main

if (__name__ == '__main__'):
  main()

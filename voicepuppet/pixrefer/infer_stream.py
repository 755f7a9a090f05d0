#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Launcher beside infer_bfmvid.py for the streaming form of the same command line (plus --chunk_ms):
    python voicepuppet/pixrefer/infer_stream.py --config_path config/params.yml --chunk_ms 40 ...
The implementation lives in voicepuppet_amd/pixrefer/infer_stream.py."""
import os
import sys

sys.path.append(os.getcwd())

from voicepuppet_amd.pixrefer.infer_stream import main

if (__name__ == '__main__'):
  main()

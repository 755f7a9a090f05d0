#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Launcher beside the reference's scripts (in place of steps 5 and 6 of its datasets/make_data_from_GRID.py):
    python voicepuppet/datasets/make_triptychs.py --clip_dir frames/ --landmarks frames/_landmark.txt --out_dir data/clip0 --list train.txt
The implementation lives in voicepuppet_amd/datasets/make_triptychs.py."""
import os
import sys

sys.path.append(os.getcwd())

from voicepuppet_amd.datasets.make_triptychs import main

if (__name__ == '__main__'):
  main()

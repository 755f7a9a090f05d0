#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Launcher beside the reference's scripts (the reference has no counterpart: it fits coefficients with FaceReconModel.pb):
    python voicepuppet/bfmnet/fit_landmarks.py --photo landmarks.txt --size H W --out photo.npz
The implementation lives in voicepuppet_amd/bfmnet/fit_landmarks.py."""
import os
import sys

sys.path.append(os.getcwd())

from voicepuppet_amd.bfmnet.fit_landmarks import main

if (__name__ == '__main__'):
  main()

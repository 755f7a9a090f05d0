"""Writes tests/golden/key_matte.npz: three 96 x 80 frames of the synthetic studio scene (tests/key_matte_ref.py) with the moments, the
model, the raw key and the matte the restatement gives for them at the defaults.  tests/test_key_matte_host.py compares the restatement
of the day with this record, so that a drift of the restatement itself is visible.  Usage: python tests/golden/make_key_matte_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import key_matte_ref as kr  # noqa: E402

PATH = os.path.join(HERE, "key_matte.npz")


def main():
  frames, alpha = kr.scene(96, 80, seed=1, n=3)
  S, model = kr.fit(frames)
  raw, matte = kr.matte(model, frames)
  np.savez_compressed(PATH, frames=frames, moments=S, model=model, raw=raw, matte=matte)
  print(PATH, os.path.getsize(PATH), "bytes; model", model)


if __name__ == "__main__":
  main()

"""The device PNG encoder (libvp_hip.so vp_png_*, voicepuppet_amd.png) against the restatement of its byte stream (tests/png_ref.py, itself
checked against PIL and zlib in tests/test_png_host.py): equal bytes, and PIL's decode of every file."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402
from test_png_host import goldens  # noqa: E402

pytestmark = pytest.mark.gpu


def pil_pixels(data):
  from PIL import Image
  im = Image.open(io.BytesIO(data))
  im.load()
  return np.asarray(im)


def device_files(frames, filter=-1, channels=None, channel_offset=0, strips=False):
  """frames: numpy [K, H, W] or [K, H, W, P] -> the K files (and the last_strips table)"""
  import torch
  from voicepuppet_amd.png import PngEncoder
  t = torch.from_numpy(np.ascontiguousarray(frames)).to("cuda")
  P = 1 if t.dim() == 3 else int(t.shape[3])
  enc = PngEncoder(int(t.shape[0]), int(t.shape[1]), int(t.shape[2]), channels=channels or P, filter=filter)
  files = enc.files(t, channel_offset=channel_offset)
  assert all(f[:47] == enc.header() for f in files)
  assert all(len(f) <= enc.capacity for f in files)
  return (files, enc.last_strips()) if strips else files


def check(img, filter=-1):
  """One uint8 image: the device's bytes are the restatement's, and PIL reads the input back."""
  want, info = png_ref.encode_strips(img, filter)
  (got,), table = device_files(img[None], filter, strips=True)
  assert np.array_equal(pil_pixels(got).reshape(img.shape), img)
  assert table[0].tolist() == [[n, int(s)] for n, s in info]
  assert got == want
  return info


def test_one_pixel():
  check(np.array([[[3, 200, 77]]], np.uint8))


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_17x5_partial_last_strip(channels):
  img = np.random.default_rng(channels).integers(0, 256, (17, 5, channels)).astype(np.uint8)
  info = check(img[..., 0] if channels == 1 else img)
  assert len(info) == 2


def test_noise_is_stored():
  info = check(np.random.default_rng(7).integers(0, 256, (48, 64, 3)).astype(np.uint8))
  assert all(s for _, s in info)


def test_long_runs_and_runs_cut_at_strip_ends():
  info = check(np.full((40, 300, 3), 77, np.uint8), filter=0)
  assert not any(s for _, s in info)
  y, x = np.mgrid[0:40, 0:300]
  half = np.where(x + y < 170, 0, 255).astype(np.uint8)
  for f in (0, -1):
    check(np.stack([half, half, half], -1), filter=f)
  check(np.full((40, 300, 3), 77, np.uint8))


@pytest.mark.parametrize("filter", [0, 1, 2, 3, 4, -1])
def test_filters_on_the_256_frame(filter):
  check(goldens()["frame"], filter)


def test_three_frames_in_one_call():
  g = goldens()
  frames = np.stack([g["frame"], g["matte"], np.random.default_rng(1).integers(0, 256, (256, 256, 3)).astype(np.uint8)])
  files = device_files(frames)
  for f, img in zip(files, frames):
    assert f == png_ref.encode(img) and np.array_equal(pil_pixels(f), img)


def test_float32_channels_3_to_6_of_a_6_channel_pixel():
  rng = np.random.default_rng(2)
  x = rng.random((2, 20, 33, 6), dtype=np.float32)
  special = np.array([-0.1, 0.0, 0.5 / 255.5, 1.0, 1.2, np.nan, -np.inf, np.inf, 254.9 / 255.5, 1.0 / 255.5], np.float32)
  x[0, 0, :special.size, 3] = special
  x[1, 19, -special.size:, 5] = special
  x[..., :3] = np.nan                                  # the channels the encode must not read as pixels
  files = device_files(x, channels=3, channel_offset=3)
  for f, frame in zip(files, x):
    want = png_ref.to_u8(frame[..., 3:6])
    assert np.array_equal(pil_pixels(f), want) and f == png_ref.encode(want)
  assert pil_pixels(files[0])[0, :6, 0].tolist() == [0, 0, 0, 255, 255, 0]
  grey = device_files(x[..., 3:4].copy(), channels=1)
  assert np.array_equal(pil_pixels(grey[1]), png_ref.to_u8(x[1, ..., 3]))


def test_one_512_frame():
  check(goldens()["sample22_panel"])


def test_length_limit_on_fibonacci_frequencies():
  """A 1-channel 16 x 1024 image, filter None, whose strip (the 16 filter bytes included, which are 16 of its 21 zeros) has the byte
  counts 1, 2, 3, 5, 8, ... 4181 and, for the bytes that are left, 5456; no two equal bytes are neighbours, so every byte is a literal
  and with end-of-block the symbol counts are 1, 1, 2, 3, 5, ...: Huffman's code for them is 18 deep."""
  fib = [1, 2]
  while sum(fib) + fib[-1] + fib[-2] <= 16 * 1025:
    fib.append(fib[-1] + fib[-2])
  fib.append(16 * 1025 - sum(fib))
  values = [3 + 7 * i for i in range(len(fib))]
  values[fib.index(21)] = 0
  data = dict(zip(values, fib))
  data[0] -= 16
  vals = np.concatenate([np.full(n, v, np.uint8) for v, n in sorted(data.items(), key=lambda kv: -kv[1])])
  flat = np.empty(16 * 1024, np.uint8)
  flat[np.concatenate([np.arange(0, flat.size, 2), np.arange(1, flat.size, 2)])] = vals      # the most frequent first, on every other place
  img = flat.reshape(16, 1024)
  assert png_ref.rows_per_strip(1024, 1) == 16
  strip = png_ref.filtered_rows(img, 0).ravel()
  assert not np.any(strip[1:] == strip[:-1])
  counts = np.bincount(strip, minlength=286)
  counts[256] = 1
  assert sorted(c for c in counts.tolist() if c) == [1] + fib
  assert max(png_ref.huff_lengths(counts.tolist(), 64)) == 18 and max(png_ref.huff_lengths(counts.tolist(), 15)) == 15
  info = check(img, filter=0)
  assert not info[0][1]


def test_two_encodes_give_the_same_bytes():
  import torch
  from voicepuppet_amd.png import PngEncoder
  img = goldens()["face3d"]
  enc = PngEncoder(1, 256, 256)
  t = torch.from_numpy(img).to("cuda")[None]
  a = enc.files(t)
  b = enc.files(t)
  assert a == b and a[0] == png_ref.encode(img)

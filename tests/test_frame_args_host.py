"""The frame and plane checks the image wrappers share (voicepuppet_amd._handle: frame_layout, rgb_frames, u8_plane), without a GPU: the
stride arithmetic reads shape and strides only, so CPU tensors cover it; the refusals' texts are the ones KeyMatte, MatteCleaner,
MatteSolver and FrameMetrics raised before they shared them, but for the stride refusal's first word, which is the caller's method."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voicepuppet_amd._handle import frame_layout, rgb_frames, u8_plane  # noqa: E402

H, W = 16, 20


def test_dense_and_padded_views():
  assert frame_layout(torch.zeros(2, H, W, 3, dtype=torch.uint8), "fit") == (3 * W, H * 3 * W)
  rows = torch.zeros(2, H, 24, 3, dtype=torch.uint8)[:, :, :W]                    # padded rows: a decoder's output
  assert not rows.is_contiguous() and frame_layout(rows, "matte") == (72, H * 72)
  frames = torch.zeros(2, H + 2, W, 3, dtype=torch.uint8)[:, :H]                  # padded frames
  assert not frames.is_contiguous() and frame_layout(frames, "solve") == (3 * W, (H + 2) * 3 * W)
  both = torch.zeros(3, H + 1, W + 3, 3, dtype=torch.uint8)[1:, :H, :W]
  assert frame_layout(both, "compare", "a") == (3 * (W + 3), (H + 1) * 3 * (W + 3))


def test_single_frame_stride_is_arbitrary():
  one = torch.zeros(H * W * 3, dtype=torch.uint8).as_strided((1, H, W, 3), (7, 3 * W, 3, 1))
  assert frame_layout(one, "fit") == (3 * W, (H - 1) * 3 * W + 3 * W)
  padded = torch.zeros(H * 72, dtype=torch.uint8).as_strided((1, H, W, 3), (1, 72, 3, 1))
  assert frame_layout(padded, "fit") == (72, (H - 1) * 72 + 3 * W)
  assert frame_layout(torch.zeros(2, H, W, 3, dtype=torch.uint8)[1:], "fit") == (3 * W, H * 3 * W)     # a larger one is kept


def test_float32_layout_is_in_bytes():
  assert frame_layout(torch.zeros(2, H, W, 3), "compare", "b") == (4 * 3 * W, 4 * H * 3 * W)
  rows = torch.zeros(2, H, 24, 3)[:, :, :W]
  assert frame_layout(rows, "compare", "b") == (4 * 72, 4 * H * 72)
  one = torch.zeros(H * W * 3).as_strided((1, H, W, 3), (5, 3 * W, 3, 1))
  assert frame_layout(one, "compare", "a") == (4 * 3 * W, 4 * ((H - 1) * 3 * W + 3 * W))


@pytest.mark.parametrize("who", ["fit", "matte", "foreground", "solve", "laplacian", "compare"])
def test_refusals_carry_the_callers_name(who):
  store = torch.zeros(2 * H * W * 4, dtype=torch.uint8)
  views = {
    "overlapping rows": store.as_strided((2, H, W, 3), (H * 3 * W, 3 * W - 1, 3, 1)),
    "overlapping frames": store.as_strided((2, H, W, 3), (H * 3 * W - 1, 3 * W, 3, 1)),
    "channels apart": store.view(2, H, W, 4)[..., :3],
    "channels first": store[:2 * H * W * 3].view(2, 3, H, W).permute(0, 2, 3, 1),
  }
  for case, t in views.items():
    with pytest.raises(ValueError) as e:
      frame_layout(t, who, "frames")
    text = str(e.value)
    assert text.startswith(who + ": frames has strides " + str(tuple(t.stride()))), case
    assert text.endswith("a pixel's values and a row's pixels must be adjacent, rows and frames must not overlap"), case


def test_shape_dtype_and_device_texts():
  """A CPU tensor is never a device tensor: every check refuses it, in the words the wrappers used before."""
  with pytest.raises(ValueError, match=r"^fit: a device uint8 tensor \[n, H, W, 3\]$"):
    rgb_frames(torch.zeros(2, H, W, 3, dtype=torch.uint8), "fit")
  with pytest.raises(ValueError, match=r"^solve: a device uint8 tensor \[n, H, W, 3\]$"):
    rgb_frames(torch.zeros(2, H, W, 4, dtype=torch.uint8), "solve")
  plane = torch.zeros(2, H, W, dtype=torch.uint8)
  with pytest.raises(ValueError, match=r"^clean: matte must be a contiguous device uint8 tensor \[n, H, W\]$"):
    u8_plane(plane, "clean", "matte")
  with pytest.raises(ValueError, match=r"^matte: raw must be a contiguous device uint8 \[>= 2, 16, 20\]$"):
    u8_plane(plane, "matte", "raw", 2, H, W)
  with pytest.raises(ValueError, match=r"^foreground: matte must be a contiguous device uint8 \[2, 16, 20\]$"):
    u8_plane(plane, "foreground", "matte", 2, H, W, exact=True)
  with pytest.raises(ValueError, match=r"^foreground: out must be a contiguous device uint8 \[>= 2, 16, 20, 3\]$"):
    u8_plane(torch.zeros(2, H, W, 3, dtype=torch.uint8), "foreground", "out", 2, H, W, channels=3)

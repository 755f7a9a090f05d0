// Constants shared by the thin-channel tile kernels (conv_thin.hip) and their launchers: the geometry of the 6 x 18 pixel halo tile a
// block stages in LDS and the size of the 3x3-neighbourhood weight image, so that the dynamic LDS of a launch is sized from the figures
// the kernel indexes with.
#pragma once

namespace vp {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// The halo tile of a 4 x 16 pixel block: 6 x 18 pixels of CIN bf16 channels at a padded pixel pitch (PIXB: the 16 lanes of a fragment
// read hit 64 distinct banks), moved as 16-byte pieces, NJ per thread of a 256-thread block; threads beyond the last piece write a dummy
// 16-byte slot of their own behind the tile.
template <int CIN_>
struct ThinHalo {
  static constexpr int CIN = CIN_, PPP = CIN / 8;                 // 16-byte pieces per pixel
  static constexpr int PIXB = CIN * 2 + 16, TPX = 6 * 18, NPIECE = TPX * PPP, NJ = (NPIECE + 255) / 256;
  static constexpr int LDS_BYTES = TPX * PIXB + 256 * 16;         // [6][18][PIXB], then 256 dummy 16-byte slots
};

// The weight image of a 4x4 stride-2 transposed convolution over the 3x3 input neighbourhood of a base pixel, in MFMA A-fragment order
// [16-row tile][tap x channel step][lane]: NT tiles, SPT = Cin / 32 MFMA steps per tap
template <int SPT, int NT> constexpr int thin_weight_image_bytes = NT * 9 * SPT * 64 * 16;

}  // namespace vp

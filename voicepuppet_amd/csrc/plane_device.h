// Device helpers of the register-loader kernels (igemm_kernel in conv_kernels.hip, wgrad_kernel in wgrad_kernels.hip).
//
// LDS plane layout: a tile of ROWS rows x 64 bytes of K is stored as 4 planes (one per 16-byte k-piece g), plane g = ROWS consecutive
// 16-byte slots.  MFMA lane (i = lane&15, g = lane>>4) reads slot(row0+i) of plane g with one ds_read_b128: the 16 lanes of every b128
// service group hit 16 distinct 16-byte slots of a 256-byte bank row (conflict-free); writers use 8-lane contiguous (row loader) or
// XOR-swizzled (transposing loader) slots.
#pragma once
#include "conv_args.h"
#include "vp_common.h"

namespace vp {

// ------------------------------------------------------------------------------------------------
// slot permutation inside a 16-row block (b = row >> 4)
//   SWZ 0: identity (row loader)
//   SWZ 1: transposing loader; a thread owns E consecutive rows and writes them in E instructions,
//          so lanes of one ds_write_b128 group are E rows apart -> spread them over the 8 slots.
// ------------------------------------------------------------------------------------------------
template <int SWZ, int E> __device__ __forceinline__ int lds_slot(int row) {
  if (SWZ == 0) return row;
  int r = row & 15, b = row >> 4;
  int s16;
  if (E == 4) s16 = (((r & 3) << 2) | (r >> 2)) ^ ((b & 1) << 2);
  else        s16 = (((r & 7) << 1) | (r >> 3)) ^ ((b & 3) << 1);
  return (row & ~15) | s16;
}

// acc[tc][tp] += A(tile tc) x B(tile tp) for one 64-byte K chunk
template <typename T, int TC, int TP, int BC, int BP, int SWZ>
__device__ __forceinline__ void mma_chunk(const uint4* __restrict__ ldsA, const uint4* __restrict__ ldsB,
                                          int rowA0, int rowB0, int lane, f32x4 (&acc)[TC][TP]) {
  constexpr int E = Elem<T>::E;
  const int i = lane & 15, g = lane >> 4;
  uint4 fa[TC], fb[TP];
#pragma unroll
  for (int t = 0; t < TC; ++t) fa[t] = ldsA[g * BC + lds_slot<SWZ, E>(rowA0 + t * 16 + i)];
#pragma unroll
  for (int t = 0; t < TP; ++t) fb[t] = ldsB[g * BP + lds_slot<SWZ, E>(rowB0 + t * 16 + i)];
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp) acc[tc][tp] = mma16<T>(fa[tc], fb[tp], acc[tc][tp]);
}

// deferred-BN affine + activation on one 16-byte piece (channels c .. c+E-1 of BN group grp)
template <typename T>
__device__ __forceinline__ uint4 prologue_piece(uint4 v, const float* __restrict__ pa, const float* __restrict__ pb, int act) {
  constexpr int E = Elem<T>::E;
  if (pa == nullptr && act == ACT_NONE) return v;
  float f[E];
  Elem<T>::unpack(v, f);
  if (pa != nullptr) {
#pragma unroll
    for (int e = 0; e < E; e += 4) {
      const float4 a4 = *reinterpret_cast<const float4*>(pa + e);
      const float4 b4 = *reinterpret_cast<const float4*>(pb + e);
      f[e + 0] = fmaf(a4.x, f[e + 0], b4.x); f[e + 1] = fmaf(a4.y, f[e + 1], b4.y);
      f[e + 2] = fmaf(a4.z, f[e + 2], b4.z); f[e + 3] = fmaf(a4.w, f[e + 3], b4.w);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) f[e] = act_apply(act, f[e]);
  return Elem<T>::pack(f);
}

// Load channels [c, c+E) of pixel (n, ih, iw) of a PixSrc (after affine + act); zeros outside.
template <typename T>
__device__ __forceinline__ uint4 load_pix_piece(const PixSrc& x, int n, int ih, int iw, int H, int W, int c, bool ok) {
  if (!ok || (unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)W) return make_uint4(0, 0, 0, 0);
  // explicit selects (no dynamic indexing of the by-value argument block: that would go to scratch)
  const bool s = c >= x.C[0];
  const int cl = s ? c - x.C[0] : c;
  const int C = s ? x.C[1] : x.C[0];
  const T* p = reinterpret_cast<const T*>(s ? x.ptr[1] : x.ptr[0]) + ((size_t)(n * H + ih) * W + iw) * C + cl;
  uint4 v = *reinterpret_cast<const uint4*>(p);
  const float* pa = s ? x.aff_a[1] : x.aff_a[0];
  const float* pb = s ? x.aff_b[1] : x.aff_b[0];
  if (pa != nullptr) {
    const int off = (n / x.group_n) * C + cl;
    pa += off; pb += off;
  }
  return prologue_piece<T>(v, pa, pb, x.act);
}

}  // namespace vp

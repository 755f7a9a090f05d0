// Device helpers of the float64 fitters (bfm_fit.hip: the landmark fit; bfm_appear.hip: the photometric fit): packed-triangle indexing,
// fixed-order block reductions and the in-LDS Cholesky solve.  Workgroups of FIT_THREADS threads.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace vp {

constexpr int FIT_THREADS = 256;

__device__ __forceinline__ int tri_idx(int i, int j) { return i * (i + 1) / 2 + j; }

// fixed-order tree over the block's 256 values; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = FIT_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double block_max(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = FIT_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = (red[t + s] > red[t] || red[t + s] != red[t + s]) ? red[t + s] : red[t];      // a NaN wins
    __syncthreads();
  }
  return red[0];
}

// In-place Cholesky of the packed lower triangle a (rows 0 .. n; row n is a right-hand side that takes the forward substitution along),
// pivots to piv [n], then the back substitution: d [n] = solution of (L L^T) d = row n.  False (for every thread) when a pivot is not > 0.
__device__ inline bool chol_solve(double* a, double* piv, double* d, int n) {
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    const double akk = a[tri_idx(k, k)];
    if (!(akk > 0.0)) return false;                 // the same value for every thread: a uniform exit
    const double pv = sqrt(akk);
    for (int i = k + 1 + t; i <= n; i += FIT_THREADS) a[tri_idx(i, k)] /= pv;
    if (t == 0) piv[k] = pv;
    __syncthreads();
    for (int i = k + 1 + ty; i <= n; i += 16) {
      const double lik = a[tri_idx(i, k)];
      const int jend = i < n ? i : n - 1;
      for (int j = k + 1 + tx; j <= jend; j += 16) a[tri_idx(i, j)] -= lik * a[tri_idx(j, k)];
    }
    __syncthreads();
  }
  if (t < n) d[t] = a[tri_idx(n, t)];
  __syncthreads();
  for (int k = n - 1; k >= 0; --k) {
    const double dk = d[k] / piv[k];
    __syncthreads();
    if (t < k) d[t] -= a[tri_idx(k, t)] * dk;
    else if (t == k) d[k] = dk;
    __syncthreads();
  }
  return true;
}

}  // namespace vp

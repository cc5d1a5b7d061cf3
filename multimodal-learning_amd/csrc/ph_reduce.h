// The two fp32 sums over a workgroup of the head and loss kernels (dense.hip, zoo.hip, zoo_rkd.hip, surv.hip).  They add the
// same values in DIFFERENT orders, so their fp32 results differ: a kernel keeps the one it has.  Every thread of the
// workgroup must call (both contain barriers) and every thread gets the total.
#pragma once
#include "ph_common.h"

// Wave totals by xor-shuffle (wave_sum), then the wave totals added serially, wave 0 first.
// sh: one float per wave (16 for the largest workgroup).  Ends with a barrier: sh may be reused at once.
__device__ __forceinline__ float block_sum_waves(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += sh[i];
  __syncthreads();
  return t;
}

// Fixed LDS tree: thread t adds element t + o for o = n / 2, n / 4, .. 1 over n = blockDim.x threads (a power of two), or
// over the compile-time N of a kernel whose workgroup size is fixed.  red: n floats.  Ends with a barrier: red may be
// reused at once.  T: float, or double for the float64 sums of survstrata.hip (red: n values of T).
template <int N = 0, typename T = float>
__device__ __forceinline__ T block_sum_tree(T v, T* red) {
  const int tid = threadIdx.x, n = N ? N : (int)blockDim.x;
  red[tid] = v;
  __syncthreads();
  for (int o = n >> 1; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const T t = red[0];
  __syncthreads();
  return t;
}

// The sort-free "all-pairs" scan of the evaluation kernels (evalmetrics.hip, survstrata.hip, surv.hip):
// thread i holds one element, every element j streams through LDS in tiles of TILE = the workgroup size, and the thread
// counts, as exact integers, the j that stand in some relation to i.  Past the end the caller stages a NaN, which compares
// false with everything, so the last tile needs no bound.  With the scan: the integer and float64 tails these kernels share.
#pragma once
#include "ph_common.h"
#include "ph_reduce.h"

// The tile protocol.  fetch(j) returns what this thread stages for element j = j0 + tid - it is called past the end too
// (j >= n): the padding is the caller's; put(tid, v) writes it to LDS; body(j0) then reads the whole tile.  The fetch stands
// before the first barrier, so its global loads are in flight while the wave waits for the tile's last readers.  Every
// thread of the workgroup must call: an inactive one takes part in the barriers and skips the body.
template <int TILE, class Fetch, class Put, class Body>
__device__ __forceinline__ void pair_tiles(int n, bool active, Fetch fetch, Put put, Body body) {
  const int tid = threadIdx.x;
  for (int j0 = 0; j0 < n; j0 += TILE) {
    const auto v = fetch(j0 + tid);
    __syncthreads();
    put(tid, v);
    __syncthreads();
    if (active) body(j0);
  }
}

// The common body: visit(jj, lim) for every slot jj of the tile; the elements jj < lim = i - j0 of a tile come before i.
template <int TILE, class Fetch, class Put, class Visit>
__device__ __forceinline__ void pair_scan(int n, int i, bool active, Fetch fetch, Put put, Visit visit) {
  pair_tiles<TILE>(n, active, fetch, put, [&](int j0) {
    const int lim = i - j0;
#pragma unroll 8
    for (int jj = 0; jj < TILE; ++jj) visit(jj, lim);
  });
}

// ---- Distinct-value placement in two scans (ph_roc_points, ph_surv_table).  Scan 1: the FIRST of the elements with equal
// keys represents them - an element whose key is not a NaN and that no earlier element equals; rep[i] = its key, NaN for
// every other element.  Scan 2: the slot of a representative = the number of representatives whose key lies beyond its own
// (LARGER: above it, else below) - distinct keys, so a permutation of 0 .. points - 1.
__device__ __forceinline__ unsigned int equal_before(bool equal, int jj, int lim) { return (jj < lim && equal) ? 1u : 0u; }
__device__ __forceinline__ bool represents(float key, unsigned int before) { return key == key && before == 0; }
template <bool LARGER>
__device__ __forceinline__ unsigned int rep_beyond(float rep_j, float key) {
  return (LARGER ? rep_j > key : rep_j < key) ? 1u : 0u;
}

// ---- The integer tail: the wave's total of v, added by lane 0 where it is not zero.  Integer atomics: the result does not
// depend on the order.  Every lane of the wave must call.  A kernel with several counters may form the totals first and
// hand them to lane0_atomic_add: the shuffles of independent sums then overlap.
template <typename T>
__device__ __forceinline__ void lane0_atomic_add(T* p, T total) {
  if ((threadIdx.x & 63) == 0 && total) atomicAdd(p, total);
}
__device__ __forceinline__ void wave_atomic_add(unsigned long long* p, unsigned long long v) {
  lane0_atomic_add(p, wave_sum_u64(v));
}
__device__ __forceinline__ void wave_atomic_add(int* p, int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  lane0_atomic_add(p, v);
}

// ---- The float64 tail: thread t adds part[t * stride + offset], part[(t + N) * stride + offset], .. in that order, then
// the fixed tree of block_sum_tree over the N threads.  Fixed order: two runs agree bitwise.  red: N doubles.
template <int N>
__device__ __forceinline__ double strided_tree_sum(const double* __restrict__ part, int n, int stride, int offset, double* red) {
  double v = 0.0;
  for (int b = threadIdx.x; b < n; b += N) v += part[(size_t)b * stride + offset];
  return block_sum_tree<N, double>(v, red);
}

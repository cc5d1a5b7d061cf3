// Device k-means class centres of the MIA-2023 CRD bank (`--pos_extra centers --nce_p N`, N > 2; reference
// "MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py":81-101,117-137 fits sklearn KMeans(n_clusters = N - 1) on a
// host copy of every class of either bank at every call, from a random initialisation).  Here a deterministic Lloyd iteration of
// the project's own, k = N - 1 centres per class written behind the bank rows:
//   km_pick    x k     farthest-point initialisation: centre 0 = the member at list position 0, centre j = the member with the
//                      largest minimum distance to centres 0 .. j - 1 (lowest list position among equal values).  Launch j
//                      resolves centre j from the per-chunk candidates of launch j - 1, copies it behind the bank, folds the
//                      distance to it into the running minimum and leaves the chunk's candidate for centre j + 1.
//   km_assign  x iters every member joins the centre of least distance (lowest centre index among equal distances); fp32
//                      partial sums and member counts per (256-row chunk, centre).
//   km_finish  x iters the partials of a centre combined in double in chunk order, divided by the count in double; a centre
//                      without members keeps its value.
// Distances are the direct form sum_f (x_f - y_f)^2: per lane 4 features left to right, then a 32-lane butterfly; no product is
// contracted into the following addition (tests/kmeans_emulation.py restates the same grouping).  Both banks and all classes go
// in every launch - grid (row chunk, class, bank); a half-wave per bank row, 16-byte loads of 4 features per lane.  No atomics,
// no host read, no allocation: the same bank gives the same bits, and the call can be captured.
#include "ph_common.h"
#include "ph_kernels.h"

namespace {

constexpr int D = 128;         // feat_dim
constexpr int KM_ROWS = 256;   // rows per chunk (CC_ROWS of the class-mean kernels)
constexpr int KM_HW = 8;       // half-waves per workgroup
constexpr int KM_UNROLL = 4;   // bank rows in flight per half-wave
constexpr int KM_KMAX = 8;

// workspace (4-byte elements), per bank and class `nchunks` records each:
//   parts [2][C][nchunks][k][128] f32 | pcnt [2][C][nchunks][k] i32 | mind [2][C][nchunks][256] f32 |
//   cval [2 parities][2][C][nchunks] f32 | cpos [2 parities][2][C][nchunks] i32
// (pick launch j reads the candidates of parity (j - 1) & 1 and writes parity j & 1: a workgroup that runs late still finds
// the candidates of the previous launch)
struct KmWs {
  float* parts; int* pcnt; float* mind; float* cval; int* cpos;
};
__host__ __device__ inline size_t km_ws_elems(int C, int nchunks, int k) {
  return (size_t)2 * C * nchunks * ((size_t)k * D + k + KM_ROWS + 4);
}
inline KmWs km_ws(void* w, int C, int nchunks, int k) {
  const size_t n = (size_t)2 * C * nchunks;
  KmWs s;
  s.parts = reinterpret_cast<float*>(w);
  s.pcnt = reinterpret_cast<int*>(s.parts + n * k * D);
  s.mind = reinterpret_cast<float*>(s.pcnt + n * k);
  s.cval = s.mind + n * KM_ROWS;
  s.cpos = reinterpret_cast<int*>(s.cval + 2 * n);
  return s;
}

__device__ __forceinline__ float half_sum(float v) {   // reduce within each 32-lane half of the wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum_f (x_f - c_f)^2 of the lane's 4 features, every operation rounded on its own
__device__ __forceinline__ float sqdist4(const f32x4 x, const f32x4 c) {
#pragma clang fp contract(off)
  const float t0 = x[0] - c[0], t1 = x[1] - c[1], t2 = x[2] - c[2], t3 = x[3] - c[3];
  float s = t0 * t0;
  s = s + t1 * t1;
  s = s + t2 * t2;
  s = s + t3 * t3;
  return s;
}

// (value, list position): the larger value wins, the lower position among equal values
__device__ __forceinline__ void far_merge(float& v, int& p, float ov, int op) {
  if (ov > v || (ov == v && op < p)) { v = ov; p = op; }
}
// block-wide (256 threads) argmax under far_merge; the result in every thread
__device__ __forceinline__ void far_block(float& v, int& p, float* shv, int* shp) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int op = __shfl_xor(p, o, 64);
    far_merge(v, p, ov, op);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shp[threadIdx.x >> 6] = p; }
  __syncthreads();
  v = shv[0]; p = shp[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) far_merge(v, p, shv[w], shp[w]);
}

// grid (nchunks, C, 2), block 256.  Launch j of the initialisation.
__global__ __launch_bounds__(256) void km_pick_kernel(float* mem1, float* mem2, const int* __restrict__ members,
                                                      const int* __restrict__ offsets, float* __restrict__ mind,
                                                      float* cval, int* cpos, int nchunks, int n_data,
                                                      int k, int j) {
  const int chunk = blockIdx.x, c = blockIdx.y, bank = blockIdx.z, C = gridDim.y;
  float* mem = bank ? mem2 : mem1;
  const int base = offsets[c], cnt = offsets[c + 1] - base;
  const int used = min((cnt + KM_ROWS - 1) / KM_ROWS, nchunks);
  const size_t rec = ((size_t)bank * C + c) * nchunks, par = (size_t)2 * C * nchunks;
  const float* cval_in = cval + ((j - 1) & 1) * par;
  const int* cpos_in = cpos + ((j - 1) & 1) * par;
  float* crow = mem + ((size_t)n_data + (size_t)c * k + j) * D;
  __shared__ float shv[4];
  __shared__ int shp[4];
  if (j >= cnt) {                                   // fewer members than centres: a zero row that takes no members
    if (chunk == 0 && threadIdx.x < D) crow[threadIdx.x] = 0.f;
    return;
  }
  int pos = 0;
  if (j > 0) {                                      // the candidates that launch j - 1 left, one per chunk
    float v = -1.f;
    int p = 0x7fffffff;
    for (int q = threadIdx.x; q < used; q += 256) far_merge(v, p, cval_in[rec + q], cpos_in[rec + q]);
    far_block(v, p, shv, shp);
    pos = (p >= 0 && p < cnt) ? p : 0;
    __syncthreads();
  }
  const float* src = mem + (size_t)members[base + pos] * D;
  if (chunk == 0 && threadIdx.x < D) crow[threadIdx.x] = src[threadIdx.x];
  if (j == k - 1 || chunk >= used) return;          // nobody reads the minimum after the last pick
  const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
  const f32x4 cen = *reinterpret_cast<const f32x4*>(src + lane * 4);
  const int lo = chunk * KM_ROWS, hi = min(cnt, lo + KM_ROWS);
  float* md = mind + rec * KM_ROWS;
  float bv = -1.f;
  int bp = 0x7fffffff;
  for (int r = lo + hw; r < hi; r += KM_HW) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(mem + (size_t)members[base + r] * D + lane * 4);
    float d = half_sum(sqdist4(x, cen));
    if (j > 0) d = fminf(md[r], d);
    if (lane == 0) md[r] = d;
    far_merge(bv, bp, d, r);
  }
  far_block(bv, bp, shv, shp);
  if (threadIdx.x == 0) { cval[(j & 1) * par + rec + chunk] = bv; cpos[(j & 1) * par + rec + chunk] = bp; }
}

// grid (nchunks, C, 2), block 256 = 8 half-waves; half-wave h walks rows h, h + 8, .. of the chunk in order.
template <int K>
__global__ __launch_bounds__(256) void km_assign_kernel(const float* __restrict__ mem1, const float* __restrict__ mem2,
                                                        const int* __restrict__ members, const int* __restrict__ offsets,
                                                        float* __restrict__ parts, int* __restrict__ pcnt,
                                                        int* __restrict__ labels, int nchunks, int n_data) {
  const int chunk = blockIdx.x, c = blockIdx.y, bank = blockIdx.z, C = gridDim.y;
  const float* mem = bank ? mem2 : mem1;
  const int base = offsets[c], cnt = offsets[c + 1] - base;
  const int lo = chunk * KM_ROWS, hi = min(cnt, lo + KM_ROWS);
  if (lo >= hi) return;
  const int keff = min(K, cnt);
  const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
  const float* cen = mem + ((size_t)n_data + (size_t)c * K) * D;
  f32x4 ce[K], acc[K];
  int na[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ce[j] = *reinterpret_cast<const f32x4*>(cen + j * D + lane * 4);
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    na[j] = 0;
  }
  int* lab = labels ? labels + (size_t)bank * offsets[C] + base : nullptr;
  for (int r0 = lo + hw; r0 < hi; r0 += KM_HW * KM_UNROLL) {
    f32x4 x[KM_UNROLL];
#pragma unroll
    for (int u = 0; u < KM_UNROLL; ++u) {
      const int r = r0 + u * KM_HW;
      x[u] = *reinterpret_cast<const f32x4*>(mem + (size_t)members[base + (r < hi ? r : lo)] * D + lane * 4);
    }
#pragma unroll
    for (int u = 0; u < KM_UNROLL; ++u) {
      const int r = r0 + u * KM_HW;
      if (r < hi) {
        float best = half_sum(sqdist4(x[u], ce[0]));
        int bj = 0;
#pragma unroll
        for (int j = 1; j < K; ++j) {
          const float d = half_sum(sqdist4(x[u], ce[j]));
          if (j < keff && d < best) { best = d; bj = j; }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (bj == j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] += x[u][e];
            na[j] += 1;
          }
        }
        if (lab && lane == 0) lab[r] = bj;
      }
    }
  }
  __shared__ float sh[KM_HW][K][D];
  __shared__ int shn[KM_HW][K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    *reinterpret_cast<f32x4*>(&sh[hw][j][lane * 4]) = acc[j];
    if (lane == 0) shn[hw][j] = na[j];
  }
  __syncthreads();
  const size_t rec = (((size_t)bank * C + c) * nchunks + chunk) * K;
  for (int e = threadIdx.x; e < K * D; e += 256) {
    const int j = e >> 7, f = e & (D - 1);
    float s = sh[0][j][f];
#pragma unroll
    for (int h = 1; h < KM_HW; ++h) s += sh[h][j][f];
    parts[(rec + j) * D + f] = s;
  }
  if (threadIdx.x < K) {
    int n = 0;
#pragma unroll
    for (int h = 0; h < KM_HW; ++h) n += shn[h][threadIdx.x];
    pcnt[rec + threadIdx.x] = n;
  }
}

// grid (k, C, 2), block 128
__global__ __launch_bounds__(128) void km_finish_kernel(float* mem1, float* mem2, const int* __restrict__ offsets,
                                                        const float* __restrict__ parts, const int* __restrict__ pcnt,
                                                        int* __restrict__ counts, int nchunks, int n_data) {
  const int j = blockIdx.x, c = blockIdx.y, bank = blockIdx.z, k = gridDim.x, C = gridDim.y, f = threadIdx.x;
  float* mem = bank ? mem2 : mem1;
  const int cnt = offsets[c + 1] - offsets[c];
  const int used = min((cnt + KM_ROWS - 1) / KM_ROWS, nchunks);
  const size_t rec = ((size_t)bank * C + c) * nchunks;
  int n = 0;
  double s = 0.0;
  for (int q = 0; q < used; ++q) {
    n += pcnt[(rec + q) * k + j];
    s += (double)parts[((rec + q) * k + j) * D + f];
  }
  if (n > 0) mem[((size_t)n_data + (size_t)c * k + j) * D + f] = (float)(s / (double)n);
  if (counts && f == 0) counts[((size_t)bank * C + c) * k + j] = n;
}

template <int K>
void km_launch_assign(dim3 grid, hipStream_t st, const float* m1, const float* m2, const int* members, const int* offsets,
                      const KmWs& w, int* labels, int nchunks, int n_data) {
  hipLaunchKernelGGL(km_assign_kernel<K>, grid, dim3(256), 0, st, m1, m2, members, offsets, w.parts, w.pcnt, labels, nchunks,
                     n_data);
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

size_t ph_crd_kmeans_centers_workspace_bytes(int num_classes, int max_class_rows, int k) {
  if (num_classes < 1 || k < 1) return 0;
  return km_ws_elems(num_classes, cdiv(max_class_rows > 0 ? max_class_rows : 1, KM_ROWS), k) * sizeof(float);
}

int ph_crd_kmeans_centers(float* mem1_ext, float* mem2_ext, const int* members, const int* offsets, int num_classes,
                          int max_class_rows, int n_data, int feat_dim, int k, int iters, int* labels, int* counts,
                          void* workspace, hipStream_t st) {
  if (feat_dim != D || k < 2 || k > KM_KMAX || iters < 1 || num_classes < 1 || n_data < 0) return PH_EINVAL;
  if (!mem1_ext || !mem2_ext || !members || !offsets || !workspace) return PH_EINVAL;
  if ((reinterpret_cast<uintptr_t>(mem1_ext) | reinterpret_cast<uintptr_t>(mem2_ext)) & 15) return PH_EINVAL;   // 16-byte row loads
  const int nchunks = cdiv(max_class_rows > 0 ? max_class_rows : 1, KM_ROWS);
  const KmWs w = km_ws(workspace, num_classes, nchunks, k);
  const dim3 grid(nchunks, num_classes, 2);
  for (int j = 0; j < k; ++j) {
    hipLaunchKernelGGL(km_pick_kernel, grid, dim3(256), 0, st, mem1_ext, mem2_ext, members, offsets, w.mind, w.cval, w.cpos,
                       nchunks, n_data, k, j);
    PH_LAUNCH_CHECK();
  }
  for (int t = 1; t <= iters; ++t) {
    int* lab = t == iters ? labels : nullptr;        // the labels of the last assignment
    switch (k) {
      case 2: km_launch_assign<2>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      case 3: km_launch_assign<3>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      case 4: km_launch_assign<4>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      case 5: km_launch_assign<5>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      case 6: km_launch_assign<6>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      case 7: km_launch_assign<7>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
      default: km_launch_assign<8>(grid, st, mem1_ext, mem2_ext, members, offsets, w, lab, nchunks, n_data); break;
    }
    PH_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_finish_kernel, dim3(k, num_classes, 2), dim3(D), 0, st, mem1_ext, mem2_ext, offsets, w.parts, w.pcnt,
                       t == iters ? counts : nullptr, nchunks, n_data);
    PH_LAUNCH_CHECK();
  }
  return PH_OK;
}

}  // extern "C"

// RKD ("MIA 2022/distiller_zoo/RKD.py":15-58) over a batch of up to 1024 rows, split by anchor ranges so that the
// replicas of a data-parallel run each take a slice of the B^3 * D angle term (csrc/zoo.hip holds the one-workgroup form
// for B <= 128 rows whose E [B][D] and A [B][B] fit its anchor kernel's LDS: ph_rkd_one_workgroup_fits).  ph_rkd_loss_grad_part computes, for the anchors
// [anchor_lo, anchor_lo + n_anchors) of the gathered rows, the part of the loss and of its gradient with respect to
// EVERY student row that those anchors (angle term) and those rows of the distance matrix (distance term) produce; the
// parts of any partition of [0, Bg) add up to the loss / gradient of the whole batch.  Global quantities (the two mean
// distances, the normalisers Bg^2 and Bg^3) are computed from all Bg rows by every part.
//
// Angle term, one workgroup per (anchor i, tile of 64 rows j), streaming tiles of 64 rows k - the shape of a fused
// attention backward, the Bg x Bg angle matrix of an anchor is never stored:
//   e_ij = (x_j - x_i) / max(|x_j - x_i|, 1e-12)        formed from the rows as they are staged into LDS; the norm is
//                                                        the difference's own (exact zero for coinciding rows)
//   A_s = E_j E_k^T, A_t alike  (exact-f32 MFMA 32x32x2, D in chunks of 32);  G = clip(A_s - A_t, -1, 1) / Bg^3
//   dE_j += G E_k               (A and G are symmetric in (j, k): only the row tile j carries accumulators)
//   dv_ij = 2 w_a (dE_j - e_ij (e_ij . dE_j)) / |x_j - x_i|   -> dx_j += dv_ij, dx_i -= sum_j dv_ij
// The dv slabs of up to 64 anchors at a time go through the workspace and are added up in a fixed order (no atomics):
// two runs give the same bits.
#include "ph_common.h"
#include "ph_kernels.h"
#include "ph_reduce.h"

namespace {

typedef float rp_f16 __attribute__((ext_vector_type(16)));

constexpr int RP_T = 64;          // rows of a j / k tile
constexpr int RP_SLAB = 64;       // anchors per angle launch (rows of the dv slab)
constexpr int RP_LD1 = 33;        // LDS row stride of the 32-column operand tiles of A = E_j E_k^T
constexpr int RP_LD2 = 96;        // ... of the 64-column E_k tile of dE += G E_k
constexpr int RP_LDG = 66;        // ... of G
constexpr float RP_EPS = 1e-12f;
constexpr int RP_THREADS = 256;   // every kernel here that sums over its workgroup is launched with 256 threads: block_sum_tree's extent

__device__ __forceinline__ float rp_huber(float z) {
  const float az = fabsf(z);
  return az < 1.f ? 0.5f * z * z : az - 0.5f;
}

// Squared norms of the row differences, N2[i][k] = |x_k - x_i|^2 summed from the differences themselves (exactly 0 for
// coinciding rows; the Gram form cancels to noise there), for 8 rows i x 64 rows k per workgroup.  The k rows are staged
// through LDS 128 columns at a time; a thread owns one row k and a quarter of the columns for all 8 rows i, the four
// quarters are added in a fixed order.  N2[i][k] and N2[k][i] see the same terms in the same order: bitwise symmetric.
constexpr int RP_NI = 8;
__global__ __launch_bounds__(256) void rkd_part_norm_kernel(const float* __restrict__ xs, const float* __restrict__ xt,
                                                            float* __restrict__ N2s, float* __restrict__ N2t, int Bg, int D) {
  __shared__ float tile[64 * 129];
  __shared__ float xi[RP_NI][128];
  __shared__ float part[4][RP_NI][64];
  const int tid = threadIdx.x, kl = tid & 63, q4 = tid >> 6, i0 = blockIdx.x * RP_NI, kb = blockIdx.y * 64;
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    const float* __restrict__ x = side ? xt : xs;
    float acc[RP_NI];
#pragma unroll
    for (int a = 0; a < RP_NI; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < D; c0 += 128) {
      __syncthreads();
      float v[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int e = tid + 256 * q, row = e >> 7, d = c0 + (e & 127);
        v[q] = (kb + row < Bg && d < D) ? x[(size_t)(kb + row) * D + d] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int e = tid + 256 * q;
        tile[(e >> 7) * 129 + (e & 127)] = v[q];
      }
      for (int e = tid; e < RP_NI * 128; e += 256) {
        const int a = e >> 7, d = c0 + (e & 127);
        xi[a][e & 127] = (i0 + a < Bg && d < D) ? x[(size_t)(i0 + a) * D + d] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int dd = 0; dd < 32; ++dd) {
        const float xv = tile[kl * 129 + q4 * 32 + dd];
#pragma unroll
        for (int a = 0; a < RP_NI; ++a) {
          const float u = xv - xi[a][q4 * 32 + dd];
          acc[a] += u * u;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < RP_NI; ++a) part[q4][a][kl] = acc[a];
    __syncthreads();
    for (int e = tid; e < RP_NI * 64; e += 256) {
      const int a = e >> 6, k = kb + (e & 63);
      if (i0 + a < Bg && k < Bg)
        (side ? N2t : N2s)[(size_t)(i0 + a) * Bg + k] = ((part[0][a][e & 63] + part[1][a][e & 63]) + part[2][a][e & 63]) + part[3][a][e & 63];
    }
  }
}

// rs[i] = sum_{k != i} sqrt(max(N2[i][k], eps)) (RKD.py:47-58: pdist's clamp and zero diagonal), one wave per row
__global__ __launch_bounds__(256) void rkd_part_rowsum_kernel(const float* __restrict__ N2s, const float* __restrict__ N2t,
                                                              float* __restrict__ rs, float* __restrict__ rt, int Bg) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= Bg) return;
  float a = 0.f, b = 0.f;
  for (int k = lane; k < Bg; k += 64) {
    if (k == i) continue;
    a += sqrtf(fmaxf(N2s[(size_t)i * Bg + k], RP_EPS));
    b += sqrtf(fmaxf(N2t[(size_t)i * Bg + k], RP_EPS));
  }
  a = wave_sum(a); b = wave_sum(b);
  if (lane == 0) { rs[i] = a; rt[i] = b; }
}

// Distance term, rows [lo, lo + gridDim.x) of the distance matrix: lrow[b] = sum_j huber(z_ij), udrow[b] = sum_j
// clip(z_ij) dhat_ij with z = d / mean_d - t / mean_t.  Every workgroup derives the two global means from rs / rt in the
// same order; workgroup 0 leaves them in sc[0..1].
__global__ __launch_bounds__(256) void rkd_part_dist_rows_kernel(const float* __restrict__ N2s, const float* __restrict__ N2t,
                                                                 const float* __restrict__ rs, const float* __restrict__ rt,
                                                                 float* __restrict__ lrow, float* __restrict__ udrow,
                                                                 float* __restrict__ sc, int Bg, int lo) {
  __shared__ float red[256];
  const int tid = threadIdx.x, i = lo + blockIdx.x;
  float a = 0.f, b = 0.f;
  for (int k = tid; k < Bg; k += 256) { a += rs[k]; b += rt[k]; }
  const float N = (float)Bg * (float)(Bg - 1);
  const float md = block_sum_tree<RP_THREADS>(a, red) / N, mt = block_sum_tree<RP_THREADS>(b, red) / N;
  float l = 0.f, ud = 0.f;
  for (int j = tid; j < Bg; j += 256) {
    if (j == i) continue;
    const float d = sqrtf(fmaxf(N2s[(size_t)i * Bg + j], RP_EPS)) / md;
    const float t = sqrtf(fmaxf(N2t[(size_t)i * Bg + j], RP_EPS)) / mt;
    const float z = d - t;
    l += rp_huber(z);
    ud += fminf(fmaxf(z, -1.f), 1.f) * d;
  }
  l = block_sum_tree<RP_THREADS>(l, red); ud = block_sum_tree<RP_THREADS>(ud, red);
  if (tid == 0) {
    lrow[blockIdx.x] = l; udrow[blockIdx.x] = ud;
    if (blockIdx.x == 0) { sc[0] = md; sc[1] = mt; }
  }
}

// Gradient of this part's distance term with respect to row m (one workgroup per row, all Bg rows):
//   dx_m = sum_l W_ml (x_m - x_l),  W_ml = w_d ((u_ml / Bg^2) ([m in part] + [l in part]) - 2 corr) / mean_d / d_ml
// where the clamp is inactive, corr = sum_{i in part, j} u_ij dhat_ij / (Bg^2 N) (the derivative through mean_d).
// WRITES dx (the angle slabs are added afterwards).
__global__ __launch_bounds__(256) void rkd_part_dist_grad_kernel(const float* __restrict__ xs, const float* __restrict__ N2s,
                                                                 const float* __restrict__ N2t, const float* __restrict__ udrow,
                                                                 const float* __restrict__ sc, float* __restrict__ dx, int Bg,
                                                                 int D, int lo, int na, float w_d) {
  __shared__ float red[256];
  __shared__ float W[1024];
  const int tid = threadIdx.x, m = blockIdx.x;
  float c = 0.f;
  for (int k = tid; k < na; k += 256) c += udrow[k];
  const float inv_n2 = 1.f / ((float)Bg * (float)Bg), N = (float)Bg * (float)(Bg - 1);
  const float corr = block_sum_tree<RP_THREADS>(c, red) * inv_n2 / N;
  const float md = sc[0], mt = sc[1];
  const float m_in = (m >= lo && m < lo + na) ? 1.f : 0.f;
  for (int l = tid; l < Bg; l += 256) {
    float w = 0.f;
    const float res = N2s[(size_t)m * Bg + l];
    if (l != m && res > RP_EPS) {
      const float dr = sqrtf(res);
      const float t = sqrtf(fmaxf(N2t[(size_t)m * Bg + l], RP_EPS)) / mt;
      const float u = fminf(fmaxf(dr / md - t, -1.f), 1.f) * inv_n2;
      const float cnt = m_in + ((l >= lo && l < lo + na) ? 1.f : 0.f);
      w = w_d * (u * cnt - 2.f * corr) / md / dr;
    }
    W[l] = w;
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256) {
    const float xm = xs[(size_t)m * D + d];
    float a = 0.f;
    for (int l = 0; l < Bg; ++l) a += W[l] * (xm - xs[(size_t)l * D + d]);
    dx[(size_t)m * D + d] = a;
  }
}

// Angle term of anchor i = a0 + blockIdx.y against the row tile j0 = 64 blockIdx.x (see the head of this file).
// N2s / N2t: the squared difference norms of rkd_part_norm_kernel.  dv: slab [gridDim.y][Bg][D]; apart: loss partials
// [n_anchors][gridDim.x], this launch's anchors from row `part_off`.  MAXC >= ceil(D / 64): accumulator tiles per wave.
template <int MAXC>
__global__ __launch_bounds__(256) void rkd_part_angle_kernel(const float* __restrict__ xs, const float* __restrict__ xt,
                                                             const float* __restrict__ N2s, const float* __restrict__ N2t,
                                                             float* __restrict__ dv, float* __restrict__ apart, int Bg, int D,
                                                             int a0, int part_off, float w_a) {
  __shared__ float xi_s[512], xi_t[512];
  __shared__ float inv_js[RP_T], inv_jt[RP_T], inv_jb[RP_T], inv_ks[RP_T], inv_kt[RP_T];
  __shared__ float stage[4 * RP_T * RP_LD1];          // >= RP_T * RP_LD2
  __shared__ float G[RP_T * RP_LDG];
  __shared__ float red[256];
  __shared__ float dots[2][RP_T];
  static_assert(4 * RP_T * RP_LD1 >= RP_T * RP_LD2, "the 64-column tile shares the staging area");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, kk = lane >> 5;
  const int i = a0 + blockIdx.y, j0 = blockIdx.x * RP_T;
  const int nc2 = (D + 63) >> 6, nc1 = 2 * nc2;
  for (int d = tid; d < 512; d += 256) {
    xi_s[d] = d < D ? xs[(size_t)i * D + d] : 0.f;
    xi_t[d] = d < D ? xt[(size_t)i * D + d] : 0.f;
  }
  if (tid < RP_T) {
    const int j = j0 + tid;
    float a = 0.f, b = 0.f, c = 0.f;
    if (j < Bg) {
      const float ns = sqrtf(N2s[(size_t)i * Bg + j]), nt = sqrtf(N2t[(size_t)i * Bg + j]);
      a = 1.f / fmaxf(ns, RP_EPS); b = 1.f / fmaxf(nt, RP_EPS);
      c = (j != i && ns > RP_EPS) ? 1.f / ns : 0.f;           // (v_ii == 0 identically; no gradient through a zero vector)
    }
    inv_js[tid] = a; inv_jt[tid] = b; inv_jb[tid] = c;
  }
  const int rj = (wave & 1) * 32, rk = (wave >> 1) * 32;      // A = E_j E_k^T: this wave's 32 x 32 quadrant
  const int rh = (wave & 1) * 32, cp = (wave >> 1) * 32;      // dE += G E_k: row half, column half of a 64-column chunk
  const float inv_n3 = 1.f / ((float)Bg * (float)Bg * (float)Bg);
  float* Ejs = stage; float* Ejt = stage + RP_T * RP_LD1; float* Eks = Ejt + RP_T * RP_LD1; float* Ekt = Eks + RP_T * RP_LD1;
  // Staging in two halves so that all loads of a chunk are in flight together: `ld*` reads the raw rows into registers
  // (0 outside Bg x D), `st*` turns them into unit vectors on the way into LDS - outside Bg x D that gives
  // (0 - x_i[d]) * 0 or (0 - 0) * inv = 0.
  float v1[4][8];                                             // A: four 64 x 32 tiles, 8 elements per thread each
  float v2[16];                                               // dE: one 64 x 64 tile
  auto ld1 = [&](int k0, int c) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q, row = e >> 5, d = c * 32 + (e & 31), j = j0 + row, k = k0 + row;
      const bool okj = j < Bg && d < D, okk = k < Bg && d < D;
      v1[0][q] = okj ? xs[(size_t)j * D + d] : 0.f;
      v1[1][q] = okj ? xt[(size_t)j * D + d] : 0.f;
      v1[2][q] = okk ? xs[(size_t)k * D + d] : 0.f;
      v1[3][q] = okk ? xt[(size_t)k * D + d] : 0.f;
    }
  };
  auto st1 = [&](int c) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q, row = e >> 5, col = e & 31, d = c * 32 + col, o = row * RP_LD1 + col;
      Ejs[o] = (v1[0][q] - xi_s[d]) * inv_js[row];
      Ejt[o] = (v1[1][q] - xi_t[d]) * inv_jt[row];
      Eks[o] = (v1[2][q] - xi_s[d]) * inv_ks[row];
      Ekt[o] = (v1[3][q] - xi_t[d]) * inv_kt[row];
    }
  };
  auto ld2 = [&](int k0, int c) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = tid + 256 * q, k = k0 + (e >> 6), d = c * 64 + (e & 63);
      v2[q] = (k < Bg && d < D) ? xs[(size_t)k * D + d] : 0.f;
    }
  };
  auto st2 = [&](int c) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = tid + 256 * q, row = e >> 6, col = e & 63;
      stage[row * RP_LD2 + col] = (v2[q] - xi_s[c * 64 + col]) * inv_ks[row];
    }
  };
  rp_f16 acc[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float lsum = 0.f;
  for (int k0 = 0; k0 < Bg; k0 += RP_T) {
    __syncthreads();            // the previous tile's readers of inv_k* and of the staging area are done
    if (tid < RP_T) {
      const int k = k0 + tid;
      inv_ks[tid] = k < Bg ? 1.f / fmaxf(sqrtf(N2s[(size_t)i * Bg + k]), RP_EPS) : 0.f;
      inv_kt[tid] = k < Bg ? 1.f / fmaxf(sqrtf(N2t[(size_t)i * Bg + k]), RP_EPS) : 0.f;
    }
    rp_f16 aS, aT;
#pragma unroll
    for (int r = 0; r < 16; ++r) { aS[r] = 0.f; aT[r] = 0.f; }
    for (int c = 0; c < nc1; ++c) {
      ld1(k0, c);
      __syncthreads();          // inv_k* written (first chunk); the previous chunk's operand reads are done
      st1(c);
      __syncthreads();
#pragma unroll
      for (int dd = 0; dd < 32; dd += 2) {
        const int oa = (rj + l32) * RP_LD1 + dd + kk, ob = (rk + l32) * RP_LD1 + dd + kk;
        aS = __builtin_amdgcn_mfma_f32_32x32x2f32(Ejs[oa], Eks[ob], aS, 0, 0, 0);
        aT = __builtin_amdgcn_mfma_f32_32x32x2f32(Ejt[oa], Ekt[ob], aT, 0, 0, 0);
      }
    }
    // accumulator element r of a lane: row (r & 3) + 8 (r >> 2) + 4 kk, column l32
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = (r & 3) + 8 * (r >> 2) + 4 * kk;
      const float z = aS[r] - aT[r];
      lsum += rp_huber(z);
      G[(rj + m) * RP_LDG + rk + l32] = fminf(fmaxf(z, -1.f), 1.f) * inv_n3;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < nc2) {
        ld2(k0, c);
        __syncthreads();        // G complete (first chunk); the staging area's readers are done
        st2(c);
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < RP_T; kq += 2)
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(G[(rh + l32) * RP_LDG + kq + kk], stage[(kq + kk) * RP_LD2 + cp + l32],
                                                        acc[c], 0, 0, 0);
      }
    }
  }
  lsum = block_sum_tree<RP_THREADS>(lsum, red);
  if (tid == 0) apart[(size_t)(part_off + blockIdx.y) * gridDim.x + blockIdx.x] = w_a * inv_n3 * lsum;
  // dv_ij = 2 w_a (dE_j - e_ij (e_ij . dE_j)) / |v_ij|: the dot product spans this wave's columns, its 32-lane halves and
  // the wave holding the other column half
  float pd[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) pd[r] = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < nc2) {
      const int d = c * 64 + cp + l32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = rh + (r & 3) + 8 * (r >> 2) + 4 * kk, jg = j0 + jl;
        const float e = (jg < Bg && d < D) ? (xs[(size_t)jg * D + d] - xi_s[d]) * inv_js[jl] : 0.f;
        pd[r] += e * acc[c][r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) pd[r] += __shfl_xor(pd[r], o, 64);
    if (l32 == 0) dots[wave >> 1][rh + (r & 3) + 8 * (r >> 2) + 4 * kk] = pd[r];
  }
  __syncthreads();
  const float sc2 = 2.f * w_a;
  float* out = dv + (size_t)blockIdx.y * Bg * D;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c < nc2) {
      const int d = c * 64 + cp + l32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = rh + (r & 3) + 8 * (r >> 2) + 4 * kk, jg = j0 + jl;
        if (jg < Bg && d < D) {
          const float e = (xs[(size_t)jg * D + d] - xi_s[d]) * inv_js[jl];
          const float dot = dots[0][jl] + dots[1][jl];
          out[(size_t)jg * D + d] = sc2 * (acc[c][r] - e * dot) * inv_jb[jl];
        }
      }
    }
  }
}

// dx_j += sum_{a < cnt} dv[a][j] - [a0 <= j < a0 + cnt] sum_k dv[j - a0][k]   (v_ij = x_j - x_i).  64 columns at a time;
// each sum is cut into four segments (one per wave) of four interleaved chains, added up in a fixed order.
__device__ __forceinline__ float rp_strided_sum(const float* __restrict__ p, size_t stride, int lo, int hi) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int q = lo;
  for (; q + 4 <= hi; q += 4) {
    s0 += p[(size_t)q * stride]; s1 += p[(size_t)(q + 1) * stride];
    s2 += p[(size_t)(q + 2) * stride]; s3 += p[(size_t)(q + 3) * stride];
  }
  for (; q < hi; ++q) s0 += p[(size_t)q * stride];
  return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(256) void rkd_part_gather_kernel(const float* __restrict__ dv, float* __restrict__ dx, int Bg, int D,
                                                              int a0, int cnt) {
  __shared__ float seg[4][64];
  const int j = blockIdx.x, dl = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool anchor = j >= a0 && j < a0 + cnt;
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int d = d0 + dl;
    float a = 0.f;
    if (d < D) {
      const int per = (cnt + 3) >> 2, lo = min(w * per, cnt), hi = min(lo + per, cnt);
      a = rp_strided_sum(dv + (size_t)j * D + d, (size_t)Bg * D, lo, hi);
      if (anchor) {
        const int perk = (Bg + 3) >> 2, klo = min(w * perk, Bg), khi = min(klo + perk, Bg);
        a -= rp_strided_sum(dv + (size_t)(j - a0) * Bg * D + d, (size_t)D, klo, khi);
      }
    }
    __syncthreads();
    seg[w][dl] = a;
    __syncthreads();
    if (w == 0 && d < D) dx[(size_t)j * D + d] += ((seg[0][dl] + seg[1][dl]) + seg[2][dl]) + seg[3][dl];
  }
}

// loss_part = w_d sum(lrow) / Bg^2 + sum(apart)
__global__ __launch_bounds__(256) void rkd_part_loss_kernel(const float* __restrict__ lrow, const float* __restrict__ apart,
                                                            float* __restrict__ loss, int Bg, int na, int n_apart, float w_d) {
  __shared__ float red[256];
  float l = 0.f, a = 0.f;
  for (int k = threadIdx.x; k < na; k += 256) l += lrow[k];
  for (int k = threadIdx.x; k < n_apart; k += 256) a += apart[k];
  l = block_sum_tree<RP_THREADS>(l, red); a = block_sum_tree<RP_THREADS>(a, red);
  if (threadIdx.x == 0) loss[0] = w_d * l / ((float)Bg * (float)Bg) + a;
}

struct RkdPartLayout {
  size_t n2s, n2t, rs, rt, lrow, udrow, apart, sc, dv, total;      // offsets in floats
};

RkdPartLayout rkd_part_layout(int Bg, int D, int na) {
  RkdPartLayout L;
  const size_t bb = (size_t)Bg * Bg, tiles = (size_t)(Bg + RP_T - 1) / RP_T;
  size_t o = 0;
  L.n2s = o; o += bb;
  L.n2t = o; o += bb;
  L.rs = o; o += Bg;
  L.rt = o; o += Bg;
  L.lrow = o; o += na;
  L.udrow = o; o += na;
  L.apart = o; o += (size_t)na * tiles;
  L.sc = o; o += 16;
  L.dv = o; o += (size_t)(na < RP_SLAB ? na : RP_SLAB) * Bg * D;
  L.total = o;
  return L;
}

bool rkd_part_shape_ok(int Bg, int D, int lo, int na) {
  return Bg >= 2 && Bg <= 1024 && D >= 1 && D <= 512 && lo >= 0 && na >= 1 && (long long)lo + na <= Bg;
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

size_t ph_rkd_part_workspace_bytes(int Bg, int D, int n_anchors) {
  if (Bg < 1 || D < 1 || n_anchors < 1) return 0;
  return rkd_part_layout(Bg, D, n_anchors).total * sizeof(float);
}

int ph_rkd_loss_grad_part(const float* f_s, const float* f_t, int Bg, int D, int anchor_lo, int n_anchors, float w_d,
                          float w_a, float* loss_part, float* dx_part, void* ws_, hipStream_t st) {
  if (!f_s || !f_t || !loss_part || !dx_part || !ws_ || !rkd_part_shape_ok(Bg, D, anchor_lo, n_anchors)) return PH_EINVAL;
  const RkdPartLayout L = rkd_part_layout(Bg, D, n_anchors);
  float* ws = reinterpret_cast<float*>(ws_);
  float *n2s = ws + L.n2s, *n2t = ws + L.n2t, *rs = ws + L.rs, *rt = ws + L.rt, *lrow = ws + L.lrow, *udrow = ws + L.udrow;
  float *apart = ws + L.apart, *sc = ws + L.sc, *dv = ws + L.dv;
  const int tiles = (Bg + RP_T - 1) / RP_T;
  hipLaunchKernelGGL(rkd_part_norm_kernel, dim3((Bg + RP_NI - 1) / RP_NI, tiles), dim3(256), 0, st, f_s, f_t, n2s, n2t, Bg, D);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rkd_part_rowsum_kernel, dim3((Bg + 3) / 4), dim3(256), 0, st, n2s, n2t, rs, rt, Bg);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rkd_part_dist_rows_kernel, dim3(n_anchors), dim3(256), 0, st, n2s, n2t, rs, rt, lrow, udrow, sc, Bg,
                     anchor_lo);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rkd_part_dist_grad_kernel, dim3(Bg), dim3(256), 0, st, f_s, n2s, n2t, udrow, sc, dx_part, Bg, D,
                     anchor_lo, n_anchors, w_d);
  PH_LAUNCH_CHECK();
  for (int a0 = anchor_lo; a0 < anchor_lo + n_anchors; a0 += RP_SLAB) {
    const int cnt = anchor_lo + n_anchors - a0 < RP_SLAB ? anchor_lo + n_anchors - a0 : RP_SLAB;
    const dim3 grid(tiles, cnt);
    if (D <= 64)
      hipLaunchKernelGGL(rkd_part_angle_kernel<1>, grid, dim3(256), 0, st, f_s, f_t, n2s, n2t, dv, apart, Bg, D, a0,
                         a0 - anchor_lo, w_a);
    else if (D <= 128)
      hipLaunchKernelGGL(rkd_part_angle_kernel<2>, grid, dim3(256), 0, st, f_s, f_t, n2s, n2t, dv, apart, Bg, D, a0,
                         a0 - anchor_lo, w_a);
    else if (D <= 256)
      hipLaunchKernelGGL(rkd_part_angle_kernel<4>, grid, dim3(256), 0, st, f_s, f_t, n2s, n2t, dv, apart, Bg, D, a0,
                         a0 - anchor_lo, w_a);
    else
      hipLaunchKernelGGL(rkd_part_angle_kernel<8>, grid, dim3(256), 0, st, f_s, f_t, n2s, n2t, dv, apart, Bg, D, a0,
                         a0 - anchor_lo, w_a);
    PH_LAUNCH_CHECK();
    hipLaunchKernelGGL(rkd_part_gather_kernel, dim3(Bg), dim3(256), 0, st, dv, dx_part, Bg, D, a0, cnt);
    PH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rkd_part_loss_kernel, dim3(1), dim3(256), 0, st, lrow, apart, loss_part, Bg, n_anchors,
                     n_anchors * tiles, w_d);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"

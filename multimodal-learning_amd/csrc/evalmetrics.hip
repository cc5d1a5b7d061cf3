// The tail of the patch-level test pass: what the reference computes on the host, with sklearn and pandas,
// after copying every prediction row off the device -
//   ph_rank_counts       roc_auc_score / average_precision_score(average="micro")   (core/utils_analysis.py:160-161,
//                        train_test_path_multi_distill.py:516-526) as exact pair counts,
//   ph_confusion_counts  f1_score of the arg-max grades (utils_analysis.py:162-163) as the C x C confusion matrix,
//   ph_group_agg         groupby('TCGA ID').agg(max | mean) of the patch rows per patient (utils_analysis.py:123),
//   ph_group_quantile    the order statistics of the same groups: the median of the survival aggregation (utils_analysis.py:467)
//                        and the percentile form of the grading one (:122) - DESIGN.md section 24.
//   ph_rank_counts_classes  the same counts per one-vs-rest column: average="macro" | "weighted" | None (utils_analysis.py:138-167),
//   ph_roc_points        the integer points of roc_curve per grade and micro (makeAUROCPlot, :172-215) - DESIGN.md section 26.
// The scores are log-probabilities (negative): nothing here relies on their sign.
#include "ph_common.h"
#include "ph_kernels.h"
#include "ph_pairscan.h"

namespace {

constexpr int RANK_TILE = 256;            // pairs per workgroup and j-tile length of the all-pairs count
constexpr int RANK_MAX_M = 1 << 20;
constexpr int CONF_THREADS = 256;
constexpr int CONF_MAX_C = 16;
constexpr int AGG_MAX_N = 1 << 24;
constexpr int AGG_MAX_C = 4096;
constexpr int QUANT_THREADS = 256;
constexpr int QUANT_MAX_GROUP = 4096;     // PH_QUANTILE_MAX_GROUP: one group's column in LDS (16 KiB)
constexpr int QUANT_WAVE_MAX_BLOCKS = 1 << 16;

// Element i of a ranking problem (ph_rank_counts, ph_roc_points): cls >= 0 - score pred[i][cls], label grade[i] == cls,
// M = N; cls == -1 - pair i = n * C + c with score pred[i] and label grade[n] == c, M = N * C (micro).
struct RocElem {
  float s;
  int lab;                     // 1 positive, 0 negative
  unsigned int bad;            // a score that is not finite; once per row, a label outside [0, C) (it makes no pair positive)
};

__device__ __forceinline__ RocElem roc_elem(const float* __restrict__ pred, const int64_t* __restrict__ grade, int i, int C,
                                            int cls) {
  RocElem e;
  int n, c;
  if (cls >= 0) { n = i; c = cls; } else { n = i / C; c = i - n * C; }
  e.s = pred[cls >= 0 ? (size_t)n * C + c : (size_t)i];       // (the micro load does not wait for the division)
  const int64_t g = grade[n];
  e.lab = g == (int64_t)c ? 1 : 0;
  const bool count_label = cls >= 0 || c == 0;
  e.bad = (isfinite(e.s) ? 0u : 1u) + ((count_label && (g < 0 || g >= (int64_t)C)) ? 1u : 0u);
  return e;
}

// What a thread stages for element j: .x = the score of a positive j, .y = of a negative one.  A NaN compares false with
// everything: the half that does not apply, the padding past the end and a NaN score all drop out of every count, so the
// scan has no label test.
__device__ __forceinline__ float2 roc_stage(const float* __restrict__ pred, const int64_t* __restrict__ grade, int j, int M,
                                            int C, int cls) {
  const float qnan = __builtin_nanf("");
  float2 v = make_float2(qnan, qnan);
  if (j < M) {
    const RocElem e = roc_elem(pred, grade, j, C, cls);
    if (e.lab) v.x = e.s; else v.y = e.s;
  }
  return v;
}

// Thread = pair i of the micro problem.  For a positive i:  ge_all = #{j: s_j >= s_i}, ge_pos = the positives among them,
// below = #{j negative: s_j < s_i}, equal = #{j negative: s_j == s_i}.  counts[0..3] += P, concordant, tied, bad (64-bit
// integer atomics: exact, independent of the order); part[block] = the fixed-tree sum (block_sum_tree: the order
// tests/eval_emulation.py restates) of ge_pos / ge_all over the block's positives (0.0 for every other thread).
__global__ __launch_bounds__(RANK_TILE) void rank_counts_kernel(const float* __restrict__ pred, const int64_t* __restrict__ grade,
                                                                int M, int C, unsigned long long* __restrict__ counts,
                                                                double* __restrict__ part) {
  __shared__ float2 sj[RANK_TILE];
  __shared__ double red[RANK_TILE];
  const int i = blockIdx.x * RANK_TILE + threadIdx.x;
  float si = 0.f;
  bool pos = false;
  unsigned int bad = 0;
  if (i < M) {
    si = pred[i];
    const int n = i / C, c = i - n * C;
    const int64_t g = grade[n];
    pos = g == (int64_t)c;
    bad = (isfinite(si) ? 0u : 1u) + ((c == 0 && (g < 0 || g >= (int64_t)C)) ? 1u : 0u);
  }
  unsigned int ge_pos = 0, ge_neg = 0, below = 0, equal = 0;
  pair_scan<RANK_TILE>(
      M, i, pos, [&](int j) { return roc_stage(pred, grade, j, M, C, -1); }, [&](int t, float2 v) { sj[t] = v; },
      [&](int jj, int) {
        const float2 w = sj[jj];
        ge_pos += w.x >= si ? 1u : 0u;
        ge_neg += w.y >= si ? 1u : 0u;
        below += w.y < si ? 1u : 0u;
        equal += w.y == si ? 1u : 0u;
      });
  const unsigned int ge_all = ge_pos + ge_neg;
  // ge_all >= 1 for a finite positive (j = i); a NaN positive has ge_all = 0: its term is left out (the flag reports it)
  const double term = (pos && ge_all > 0) ? (double)ge_pos / (double)ge_all : 0.0;
  const double tsum = block_sum_tree<RANK_TILE, double>(term, red);
  if (threadIdx.x == 0) part[blockIdx.x] = tsum;
  const unsigned long long tot[4] = {wave_sum_u64(pos ? 1ull : 0ull), wave_sum_u64(below), wave_sum_u64(equal),
                                     wave_sum_u64(bad)};       // (the four sums first: their shuffles overlap)
#pragma unroll
  for (int k = 0; k < 4; ++k) lane0_atomic_add(&counts[k], tot[k]);
}

// One workgroup: the blocks' parts in the fixed order of strided_tree_sum.
__global__ __launch_bounds__(RANK_TILE) void rank_finish_kernel(const double* __restrict__ part, int nblocks,
                                                                double* __restrict__ ap_sum) {
  __shared__ double red[RANK_TILE];
  const double s = strided_tree_sum<RANK_TILE>(part, nblocks, 1, 0, red);
  if (threadIdx.x == 0) ap_sum[0] = s;
}

// ---- ph_rank_counts_classes: the counts of rank_counts_kernel for every one-vs-rest column at once.
// Row n is a positive of class g = grade[n] only (of none when g lies outside [0, C)), so thread = row n with
// s_i = pred[n][g]; the rows j stream through LDS in tiles of 256 rows x C columns (staged once for all classes) and the
// thread reads column g of each: w = sj[jj][g], positive when gj[jj] == g.  The last tile is padded with NaN scores, which
// drop out of every comparison.  acc[c][0..3] collects P, concordant, tied, bad of the block per class in LDS (32-bit: at
// most 256 * 2^20 per block), then 64-bit atomics into counts; part[block][c] = the fixed tree over the block's terms of class c.
__global__ __launch_bounds__(RANK_TILE) void rank_counts_classes_kernel(const float* __restrict__ pred,
                                                                        const int64_t* __restrict__ grade, int N, int C,
                                                                        unsigned long long* __restrict__ counts,
                                                                        double* __restrict__ part) {
  __shared__ float sj[RANK_TILE * CONF_MAX_C];
  __shared__ int gj[RANK_TILE];
  __shared__ double red[RANK_TILE];
  __shared__ unsigned int acc[CONF_MAX_C * 4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x * RANK_TILE + tid;
  const float qnan = __builtin_nanf("");
  if (tid < C * 4) acc[tid] = 0;
  __syncthreads();
  int g = -1;                  // the class this row is a positive of
  float si = 0.f;
  if (n < N) {
    const int64_t g64 = grade[n];
    const bool in_range = g64 >= 0 && g64 < (int64_t)C;
    if (in_range) {
      g = (int)g64;
      si = pred[(size_t)n * C + g];
      atomicAdd(&acc[g * 4 + 0], 1u);
    } else {
      atomicAdd(&acc[3], 1u);                      // (class 0 carries the labels out of range, as the micro kernel has it)
    }
    for (int c = 0; c < C; ++c)
      if (!isfinite(pred[(size_t)n * C + c])) atomicAdd(&acc[c * 4 + 3], 1u);
  }
  const bool pos = g >= 0;
  unsigned int ge_pos = 0, ge_all = 0, below = 0, equal = 0;
  // A thread fetches the label of row j.  The row's C scores (a run-time count: not for registers) go from global memory to
  // LDS in put, as part of the tile's RANK_TILE * C consecutive words.
  pair_scan<RANK_TILE>(
      N, n, pos,
      [&](int j) {
        const int64_t v = j < N ? grade[j] : (int64_t)-1;
        return make_int2((v >= 0 && v < (int64_t)C) ? (int)v : -1, j - tid);
      },
      [&](int t, int2 v) {               // v.x = the label, v.y = j0
        gj[t] = v.x;
        const int words = min(RANK_TILE, N - v.y) * C;
        for (int k = t; k < RANK_TILE * C; k += RANK_TILE) sj[k] = k < words ? pred[(size_t)v.y * C + k] : qnan;
      },
      [&](int jj, int) {
        const float w = sj[jj * C + g];
        const bool p = gj[jj] == g, ge = w >= si;        // (& of evaluated flags: the scan stays free of branches)
        ge_all += ge ? 1u : 0u;
        ge_pos += (p & ge) ? 1u : 0u;
        below += (!p & (w < si)) ? 1u : 0u;
        equal += (!p & (w == si)) ? 1u : 0u;
      });
  if (pos) {
    if (below) atomicAdd(&acc[g * 4 + 1], below);
    if (equal) atomicAdd(&acc[g * 4 + 2], equal);
  }
  // ge_all >= 1 for a positive whose score is not a NaN (j = n); a NaN positive has ge_all = 0: its term is left out
  const double term = (pos && ge_all > 0) ? (double)ge_pos / (double)ge_all : 0.0;
  for (int c = 0; c < C; ++c) {
    const double tsum = block_sum_tree<RANK_TILE, double>(g == c ? term : 0.0, red);
    if (tid == 0) part[(size_t)blockIdx.x * C + c] = tsum;
  }
  if (tid < C * 4 && acc[tid]) atomicAdd(&counts[tid], (unsigned long long)acc[tid]);
}

// Workgroup c: the finish of rank_finish_kernel over part[b][c], b = 0 .. nblocks - 1.
__global__ __launch_bounds__(RANK_TILE) void rank_finish_classes_kernel(const double* __restrict__ part, int nblocks, int C,
                                                                        double* __restrict__ ap_sum) {
  __shared__ double red[RANK_TILE];
  const double s = strided_tree_sum<RANK_TILE>(part, nblocks, C, blockIdx.x, red);
  if (threadIdx.x == 0) ap_sum[blockIdx.x] = s;
}

// ---- ph_roc_points: distinct-value placement (ph_pairscan.h) of the scores of the selected problem.
// Pass 1, thread = element i: tp_i / fp_i = #{positive / negative j: s_j >= s_i}; rep[i] = s_i where i represents its score,
// NaN otherwise; tpfp[i] = (tp_i, fp_i).  npoints[0] += representatives, npoints[1] += bad.
__global__ __launch_bounds__(RANK_TILE) void roc_count_kernel(const float* __restrict__ pred, const int64_t* __restrict__ grade,
                                                              int M, int C, int cls, float* __restrict__ rep,
                                                              int2* __restrict__ tpfp, int* __restrict__ npoints) {
  __shared__ float2 sj[RANK_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * RANK_TILE + tid;
  const bool live = i < M;
  const float qnan = __builtin_nanf("");
  float si = qnan;
  unsigned int bad = 0;
  if (live) {
    const RocElem e = roc_elem(pred, grade, i, C, cls);
    si = e.s;
    bad = e.bad;
  }
  unsigned int tp = 0, fp = 0, before = 0;
  pair_scan<RANK_TILE>(
      M, i, true, [&](int j) { return roc_stage(pred, grade, j, M, C, cls); }, [&](int t, float2 v) { sj[t] = v; },
      [&](int jj, int lim) {
        const float2 w = sj[jj];
        tp += w.x >= si ? 1u : 0u;
        fp += w.y >= si ? 1u : 0u;
        before += equal_before(w.x == si || w.y == si, jj, lim);
      });
  const bool is_rep = live && represents(si, before);
  if (live) {
    rep[i] = is_rep ? si : qnan;
    tpfp[i] = make_int2((int)tp, (int)fp);
  }
  wave_atomic_add(&npoints[0], is_rep ? 1 : 0);
  wave_atomic_add(&npoints[1], (int)bad);
}

// Pass 2: a representative leaves its threshold and counts in its slot, the number of representatives with a LARGER score.
__global__ __launch_bounds__(RANK_TILE) void roc_place_kernel(const float* __restrict__ rep, const int2* __restrict__ tpfp, int M,
                                                              int* __restrict__ fps, int* __restrict__ tps,
                                                              float* __restrict__ thr) {
  __shared__ float sj[RANK_TILE];
  const int i = blockIdx.x * RANK_TILE + threadIdx.x;
  const float qnan = __builtin_nanf("");
  const float si = i < M ? rep[i] : qnan;
  const bool is_rep = si == si;
  unsigned int slot = 0;
  pair_scan<RANK_TILE>(
      M, i, is_rep, [&](int j) { return j < M ? rep[j] : qnan; }, [&](int t, float v) { sj[t] = v; },
      [&](int jj, int) { slot += rep_beyond<true>(sj[jj], si); });
  if (is_rep && slot < (unsigned int)M) {
    const int2 c = tpfp[i];
    thr[slot] = si;
    tps[slot] = c.x;
    fps[slot] = c.y;
  }
}

// conf[t * C + p] += 1 for every row whose label t lies in [0, C), p = the first maximum of the row (np.argmax: a later equal
// value does not replace it).  A row whose label is out of range is left out - it has no cell.  Per-block histogram in LDS.
__global__ __launch_bounds__(CONF_THREADS) void confusion_counts_kernel(const float* __restrict__ pred, const int64_t* __restrict__ grade,
                                                                        int N, int C, unsigned long long* __restrict__ conf) {
  __shared__ unsigned int hist[CONF_MAX_C * CONF_MAX_C];
  const int tid = threadIdx.x;
  for (int k = tid; k < C * C; k += CONF_THREADS) hist[k] = 0;
  __syncthreads();
  const int n = blockIdx.x * CONF_THREADS + tid;
  if (n < N) {
    const float* row = pred + (size_t)n * C;
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > best) { best = v; arg = c; }
    }
    const int64_t g = grade[n];
    if (g >= 0 && g < (int64_t)C) atomicAdd(&hist[(int)g * C + arg], 1u);
  }
  __syncthreads();
  for (int k = tid; k < C * C; k += CONF_THREADS)
    if (hist[k]) atomicAdd(&conf[k], (unsigned long long)hist[k]);
}

// Thread = (group g, column c).  Rows order[offsets[g]] .. order[offsets[g + 1] - 1], in that (ascending) order.
// mean: float64 running sum, one division, one rounding to float32.  max: starts at -inf (the inputs are negative).
// A row index outside [0, N) is skipped and the offsets are clamped to [0, N]: device data cannot make the kernel read
// outside x (the entry validates the host copy of the offsets).
__global__ void group_agg_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets, const int32_t* __restrict__ order,
                                 int N, int C, int G, int fun, float* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)G * C) return;
  const int g = (int)(t / C), c = (int)(t - (size_t)g * C);
  const int lo = min(max(offsets[g], 0), N), hi = min(max(offsets[g + 1], lo), N);
  if (fun == 0) {
    double acc = 0.0;
    for (int k = lo; k < hi; ++k) {
      const int r = order[k];
      if (r < 0 || r >= N) continue;
      acc += (double)x[(size_t)r * C + c];
    }
    out[t] = (float)(acc / (double)(hi - lo));
  } else {
    float m = -INFINITY;
    for (int k = lo; k < hi; ++k) {
      const int r = order[k];
      if (r < 0 || r >= N) continue;
      m = fmaxf(m, x[(size_t)r * C + c]);
    }
    out[t] = m;
  }
}

// ---- ph_group_quantile: numpy's percentile, method "linear", of every column of every group.
// n values, s ascending:  h = (n - 1) q,  lo = floor(h),  hi = min(lo + 1, n - 1),  t = h - lo,  a = s[lo],  b = s[hi],
// out = (float)(t == 0 || a == b ? a : a + (b - a) t) in double.  No sort: the stable rank of element k,
//   rank_k = #{m : x_m < x_k} + #{m before k in CSR order : x_m == x_k},
// is a permutation of 0 .. n - 1 when no value is a NaN, so exactly one element has rank lo and one has rank hi; they hand
// a and b over (no atomics: independent of scheduling).  A NaN in the column gives NaN.  A row index outside [0, N) is an
// absent element (it holds a NaN, which drops out of every comparison, and is not counted in n); the offsets are clamped
// to [0, N] and the group length to the form's capacity: device data cannot make either kernel read outside x or its LDS.
struct QuantileSel {
  int lo, hi;
  double t;
};

__device__ __forceinline__ QuantileSel quantile_sel(int n, double q) {
  const double h = (double)(n - 1) * q, fl = floor(h);
  QuantileSel s;
  s.lo = min(max((int)fl, 0), n - 1);
  s.hi = min(s.lo + 1, n - 1);
  s.t = h - fl;
  return s;
}

// (two roundings, a product and a sum, as the numpy restatement has them: no fused multiply-add)
__device__ __forceinline__ float quantile_lerp(float a, float b, double t) {
#pragma clang fp contract(off)
  const double da = (double)a, db = (double)b;
  return (float)((t == 0.0 || da == db) ? da : da + (db - da) * t);
}

// Groups of at most 64 rows: one wave per (group, column), one value per lane, the other lanes' values by cross-lane reads.
__global__ __launch_bounds__(QUANT_THREADS) void group_quantile_wave_kernel(const float* __restrict__ x,
                                                                            const int32_t* __restrict__ offsets,
                                                                            const int32_t* __restrict__ order, int N, int C,
                                                                            int G, double q, float* __restrict__ out) {
  constexpr int WAVES = QUANT_THREADS / 64;
  const int lane = threadIdx.x & 63;
  const float qnan = __builtin_nanf("");
  const size_t items = (size_t)G * C, stride = (size_t)gridDim.x * WAVES;
  for (size_t t = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < items; t += stride) {
    const int g = (int)(t / C), c = (int)(t - (size_t)g * C);
    const int lo = min(max(offsets[g], 0), N), hi = min(max(offsets[g + 1], lo), N);
    const int n = min(hi - lo, 64);
    float v = qnan;
    bool valid = false;
    if (lane < n) {
      const int r = order[lo + lane];
      if (r >= 0 && r < N) {
        v = x[(size_t)r * C + c];
        valid = true;
      }
    }
    const int n_eff = __popcll(__ballot(valid));
    const bool has_nan = __ballot(valid && v != v) != 0ull;
    int rank = 0;
    for (int m = 0; m < n; ++m) {
      const float w = __shfl(v, m, 64);
      rank += (w < v ? 1 : 0) + ((w == v && m < lane) ? 1 : 0);
    }
    float res = qnan;
    if (n_eff > 0 && !has_nan) {        // (wave-uniform)
      const QuantileSel s = quantile_sel(n_eff, q);
      const unsigned long long ma = __ballot(valid && rank == s.lo), mb = __ballot(valid && rank == s.hi);
      if (ma != 0ull && mb != 0ull) {
        const float a = __shfl(v, __ffsll((long long)ma) - 1, 64), b = __shfl(v, __ffsll((long long)mb) - 1, 64);
        res = quantile_lerp(a, b, s.t);
      }
    }
    if (lane == 0) out[t] = res;
  }
}

// Larger groups (up to QUANT_MAX_GROUP rows): one workgroup per group, the columns looped; the group's column staged in
// LDS, thread tid ranks the elements tid, tid + 256, .. (four at a time in registers against every staged value).
__global__ __launch_bounds__(QUANT_THREADS) void group_quantile_block_kernel(const float* __restrict__ x,
                                                                             const int32_t* __restrict__ offsets,
                                                                             const int32_t* __restrict__ order, int N, int C,
                                                                             int G, double q, float* __restrict__ out) {
  __shared__ float s[QUANT_MAX_GROUP];
  __shared__ unsigned int red[QUANT_THREADS / 64];
  __shared__ float sel[2];
  const int tid = threadIdx.x, g = blockIdx.x;
  const float qnan = __builtin_nanf("");
  if (g >= G) return;
  const int lo = min(max(offsets[g], 0), N), hi = min(max(offsets[g + 1], lo), N);
  const int n = min(hi - lo, QUANT_MAX_GROUP);
  for (int c = 0; c < C; ++c) {
    unsigned int cnt = 0;              // valid elements | NaN values << 16 of this thread
    for (int k = tid; k < n; k += QUANT_THREADS) {
      const int r = order[lo + k];
      float v = qnan;
      if (r >= 0 && r < N) {
        v = x[(size_t)r * C + c];
        cnt += 1u + (v != v ? 1u << 16 : 0u);
      }
      s[k] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = cnt;
    if (tid == 0) sel[0] = sel[1] = qnan;
    __syncthreads();
    unsigned int tot = 0;
#pragma unroll
    for (int w = 0; w < QUANT_THREADS / 64; ++w) tot += red[w];
    // (at most 4096 of either: the two halves of the packed sum never carry into each other)
    const int n_eff = (int)(tot & 0xffffu);
    const bool has_nan = (tot >> 16) != 0u;
    if (n_eff > 0 && !has_nan) {       // (uniform over the workgroup)
      const QuantileSel qs = quantile_sel(n_eff, q);
      for (int k0 = tid; k0 < n; k0 += 4 * QUANT_THREADS) {
        float xk[4];
        int rank[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + u * QUANT_THREADS;
          xk[u] = k < n ? s[k] : qnan;
          rank[u] = 0;
        }
        for (int m = 0; m < n; ++m) {
          const float w = s[m];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            rank[u] += (w < xk[u] ? 1 : 0) + ((w == xk[u] && m < k0 + u * QUANT_THREADS) ? 1 : 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (xk[u] != xk[u]) continue;        // an absent element (or past the end): no rank
          if (rank[u] == qs.lo) sel[0] = xk[u];
          if (rank[u] == qs.hi) sel[1] = xk[u];
        }
      }
      __syncthreads();
      if (tid == 0) out[(size_t)g * C + c] = quantile_lerp(sel[0], sel[1], qs.t);
    } else if (tid == 0) {
      out[(size_t)g * C + c] = qnan;
    }
    __syncthreads();                   // s, red and sel are rewritten for the next column
  }
}

bool rank_shape_ok(int N, int C) { return N >= 1 && C >= 1 && (int64_t)N * C <= RANK_MAX_M; }

// ph_rank_counts_classes and ph_roc_points: the per-column problems have N elements each
bool class_shape_ok(int N, int C) { return N >= 1 && N <= RANK_MAX_M && C >= 1 && C <= CONF_MAX_C; }

// What ph_group_agg and ph_group_quantile check alike: the pointers, the N / C / G ranges and the host offsets (from 0 to N, no
// group empty or negative, and none longer than max_len where max_len > 0).  *largest: the longest group.
bool group_args_ok(const float* x, const int32_t* offsets, const int32_t* order, const int32_t* offsets_host, int N, int C, int G,
                   const float* out, int max_len, int* largest) {
  if (!x || !offsets || !order || !offsets_host || !out) return false;
  if (N < 1 || N > AGG_MAX_N || C < 1 || C > AGG_MAX_C || G < 1 || G > N) return false;
  if (offsets_host[0] != 0 || offsets_host[G] != N) return false;
  *largest = 0;
  for (int g = 0; g < G; ++g) {
    const int64_t len = (int64_t)offsets_host[g + 1] - (int64_t)offsets_host[g];
    if (len <= 0 || (max_len > 0 && len > max_len)) return false;
    if ((int)len > *largest) *largest = (int)len;
  }
  return true;
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

size_t ph_rank_counts_workspace_bytes(int N, int C) {
  if (!rank_shape_ok(N, C)) return 0;
  return sizeof(double) * (size_t)cdiv(N * C, RANK_TILE);
}

int ph_rank_counts(const float* pred, const int64_t* grade, int N, int C, int64_t* counts, double* ap_sum, void* workspace,
                   hipStream_t st) {
  if (!pred || !grade || !counts || !ap_sum || !workspace || !rank_shape_ok(N, C)) return PH_EINVAL;
  const int M = N * C, nblocks = cdiv(M, RANK_TILE);
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 4, st) != hipSuccess) return PH_ELAUNCH;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(rank_counts_kernel, dim3(nblocks), dim3(RANK_TILE), 0, st, pred, grade, M, C,
                     reinterpret_cast<unsigned long long*>(counts), part);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_finish_kernel, dim3(1), dim3(RANK_TILE), 0, st, part, nblocks, ap_sum);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

size_t ph_rank_counts_classes_workspace_bytes(int N, int C) {
  if (!class_shape_ok(N, C)) return 0;
  return sizeof(double) * (size_t)cdiv(N, RANK_TILE) * (size_t)C;
}

int ph_rank_counts_classes(const float* pred, const int64_t* grade, int N, int C, int64_t* counts, double* ap_sum,
                           void* workspace, hipStream_t st) {
  if (!pred || !grade || !counts || !ap_sum || !workspace || !class_shape_ok(N, C)) return PH_EINVAL;
  const int nblocks = cdiv(N, RANK_TILE);
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 4 * C, st) != hipSuccess) return PH_ELAUNCH;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(rank_counts_classes_kernel, dim3(nblocks), dim3(RANK_TILE), 0, st, pred, grade, N, C,
                     reinterpret_cast<unsigned long long*>(counts), part);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_finish_classes_kernel, dim3(C), dim3(RANK_TILE), 0, st, part, nblocks, C, ap_sum);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

size_t ph_roc_points_workspace_bytes(int N, int C) {
  if (!class_shape_ok(N, C)) return 0;
  const int64_t pairs = (int64_t)N * C;                 // (the micro problem is served only where it fits)
  return (sizeof(int2) + sizeof(float)) * (size_t)(pairs <= RANK_MAX_M ? pairs : (int64_t)N);
}

int ph_roc_points(const float* pred, const int64_t* grade, int N, int C, int cls, int32_t* fps, int32_t* tps, float* thr,
                  int32_t* npoints, void* workspace, hipStream_t st) {
  if (!pred || !grade || !fps || !tps || !thr || !npoints || !workspace || !class_shape_ok(N, C)) return PH_EINVAL;
  if (cls < -1 || cls >= C || (cls == -1 && (int64_t)N * C > RANK_MAX_M)) return PH_EINVAL;
  const int M = cls >= 0 ? N : N * C, nblocks = cdiv(M, RANK_TILE);
  if (hipMemsetAsync(npoints, 0, sizeof(int32_t) * 2, st) != hipSuccess) return PH_ELAUNCH;
  int2* tpfp = static_cast<int2*>(workspace);           // [M] (tp, fp), then rep [M]
  float* rep = reinterpret_cast<float*>(tpfp + M);
  hipLaunchKernelGGL(roc_count_kernel, dim3(nblocks), dim3(RANK_TILE), 0, st, pred, grade, M, C, cls, rep, tpfp, npoints);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(roc_place_kernel, dim3(nblocks), dim3(RANK_TILE), 0, st, rep, tpfp, M, fps, tps, thr);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_confusion_counts(const float* pred, const int64_t* grade, int N, int C, int64_t* conf, hipStream_t st) {
  if (!pred || !grade || !conf || N < 1 || C < 1 || C > CONF_MAX_C) return PH_EINVAL;
  if (hipMemsetAsync(conf, 0, sizeof(int64_t) * C * C, st) != hipSuccess) return PH_ELAUNCH;
  hipLaunchKernelGGL(confusion_counts_kernel, dim3(cdiv(N, CONF_THREADS)), dim3(CONF_THREADS), 0, st, pred, grade, N, C,
                     reinterpret_cast<unsigned long long*>(conf));
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_group_agg(const float* x, const int32_t* offsets, const int32_t* order, const int32_t* offsets_host, int N, int C, int G,
                 int fun, float* out, hipStream_t st) {
  int largest;
  if (!group_args_ok(x, offsets, order, offsets_host, N, C, G, out, 0, &largest)) return PH_EINVAL;
  if (fun != PH_AGG_MEAN && fun != PH_AGG_MAX) return PH_EINVAL;
  const size_t n = (size_t)G * C;
  hipLaunchKernelGGL(group_agg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, offsets, order, N, C, G, fun, out);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_group_quantile(const float* x, const int32_t* offsets, const int32_t* order, const int32_t* offsets_host, int N, int C,
                      int G, double q, float* out, hipStream_t st) {
  int largest;                                                            // (a longer group does not fit the LDS stage)
  if (!group_args_ok(x, offsets, order, offsets_host, N, C, G, out, PH_QUANTILE_MAX_GROUP, &largest)) return PH_EINVAL;
  if (!(q >= 0.0 && q <= 1.0)) return PH_EINVAL;                          // (a NaN q fails both comparisons)
  static_assert(PH_QUANTILE_MAX_GROUP == QUANT_MAX_GROUP, "the header's limit is the kernel's LDS stage");
  if (largest <= 64) {
    const size_t items = (size_t)G * C, waves = QUANT_THREADS / 64;
    const size_t blocks = (items + waves - 1) / waves;
    hipLaunchKernelGGL(group_quantile_wave_kernel, dim3((unsigned)(blocks < (size_t)QUANT_WAVE_MAX_BLOCKS ? blocks : QUANT_WAVE_MAX_BLOCKS)),
                       dim3(QUANT_THREADS), 0, st, x, offsets, order, N, C, G, q, out);
  } else {
    hipLaunchKernelGGL(group_quantile_block_kernel, dim3((unsigned)G), dim3(QUANT_THREADS), 0, st, x, offsets, order, N, C, G, q, out);
  }
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"

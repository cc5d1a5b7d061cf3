// The survival side of the patient-level test pass: what core/utils_analysis.py computes on the host,
// with numpy and lifelines, from the per-patient hazards -
//   ph_surv_strata       np.percentile(data['Hazard'], [33, 66]) and hazard2grade (:259-263, :398-418, :722): the risk strata,
//   ph_surv_table        lifelines' event table per stratum over every distinct observed time (kmf.fit, logrank_test),
//   ph_surv_logrank_km   the two-sample log-rank sums (O - E, V) of chosen stratum pairs and the Kaplan-Meier estimate per stratum
//                        at every slot of the table (makeKaplanMeierPlot, :719-780).
// No sort anywhere: ranks and slots are exact integer counts from all-pairs passes over LDS tiles of 256, as ph_roc_points has
// them; every workgroup walks the tiles b, b + gridDim.x, .. of its side (at most SURV_MAX_BLOCKS workgroups).
#include "ph_common.h"
#include "ph_pairscan.h"

namespace {

constexpr int SURV_TILE = 256;           // rows per workgroup pass and j-tile length
constexpr int SURV_MAX_N = 1 << 20;
constexpr int SURV_MAX_K = 7;
constexpr int SURV_MAX_G = 8;
constexpr int SURV_MAX_P = 28;
constexpr int SURV_MAX_BLOCKS = 1024;    // the cap of every grid-stride loop below: N = 262 145 is the first size that wraps
constexpr int SURV_CHUNK = 128;          // pairs added into 8-bit packed fields before they are unpacked (128 <= 255)
constexpr size_t STRATA_WS_BYTES = 64;   // picked f32 [2 * 7] (the values of rank lo and hi per cut), then the NaN count

// per cut: the ranks of the two order statistics and the weight between them (host arithmetic, float64)
struct StrataSel {
  int lo[SURV_MAX_K], hi[SURV_MAX_K];
  double t[SURV_MAX_K];
};

struct SurvPairs {
  int a[SURV_MAX_P], b[SURV_MAX_P];
};

int surv_grid(int items) { return cdiv(items, SURV_TILE) < SURV_MAX_BLOCKS ? cdiv(items, SURV_TILE) : SURV_MAX_BLOCKS; }

// numpy's _lerp with both of its forms, unfused (a product, then a sum; the cut stays a double).  t == 0 or a == b returns a
// itself, where numpy evaluates a + (b - a) t and gets NaN from an infinite a or b: the one divergence, for infinite values only.
__device__ __forceinline__ double strata_cut(float a, float b, double t) {
#pragma clang fp contract(off)
  const double da = (double)a, db = (double)b;
  if (t == 0.0 || da == db) return da;
  const double diff = db - da;
  if (t < 0.5) {
    const double prod = diff * t;
    return da + prod;
  }
  const double prod = diff * (1.0 - t);
  return db - prod;
}

// Pass 1 of ph_surv_strata, thread = row i: rank_i = #{j: h_j < h_i} + #{j < i: h_j == h_i} - a permutation of 0 .. N - 1 when
// no hazard is a NaN, so for every cut exactly one row has rank lo and one has rank hi; they leave their values in picked.
// A NaN compares false everywhere (the padding of the last tile too); nan[0] += the NaN hazards (integer atomics).
__global__ __launch_bounds__(SURV_TILE) void strata_rank_kernel(const float* __restrict__ hazard, int N, int K, StrataSel sel,
                                                                float* __restrict__ picked, int* __restrict__ nan) {
  __shared__ float sj[SURV_TILE];
  const int tid = threadIdx.x;
  const float qnan = __builtin_nanf("");
  for (int i0 = blockIdx.x * SURV_TILE; i0 < N; i0 += gridDim.x * SURV_TILE) {
    const int i = i0 + tid;
    const bool live = i < N;
    const float hv = live ? hazard[i] : qnan;
    int rank = 0;
    pair_scan<SURV_TILE>(
        N, i, true, [&](int j) { return j < N ? hazard[j] : qnan; }, [&](int t, float v) { sj[t] = v; },
        [&](int jj, int lim) {
          const float w = sj[jj];
          rank += (w < hv ? 1 : 0) + (int)equal_before(w == hv, jj, lim);
        });
    if (live && hv == hv) {
#pragma unroll
      for (int k = 0; k < SURV_MAX_K; ++k) {
        if (k >= K) break;
        if (rank == sel.lo[k]) picked[2 * k] = hv;
        if (rank == sel.hi[k]) picked[2 * k + 1] = hv;
      }
    }
    wave_atomic_add(&nan[0], (live && hv != hv) ? 1 : 0);
  }
}

// Pass 2: every thread forms the K cuts from picked (a NaN hazard anywhere: every cut NaN), applies the reference's patch
// (K == 2 and cuts[0] == cuts[1]: cuts[0] = 2.99997) and gives its rows the FIRST k with (double)h < cuts[k], else K.
// sizes and bad by integer atomics (a per-workgroup histogram in LDS first); thread 0 of workgroup 0 writes the cuts.
__global__ __launch_bounds__(SURV_TILE) void strata_group_kernel(const float* __restrict__ hazard, int N, int K, StrataSel sel,
                                                                 const float* __restrict__ picked, const int* __restrict__ nan,
                                                                 double* __restrict__ cuts, int* __restrict__ group,
                                                                 int* __restrict__ sizes, int* __restrict__ bad) {
  __shared__ int hist[SURV_MAX_G + 1];                  // [G] the strata, [8] the non-finite hazards
  const int tid = threadIdx.x;
  if (tid <= SURV_MAX_G) hist[tid] = 0;
  __syncthreads();
  const bool any_nan = nan[0] > 0;
  double c[SURV_MAX_K];
#pragma unroll
  for (int k = 0; k < SURV_MAX_K; ++k) {
    c[k] = __builtin_nan("");
    if (k < K && !any_nan) c[k] = strata_cut(picked[2 * k], picked[2 * k + 1], sel.t[k]);
  }
  if (K == 2 && c[0] == c[1]) c[0] = 2.99997;
  if (blockIdx.x == 0 && tid == 0) {
#pragma unroll
    for (int k = 0; k < SURV_MAX_K; ++k)
      if (k < K) cuts[k] = c[k];
  }
  for (int i = blockIdx.x * SURV_TILE + tid; i < N; i += gridDim.x * SURV_TILE) {
    const float h = hazard[i];
    const double hd = (double)h;
    int g = K;
#pragma unroll
    for (int k = SURV_MAX_K - 1; k >= 0; --k)
      if (k < K && hd < c[k]) g = k;
    group[i] = g;
    atomicAdd(&hist[g], 1);
    if (!isfinite(h)) atomicAdd(&hist[SURV_MAX_G], 1);
  }
  __syncthreads();
  if (tid <= K && hist[tid]) atomicAdd(&sizes[tid], hist[tid]);
  if (tid == SURV_MAX_G && hist[tid]) atomicAdd(&bad[0], hist[tid]);
}

// ---- ph_surv_table.  A row takes part when its group lies in [0, G) and its time is not a NaN.
__device__ __forceinline__ bool surv_row_ok(float t, int g, int G) { return g >= 0 && g < G && t == t; }

// the time of row j where it takes part, NaN where it does not or lies past the end
__device__ __forceinline__ float surv_time(const float* __restrict__ survtime, const int* __restrict__ group, int j, int N, int G) {
  if (j < N) {
    const float t = survtime[j];
    if (surv_row_ok(t, group[j], G)) return t;
  }
  return __builtin_nanf("");
}

// Distinct-value placement (ph_pairscan.h) of the times.  Pass 1, thread = row i: rep[i] = t_i where i represents its time, NaN
// otherwise; npoints[0] += representatives, npoints[1] += the rows that take part in nothing.
__global__ __launch_bounds__(SURV_TILE) void surv_rep_kernel(const float* __restrict__ survtime, const int* __restrict__ group, int N,
                                                             int G, float* __restrict__ rep, int* __restrict__ npoints) {
  __shared__ float sj[SURV_TILE];
  for (int i0 = blockIdx.x * SURV_TILE; i0 < N; i0 += gridDim.x * SURV_TILE) {
    const int i = i0 + threadIdx.x;
    const bool live = i < N;
    const float ti = surv_time(survtime, group, i, N, G);
    unsigned int before = 0;
    pair_scan<SURV_TILE>(
        N, i, true, [&](int j) { return surv_time(survtime, group, j, N, G); }, [&](int t, float v) { sj[t] = v; },
        [&](int jj, int lim) { before += equal_before(sj[jj] == ti, jj, lim); });
    const bool is_rep = represents(ti, before);
    if (live) rep[i] = is_rep ? ti : __builtin_nanf("");
    wave_atomic_add(&npoints[0], is_rep ? 1 : 0);
    wave_atomic_add(&npoints[1], (live && ti != ti) ? 1 : 0);
  }
}

// Pass 2, thread = representative i: its slot = the number of representatives with a SMALLER time, and the three counts of
// its time over all rows j per group.  Row j carries one 8-bit field per group in a 64-bit word (wo: 1 in the field of its
// group when it has an event, wc: when it has none); the selected words of SURV_CHUNK rows are added packed (a field
// reaches at most 128) and then unpacked into the 32-bit counters.
struct SurvStage {             // what row j brings: its time and its rep entry (NaN: none), wo and wc
  float t, r;
  unsigned long long wo, wc;
};

__global__ __launch_bounds__(SURV_TILE) void surv_place_kernel(const float* __restrict__ survtime, const float* __restrict__ event,
                                                               const int* __restrict__ group, const float* __restrict__ rep, int N,
                                                               int G, float* __restrict__ times, int* __restrict__ at_risk,
                                                               int* __restrict__ observed, int* __restrict__ censored) {
  __shared__ float st[SURV_TILE], sr[SURV_TILE];
  __shared__ unsigned long long swo[SURV_TILE], swc[SURV_TILE];
  const int tid = threadIdx.x;
  const float qnan = __builtin_nanf("");
  for (int i0 = blockIdx.x * SURV_TILE; i0 < N; i0 += gridDim.x * SURV_TILE) {
    const int i = i0 + tid;
    const float ti = i < N ? rep[i] : qnan;
    const bool is_rep = ti == ti;
    unsigned int slot = 0, cge[SURV_MAX_G], cob[SURV_MAX_G], cce[SURV_MAX_G];
#pragma unroll
    for (int g = 0; g < SURV_MAX_G; ++g) cge[g] = cob[g] = cce[g] = 0;
    pair_tiles<SURV_TILE>(
        N, is_rep,
        [&](int j) {
          SurvStage s = {qnan, qnan, 0ull, 0ull};
          if (j < N) {
            const float tj = survtime[j];
            const int gj = group[j];
            s.r = rep[j];
            if (surv_row_ok(tj, gj, G)) {
              s.t = tj;
              const unsigned long long w = 1ull << (8 * gj);
              if (event[j] > 0.f) s.wo = w; else s.wc = w;
            }
          }
          return s;
        },
        [&](int t, const SurvStage& s) { st[t] = s.t; sr[t] = s.r; swo[t] = s.wo; swc[t] = s.wc; },
        [&](int) {
          for (int c0 = 0; c0 < SURV_TILE; c0 += SURV_CHUNK) {
            unsigned long long age = 0ull, aob = 0ull, ace = 0ull;
#pragma unroll 8
            for (int jj = c0; jj < c0 + SURV_CHUNK; ++jj) {
              const float tj = st[jj];
              const unsigned long long o = swo[jj], c = swc[jj];
              age += tj >= ti ? (o | c) : 0ull;
              aob += tj == ti ? o : 0ull;
              ace += tj == ti ? c : 0ull;
              slot += rep_beyond<false>(sr[jj], ti);
            }
#pragma unroll
            for (int g = 0; g < SURV_MAX_G; ++g) {
              cge[g] += (unsigned int)(age >> (8 * g)) & 0xffu;
              cob[g] += (unsigned int)(aob >> (8 * g)) & 0xffu;
              cce[g] += (unsigned int)(ace >> (8 * g)) & 0xffu;
            }
          }
        });
    if (is_rep && slot < (unsigned int)N) {
      times[slot] = ti;
      const size_t row = (size_t)slot * G;
#pragma unroll
      for (int g = 0; g < SURV_MAX_G; ++g) {
        if (g < G) {
          at_risk[row + g] = (int)cge[g];
          observed[row + g] = (int)cob[g];
          censored[row + g] = (int)cce[g];
        }
      }
    }
  }
}

// ---- ph_surv_logrank_km.  The slot count is read on the device and clamped to the arrays' capacity.
__device__ __forceinline__ int surv_points(const int* __restrict__ npoints, int N) { return min(max(npoints[0], 0), N); }

// the Kaplan-Meier factor of one slot of one group: 1 - d / n in float64, 1 where nobody is at risk
__device__ __forceinline__ double km_factor(int n, int d) { return n > 0 ? 1.0 - (double)d / (double)n : 1.0; }

// Tile = 256 slots.  part[tile][p] = the fixed-tree sums of the slots' (O - E, V) terms of pair p (0.0 for the slots past the
// end); tprod[tile][g] = the product of the tile's Kaplan-Meier factors of group g, multiplied in slot order by one thread.
__global__ __launch_bounds__(SURV_TILE) void surv_terms_kernel(const int* __restrict__ at_risk, const int* __restrict__ observed,
                                                               const int* __restrict__ npoints, int N, int G, SurvPairs pairs, int P,
                                                               double* __restrict__ part, double* __restrict__ tprod) {
#pragma clang fp contract(off)
  __shared__ double red[SURV_TILE];
  const int tid = threadIdx.x;
  const int np = surv_points(npoints, N), tiles = (np + SURV_TILE - 1) / SURV_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int k = tile * SURV_TILE + tid;
    const bool live = k < np;
    for (int p = 0; p < P; ++p) {
      double oe = 0.0, v = 0.0;
      if (live) {
        const size_t row = (size_t)k * G;
        const double na = (double)at_risk[row + pairs.a[p]], nb = (double)at_risk[row + pairs.b[p]];
        const double da = (double)observed[row + pairs.a[p]], db = (double)observed[row + pairs.b[p]];
        const double n = na + nb, d = da + db;
        if (d > 0.0) {         // (an event among the pair's members: n >= d > 0)
          const double dn = d * na;
          oe = da - dn / n;
          if (n > 1.0) {
            const double num = na * (n - na) * d * (n - d), den = n * n * (n - 1.0);
            v = num / den;
          }
        }
      }
      const double s_oe = block_sum_tree<SURV_TILE>(oe, red);
      const double s_v = block_sum_tree<SURV_TILE>(v, red);
      if (tid == 0) {
        part[((size_t)tile * P + p) * 2] = s_oe;
        part[((size_t)tile * P + p) * 2 + 1] = s_v;
      }
    }
    if (tid < G) {
      double acc = 1.0;
      const int end = min(tile * SURV_TILE + SURV_TILE, np);
      for (int kk = tile * SURV_TILE; kk < end; ++kk) acc *= km_factor(at_risk[(size_t)kk * G + tid], observed[(size_t)kk * G + tid]);
      tprod[(size_t)tile * G + tid] = acc;
    }
  }
}

// One workgroup.  stat[p] = per pair and sum, the tiles' parts in the fixed order of strided_tree_sum.
// tpre[tile][g] = the product of the tiles before `tile`, multiplied in tile order by thread g.
__global__ __launch_bounds__(SURV_TILE) void surv_finish_kernel(const double* __restrict__ part, const double* __restrict__ tprod,
                                                                const int* __restrict__ npoints, int N, int G, int P,
                                                                double* __restrict__ stat, double* __restrict__ tpre) {
  __shared__ double red[SURV_TILE];
  const int tid = threadIdx.x;
  const int np = surv_points(npoints, N), tiles = (np + SURV_TILE - 1) / SURV_TILE;
  for (int w = 0; w < 2 * P; ++w) {
    const double s = strided_tree_sum<SURV_TILE>(part, tiles, 2 * P, w, red);
    if (tid == 0) stat[w] = s;
  }
  if (tid < G) {
    double acc = 1.0;
    for (int t = 0; t < tiles; ++t) {
      tpre[(size_t)t * G + tid] = acc;
      acc *= tprod[(size_t)t * G + tid];
    }
  }
}

// Thread = (tile, group): surv[k][g] for the tile's slots, from tpre[tile][g] on in slot order.
__global__ __launch_bounds__(SURV_TILE) void surv_km_kernel(const int* __restrict__ at_risk, const int* __restrict__ observed,
                                                            const int* __restrict__ npoints, int N, int G,
                                                            const double* __restrict__ tpre, double* __restrict__ surv) {
  const int np = surv_points(npoints, N), tiles = (np + SURV_TILE - 1) / SURV_TILE;
  const int items = tiles * G;
  for (int it = blockIdx.x * SURV_TILE + threadIdx.x; it < items; it += gridDim.x * SURV_TILE) {
    const int tile = it / G, g = it - tile * G;
    double acc = tpre[it];
    const int end = min(tile * SURV_TILE + SURV_TILE, np);
    for (int kk = tile * SURV_TILE; kk < end; ++kk) {
      acc *= km_factor(at_risk[(size_t)kk * G + g], observed[(size_t)kk * G + g]);
      surv[(size_t)kk * G + g] = acc;
    }
  }
}

bool surv_n_ok(int N) { return N >= 2 && N <= SURV_MAX_N; }
bool strata_shape_ok(int N, int K) { return surv_n_ok(N) && K >= 1 && K <= SURV_MAX_K; }
bool table_shape_ok(int N, int G) { return surv_n_ok(N) && G >= 1 && G <= SURV_MAX_G; }
bool logrank_shape_ok(int N, int G, int P) { return table_shape_ok(N, G) && P >= 0 && P <= SURV_MAX_P; }

// h = (N - 1) (q / 100), lo = floor(h), hi = min(lo + 1, N - 1), t = h - lo: numpy's virtual index and gamma, unfused
StrataSel strata_sel(int N, const double* q, int K) {
#pragma clang fp contract(off)
  StrataSel s = {};
  for (int k = 0; k < K; ++k) {
    const double frac = q[k] / 100.0;
    const double h = (double)(N - 1) * frac;
    const double fl = __builtin_floor(h);
    int lo = (int)fl;
    lo = lo < 0 ? 0 : (lo > N - 1 ? N - 1 : lo);
    s.lo[k] = lo;
    s.hi[k] = lo + 1 < N - 1 ? lo + 1 : N - 1;
    s.t[k] = h - fl;
  }
  return s;
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

size_t ph_surv_strata_workspace_bytes(int N, int K) { return strata_shape_ok(N, K) ? STRATA_WS_BYTES : 0; }

int ph_surv_strata(const float* hazard, int N, const double* q, int K, double* cuts, int32_t* group, int32_t* sizes, int32_t* bad,
                   void* workspace, hipStream_t st) {
  if (!hazard || !q || !cuts || !group || !sizes || !bad || !workspace || !strata_shape_ok(N, K)) return PH_EINVAL;
  for (int k = 0; k < K; ++k)
    if (!(q[k] >= 0.0 && q[k] <= 100.0)) return PH_EINVAL;                // (a NaN q fails both comparisons)
  static_assert(sizeof(float) * 2 * SURV_MAX_K + sizeof(int) <= STRATA_WS_BYTES, "picked and the NaN count fit the workspace");
  const StrataSel sel = strata_sel(N, q, K);
  float* picked = static_cast<float*>(workspace);
  int* nan = reinterpret_cast<int*>(picked + 2 * SURV_MAX_K);
  if (hipMemsetAsync(workspace, 0, STRATA_WS_BYTES, st) != hipSuccess) return PH_ELAUNCH;
  if (hipMemsetAsync(sizes, 0, sizeof(int32_t) * (K + 1), st) != hipSuccess) return PH_ELAUNCH;
  if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return PH_ELAUNCH;
  const int blocks = surv_grid(N);
  hipLaunchKernelGGL(strata_rank_kernel, dim3(blocks), dim3(SURV_TILE), 0, st, hazard, N, K, sel, picked, nan);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(strata_group_kernel, dim3(blocks), dim3(SURV_TILE), 0, st, hazard, N, K, sel, picked, nan, cuts, group, sizes,
                     bad);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

size_t ph_surv_table_workspace_bytes(int N, int G) { return table_shape_ok(N, G) ? sizeof(float) * (size_t)N : 0; }

int ph_surv_table(const float* survtime, const float* event, const int32_t* group, int N, int G, float* times, int32_t* at_risk,
                  int32_t* observed, int32_t* censored, int32_t* npoints, void* workspace, hipStream_t st) {
  if (!survtime || !event || !group || !times || !at_risk || !observed || !censored || !npoints || !workspace ||
      !table_shape_ok(N, G))
    return PH_EINVAL;
  if (hipMemsetAsync(npoints, 0, sizeof(int32_t) * 2, st) != hipSuccess) return PH_ELAUNCH;
  float* rep = static_cast<float*>(workspace);
  const int blocks = surv_grid(N);
  hipLaunchKernelGGL(surv_rep_kernel, dim3(blocks), dim3(SURV_TILE), 0, st, survtime, group, N, G, rep, npoints);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(surv_place_kernel, dim3(blocks), dim3(SURV_TILE), 0, st, survtime, event, group, rep, N, G, times, at_risk,
                     observed, censored);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

size_t ph_surv_logrank_km_workspace_bytes(int N, int G, int P) {
  if (!logrank_shape_ok(N, G, P)) return 0;
  return sizeof(double) * (size_t)cdiv(N, SURV_TILE) * (size_t)(2 * P + 2 * G);
}

int ph_surv_logrank_km(const int32_t* at_risk, const int32_t* observed, const int32_t* npoints, int N, int G, const int32_t* pairs,
                       int P, double* stat, double* surv, void* workspace, hipStream_t st) {
  if (!at_risk || !observed || !npoints || !surv || !workspace || !logrank_shape_ok(N, G, P)) return PH_EINVAL;
  if (P > 0 && (!pairs || !stat)) return PH_EINVAL;
  SurvPairs pr = {};
  for (int p = 0; p < P; ++p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= G || b < 0 || b >= G || a == b) return PH_EINVAL;
    pr.a[p] = a;
    pr.b[p] = b;
  }
  const int tiles = cdiv(N, SURV_TILE);
  double* part = static_cast<double*>(workspace);       // [tiles][P][2], then tprod [tiles][G], then tpre [tiles][G]
  double* tprod = part + (size_t)tiles * 2 * P;
  double* tpre = tprod + (size_t)tiles * G;
  hipLaunchKernelGGL(surv_terms_kernel, dim3(tiles < SURV_MAX_BLOCKS ? tiles : SURV_MAX_BLOCKS), dim3(SURV_TILE), 0, st, at_risk,
                     observed, npoints, N, G, pr, P, part, tprod);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(surv_finish_kernel, dim3(1), dim3(SURV_TILE), 0, st, part, tprod, npoints, N, G, P, stat, tpre);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(surv_km_kernel, dim3(surv_grid(tiles * G)), dim3(SURV_TILE), 0, st, at_risk, observed, npoints, N, G, tpre,
                     surv);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"

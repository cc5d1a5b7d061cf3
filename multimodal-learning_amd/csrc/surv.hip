// The survival (Cox) task of the stage-1 mean-teacher trainer (MICCAI-2022/train_test_MT.py:149-152,180-203 with
// --task surv): the sigmoid-range head of the three networks (networks_new.py:236-237,327-328, resnets.py:252-253), the
// fused per-step survival loss (three Cox partial likelihoods sharing one risk-set pass + the MSE consistency terms of
// CL_utils/KD_losses.py:20-22) and the concordance counts behind the evaluation's C-index (utils.py:424-425).
#include "ph_common.h"
#include "ph_kernels.h"
#include "ph_pairscan.h"

namespace {

constexpr int SURV_MAX_B = 4096;        // one workgroup, everything in LDS (as cox_kernel in zoo.hip)
constexpr int SURV_THREADS = 1024;
constexpr int CIDX_TILE = 256;          // rows per workgroup and j-tile length of the concordance counts
constexpr int CIDX_MAX_N = 1 << 20;

// pred = sigmoid(h) * range[0] + shift[0]; sigma kept for the backward.  range / shift are the module's parameters
// (device memory: the EMA update and load_state_dict change them like any other parameter).
__global__ void sigmoid_range_fwd_kernel(const float* __restrict__ h, const float* __restrict__ range,
                                         const float* __restrict__ shift, float* __restrict__ pred,
                                         float* __restrict__ sigma, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = 1.f / (1.f + expf(-h[i]));
  sigma[i] = s;
  pred[i] = s * range[0] + shift[0];
}

__global__ void sigmoid_range_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ sigma,
                                         const float* __restrict__ range, float* __restrict__ dh, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = sigma[i];
  dh[i] = dpred[i] * range[0] * s * (1.f - s);
}

// Addressing of the survival rows: quantity k (SURV_Q_* below, the order of the packed staging block) of global row i.
// SurvPtrRows: one device vector per quantity (ph_surv_stage1_loss_grad).  SurvGatheredRows: the all-gathered staging
// blocks [world][8][n], rank-blocked as the collective lands them (ph_surv_stage1_loss_grad_gathered): global row i is row
// i % n of rank i / n's block.
enum { SURV_Q_P0 = 0, SURV_Q_Q0 = 3, SURV_Q_T = 6, SURV_Q_C = 7, SURV_NQ = 8 };

struct SurvPtrRows {
  const float* q[SURV_NQ];
  __device__ __forceinline__ float operator()(int k, int i) const { return q[k][i]; }
};

struct SurvGatheredRows {
  const float* rows;
  int n;
  __device__ __forceinline__ float operator()(int k, int i) const {
    const int r = i / n;
    return rows[((size_t)r * SURV_NQ + k) * n + (i - r * n)];
  }
};

// One workgroup.  For each student prediction k (0 fuse, 1 path, 2 omic):
//   S_ki = sum_j [t_j >= t_i] exp(p_kj);  cox_k = -mean_i c_i (p_ki - log S_ki)           (utils.py:361-376)
//   d cox_k / d p_kl = -(c_l - exp(p_kl) sum_i c_i [t_l >= t_i] / S_ki) / B
// The three risk sums share one pass over t (LDS).  The per-prediction summation order is cox_kernel's, so each Cox
// term is bitwise the one ph_cox_loss_grad computes, and with nt = 0 each gradient row is lambda_cox times its dtheta
// (bitwise at lambda_cox = 1; tests/test_gpu_zoo_sweep.py).  KD terms: mse(a, b) = mean_i (a_i - b_i)^2 over the EMA
// teacher's predictions q (constants), combined as train_test_MT.py:180-201 for nt = 1 / 2 / 3 (nt = 0: off).
// The body is shared by both addressing forms: every sum runs over the B global rows in the same order whatever the
// addressing, so the gathered form is bitwise the form on the concatenated vectors.  dgrad [3][nout] receives the rows
// lo .. lo + nout - 1 (each row's gradient is computed on its own: the range changes no value).
template <class Rows>
__device__ __forceinline__ void surv_stage1_body(const Rows& rows, int B, int nt, float lambda_cox, float kd_weight,
                                                 float* __restrict__ terms, float* __restrict__ dgrad, int lo, int nout) {
  __shared__ float tt[SURV_MAX_B];
  __shared__ float ex[3][SURV_MAX_B];
  __shared__ float w[3][SURV_MAX_B];      // c_i / S_ki
  __shared__ float red[SURV_THREADS];
  const int tid = threadIdx.x;
  auto p = [&](int k, int i) { return rows(SURV_Q_P0 + k, i); };
  auto q = [&](int k, int i) { return rows(SURV_Q_Q0 + k, i); };
  for (int i = tid; i < B; i += SURV_THREADS) {
    tt[i] = rows(SURV_Q_T, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) ex[k][i] = expf(p(k, i));
  }
  __syncthreads();
  float l[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < B; i += SURV_THREADS) {
    float s[3] = {0.f, 0.f, 0.f};
    const float ti = tt[i];
    for (int j = 0; j < B; ++j) {
      const bool r = tt[j] >= ti;
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += r ? ex[k][j] : 0.f;
    }
    const float ci = rows(SURV_Q_C, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w[k][i] = ci / s[k];
      l[k] += (p(k, i) - logf(s[k])) * ci;
    }
  }
  float cox[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) cox[k] = -block_sum_tree(l[k], red) / (float)B;     // (block_sum_tree ends with a barrier: w is complete)
  // consistency terms; m[a][b] = mse(p_a, q_b) for the pairs the teacher count uses
  float kd[3] = {0.f, 0.f, 0.f};
  if (nt > 0) {
    float part[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) part[a][b] = 0.f;
    for (int i = tid; i < B; i += SURV_THREADS) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float d = p(a, i) - q(b, i);
          part[a][b] += d * d;
        }
    }
    float m[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) m[a][b] = 0.f;
    m[0][0] = block_sum_tree(part[0][0], red) / (float)B;
    m[1][1] = block_sum_tree(part[1][1], red) / (float)B;
    m[2][2] = block_sum_tree(part[2][2], red) / (float)B;
    if (nt >= 2) {
      m[1][0] = block_sum_tree(part[1][0], red) / (float)B;
      m[2][0] = block_sum_tree(part[2][0], red) / (float)B;
    }
    if (nt == 3) {
      m[1][2] = block_sum_tree(part[1][2], red) / (float)B;
      m[2][1] = block_sum_tree(part[2][1], red) / (float)B;
    }
    kd[0] = m[0][0];
    if (nt == 1) {
      kd[1] = m[1][1];
      kd[2] = m[2][2];
    } else if (nt == 2) {
      kd[1] = (m[1][1] + m[1][0]) / 2.f;
      kd[2] = (m[2][2] + m[2][0]) / 2.f;
    } else {
      kd[1] = (m[1][1] + m[1][0] + m[1][2]) / 3.f;
      kd[2] = (m[2][2] + m[2][0] + m[2][1]) / 3.f;
    }
  }
  if (tid == 0) {
    terms[0] = cox[0]; terms[1] = cox[1]; terms[2] = cox[2];
    terms[3] = kd[0]; terms[4] = kd[1]; terms[5] = kd[2];
    // train_test_MT.py:152 loss_cox = path + omic + fuse, :203 loss_pred_KD = KD_weight * (fuse + path + omic), :217
    const float lc = (cox[1] + cox[2]) + cox[0], lk = kd_weight * ((kd[0] + kd[1]) + kd[2]);
    terms[6] = lc;
    terms[7] = lk;
    terms[8] = lambda_cox * lc + lk;
  }
  if (!dgrad) return;
  const float inv_b = 1.f / (float)B;
  for (int lr = tid; lr < nout; lr += SURV_THREADS) {
    const int l0 = lo + lr;
    float a[3] = {0.f, 0.f, 0.f};
    const float tl = tt[l0];
    for (int i = 0; i < B; ++i) {
      const bool r = tl >= tt[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] += r ? w[k][i] : 0.f;
    }
    const float cl = rows(SURV_Q_C, l0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float g = lambda_cox * (-(cl - ex[k][l0] * a[k]) * inv_b);
      if (nt > 0) {
        const float pk = p(k, l0);
        float dk;
        if (k == 0 || nt == 1) {
          dk = 2.f * (pk - q(k, l0)) * inv_b;
        } else {
          const int o = 3 - k;      // the other modality's teacher
          float s = (pk - q(k, l0)) + (pk - q(0, l0));
          if (nt == 3) s += pk - q(o, l0);
          dk = 2.f * s * inv_b / (float)nt;
        }
        g += kd_weight * dk;
      }
      dgrad[(size_t)k * nout + lr] = g;
    }
  }
}

__global__ __launch_bounds__(SURV_THREADS) void surv_stage1_kernel(
    const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ p2, const float* __restrict__ q0,
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ t, const float* __restrict__ c,
    int B, int nt, float lambda_cox, float kd_weight, float* __restrict__ terms, float* __restrict__ dgrad) {
  const SurvPtrRows rows = {{p0, p1, p2, q0, q1, q2, t, c}};
  surv_stage1_body(rows, B, nt, lambda_cox, kd_weight, terms, dgrad, 0, B);
}

// The same over the all-gathered staging blocks [world][8][n] (B = world * n); dgrad [3][n] = this rank's rows.
__global__ __launch_bounds__(SURV_THREADS) void surv_stage1_gathered_kernel(const float* __restrict__ gathered, int world,
                                                                            int n, int rank, int nt, float lambda_cox,
                                                                            float kd_weight, float* __restrict__ terms,
                                                                            float* __restrict__ dgrad) {
  const SurvGatheredRows rows = {gathered, n};
  surv_stage1_body(rows, world * n, nt, lambda_cox, kd_weight, terms, dgrad, rank * n, n);
}

// This replica's survival rows into one staging block [8][n] (quantity-major, SURV_Q_* order), the one buffer the
// all-gather carries.  nt = 0: the three teacher rows are written as zeros (their pointers may be NULL).
__global__ void surv_pack_rows_kernel(const float* __restrict__ p0, const float* __restrict__ p1,
                                      const float* __restrict__ p2, const float* __restrict__ q0,
                                      const float* __restrict__ q1, const float* __restrict__ q2,
                                      const float* __restrict__ t, const float* __restrict__ c, int n, int nt,
                                      float* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= n) return;
  const float* src = k == 0 ? p0 : k == 1 ? p1 : k == 2 ? p2 : k == 3 ? q0 : k == 4 ? q1 : k == 5 ? q2 : k == 6 ? t : c;
  const bool zero = nt == 0 && k >= SURV_Q_Q0 && k < SURV_Q_T;
  rows[(size_t)k * n + i] = zero ? 0.f : src[i];
}

// ema = hyper[3] * ema + hyper[4] * p over parameters the optimiser does not update (requires_grad False: output_range /
// output_shift), with the EMA rate the fused Adam step reads (update_ema_variables, train_test_MT.py:34-38, loops over
// every parameter)
__global__ void ema_update_dev_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n,
                                      const float* __restrict__ hyper) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ema[i] = hyper[3] * ema[i] + hyper[4] * p[i];
}

// Concordance counts (lifelines' concordance_index(t, -h, e) rule).  Pair (i, j) is comparable iff e_i = 1 and
// (t_i < t_j, or t_i == t_j and e_j = 0); concordant iff h_i > h_j; tied iff h_i == h_j.  Thread = row i, the j rows
// stream through LDS in tiles.  Integer counts, added with 64-bit integer atomics: exact, so the result does not depend
// on the order of the rows or of the additions.  counts[v*3 + {0,1,2}] = comparable, concordant, tied.
// A time past the end is staged as a NaN: it is comparable with nothing, as is a NaN time among the rows.
struct CidxStage {
  float t, e, h[3];
};

__global__ __launch_bounds__(CIDX_TILE) void cindex_counts_kernel(const float* __restrict__ t, const float* __restrict__ e,
                                                                  const float* __restrict__ h0, const float* __restrict__ h1,
                                                                  const float* __restrict__ h2, int nvec, int N,
                                                                  unsigned long long* __restrict__ counts) {
  __shared__ float st[CIDX_TILE], se[CIDX_TILE], sh[3][CIDX_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * CIDX_TILE + tid;
  const float* hv[3] = {h0, h1, h2};
  const bool live = i < N;
  const float ti = live ? t[i] : 0.f;
  const bool ev = live && e[i] > 0.5f;
  float hi[3] = {0.f, 0.f, 0.f};
  for (int v = 0; v < nvec; ++v) hi[v] = live ? hv[v][i] : 0.f;
  unsigned int comp = 0, conc[3] = {0u, 0u, 0u}, tie[3] = {0u, 0u, 0u};
  pair_scan<CIDX_TILE>(
      N, i, ev,
      [&](int j) {
        CidxStage s = {__builtin_nanf(""), 0.f, {0.f, 0.f, 0.f}};
        if (j < N) {
          s.t = t[j];
          s.e = e[j];
#pragma unroll                   // (constant indices: the staged values stay in registers)
          for (int v = 0; v < 3; ++v)
            if (v < nvec) s.h[v] = hv[v][j];
        }
        return s;
      },
      [&](int k, const CidxStage& s) {
        st[k] = s.t;
        se[k] = s.e;
#pragma unroll
        for (int v = 0; v < 3; ++v) sh[v][k] = s.h[v];
      },
      [&](int jj, int) {
        const float tj = st[jj];
        const bool cmp = ti < tj || (ti == tj && se[jj] <= 0.5f);
        if (!cmp) return;
        ++comp;
        for (int v = 0; v < nvec; ++v) {
          const float hj = sh[v][jj];
          conc[v] += hi[v] > hj;
          tie[v] += hi[v] == hj;
        }
      });
  for (int v = 0; v < nvec; ++v) {
    wave_atomic_add(&counts[v * 3 + 0], comp);
    wave_atomic_add(&counts[v * 3 + 1], conc[v]);
    wave_atomic_add(&counts[v * 3 + 2], tie[v]);
  }
}

}  // namespace

#include "pathomic_hip.h"

extern "C" {

int ph_sigmoid_range_fwd(const float* hazard, const float* range, const float* shift, float* pred, float* sigma, int n,
                         hipStream_t st) {
  if (!hazard || !range || !shift || !pred || !sigma || n < 1) return PH_EINVAL;
  hipLaunchKernelGGL(sigmoid_range_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, hazard, range, shift, pred, sigma, n);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_sigmoid_range_bwd(const float* dpred, const float* sigma, const float* range, float* dhazard, int n, hipStream_t st) {
  if (!dpred || !sigma || !range || !dhazard || n < 1) return PH_EINVAL;
  hipLaunchKernelGGL(sigmoid_range_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dpred, sigma, range, dhazard, n);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_ema_update_dev(float* ema, const float* p, size_t n, const float* hyper, hipStream_t st) {
  if (!ema || !p || !hyper) return PH_EINVAL;
  if (n == 0) return PH_OK;
  hipLaunchKernelGGL(ema_update_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ema, p, n, hyper);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_surv_stage1_loss_grad(const float* pred, const float* pred_path, const float* pred_omic, const float* ema_pred,
                             const float* ema_pred_path, const float* ema_pred_omic, const float* survtime,
                             const float* censor, int B, int num_teachers, float lambda_cox, float kd_weight, float* terms,
                             float* dgrad, hipStream_t st) {
  if (!pred || !pred_path || !pred_omic || !survtime || !censor || !terms || B < 1 || B > SURV_MAX_B) return PH_EINVAL;
  if (num_teachers < 0 || num_teachers > 3) return PH_EINVAL;
  if (num_teachers > 0 && (!ema_pred || !ema_pred_path || !ema_pred_omic)) return PH_EINVAL;
  hipLaunchKernelGGL(surv_stage1_kernel, dim3(1), dim3(SURV_THREADS), 0, st, pred, pred_path, pred_omic, ema_pred,
                     ema_pred_path, ema_pred_omic, survtime, censor, B, num_teachers, lambda_cox, kd_weight, terms, dgrad);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_surv_pack_rows(const float* pred, const float* pred_path, const float* pred_omic, const float* ema_pred,
                      const float* ema_pred_path, const float* ema_pred_omic, const float* survtime, const float* censor, int n,
                      int num_teachers, float* rows, hipStream_t st) {
  if (!pred || !pred_path || !pred_omic || !survtime || !censor || !rows || n < 1 || n > SURV_MAX_B) return PH_EINVAL;
  if (num_teachers < 0 || num_teachers > 3) return PH_EINVAL;
  if (num_teachers > 0 && (!ema_pred || !ema_pred_path || !ema_pred_omic)) return PH_EINVAL;
  hipLaunchKernelGGL(surv_pack_rows_kernel, dim3((n + 255) / 256, SURV_NQ), dim3(256), 0, st, pred, pred_path, pred_omic,
                     ema_pred, ema_pred_path, ema_pred_omic, survtime, censor, n, num_teachers, rows);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_surv_stage1_loss_grad_gathered(const float* rows, int world, int n, int rank, int num_teachers, float lambda_cox,
                                      float kd_weight, float* terms, float* dgrad_local, hipStream_t st) {
  if (!rows || !terms || world < 1 || n < 1 || rank < 0 || rank >= world) return PH_EINVAL;
  if ((int64_t)world * n > SURV_MAX_B || num_teachers < 0 || num_teachers > 3) return PH_EINVAL;
  hipLaunchKernelGGL(surv_stage1_gathered_kernel, dim3(1), dim3(SURV_THREADS), 0, st, rows, world, n, rank, num_teachers,
                     lambda_cox, kd_weight, terms, dgrad_local);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_cindex_counts(const float* survtime, const float* event, const float* h0, const float* h1, const float* h2, int nvec,
                     int N, int64_t* counts, hipStream_t st) {
  if (!survtime || !event || !h0 || !counts || nvec < 1 || nvec > 3 || N < 2 || N > CIDX_MAX_N) return PH_EINVAL;
  if ((nvec > 1 && !h1) || (nvec > 2 && !h2)) return PH_EINVAL;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * nvec, st) != hipSuccess) return PH_ELAUNCH;
  hipLaunchKernelGGL(cindex_counts_kernel, dim3((N + CIDX_TILE - 1) / CIDX_TILE), dim3(CIDX_TILE), 0, st, survtime, event,
                     h0, h1, h2, nvec, N, reinterpret_cast<unsigned long long*>(counts));
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"

// What the stage-2 trainers' train() keeps between the batch body and the test pass - on the host
// there, through seven or more .item() / .cpu() reads per step (MICCAI-2022 train_test_path_multi_distill.py:305, :317-324,
// :340; "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":300-304, :338-342, :380-383):
//   ph_epoch_record_add  one capturable launch per step that adds the step's device scalars, the GK-Refine weight vector, the
//                        count of correct predictions and the mean query weights into a persistent record of float64 sums and
//                        int64 counts; read once per epoch,
//   ph_stage1_record_add the same for the stage-1 teacher step: the scalars, the correct counts of up to
//                        three heads, and under survival the step's five per-sample columns appended to a device store at a
//                        cursor that lives in the record,
//   ph_store_rows        `store[index] = rows` (optionally softmax(rows, 1)) of the MIA-2023 per-sample stores,
//   ph_sim_audit         evaluate_feature / evaluate_logits (:162-196) over two stores without an n x n matrix: both cosine
//                        Gram tiles by exact-f32 MFMA 32x32x2 (the tiles of zoo_rkd.hip), class test and sums in the epilogue.
// No float atomics anywhere: every float64 sum has a fixed order, two runs give the same bits.
#include "ph_common.h"
#include "ph_reduce.h"
#include "pathomic_hip.h"

namespace {

typedef float er_f16 __attribute__((ext_vector_type(16)));

constexpr int ER_THREADS = 256;
constexpr int ER_MAX_SCALARS = PH_EPOCHREC_MAX_SCALARS;
constexpr int ER_MAX_B = 1 << 20;
constexpr int ER_MAX_C = 16;
constexpr int S1_MAX_B = 1 << 16;     // rows of one ph_stage1_record_add call (three 20-bit counts share a word)
constexpr int S1_MAX_CAP = 1 << 20;   // columns of the survival store: the range of ph_cindex_counts
constexpr int SR_MAX_B = 1 << 16;
constexpr int SR_MAX_D = 4096;
constexpr int SA_T = 64;            // rows of an i / j tile
constexpr int SA_LD = 33;           // LDS row stride of the 32-column operand tiles (odd: the MFMA operand reads of 32 rows
                                    // at one column hit 32 different banks)
constexpr int SA_MAX_N = 65536;
constexpr int SA_MAX_D = 512;
constexpr int SA_MAX_SPLIT = 16;    // j-tile ranges per i tile (workgroups = tiles x split)

struct ErScalars {
  const float* p[ER_MAX_SCALARS];
  int mode[ER_MAX_SCALARS];
};

// The scalar rule of both records, one copy: thread k < ns reads scalar k, widens it to float64 and adds it to sums[k]; added[k]
// counts the additions.  PH_REC_ADD: a NaN propagates; PH_REC_ADD_POSITIVE: `if v > 0.0: acc += v` - false for 0.0, -0.0,
// negatives and a NaN.
__device__ __forceinline__ void rec_add_scalars(double* sums, long long* added, const ErScalars& sc, int ns, int tid) {
  if (tid < ns) {
    const float v = *sc.p[tid];
    if (sc.mode[tid] == PH_REC_ADD || v > 0.0f) { sums[tid] += (double)v; added[tid] += 1; }
  }
}

// The FIRST maximum of a row of C values (a strict `>` scan from column 0, as ph_confusion_counts; a NaN never wins).
__device__ __forceinline__ int first_argmax(const float* __restrict__ row, int C) {
  float best = row[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = row[c];
    if (v > best) { best = v; arg = c; }
  }
  return arg;
}

// One workgroup.  Record words (8 bytes each): [0, 16) scalar sums, [16, 32) weight-vector sums, [32, 34) sums of the row
// means (float64); [34] correct, [35] bad labels, [36] steps, [37] rows seen (int64); [38, 40) spare; [40, 56) additions per
// scalar (int64).
__global__ __launch_bounds__(ER_THREADS) void epoch_record_add_kernel(double* rec, ErScalars sc, int ns,
                                                                      const float* __restrict__ wvec, int nw,
                                                                      const float* __restrict__ pred,
                                                                      const int64_t* __restrict__ grade, int B, int C,
                                                                      const float* __restrict__ row0,
                                                                      const float* __restrict__ row1, int nrow) {
  __shared__ double redd[ER_THREADS];
  __shared__ unsigned long long redu[ER_THREADS];
  const int tid = threadIdx.x;
  long long* reci = reinterpret_cast<long long*>(rec);
  rec_add_scalars(rec, reci + 40, sc, ns, tid);
  if (tid >= 64 && tid < 64 + nw) rec[16 + tid - 64] += (double)wvec[tid - 64];
  if (pred) {                                   // (uniform over the workgroup: the trees below contain barriers)
    unsigned long long ok = 0, bad = 0;
    for (int n = tid; n < B; n += ER_THREADS) {
      const int arg = first_argmax(pred + (size_t)n * C, C);
      const int64_t g = grade[n];
      if (g < 0 || g >= (int64_t)C) ++bad; else if (g == (int64_t)arg) ++ok;
    }
    // both counts in one tree: bad in the high half (B <= 2^20 rows)
    const unsigned long long t = block_sum_tree<ER_THREADS>(ok | (bad << 32), redu);
    if (tid == 0) {
      reci[34] += (long long)(t & 0xffffffffull);
      reci[35] += (long long)(t >> 32);
      reci[37] += B;
    }
  }
  for (int k = 0; k < 2; ++k) {
    const float* __restrict__ row = k ? row1 : row0;
    if (!row) continue;
    double s = 0.0;                              // element t, t + 256, .. per thread, then the tree: a fixed order
    for (int n = tid; n < nrow; n += ER_THREADS) s += (double)row[n];
    s = block_sum_tree<ER_THREADS>(s, redd);
    if (tid == 0) rec[32 + k] += s / (double)nrow;
  }
  if (tid == 0) reci[36] += 1;
}

struct S1Heads { const float* p[3]; };
struct S1Cols { const float* p[5]; };

// One workgroup (a step's rows are few, and a single workgroup needs no ordering between blocks: every thread reads the cursor,
// a barrier follows, and only then does thread 0 advance it).  Record words (8 bytes each): [0, 16) scalar sums (float64);
// [16, 32) additions per scalar; [32, 35) correct rows of head 0 / 1 / 2; [35] bad labels; [36] steps; [37] rows seen;
// [38] the store cursor = rows appended so far; [39] overflow = rows dropped because the store was full (int64); [40, 48) spare.
__global__ __launch_bounds__(ER_THREADS) void stage1_record_add_kernel(double* rec, ErScalars sc, int ns, S1Heads hd, int nh,
                                                                       const int64_t* __restrict__ grade, int B, int C,
                                                                       S1Cols cols, float* __restrict__ store, int cap) {
  __shared__ unsigned long long redu[ER_THREADS];
  const int tid = threadIdx.x;
  long long* reci = reinterpret_cast<long long*>(rec);
  const long long cur = reci[38];               // read by every thread BEFORE the barrier, written by thread 0 after it
  __syncthreads();
  rec_add_scalars(rec, reci + 16, sc, ns, tid);
  if (nh > 0) {                                 // (uniform over the workgroup: the trees below contain barriers)
    unsigned long long ok = 0, bad = 0;         // three 20-bit fields: B <= 65536 rows per call
    for (int n = tid; n < B; n += ER_THREADS) {
      const int64_t g = grade[n];
      if (g < 0 || g >= (int64_t)C) { ++bad; continue; }          // once, whatever the number of heads
      for (int h = 0; h < nh; ++h)
        if ((int64_t)first_argmax(hd.p[h] + (size_t)n * C, C) == g) ok += 1ull << (20 * h);
    }
    const unsigned long long t = block_sum_tree<ER_THREADS>(ok, redu), tb = block_sum_tree<ER_THREADS>(bad, redu);
    if (tid == 0) {
      for (int h = 0; h < nh; ++h) reci[32 + h] += (long long)((t >> (20 * h)) & 0xfffffull);
      reci[35] += (long long)tb;
    }
  }
  if (store) {
    // rows [0, fit) of the step land at [cur, cur + fit); nothing is written at or past cap, whatever the cursor holds
    const long long room = (cur >= 0 && cur < (long long)cap) ? (long long)cap - cur : 0;
    const int fit = room < (long long)B ? (int)room : B;
    for (int n = tid; n < fit; n += ER_THREADS) {
#pragma unroll
      for (int k = 0; k < 5; ++k) store[(size_t)k * cap + (size_t)(cur + n)] = cols.p[k][n];
    }
    if (tid == 0) { reci[38] = cur + fit; reci[39] += B - fit; }
  }
  if (tid == 0) {
    if (nh > 0 || store) reci[37] += B;
    reci[36] += 1;
  }
}

// One wave per source row b.  The row is written unless its index is out of range (counted) or a LATER row of the batch
// carries the same index (numpy's a[index] = rows keeps the last writer).
__global__ __launch_bounds__(64) void store_rows_kernel(const float* __restrict__ rows, const int64_t* __restrict__ index,
                                                        int B, int D, float* __restrict__ store, int64_t n, int softmax,
                                                        unsigned long long* __restrict__ skipped) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t idx = index[b];
  if (idx < 0 || idx >= n) {
    if (lane == 0) atomicAdd(skipped, 1ull);     // (an integer total: exact in any order)
    return;
  }
  int later = 0;
  for (int q = b + 1 + lane; q < B; q += 64) later |= (index[q] == idx) ? 1 : 0;
  if (__any(later)) return;
  const float* __restrict__ src = rows + (size_t)b * D;
  float* __restrict__ dst = store + (size_t)idx * D;
  if (!softmax) {
    for (int d = lane; d < D; d += 64) dst[d] = src[d];
    return;
  }
  float mx = -INFINITY;
  for (int d = lane; d < D; d += 64) mx = fmaxf(mx, src[d]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += expf(src[d] - mx);
  s = wave_sum(s);
  for (int d = lane; d < D; d += 64) dst[d] = expf(src[d] - mx) / s;
}

// 1 / |row| of both stores, the squares summed in float64 (element t, t + 64, .. per lane, then the xor tree); 0 for a zero
// row (sklearn's normalize leaves it zero: similarity 0 with everything).  One wave per row.
__global__ __launch_bounds__(64) void sim_invnorm_kernel(const float* __restrict__ F, const float* __restrict__ P, int n, int Df,
                                                         int Dp, float* __restrict__ invF, float* __restrict__ invP) {
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int side = 0; side < 2; ++side) {
    const float* __restrict__ x = (side ? P : F) + (size_t)r * (side ? Dp : Df);
    const int D = side ? Dp : Df;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) { const double v = (double)x[d]; s += v * v; }
    s = wave_sum_d(s);
    if (lane == 0) (side ? invP : invF)[r] = s > 0.0 ? (float)(1.0 / sqrt(s)) : 0.f;
  }
}

// Workgroup (bx, by): the 64 rows i of tile bx against the j tiles by, by + gridDim.y, ..  Per j tile both Gram tiles
// S = X^ X^T (X^ the rows scaled by 1 / |row| as they are staged), D in zero-padded chunks of 32; wave w owns the 32 x 32
// quadrant (w & 1, w >> 1).  Epilogue per accumulator element: the class test and the five float64 sums, per lane over its
// elements and tiles in order, then one tree per sum.  part[(bx * gridDim.y + by) * 8 + k]: k = 0 teacher intra,
// 1 teacher inter, 2 student intra, 3 student inter, 4 sum |S_f - S_p| (float64); 5 intra pairs, 6 inter pairs (uint64).
__global__ __launch_bounds__(ER_THREADS) void sim_audit_kernel(const float* __restrict__ F, const float* __restrict__ P,
                                                               const int64_t* __restrict__ labels,
                                                               const float* __restrict__ invF, const float* __restrict__ invP,
                                                               int n, int Df, int Dp, double* __restrict__ part) {
  __shared__ float Ei[SA_T * SA_LD], Ej[SA_T * SA_LD];
  __shared__ float inv_i[2][SA_T], inv_j[2][SA_T];
  __shared__ long long lab_i[SA_T], lab_j[SA_T];
  __shared__ double redd[ER_THREADS];
  __shared__ unsigned long long redu[ER_THREADS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, kk = lane >> 5;
  const int i0 = blockIdx.x * SA_T, ntiles = (n + SA_T - 1) / SA_T;
  const int ri = (wave & 1) * 32, rj = (wave >> 1) * 32;
  if (tid < SA_T) {
    const int i = i0 + tid;
    inv_i[0][tid] = i < n ? invF[i] : 0.f;
    inv_i[1][tid] = i < n ? invP[i] : 0.f;
    lab_i[tid] = (labels && i < n) ? (long long)labels[i] : 0;
  }
  double s_ti = 0.0, s_to = 0.0, s_si = 0.0, s_so = 0.0, s_ad = 0.0;
  unsigned long long c_in = 0, c_out = 0;
  for (int jt = blockIdx.y; jt < ntiles; jt += gridDim.y) {
    const int j0 = jt * SA_T;
    __syncthreads();            // the previous tile's readers of inv_j / lab_j and of the operand tiles are done
    if (tid < SA_T) {
      const int j = j0 + tid;
      inv_j[0][tid] = j < n ? invF[j] : 0.f;
      inv_j[1][tid] = j < n ? invP[j] : 0.f;
      lab_j[tid] = (labels && j < n) ? (long long)labels[j] : 0;
    }
    er_f16 acc[2];
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const float* __restrict__ X = side ? P : F;
      const int D = side ? Dp : Df, nc = (D + 31) >> 5;
      er_f16 a;
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = 0.f;
      for (int c = 0; c < nc; ++c) {
        float vi[8], vj[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int e = tid + 256 * q, row = e >> 5, d = c * 32 + (e & 31), i = i0 + row, j = j0 + row;
          vi[q] = (i < n && d < D) ? X[(size_t)i * D + d] : 0.f;
          vj[q] = (j < n && d < D) ? X[(size_t)j * D + d] : 0.f;
        }
        __syncthreads();        // inv_j written (first chunk); the previous chunk's operand reads are done
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int e = tid + 256 * q, row = e >> 5, o = row * SA_LD + (e & 31);
          Ei[o] = vi[q] * inv_i[side][row];
          Ej[o] = vj[q] * inv_j[side][row];
        }
        __syncthreads();
#pragma unroll
        for (int dd = 0; dd < 32; dd += 2)
          a = __builtin_amdgcn_mfma_f32_32x32x2f32(Ei[(ri + l32) * SA_LD + dd + kk], Ej[(rj + l32) * SA_LD + dd + kk], a, 0, 0, 0);
      }
      acc[side] = a;
    }
    // accumulator element r of a lane: row (r & 3) + 8 (r >> 2) + 4 kk of the quadrant, column l32
    const int jl = rj + l32, j = j0 + jl;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = ri + (r & 3) + 8 * (r >> 2) + 4 * kk, i = i0 + il;
      if (i < n && j < n) {
        const float sf = acc[0][r], sp = acc[1][r];
        const double df = (double)sf, dp = (double)sp;
        if (lab_i[il] == lab_j[jl]) { s_ti += df; s_si += dp; ++c_in; } else { s_to += df; s_so += dp; ++c_out; }
        s_ad += (double)fabsf(sf - sp);
      }
    }
  }
  double* out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 8;
  const double t0 = block_sum_tree<ER_THREADS>(s_ti, redd), t1 = block_sum_tree<ER_THREADS>(s_to, redd);
  const double t2 = block_sum_tree<ER_THREADS>(s_si, redd), t3 = block_sum_tree<ER_THREADS>(s_so, redd);
  const double t4 = block_sum_tree<ER_THREADS>(s_ad, redd);
  const unsigned long long u0 = block_sum_tree<ER_THREADS>(c_in, redu), u1 = block_sum_tree<ER_THREADS>(c_out, redu);
  if (tid == 0) {
    out[0] = t0; out[1] = t1; out[2] = t2; out[3] = t3; out[4] = t4;
    reinterpret_cast<unsigned long long*>(out)[5] = u0;
    reinterpret_cast<unsigned long long*>(out)[6] = u1;
    out[7] = 0.0;
  }
}

// One workgroup: partial t, t + 256, .. per thread in that order, then the tree.
__global__ __launch_bounds__(ER_THREADS) void sim_audit_finish_kernel(const double* __restrict__ part, int nparts,
                                                                      double* __restrict__ sums, int64_t* __restrict__ counts) {
  __shared__ double redd[ER_THREADS];
  __shared__ unsigned long long redu[ER_THREADS];
  const int tid = threadIdx.x;
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int p = tid; p < nparts; p += ER_THREADS) s += part[(size_t)p * 8 + k];
    s = block_sum_tree<ER_THREADS>(s, redd);
    if (tid == 0) sums[k] = s;
  }
  for (int k = 0; k < 2; ++k) {
    unsigned long long s = 0;
    for (int p = tid; p < nparts; p += ER_THREADS) s += reinterpret_cast<const unsigned long long*>(part)[(size_t)p * 8 + 5 + k];
    s = block_sum_tree<ER_THREADS>(s, redu);
    if (tid == 0) counts[k] = (int64_t)s;
  }
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool sim_shape_ok(int n, int Df, int Dp) {
  return n >= 1 && n <= SA_MAX_N && Df >= 1 && Df <= SA_MAX_D && Dp >= 1 && Dp <= SA_MAX_D;
}
inline int sim_split(int ntiles) { return ntiles < SA_MAX_SPLIT ? ntiles : SA_MAX_SPLIT; }
inline size_t sim_part_bytes(int n) {
  const int ntiles = cdiv(n, SA_T);
  return sizeof(double) * 8 * (size_t)ntiles * (size_t)sim_split(ntiles);
}
inline size_t sim_inv_bytes(int n) { return ((sizeof(float) * (size_t)n + 255) / 256) * 256; }

}  // namespace

extern "C" {

int ph_epoch_record_add(void* record, const float* const* scalars, const int32_t* modes, int n_scalars, const float* wvec,
                        int n_w, const float* pred, const int64_t* grade, int B, int C, const float* row0, const float* row1,
                        int n_row, hipStream_t st) {
  static_assert(PH_EPOCHREC_WORDS >= 56 && PH_EPOCHREC_MAX_SCALARS == 16, "the header's record is the kernel's");
  if (!record || !aligned(record, 8)) return PH_EINVAL;
  if (n_scalars < 0 || n_scalars > ER_MAX_SCALARS || n_w < 0 || n_w > ER_MAX_SCALARS) return PH_EINVAL;
  if (n_scalars > 0 && (!scalars || !modes)) return PH_EINVAL;
  if (n_w > 0 && (!wvec || !aligned(wvec, 4))) return PH_EINVAL;
  if ((pred == nullptr) != (grade == nullptr)) return PH_EINVAL;
  if (pred && (B < 1 || B > ER_MAX_B || C < 1 || C > ER_MAX_C || !aligned(pred, 4) || !aligned(grade, 8))) return PH_EINVAL;
  if (row1 && !row0) return PH_EINVAL;
  if (row0 && (n_row < 1 || n_row > ER_MAX_B || !aligned(row0, 4) || !aligned(row1, 4))) return PH_EINVAL;
  if (n_scalars == 0 && n_w == 0 && !pred && !row0) return PH_EINVAL;       // nothing to add
  ErScalars sc;
  for (int k = 0; k < ER_MAX_SCALARS; ++k) { sc.p[k] = nullptr; sc.mode[k] = 0; }
  for (int k = 0; k < n_scalars; ++k) {
    if (!scalars[k] || !aligned(scalars[k], 4) || (modes[k] != PH_REC_ADD && modes[k] != PH_REC_ADD_POSITIVE)) return PH_EINVAL;
    sc.p[k] = scalars[k]; sc.mode[k] = modes[k];
  }
  hipLaunchKernelGGL(epoch_record_add_kernel, dim3(1), dim3(ER_THREADS), 0, st, static_cast<double*>(record), sc, n_scalars,
                     wvec, n_w, pred, grade, B, C, row0, row1, n_row);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_stage1_record_add(void* record, const float* const* scalars, const int32_t* modes, int n_scalars, const float* pred0,
                         const float* pred1, const float* pred2, int n_heads, const int64_t* grade, int B, int C,
                         const float* h_fuse, const float* h_path, const float* h_omic, const float* censor,
                         const float* survtime, float* store, int cap, hipStream_t st) {
  static_assert(PH_STAGE1REC_WORDS >= 40, "the header's record is the kernel's");
  if (!record || !aligned(record, 8)) return PH_EINVAL;
  if (n_scalars < 0 || n_scalars > ER_MAX_SCALARS || n_heads < 0 || n_heads > 3) return PH_EINVAL;
  if (n_scalars > 0 && (!scalars || !modes)) return PH_EINVAL;
  const float* heads[3] = {pred0, pred1, pred2};
  for (int h = 0; h < 3; ++h)                                              // exactly the first n_heads are given
    if ((heads[h] != nullptr) != (h < n_heads) || !aligned(heads[h], 4)) return PH_EINVAL;
  if ((grade != nullptr) != (n_heads > 0) || !aligned(grade, 8)) return PH_EINVAL;
  const void* surv[6] = {h_fuse, h_path, h_omic, censor, survtime, store};
  int given = 0;
  for (int k = 0; k < 6; ++k) {
    if (surv[k]) ++given;
    if (!aligned(surv[k], 4)) return PH_EINVAL;
  }
  if (given != 0 && given != 6) return PH_EINVAL;                          // all of them, or none
  if ((n_heads > 0 || given) && (B < 1 || B > S1_MAX_B)) return PH_EINVAL;
  if (n_heads > 0 && (C < 1 || C > ER_MAX_C)) return PH_EINVAL;
  if (given && (cap < 1 || cap > S1_MAX_CAP)) return PH_EINVAL;
  if (n_scalars == 0 && n_heads == 0 && !given) return PH_EINVAL;          // nothing to add
  ErScalars sc;
  for (int k = 0; k < ER_MAX_SCALARS; ++k) { sc.p[k] = nullptr; sc.mode[k] = 0; }
  for (int k = 0; k < n_scalars; ++k) {
    if (!scalars[k] || !aligned(scalars[k], 4) || (modes[k] != PH_REC_ADD && modes[k] != PH_REC_ADD_POSITIVE)) return PH_EINVAL;
    sc.p[k] = scalars[k]; sc.mode[k] = modes[k];
  }
  S1Heads hd{{pred0, pred1, pred2}};
  S1Cols cols{{h_fuse, h_path, h_omic, censor, survtime}};
  hipLaunchKernelGGL(stage1_record_add_kernel, dim3(1), dim3(ER_THREADS), 0, st, static_cast<double*>(record), sc, n_scalars, hd,
                     n_heads, grade, B, C, cols, store, cap);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_store_rows(const float* rows, const int64_t* index, int B, int D, float* store, int64_t n, int softmax,
                  int64_t* skipped, hipStream_t st) {
  if (!rows || !index || !store || !skipped) return PH_EINVAL;
  if (!aligned(rows, 4) || !aligned(store, 4) || !aligned(index, 8) || !aligned(skipped, 8)) return PH_EINVAL;
  if (B < 1 || B > SR_MAX_B || D < 1 || D > SR_MAX_D || n < 1 || n > ((int64_t)1 << 31) || (softmax != 0 && softmax != 1))
    return PH_EINVAL;
  hipLaunchKernelGGL(store_rows_kernel, dim3(B), dim3(64), 0, st, rows, index, B, D, store, n, softmax,
                     reinterpret_cast<unsigned long long*>(skipped));
  PH_LAUNCH_CHECK();
  return PH_OK;
}

size_t ph_sim_audit_workspace_bytes(int n, int Df, int Dp) {
  if (!sim_shape_ok(n, Df, Dp)) return 0;
  return 2 * sim_inv_bytes(n) + sim_part_bytes(n);
}

int ph_sim_audit(const float* F, const float* P, const int64_t* labels, int n, int Df, int Dp, double* sums, int64_t* counts,
                 void* workspace, hipStream_t st) {
  if (!F || !P || !sums || !counts || !workspace || !sim_shape_ok(n, Df, Dp)) return PH_EINVAL;
  if (!aligned(F, 4) || !aligned(P, 4) || !aligned(labels, 8) || !aligned(sums, 8) || !aligned(counts, 8) ||
      !aligned(workspace, 256))
    return PH_EINVAL;
  const int ntiles = cdiv(n, SA_T), split = sim_split(ntiles);
  char* ws = static_cast<char*>(workspace);
  float* invF = reinterpret_cast<float*>(ws);
  float* invP = reinterpret_cast<float*>(ws + sim_inv_bytes(n));
  double* part = reinterpret_cast<double*>(ws + 2 * sim_inv_bytes(n));
  if (hipMemsetAsync(sums, 0, sizeof(double) * 5, st) != hipSuccess) return PH_ELAUNCH;
  hipLaunchKernelGGL(sim_invnorm_kernel, dim3(n), dim3(64), 0, st, F, P, n, Df, Dp, invF, invP);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(sim_audit_kernel, dim3(ntiles, split), dim3(ER_THREADS), 0, st, F, P, labels, invF, invP, n, Df, Dp, part);
  PH_LAUNCH_CHECK();
  hipLaunchKernelGGL(sim_audit_finish_kernel, dim3(1), dim3(ER_THREADS), 0, st, part, ntiles * split, sums, counts);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

}  // extern "C"

// Weight packing: OIHW fp32 -> the layouts the convolution kernels read.  Every packer and its launcher lives
// here.  One table kernel per arithmetic packs a whole network (PhPackAll, both orientations of every unit) or, as a one-entry table
// in its one-orientation form, a single convolution.  The layout of every unit is the host's decision (PhPackAll::frag): the device
// code tests the flag and holds no shape rule.
#include <iterator>
#include "ph_common.h"
#include "ph_kernels.h"

namespace {

// first tile (32 output x 32 input channels, all taps: one workgroup) of every table entry
struct PackTiles { int tstart[21]; };

// fragment-major order of a 64 x 64 (row, k) block for the register-window kernels (conv_tap5/6/6b/7.hip): [k-step 2][N tile 4][lane 64][8]:
// row r = 4 li + n, k = 32 ks + 8 lg + j, lane = 16 lg + li -> element ((ks * 4 + n) * 64 + lane) * 8 + j of the block's 4096
__device__ __forceinline__ size_t frag64_index(int r, int k) {
  return (size_t)(((k >> 5) * 4 + (r & 3)) * 512 + ((((k >> 3) & 3) << 4) + (r >> 2)) * 8 + (k & 7));
}
// ... of element (r, k) of a [rows][K] matrix cut into such blocks, [rows / 64][K / 64] x 4096 elements
__device__ __forceinline__ size_t frag64_tiled(int r, int k, int K) {
  return (size_t)((r >> 6) * (K >> 6) + (k >> 6)) * 4096 + frag64_index(r & 63, k & 63);
}

enum { PACK_BOTH = 0, PACK_FWD = 1, PACK_DGRAD = 2 };

// Tiled through LDS: one workgroup per (conv, 32 output channels, 32 input channels), all taps.  The OIHW rows are read as contiguous
// runs of 32*NT floats and both layouts leave as 64-byte runs (an element-per-thread pack writes the dgrad layout [tap][I][O] as
// 2-byte words scattered with a stride of O elements: 110 us for the 11 M weights of a ResNet-18, twice per step).
// NP planes: 1 = bf16 rounding (perf mode), 3 = the split planes.  ORI: both orientations of a network's units, or the one a single
// convolution is about to read (then at dst_fwd / dst_dg alike: the head of its workspace).
template <int NP, int ORI = PACK_BOTH>
__global__ __launch_bounds__(256) void pack_all_tiled_kernel(PhPackAll t, PackTiles pt, bf16* __restrict__ packed) {
  __shared__ bf16 sh[NP][32][32 * 9 + 2];
  int u = 0;
#pragma unroll 1
  while (u + 1 < t.n && (int)blockIdx.x >= pt.tstart[u + 1]) ++u;
  const int O = t.O[u], I = t.I[u], NT = t.NT[u];
  const int tile = (int)blockIdx.x - pt.tstart[u];
  const int itiles = I >> 5;
  const int o0 = (tile / itiles) << 5, i0 = (tile % itiles) << 5;
  const size_t n = (size_t)NT * O * I;
  const int run = 32 * NT;   // contiguous floats per output-channel row of the tile
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int o = idx / run, r = idx - o * run;
    const float v = t.w[u][((size_t)(o0 + o) * I + i0) * NT + r];
    if constexpr (NP == 1) {
      sh[0][o][r] = (bf16)v;
    } else {
      bf16 a, b, c;
      split3_bf16(v, a, b, c);
      sh[0][o][r] = a; sh[1][o][r] = b; sh[2][o][r] = c;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int x = idx & 31, y = (idx >> 5) & 31, tp = idx >> 10;
    // forward layout [tap][O][I]: x = input channel (fastest), y = output channel
    const size_t fdst = t.dst_fwd[u] + ((size_t)tp * O + o0 + y) * I + i0 + x;
    // dgrad layout [tap][I][O]: x = output channel (fastest), y = input channel
    const size_t ddst = t.dst_dg[u] + ((size_t)tp * I + i0 + y) * O + o0 + x;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
      if constexpr (ORI != PACK_DGRAD) packed[fdst + pl * n] = sh[pl][y][x * NT + tp];
      if constexpr (ORI != PACK_FWD) packed[ddst + pl * n] = sh[pl][x][y * NT + tp];
    }
    // perf mode, PH_WFRAG_COPY: a fragment-major copy of the orientation in plane 1 of its region (a split plane this mode does not
    // read): [tap][rows / 64][K / 64] x 4096 elements
    if constexpr (NP == 1) {
      if (ORI != PACK_DGRAD && (t.frag[u] & 3))      // forward: row o, k i
        packed[t.dst_fwd[u] + n + (size_t)tp * O * I + frag64_tiled(o0 + y, i0 + x, I)] = sh[0][y][x * NT + tp];
      if (ORI != PACK_FWD && (t.frag[u] >> 2))       // dgrad: row = input channel, k = output channel
        packed[t.dst_dg[u] + n + (size_t)tp * I * O + frag64_tiled(i0 + y, o0 + x, O)] = sh[0][x][y * NT + tp];
    }
  }
}

// PH_PREC_FP16X3 layout: per (tap, output row) the K direction holds, for every 64-channel slice, the three fp16 blocks
// [hi * 2^11 | lo | hi] of the weights' half-pair split (w ~= hi + lo * 2^-11): the K loop of a convolution multiplies them
// with the activation blocks (hi, hi, lo) and accumulates 2^11 * (x * w) in ONE accumulator set.  |w| < 32 (hi * 2^11 is fp16).
__device__ __forceinline__ size_t hp_k(int k) { return (size_t)(k >> 6) * 192 + (k & 63); }
__device__ __forceinline__ void hp_w3(float v, f16& b0, f16& b1, f16& b2) {
  hp_split(v, b2, b1);
  b0 = (f16)((float)b2 * PH_HP_LO);
}
// The fragment-major forms put the three blocks of a 64 x 64 block 4096 elements apart, each in frag64_index order.
// ONE: a single convolution, the orientation `dgrad_only` alone.
template <bool ONE>
__global__ __launch_bounds__(256) void pack_all_tiled_hp_kernel(PhPackAll t, PackTiles pt, f16* __restrict__ packed, int dgrad_only) {
  __shared__ float sh[32][32 * 9 + 1];
  int u = 0;
#pragma unroll 1
  while (u + 1 < t.n && (int)blockIdx.x >= pt.tstart[u + 1]) ++u;
  const int O = t.O[u], I = t.I[u], NT = t.NT[u];
  const int ffwd = t.frag[u] & 3, fdg = (t.frag[u] >> 2) & 3;
  const int tile = (int)blockIdx.x - pt.tstart[u];
  const int itiles = I >> 5;
  const int o0 = (tile / itiles) << 5, i0 = (tile % itiles) << 5;
  const int run = 32 * NT;
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int o = idx / run, r = idx - o * run;
    sh[o][r] = t.w[u][((size_t)(o0 + o) * I + i0) * NT + r];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 32 * run; idx += 256) {
    const int x = idx & 31, y = (idx >> 5) & 31, tp = idx >> 10;
    f16 b0, b1, b2;
    if (!ONE || dgrad_only == 0) {   // forward layout [tap][O][3 I]: x = input channel (fastest), y = output channel
      hp_w3(sh[y][x * NT + tp], b0, b1, b2);
      if (ffwd == PH_WFRAG_TAP5) {
        // conv_tap5.hip's 64 x 64 x 9 slab set: per tap [block 3] x 4096 elements
        f16* d = packed + t.dst_fwd[u] + (size_t)tp * 12288 + frag64_index(o0 + y, i0 + x);
        d[0] = b0; d[4096] = b1; d[8192] = b2;
      } else if (ffwd == PH_WFRAG_TAP6) {
        // conv_tap6.hip (the stride-2 convolutions, forward orientation only): [tap][O / 64][I / 64][block 3] x 4096 elements
        const int o = o0 + y, i = i0 + x;
        f16* d = packed + t.dst_fwd[u] + (size_t)tp * O * 3 * I + (size_t)(((o >> 6) * (I >> 6) + (i >> 6)) * 3) * 4096 + frag64_index(o & 63, i & 63);
        d[0] = b0; d[4096] = b1; d[8192] = b2;
      } else {
        f16* d = packed + t.dst_fwd[u] + ((size_t)tp * O + o0 + y) * (3 * (size_t)I) + hp_k(i0 + x);
        d[0] = b0; d[64] = b1; d[128] = b2;
      }
    }
    if (!ONE || dgrad_only == 1) {   // dgrad layout [tap][I][3 O]: x = output channel (fastest), y = input channel
      hp_w3(sh[x][y * NT + tp], b0, b1, b2);
      if (fdg == PH_WFRAG_TAP5) {
        f16* d = packed + t.dst_dg[u] + (size_t)tp * 12288 + frag64_index(i0 + y, o0 + x);
        d[0] = b0; d[4096] = b1; d[8192] = b2;
      } else {
        f16* d = packed + t.dst_dg[u] + ((size_t)tp * I + i0 + y) * (3 * (size_t)O) + hp_k(o0 + x);
        d[0] = b0; d[64] = b1; d[128] = b2;
      }
    }
  }
}

// stem: w [64][3][7][7] -> three bf16 split planes [3][kh 7][cout 64][kw 8 x ch 4], zero padded
__global__ void pack_w_stem_kernel(const float* __restrict__ w, bf16* __restrict__ planes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 7 * 64 * 32) return;
  const int k = i & 31, co = (i >> 5) & 63, kh = i >> 11;
  const int kw = k >> 2, ch = k & 3;
  float v = 0.f;
  if (kw < 7 && ch < 3) v = w[((co * 3 + ch) * 7 + kh) * 7 + kw];
  bf16 a, b, c;
  split3_bf16(v, a, b, c);
  planes[i] = a; planes[7 * 64 * 32 + i] = b; planes[2 * 7 * 64 * 32 + i] = c;
}

// stem, PH_PREC_FP16X3: three fp16 planes [3][kh 7][cout 64][kw 8 x ch 4] = w hi * 2^11, w lo, w hi (the layout of the
// three bf16 split planes): the kernel multiplies them with the activation planes (hi, hi, lo)
__global__ void pack_w_stem_hp_kernel(const float* __restrict__ w, f16* __restrict__ packed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 7 * 64 * 32) return;
  const int k = i & 31, co = (i >> 5) & 63, kh = i >> 11;
  const int kw = k >> 2, ch = k & 3;
  float v = 0.f;
  if (kw < 7 && ch < 3) v = w[((co * 3 + ch) * 7 + kh) * 7 + kw];
  f16 b0, b1, b2;
  hp_w3(v, b0, b1, b2);
  packed[i] = b0; packed[7 * 64 * 32 + i] = b1; packed[2 * 7 * 64 * 32 + i] = b2;
}

// A table the kernels can tile (whole 32 x 32 tiles, at most 9 taps) whose layouts exist for its shapes: the fragment-major forms
// are those of their kernels' weight shapes only, the dgrad orientation has no PH_WFRAG_TAP6, the split planes no copy.  Fills the
// tile starts.  Nothing can build a table that fails the tiling: every plan and entry point takes channel counts that are multiples
// of 64 and 1x1 / 3x3 kernels, and a plan cuts its units into tables of std::size(PhPackAll::w).
bool table_ok(const PhPackAll* t, int nplanes, PackTiles* pt) {
  if (t->n < 1 || t->n > (int)std::size(t->w) || (nplanes != 1 && nplanes != 3 && nplanes != -3)) return false;
  pt->tstart[0] = 0;
  for (int u = 0; u < t->n; ++u) {
    const int O = t->O[u], I = t->I[u], NT = t->NT[u];
    if (O < 32 || I < 32 || (O & 31) || (I & 31) || NT < 1 || NT > 9) return false;
    pt->tstart[u + 1] = pt->tstart[u] + (O >> 5) * (I >> 5);
    if (t->frag[u] < 0 || t->frag[u] > 15) return false;
    const int ff = t->frag[u] & 3, fd = t->frag[u] >> 2;
    if (nplanes == 3) {
      if (ff || fd) return false;
    } else if (nplanes == 1) {
      if (ff > PH_WFRAG_COPY || fd > PH_WFRAG_COPY) return false;
      if (ff && !ph_tapconv7_wshape(O, I, NT) && !ph_tapconv6b_wshape(O, I, NT)) return false;
      if (fd && !ph_tapconv7_wshape(I, O, NT)) return false;
    } else {
      if ((ff == PH_WFRAG_TAP5 || fd == PH_WFRAG_TAP5) && !(O == 64 && I == 64 && NT == 9)) return false;
      if (ff == PH_WFRAG_TAP6 && !(O == 2 * I && NT == 9)) return false;
      if (ff > PH_WFRAG_TAP6 || fd > PH_WFRAG_TAP5) return false;
    }
  }
  return true;
}

}  // namespace

int ph_pack_all_launch(const PhPackAll* t, void* packed, int nplanes, hipStream_t st) {
  PackTiles pt;
  if (!table_ok(t, nplanes, &pt)) return PH_EINVAL;
  const dim3 grid(pt.tstart[t->n]), block(256);
  if (nplanes == -3) hipLaunchKernelGGL(pack_all_tiled_hp_kernel<false>, grid, block, 0, st, *t, pt, (f16*)packed, 0);
  else if (nplanes == 1) hipLaunchKernelGGL(pack_all_tiled_kernel<1>, grid, block, 0, st, *t, pt, (bf16*)packed);
  else hipLaunchKernelGGL(pack_all_tiled_kernel<3>, grid, block, 0, st, *t, pt, (bf16*)packed);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_pack_w_launch(const float* w, void* packed, int O, int I, int KS, int dgrad, int nplanes, int frag, hipStream_t st) {
  if ((KS != 1 && KS != 3) || frag < 0 || frag > 3) return PH_EINVAL;      // (frag: one orientation's PH_WFRAG_*)
  PhPackAll t{};
  t.n = 1; t.w[0] = w; t.O[0] = O; t.I[0] = I; t.NT[0] = KS * KS;
  t.frag[0] = dgrad ? frag << 2 : frag;
  PackTiles pt;
  if (!table_ok(&t, nplanes, &pt)) return PH_EINVAL;
  const dim3 grid(pt.tstart[1]), block(256);
  if (nplanes == -3) hipLaunchKernelGGL(pack_all_tiled_hp_kernel<true>, grid, block, 0, st, t, pt, (f16*)packed, dgrad ? 1 : 0);
  else if (nplanes == 1 && !dgrad) hipLaunchKernelGGL((pack_all_tiled_kernel<1, PACK_FWD>), grid, block, 0, st, t, pt, (bf16*)packed);
  else if (nplanes == 1) hipLaunchKernelGGL((pack_all_tiled_kernel<1, PACK_DGRAD>), grid, block, 0, st, t, pt, (bf16*)packed);
  else if (!dgrad) hipLaunchKernelGGL((pack_all_tiled_kernel<3, PACK_FWD>), grid, block, 0, st, t, pt, (bf16*)packed);
  else hipLaunchKernelGGL((pack_all_tiled_kernel<3, PACK_DGRAD>), grid, block, 0, st, t, pt, (bf16*)packed);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_pack_w_stem_launch(const float* w, void* planes, hipStream_t st) {
  hipLaunchKernelGGL(pack_w_stem_kernel, dim3((7 * 64 * 32 + 255) / 256), dim3(256), 0, st, w, (bf16*)planes);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_pack_w_stem_hp_launch(const float* w, void* packed, hipStream_t st) {
  hipLaunchKernelGGL(pack_w_stem_hp_kernel, dim3((7 * 64 * 32 + 255) / 256), dim3(256), 0, st, w, (f16*)packed);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

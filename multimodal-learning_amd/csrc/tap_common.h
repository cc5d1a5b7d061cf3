// Pieces shared by the tap-convolution translation units.
//   conv_tap.hip .. conv_tap7.hip, conv_tap6b.hip: the debug-build phase tracer macros.
//   conv_tap.hip, conv_tap2.hip: the row-pair swizzled LDS image (lds_off) and the MFMA-row -> pixel permutation.
//   conv_tap2.hip .. conv_tap7.hip, conv_tap6b.hip (the LDS-DMA kernels): lds_dma16 (conv_tap2.hip: its own form), the zero / NaN
//     halo source tables, the counted-wait, barrier and scheduling macros, RSRC_FLAGS; conv_wgrad.hip takes lds_dma16 too.
//   conv_tap2 / 3 / 4: bn_relu_chunk (the input's BatchNorm + ReLU applied in LDS).
//   conv_tap3 .. conv_tap7, conv_tap6b: halo_off (the column-swizzled halo image); conv_tap5 / 6 / 6b / 7: ph_wait_vmcnt.
//   conv_tap2 .. conv_tap7, conv_tap6b (the persistent kernels): ph_fdiv (conv_tap4: its own integer form) and PH_TILE_LIST.
//   conv_tap6 / 6b / 7 take the nine-set weight window from tap_window.h, which includes this file.
//   conv_tap4 .. conv_tap7, conv_tap6b (host): ph_launch_persistent; the stat_parts functions share ph_persistent_wgs with it.
#pragma once
#include <mutex>
#include "ph_common.h"
#include "ph_kernels.h"

// Debug build only (make trace): per-workgroup phase timestamps (100 MHz wall clock) of a tap-conv kernel; the
// including file defines the buffer `__device__ unsigned long long ph_tap_trace[PH_TRACE_WGS * 12]`,
// read back by tests/trace_tapconv_gpu.py.  Not part of the product library or of the public C-ABI.
#ifdef PH_TAP_TRACE
#define PH_TRACE_WGS 65536
#define PH_TRACE(k)                                                                                        \
  do {                                                                                                     \
    const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                   \
    if (threadIdx.x == 0 && wg_ < PH_TRACE_WGS) ph_tap_trace[(size_t)wg_ * 12 + (k)] = wall_clock64();      \
  } while (0)
#define PH_TRACE_HWID()                                                                                    \
  do {                                                                                                     \
    const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                   \
    if (threadIdx.x == 0 && wg_ < PH_TRACE_WGS)                                                            \
      ph_tap_trace[(size_t)wg_ * 12 + 7] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) |   \
                                          (unsigned)__builtin_amdgcn_s_getreg(63492);                      \
  } while (0)
#define PH_TRACE_ACC(k, v)                                                                                 \
  do {                                                                                                     \
    const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                   \
    if (threadIdx.x == 0 && wg_ < PH_TRACE_WGS) ph_tap_trace[(size_t)wg_ * 12 + (k)] = (v);                \
  } while (0)
#define PH_TRACE_ACC_T(k, v, thr)                                                                          \
  do {                                                                                                     \
    const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                   \
    if (threadIdx.x == (thr) && wg_ < PH_TRACE_WGS) ph_tap_trace[(size_t)wg_ * 12 + (k)] = (v);            \
  } while (0)
#define PH_CLK() clock64()
#else
#define PH_TRACE_ACC_T(k, v, thr)
#define PH_TRACE(k)
#define PH_TRACE_HWID()
#define PH_TRACE_ACC(k, v)
#define PH_CLK() 0ull
#endif


// LDS image addressing shared by the A (halo pixels) and B (weight rows) tiles: 128-B rows (64 bf16), two rows
// per 256-B bank row; the 16-B chunk index is XOR-swizzled with 3 bits of the row-pair index, the row's half of the
// bank row stays where it is.  A ds_read_b128 lane group (16 lanes, MI355X_MICROARCH.md: LDS) must touch 16 distinct
// 16-B slots of the 256-B bank row.  With the lane->pixel permutation below a group reads 16 CONSECUTIVE pixels:
// eight row pairs with eight different swizzle terms when the run starts on an even pixel, and when it starts on an
// odd one (the dx = 1 taps) its first and last pixel share a swizzle term but sit in opposite halves.  (Round 1 XORed
// FOUR bits of the row pair into the slot: equally conflict-free on even runs, but on odd runs the last pixel then
// lands on the first pixel's slot - 2-way on a third of the taps: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.18 -> 0.00
// for the dense kernel, 0.11 -> 0.00 for the layer-1 kernel; the kernel times did not move, the LDS array was not the limit.)  B rows are consecutive channels per lane, i.e. the
// hardware groups see rows {0-3, 12-15, 20-27} + const: row pairs 0,1,6,7,10,11,12,13 -> terms 0,1,6,7,2,3,4,5.
#define PH_SWZ_MASK 7   // (bits of the row-pair index in the swizzle: the LDS-DMA source mapping in conv_tap2.hip uses it too)
__device__ __forceinline__ int lds_off(int row, int chunk) {
  return (row >> 1) * 256 + ((((row & 1) << 3) | (chunk ^ ((row >> 1) & PH_SWZ_MASK))) << 4);
}
// MFMA A-fragment row i (0..31) -> pixel (fr, c) inside a 2 x 16 patch such that the hardware's
// ds_read_b128 lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} each read 16 CONSECUTIVE pixels of one row
__device__ __forceinline__ void frag_row_to_pixel(int i, int& fr, int& c) {
  const int k = i >> 2;
  fr = __popc(k) & 1;
  c = ((k >> 1) << 2) | (i & 3);
}

// ---- LDS-DMA operand streams (conv_tap2.hip's header comment says why they are inline asm with hand-counted vmcnt)
typedef __attribute__((address_space(3))) unsigned char lds_uchar;

// one LDS-DMA wave-instruction: lane l copies 16 B from its global address g to LDS byte lds_addr + 16*l.  lds_addr is
// wave-uniform by construction; readfirstlane states it for builds that do not prove it - it folds away at -O3.  The s_nop covers
// the hazard between the scalar write of m0 and the LDS-DMA that reads it.  (conv_tap2.hip has a form without the readfirstlane,
// conv_tap3.hip one with a scalar base.)
__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(__builtin_amdgcn_readfirstlane((int)lds_addr)), "v"(g) : "memory");
}

#define PH_WAIT_VMCNT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
#define PH_BARRIER() asm volatile("s_barrier" ::: "memory")
#define PH_SB() __builtin_amdgcn_sched_barrier(0)      // keeps the compiler from regrouping across a hand-scheduled slot
#define PH_NOP ((void)0)                               // empty filler statement of such a slot
// counted wait on a table entry: n is a compile-time constant after unrolling at every call site, so the switch folds to the one
// s_waitcnt.  63 is the counter's maximum - nothing this wave issued can still be in question - and emits nothing.
__device__ __forceinline__ void ph_wait_vmcnt(int n) {
  switch (n) {
#define PH_W(N) case N: PH_WAIT_VMCNT(N); break;
#define PH_W8(A, B, C, D, E, F, G, H) PH_W(A) PH_W(B) PH_W(C) PH_W(D) PH_W(E) PH_W(F) PH_W(G) PH_W(H)
    PH_W8(0, 1, 2, 3, 4, 5, 6, 7) PH_W8(8, 9, 10, 11, 12, 13, 14, 15) PH_W8(16, 17, 18, 19, 20, 21, 22, 23) PH_W8(24, 25, 26, 27, 28, 29, 30, 31)
    PH_W8(32, 33, 34, 35, 36, 37, 38, 39) PH_W8(40, 41, 42, 43, 44, 45, 46, 47) PH_W8(48, 49, 50, 51, 52, 53, 54, 55)
    PH_W(56) PH_W(57) PH_W(58) PH_W(59) PH_W(60) PH_W(61) PH_W(62)
#undef PH_W8
#undef PH_W
    case 63: break;
    default: PH_WAIT_VMCNT(0); break;
  }
}

// buffer resource word 3 of the kernels that store through one: raw buffer, 32-bit offsets (gfx90a / gfx94x / gfx950 data format word)
constexpr int RSRC_FLAGS = 0x00020000;

namespace {
// sources of out-of-image halo pixels (one copy per code object).  Zeros - or, when the input's BatchNorm + ReLU is applied in LDS
// (PhTapConv::in_scale), quiet NaNs: padding must be zero AFTER that map, for any scale / shift, and fma(NaN, s, b) = NaN, the
// ReLU's v_max_f32(NaN, 0) returns the number, 0.
__device__ const u32x4 ph_zero16[4] = {};
__device__ const u32x4 ph_nan16[4] = {{0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u}, {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u},
                                      {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u}, {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u}};
}  // namespace

// relu(x * s + h) on the 8 bf16 values of one 16-byte chunk (channel 2q in the low half of dword q), result rounded to
// bf16 like the stand-alone bn_apply pass stores it
__device__ __forceinline__ u32x4 bn_relu_chunk(u32x4 v, const f32x4& sA, const f32x4& sB, const f32x4& hA, const f32x4& hB) {
  u32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float x0 = __builtin_bit_cast(float, v[q] << 16), x1 = __builtin_bit_cast(float, v[q] & 0xffff0000u);
    const float s0 = q < 2 ? sA[2 * q] : sB[2 * q - 4], s1 = q < 2 ? sA[2 * q + 1] : sB[2 * q - 3];
    const float h0 = q < 2 ? hA[2 * q] : hB[2 * q - 4], h1 = q < 2 ? hA[2 * q + 1] : hB[2 * q - 3];
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
    bf2 r;
    r[0] = (bf16)fmaxf(x0 * s0 + h0, 0.f);
    r[1] = (bf16)fmaxf(x1 * s1 + h1, 0.f);
    o[q] = __builtin_bit_cast(unsigned, r);
  }
  return o;
}

// halo image of the 16x16x32 kernels (conv_tap3.hip's header comment): pixel (hr, hc) of a halo HPW pixels wide, 16-byte chunk c of
// its 64 channels -> LDS byte offset inside an image buffer.  Swizzled by the pixel column only: linear in the halo row.
template <int HPW>
__device__ __forceinline__ int halo_off(int hr, int hc, int c) {
  return (HPW / 2 * hr + (hc >> 1)) * 256 + ((hc & 1) << 7) + ((c ^ (((hc >> 1) & 3) << 1)) << 4);
}

// ---- tile list of a persistent workgroup (conv_tap2 .. conv_tap7, conv_tap6b).  What a linear tile id MEANS - image-major or
// Cout-block-major, the input pointer - is each kernel's `decode`; the division it needs and the walk over the ids are here.
// q = a / d for 0 <= a < 2^22 with a precomputed float reciprocal and one correction step (a decode runs once per tile on the
// critical path; hardware integer division costs ~40 instructions per quotient)
__device__ __forceinline__ int ph_fdiv(int a, int d, float rcp) {
  int q = (int)((float)a * rcp);
  int r = a - q * d;
  if (r >= d) ++q;
  if (r < 0) --q;
  return q;
}
// The workgroups of one XCD (blockIdx.x % 8: hardware round-robin) walk one contiguous eighth of the list, so neighbouring halos
// and the weight block of a Cout block are shared inside one L2.  PH_TILE_LIST(tile_id, total) declares tile_id(k): the k-th tile of
// this workgroup, -1 when its list is exhausted.  (A macro that declares a lambda, not a struct or a function: those are simplified
// on their own before they are inlined, and the kernels that walk the list then compile to another schedule - profiles/EXPERIMENTS.md.)
#define PH_TILE_LIST(TILE_ID, TOTAL)                                     \
  const int tl_wgs = gridDim.x;                                          \
  const bool tl_xcd_map = (tl_wgs & 7) == 0 && tl_wgs < (TOTAL);         \
  const int tl_per_xcd = ((TOTAL) + 7) >> 3;                             \
  auto TILE_ID = [&](int k) -> int {                                     \
    if (!tl_xcd_map) {                                                   \
      const int t = (int)blockIdx.x + k * tl_wgs;                        \
      return t < (TOTAL) ? t : -1;                                       \
    }                                                                    \
    const int local = ((int)blockIdx.x >> 3) + k * (tl_wgs >> 3);        \
    const int t = ((int)blockIdx.x & 7) * tl_per_xcd + local;            \
    return (local < tl_per_xcd && t < (TOTAL)) ? t : -1;                 \
  }

// ---- host side of the persistent kernels: one workgroup per CU (LDS) walks a tile list of C::TH x C::TW pixels x C::BNT channels.
// Workgroups of a launch = the BatchNorm partial rows it writes (the stat_parts functions).
template <class C>
int ph_persistent_wgs(const PhTapConv& p) {
  const int total = cdiv(p.OHt, C::TH) * cdiv(p.OWt, C::TW) * (p.Cout / C::BNT) * p.B;
  const int resident = ph_num_cus();
  return total < resident ? total : resident;
}
// The launch.  KERN is a template parameter, not a run-time pointer: every kernel keeps its own once_flag and so gets its own raised
// dynamic-LDS limit (thread-safe).  cls: profiling class; S, es: stride and element size of ph_tapconv_bytes.
template <auto KERN, class C>
int ph_launch_persistent(const PhTapConv& p, hipStream_t st, int cls, int S, int es) {
  static std::once_flag once;
  static hipError_t attr_rc = hipSuccess;
  std::call_once(once, [] {
    attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
  });
  if (attr_rc != hipSuccess) return PH_ELAUNCH;
  void* tok = nullptr;
  if (ph_prof_on())
    ph_prof_begin2(cls, 2.0 * p.B * p.OHt * p.OWt * (double)p.Cout * p.ntaps * p.Cin, ph_tapconv_bytes(p, S, es), st, &tok);
  hipLaunchKernelGGL(KERN, dim3(ph_persistent_wgs<C>(p)), dim3(C::NTH), C::LDS_BYTES, st, p);
  ph_prof_end(tok, st);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

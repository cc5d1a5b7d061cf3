// Weight-gradient (wgrad) of the 3x3 / 1x1 convolutions on MFMA.
//
//   dW[tap][cout][cin] = sum_{b,r,c} dY[b,r,c,cout] * X[b, r*S + kh - pad, c*S + kw - pad, cin]
// GEMM view: M = cout, N = cin, K = pixels (huge).  Both operands are K-major in HBM (NHWC: pixel is the
// slow index), so both MFMA fragments are fetched from LDS with the CDNA4 transposing read
// ds_read_b64_tr_b16 - the tiles are staged exactly as they lie in HBM (coalesced 16-B rows), no
// transposed copy is ever made.  One workgroup owns a 64x64 (cout x cin) block for ALL taps and walks a
// chunk of spatial tiles, keeping 9 x 32x32 accumulators per wave in registers (144 VGPRs); the X halo
// tile is staged once per spatial tile and re-read by all 9 taps.  Partial sums go to a slab
// [chunk][tap][cout][cin] and are combined in fixed order by a reduce kernel (bitwise reproducible,
// no float atomics).
#include "ph_common.h"
#include "ph_kernels.h"
#include "tap_common.h"

// PH_WG_LEAN=0 (ph_debug_set_wg_lean(0)): the perf-mode weight gradients run the loop of wgrad_kernel<.., LEAN = false> - bitwise the
// same gradients
PH_SWITCH(wg_lean, "PH_WG_LEAN")

namespace {

// 32-B piece swizzle of a [pixel][64 ch] bf16 image (128-B rows): makes the 4-row tr-reads conflict-free
__device__ __forceinline__ int sw_piece(int pix, int piece) { return piece ^ (((pix >> 1) & 1) << 1); }

template <typename T, int S, int TH, int KS>
struct WgCfg {
  static constexpr bool SPLIT = is_f32<T>::value;
  static constexpr bool HPM = is_hp<T>::value;   // PH_PREC_FP16X3: both operands are half-pair tensors, three passes over the chunk
  static constexpr int TW = 16, BM = TH * TW;
  static constexpr int HPH = (TH - 1) * S + KS, HPW = (TW - 1) * S + KS, HP = HPH * HPW;
  static constexpr int HPP = (HP + 7) / 8 * 8;            // halo pixels padded to whole 1-KiB LDS-DMA pieces
  static constexpr int D_BYTES = BM * 128, X_BYTES = HPP * 128;
  static constexpr int NP = SPLIT ? PH_NPLANES : 1;
  // perf mode: two LDS buffers (tile t+1 lands by LDS-DMA while tile t feeds the MFMAs)
  static constexpr int LDS_BYTES = SPLIT ? (D_BYTES + X_BYTES) * NP : 2 * (D_BYTES + X_BYTES);
  static constexpr int NT = KS * KS;
  // LDS-DMA pieces (1 KiB = 8 pixel rows, one wave-instruction) per wave and tile: dz, halo (the last one may be a partial round)
  static constexpr int NDP = BM * 8 / 256, NHP = (HPP * 8 + 255) / 256, NPIECES = NDP + NHP;
};

// stage 8 channels of one pixel into plane 0 (bf16) or into the 3 split planes (fp32 source)
template <typename T>
__device__ __forceinline__ void stage_row(const T* src, bool ok, unsigned char* base, int plane_bytes, int off) {
  if constexpr (!is_f32<T>::value) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const u32x4*>(src);
    *reinterpret_cast<u32x4*>(base + off) = v;
  } else {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = 0.f;
    if (ok) load8(src, v);
    bf16x8 p0, p1, p2;
#pragma unroll
    for (int q = 0; q < 8; ++q) { bf16 a, b, c; split3_bf16(v[q], a, b, c); p0[q] = a; p1[q] = b; p2[q] = c; }
    *reinterpret_cast<bf16x8*>(base + off) = p0;
    *reinterpret_cast<bf16x8*>(base + plane_bytes + off) = p1;
    *reinterpret_cast<bf16x8*>(base + 2 * plane_bytes + off) = p2;
  }
}

__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* base, int off0, int off1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off0));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off1));
  union { s16x4 s[2]; bf16x8 v; } u;
  u.s[0] = a; u.s[1] = b;
  return u.v;
}

// LEAN (perf mode only; PH_WG_LEAN, default on): the halo-row-major MFMA stream and the precomputed LDS-DMA issue below.  LEAN =
// false is the loop as it was - the A/B arm and the reference of tests/test_gpu_wgrad_lean.py; both arms write bitwise the same slab.
// (A template parameter, i.e. two kernels: a run-time flag inside one kernel would make each arm pay for the other's registers.)
template <typename T, int S, int TH, int KS, bool LEAN>
__global__ __launch_bounds__(256) void wgrad_kernel(PhWgrad p) {
  using C = WgCfg<T, S, TH, KS>;
  constexpr bool SPLIT = C::SPLIT, HPM = C::HPM;
  constexpr int TW = C::TW, BM = C::BM, HPH = C::HPH, HPW = C::HPW, HP = C::HP, NT = C::NT, NP = C::NP;
  static_assert(!(LEAN && SPLIT), "the lean loop is a perf-mode (LDS-DMA) loop");
  typedef typename std::conditional<HPM, f16, T>::type TI;       // element type as the staging code addresses it
  constexpr int EW = HPM ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ldsD = smem;                      // NP planes of D_BYTES
  unsigned char* ldsX = smem + C::D_BYTES * NP;    // NP planes of X_BYTES

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (scalar) by construction
  const int cf = wave >> 1, kf = wave & 1;     // 32-wide cout / cin fragment of this wave
  const int cin_blocks = p.Cin >> 6;
  const int co0 = (blockIdx.x / cin_blocks) << 6, ci0 = (blockIdx.x % cin_blocks) << 6;
  const int chunk = blockIdx.y;
  const int tiles_w = (p.OW + TW - 1) / TW, tiles_h = (p.OH + TH - 1) / TH;
  const int tiles_img = tiles_w * tiles_h, ntiles = tiles_img * p.B;
  const int t_begin = chunk * p.tiles_per_chunk;
  const int t_end = min(ntiles, t_begin + p.tiles_per_chunk);
  const TI* X = reinterpret_cast<const TI*>(p.x);
  const TI* DY = reinterpret_cast<const TI*>(p.dy);
  const long xpix = (p.x_pix_stride ? p.x_pix_stride : p.Cin) * EW;
  const long xrow = (p.x_row_stride ? p.x_row_stride : (long)p.IW * p.Cin) * EW;
  const long ximg = (p.x_img_stride ? p.x_img_stride : (long)p.IH * p.IW * p.Cin) * EW;
  const long dpix = (long)p.Cout * EW;      // elements per dy pixel record

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

  // tr-read lane roles: within each 16-lane group, lane 4q+p supplies row q, columns 4p..4p+3
  const int q4 = (lane & 15) >> 2, p4 = lane & 3, colhalf = (lane >> 4) & 1, khalf = lane >> 5;
  const int pieceA = cf * 2 + colhalf, pieceB = kf * 2 + colhalf;

  // ---- MFMA over one staged tile (K = the tile's pixels, 16 per MFMA)
  auto compute = [&](const unsigned char* dD, const unsigned char* dX) {
#pragma unroll 2
    for (int kk = 0; kk < BM / 16; ++kk) {
      // the two 4-pixel row groups this lane's tr-reads address
      const int t0 = kk * 16 + 8 * khalf + q4, t1 = t0 + 4;
      const int offA0 = t0 * 128 + sw_piece(t0, pieceA) * 32 + p4 * 8;
      const int offA1 = t1 * 128 + sw_piece(t1, pieceA) * 32 + p4 * 8;
      bf16x8 a[NP];      // (third plane: only in the six-product mode)
#ifdef PH_ABL_WG_NOLDS   // timing ablation only (garbage results): no fragment reads
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) { bf16x8 z; asm volatile("" : "=v"(z)); a[pl] = z; }
#else
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        if (pl < 2 || p.prod6) a[pl] = tr_pair(dD + pl * C::D_BYTES, offA0, offA1);
#endif
      const int hb0 = ((t0 >> 4) * S) * HPW + (t0 & 15) * S;
      const int hb1 = ((t1 >> 4) * S) * HPW + (t1 & 15) * S;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int toff = (t / KS) * HPW + (t % KS);
        const int h0 = hb0 + toff, h1 = hb1 + toff;
        const int offB0 = h0 * 128 + sw_piece(h0, pieceB) * 32 + p4 * 8;
        const int offB1 = h1 * 128 + sw_piece(h1, pieceB) * 32 + p4 * 8;
        bf16x8 bq[NP];
#ifdef PH_ABL_WG_NOLDS
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) { bf16x8 z; asm volatile("" : "=v"(z) : "v"(offB0 + offB1)); bq[pl] = z; }
#else
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
          if (pl < 2 || p.prod6) bq[pl] = tr_pair(dX + pl * C::X_BYTES, offB0, offB1);
#endif
        if constexpr (SPLIT) {
#define PH_MM(PI, PJ) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PI], bq[PJ], acc[t], 0, 0, 0);
          if (p.prod6) { PH_SPLIT_PAIRS_LO(PH_MM) }
          PH_SPLIT_PAIRS_HI(PH_MM)
#undef PH_MM
        } else if constexpr (HPM) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, bq[0]), acc[t], 0, 0, 0);
        } else {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bq[0], acc[t], 0, 0, 0);
        }
      }
    }
  };

  // ---- the same MFMA stream with the fragment reads issued THREE taps ahead of the MFMA that consumes them (perf mode, 3 x 3
  // stride 1: the 13 large launches of a step).  compute() above leaves the order to the compiler, which reads a tap's fragments
  // right in front of its MFMA and relies on a second wave of the SIMD to cover the latency - in the step the kernel runs one
  // workgroup per CU beside the BatchNorm-backward passes and 60 % of its time was exposed (skip-ablation: -0.86 ms per step).
  // Every fragment address is one of five per-lane base registers + an immediate: halo pixel h = 18 kk + u + toff (u = 8 khalf +
  // q4, + 4 for the second row group), swizzle bit = bit 1 of h = (kk & 1) ^ bit1(toff) ^ bit1(u) ^ (bit0(u) & bit0(toff)).
  constexpr bool PIPE = !SPLIT && S == 1 && KS == 3 && (BM / 16 == TH);      // (half-pair mode: every pass of its item stream)
  constexpr int PBUF = C::D_BYTES + C::X_BYTES;
  const int u_lane = 8 * khalf + q4;
  const int baseA = u_lane * 128 + ((pieceA ^ (((u_lane >> 1) & 1) << 1)) << 5) + p4 * 8;
  const int baseB = u_lane * 128 + (pieceB << 5) + p4 * 8;
  const int bE0 = baseB ^ (((u_lane >> 1) & 1) << 6), bE1 = bE0 ^ 64;                          // taps with an even toff
  const int bO0 = baseB ^ ((((u_lane >> 1) ^ u_lane) & 1) << 6), bO1 = bO0 ^ 64;               // taps with an odd toff
  // (the accumulators live in AGPRs from here on: without this the loop-carried values sat in vector registers and were copied
  // to the accumulation registers and back around every tile - 144 + 144 moves and 190 vector registers)
  if constexpr (PIPE) {
#pragma unroll
    for (int t = 0; t < NT; ++t) asm volatile("" : "+a"(acc[t]));
  }
  auto compute_p = [&](const int boff) __attribute__((always_inline)) {      // boff: byte offset of the LDS buffer pair (ONE body:
    if constexpr (PIPE) {                                                      // two copies made a 144-register phi of the accumulators)
      const unsigned char* dD = smem + boff;
      const unsigned char* dX = dD + C::D_BYTES;
      constexpr int NI = (BM / 16) * 9, LA = 3;
      bf16x8 af[2], bfr[4];
      auto ldA = [&](const int kk) { return tr_pair(dD, baseA + kk * 2048, baseA + 512 + kk * 2048); };
      auto ldB = [&](const int i) {
        const int kk = i / 9, t = i % 9;
        const int toff = (t / 3) * HPW + (t % 3);
        const int flip = ((kk & 1) ^ ((toff >> 1) & 1)) & 1;
        const int base = (toff & 1) ? (flip ? bO1 : bO0) : (flip ? bE1 : bE0);
        const int imm = (kk * HPW + toff) * 128;
        return tr_pair(dX, base + imm, base + imm + 512);
      };
      af[0] = ldA(0);
#pragma unroll
      for (int i = 0; i < LA; ++i) bfr[i] = ldB(i);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int kk = i / 9, t = i % 9;
        if (i + LA < NI) bfr[(i + LA) & 3] = ldB(i + LA);
        if (t == 4 && kk + 1 < BM / 16) af[(kk + 1) & 1] = ldA(kk + 1);
        if constexpr (HPM) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[t]) : "v"(af[kk & 1]), "v"(bfr[i & 3]));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[t]) : "v"(af[kk & 1]), "v"(bfr[i & 3]));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // ---- LEAN: the same 72 MFMAs walked by HALO ROW.  The x fragment of (k-step kk, tap kh, kw) is halo pixel (kk + kh) HPW + kw + u:
  // it depends on h = kk + kh and kw only, so compute_p reads each of the (TH + 2) * 3 = 30 distinct fragments up to three times (72
  // read pairs + 8 for dz = 160 ds_read_b64_tr_b16 per tile; the LDS allowed 320 cycles per k-step against 288 of MFMA).  Here fragment
  // j = 3 h + kw is read ONCE (30 + 8 pairs = 76 reads) and feeds acc[3 kh + kw] += A(h - kh) * B(h, kw) for every kh with 0 <= h - kh <
  // TH: 3 / 6 / 9 ... 9 / 6 / 3 MFMAs per halo row.  Every accumulator still receives its TH products in increasing kk from the same
  // operand bytes, so the slab is bitwise compute_p's.  What that loop learned is kept: an address is one of the five base registers
  // + an immediate (swizzle bit = bit 1 of the halo pixel = bit1(hoff) ^ bit1(u) ^ (bit0(hoff) & bit0(u)), hoff = h HPW + kw), the x
  // reads run three fragments (>= 3 MFMAs, 9 in the full rows) ahead in a ring of four, A(h + 1) is read in the middle of row h into
  // a ring of four (A(h - 3) was last used in row h - 1), MFMAs are asm volatile behind sched_barriers, one body for both buffers.
  // dma(k): piece k of the NEXT item's operands, one behind each of the first ten MFMAs (below: why no read of this buffer can see
  // one).  The slots are early on purpose: a piece issued late in the stream has not landed at the vmcnt(0) that ends the tile.  One
  // piece every 7th MFMA (the last one 5 MFMAs before the wait) cost 0.1 - 0.2 ms of the 22.4 ms B = 256 trunk against these slots,
  // one every 3rd measured the same as these; the B = 64 step did not tell the three apart (profiles/EXPERIMENTS.md).
  auto compute_l = [&](const int boff, auto dma) __attribute__((always_inline)) {
    if constexpr (PIPE && LEAN) {
      const unsigned char* dD = smem + boff;
      const unsigned char* dX = dD + C::D_BYTES;
      constexpr int NF = (TH + 2) * 3, LF = 3, DMA_FIRST = 0, DMA_STEP = 1;
      bf16x8 af[4], bfr[4];
      auto ldA = [&](const int kk) { return tr_pair(dD, baseA + kk * 2048, baseA + 512 + kk * 2048); };
      auto ldB = [&](const int j) {
        const int hoff = (j / 3) * HPW + (j % 3);
        const int flip = (hoff >> 1) & 1;
        const int base = (hoff & 1) ? (flip ? bO1 : bO0) : (flip ? bE1 : bE0);
        return tr_pair(dX, base + hoff * 128, base + hoff * 128 + 512);
      };
      af[0] = ldA(0);
#pragma unroll
      for (int j = 0; j < LF; ++j) bfr[j] = ldB(j);
      int m = 0;      // (MFMA index: a constant after unrolling)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int h = j / 3, kw = j % 3;
        if (j + LF < NF) bfr[(j + LF) & 3] = ldB(j + LF);
        if (kw == 1 && h + 1 < TH) af[(h + 1) & 3] = ldA(h + 1);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int kk = h - kh;
          if (kk >= 0 && kk < TH) {
            if constexpr (HPM) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[kh * 3 + kw]) : "v"(af[kk & 3]), "v"(bfr[j & 3]));
            else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[kh * 3 + kw]) : "v"(af[kk & 3]), "v"(bfr[j & 3]));
            __builtin_amdgcn_sched_barrier(0);
            if (m >= DMA_FIRST && (m - DMA_FIRST) % DMA_STEP == 0) { dma((m - DMA_FIRST) / DMA_STEP); __builtin_amdgcn_sched_barrier(0); }
            ++m;
          }
        }
      }
      static_assert((TH * 9 - 1 - DMA_FIRST) / DMA_STEP + 1 >= C::NPIECES, "every piece of the next item has a slot in the MFMA stream");
    }
  };

  if constexpr (SPLIT) {
    for (int tt = t_begin; tt < t_end; ++tt) {
      const int b = tt / tiles_img, ti = tt - b * tiles_img;
      const int r0 = (ti / tiles_w) * TH, c0 = (ti % tiles_w) * TW;
      __syncthreads();
      // ---- stage dY tile [BM pix][64 cout] and X halo [HP pix][64 cin]
      for (int i = tid; i < BM * 8; i += 256) {
        const int pix = i >> 3, ch = i & 7;
        const int r = r0 + (pix >> 4), c = c0 + (pix & 15);
        const bool ok = r < p.OH && c < p.OW;
        const int off = pix * 128 + sw_piece(pix, ch >> 1) * 32 + (ch & 1) * 16;
        stage_row<T>(DY + (((size_t)b * p.OH + r) * p.OW + c) * p.Cout + co0 + ch * 8, ok, ldsD, C::D_BYTES, off);
      }
      const int iy_base = r0 * S - p.pad, ix_base = c0 * S - p.pad;
      for (int i = tid; i < HP * 8; i += 256) {
        const int pix = i >> 3, ch = i & 7;
        const int hr = pix / HPW, hc = pix - hr * HPW;
        const int iy = iy_base + hr, ix = ix_base + hc;
        const bool ok = iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW;
        const int off = pix * 128 + sw_piece(pix, ch >> 1) * 32 + (ch & 1) * 16;
        stage_row<T>(X + (size_t)b * ximg + (size_t)iy * xrow + (size_t)ix * xpix + ci0 + ch * 8, ok, ldsX, C::X_BYTES, off);
      }
      __syncthreads();
      compute(ldsD, ldsX);
    }
  } else if constexpr (!LEAN) {
    // perf mode: LDS-DMA (global_load_lds_dwordx4) straight from HBM/L2 into the swizzled LDS image.  The LDS
    // destination of one wave-instruction is linear (base + lane*16 = 8 pixel rows), so the XOR swizzle is
    // applied to the per-lane SOURCE chunk instead; out-of-image pixels read a zero page.  Tile t+1 is issued
    // into the other buffer before the MFMAs of tile t and waited for (s_waitcnt vmcnt(0)) only after them, in
    // front of the one barrier per tile.  The DMA is inline asm: with the builtin the compiler orders every
    // ds_read behind an outstanding LDS-DMA ("may alias") and put that vmcnt(0) in FRONT of the MFMA block, i.e.
    // the two buffers never overlapped anything.
    const unsigned lds0 = (unsigned)(size_t)(lds_uchar*)smem;
    constexpr int BUF = C::D_BYTES + C::X_BYTES;
    const unsigned char* zero = reinterpret_cast<const unsigned char*>(p.zeros);
    // Half-pair mode: dz' = dh + dl 2^-11 (times the tensor's power-of-two scale, undone by the reduce kernel), x = xh +
    // xl 2^-11, so dW = sum dh xh + 2^-11 sum (dh xl + dl xh): the chunk's tiles are walked three times - (dh, xl), (dl, xh),
    // then the accumulators are multiplied by 2^-11, then (dh, xh) - as ONE stream of 3 * ntiles items through the same
    // two LDS buffers; a 64-channel block of a pixel record is [hi 64 | lo 64] fp16 (ph_common.h).
    const int nt = t_end > t_begin ? t_end - t_begin : 0;
    const bool hi1 = HPM && p.hp_hi_only;      // PH_PREC_FP16X1: ONE pass, (dz hi, x hi)
    const int nitems = (HPM && !hi1) ? 3 * nt : nt;
    const int dblk = HPM ? (co0 >> 6) * 128 : co0, xblk = HPM ? (ci0 >> 6) * 128 : ci0;
    auto issue = [&](int item, int buf) {
      int pass = 0, tt = t_begin + item;
      if constexpr (HPM) { if (!hi1) { pass = item / nt; tt = t_begin + (item - pass * nt); } else pass = 2; }
      const int dpl = (HPM && pass == 1) ? 64 : 0, xpl = (HPM && pass == 0) ? 64 : 0;     // lo plane of dz' / of x
      const int b = tt / tiles_img, ti = tt - b * tiles_img;
      const int r0 = (ti / tiles_w) * TH, c0 = (ti % tiles_w) * TW;
      unsigned char* dD = smem + buf * BUF;
      unsigned char* dX = dD + C::D_BYTES;
      for (int i0 = wave * 64; i0 < BM * 8; i0 += 256) {
        const int i = i0 + lane, pix = i >> 3, pos = i & 7;
        const int ch = sw_piece(pix, pos >> 1) * 2 + (pos & 1);          // source chunk of this LDS slot
        const int r = r0 + (pix >> 4), c = c0 + (pix & 15);
        const bool ok = r < p.OH && c < p.OW;
        const void* src = ok ? (const void*)(DY + (((size_t)b * p.OH + r) * p.OW + c) * dpix + dblk + dpl + ch * 8)
                             : (const void*)zero;
        lds_dma16(src, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(dD - smem) + i0 * 16));
      }
      const int iy_base = r0 * S - p.pad, ix_base = c0 * S - p.pad;
      for (int i0 = wave * 64; i0 < C::HPP * 8; i0 += 256) {
        const int i = i0 + lane, pix = i >> 3, pos = i & 7;
        const int ch = sw_piece(pix, pos >> 1) * 2 + (pos & 1);
        const int hr = pix / HPW, hc = pix - hr * HPW;
        const int iy = iy_base + hr, ix = ix_base + hc;
        const bool ok = pix < HP && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW;
        const void* src = ok ? (const void*)(X + (size_t)b * ximg + (size_t)iy * xrow + (size_t)ix * xpix + xblk + xpl + ch * 8)
                             : (const void*)zero;
        lds_dma16(src, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(dX - smem) + i0 * 16));
      }
    };
    if (nitems > 0) issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (int it = 0; it < nitems; ++it) {
#ifndef PH_ABL_WG_NODMA   // timing ablation only (garbage results): no operand traffic
      if (it + 1 < nitems) issue(it + 1, buf ^ 1);
#endif
      if constexpr (HPM) {
        if (!hi1 && it == 2 * nt) {      // the cross terms are complete: weight them before the leading products accumulate
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              if constexpr (PIPE) {      // one register at a time through ONE vector register (all 144 at once cost the second wave per SIMD)
                float tmp_;
                asm volatile("v_accvgpr_read_b32 %1, %0\n\ts_nop 4\n\tv_mul_f32 %1, %2, %1\n\ts_nop 4\n\tv_accvgpr_write_b32 %0, %1\n\ts_nop 4"
                             : "+a"(acc[t][q]), "=&v"(tmp_) : "v"(PH_HP_LO_INV));
              } else {
                acc[t][q] *= PH_HP_LO_INV;
              }
            }
        }
      }
      if constexpr (PIPE) compute_p(buf * PBUF);
      else compute(smem + buf * BUF, smem + buf * BUF + C::D_BYTES);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the next item have landed
      __syncthreads();                                    // ... and everybody's; buffer buf is free again
      buf ^= 1;
    }
  } else {
    // perf mode, LEAN: the same LDS image, items, buffers, wait and barrier as above; only HOW a piece's source address is found
    // changes.  Above, every piece of every tile decodes the tile (two integer divisions), its pixel (a division by HPW) and four
    // range compares behind two branches: ~350 executed instructions per tile and wave for 10 LDS-DMAs, in front of the MFMAs, where
    // one wave per SIMD hides none of it.  Here, ONCE per kernel and lane: the byte offset of each of its pieces from the tile's
    // origin (swizzled source chunk included; strides from PhWgrad, so the strided 1 x 1 view works) and a position word (one bit
    // for its tile row, one for its column).  Per tile, wave-uniform (scalar): the two 64-bit origins and a validity word (the
    // rows and columns of the tile inside the image), from (image, tile row, tile column) counters.  Per piece: and + compare of
    // position and validity word, 64-bit add, select of the zero page - 6 vector instructions, no branch.  (No "tile is interior"
    // short cut: at the 64 / 32 / 16 pixel maps of ResNet layers 2 - 4 with pad 1, 20 of 32 / 8 of 8 / 2 of 2 tiles touch a border,
    // and the test would cost a branch to save two instructions per piece.)
    static_assert(BM * 8 % 256 == 0, "whole dz pieces per wave");
    constexpr int NDP = C::NDP, NHP = C::NHP, NPC = C::NPIECES;
    constexpr bool H_TAIL = (C::HPP * 8) % 256 != 0;      // the last halo piece exists for the first waves only
    typedef typename std::conditional<(HPH + HPW < 32), unsigned, unsigned long long>::type hmask_t;
    const unsigned lds0 = (unsigned)(size_t)(lds_uchar*)smem;
    constexpr int BUF = C::D_BYTES + C::X_BYTES;
    const unsigned char* zero = reinterpret_cast<const unsigned char*>(p.zeros);
    const int nt = t_end > t_begin ? t_end - t_begin : 0;
    const bool hi1 = HPM && p.hp_hi_only;
    const int nitems = (HPM && !hi1) ? 3 * nt : nt;      // (half-pair mode: the three passes as ONE item stream, as above)
    const int dblk = HPM ? (co0 >> 6) * 128 : co0, xblk = HPM ? (ci0 >> 6) * 128 : ci0;
    unsigned d_off[NDP], d_pos[NDP], h_off[NHP];
    hmask_t h_pos[NHP];
#pragma unroll
    for (int k = 0; k < NDP; ++k) {
      const int i = wave * 64 + 256 * k + lane, pix = i >> 3, pos = i & 7;
      const int ch = sw_piece(pix, pos >> 1) * 2 + (pos & 1);          // source chunk of this LDS slot
      d_off[k] = (unsigned)((((long)(pix >> 4) * p.OW + (pix & 15)) * dpix + ch * 8) * 2);
      d_pos[k] = (1u << (pix >> 4)) | (1u << (TH + (pix & 15)));
    }
#pragma unroll
    for (int k = 0; k < NHP; ++k) {
      const int i = wave * 64 + 256 * k + lane, pix = i >> 3, pos = i & 7;
      const int ch = sw_piece(pix, pos >> 1) * 2 + (pos & 1);
      const int hr = pix / HPW, hc = pix - hr * HPW;
      const bool in = pix < HP;      // (the pixels that pad the halo to whole pieces are never read: the bit no validity word has)
      h_off[k] = in ? (unsigned)(((long)hr * xrow + (long)hc * xpix + ch * 8) * 2) : 0u;
      h_pos[k] = in ? ((hmask_t)1 << hr) | ((hmask_t)1 << (HPH + hc)) : (hmask_t)1 << (HPH + HPW);
    }
    // tile cursor of the next item to issue: (image, tile row, tile column) counters, the origins kept by ADDING the byte step of a
    // tile column, tile row or image - the two divisions and the 64-bit products run once per kernel (half-pair mode: once per pass)
    typedef const unsigned char* bptr;
    const int b_s = t_begin / tiles_img, ti_s = t_begin - b_s * tiles_img;
    const int trow_s = ti_s / tiles_w, tcol_s = ti_s - trow_s * tiles_w;
    auto d_at = [&](int b, int trow, int tcol) {
      return reinterpret_cast<bptr>(DY) + ((((long)b * p.OH + trow * TH) * p.OW + tcol * TW) * dpix + dblk) * 2;
    };
    auto x_at = [&](int b, int trow, int tcol) {
      return reinterpret_cast<bptr>(X) + ((long)b * ximg + (long)(trow * TH * S - p.pad) * xrow + (long)(tcol * TW * S - p.pad) * xpix + xblk) * 2;
    };
    const long d_col = (long)TW * dpix * 2, d_row = (long)TH * p.OW * dpix * 2, d_img = (long)p.OH * p.OW * dpix * 2;
    const long x_col = (long)TW * S * xpix * 2, x_row = (long)TH * S * xrow * 2, x_img = ximg * 2;
    int crow = trow_s, ccol = tcol_s, cpass = hi1 ? 2 : 0, cleft = nt;
    bptr od, od_r, od_i, ox, ox_r, ox_i;      // origins of the cursor's tile, of its tile row's first tile, of its image's first tile
    unsigned dv_r, dv_c;                      // validity words of the cursor's tile: its row part, its column part
    hmask_t hv_r, hv_c;
    auto span = [](int lo, int hi) -> hmask_t {      // bits lo .. hi - 1
      return hi > lo ? (((hmask_t)1 << hi) - 1) & ~(((hmask_t)1 << lo) - 1) : (hmask_t)0;
    };
    auto row_words = [&]() {
      const int r0 = crow * TH, iy_base = r0 * S - p.pad;
      dv_r = (unsigned)span(0, min(TH, p.OH - r0));
      hv_r = span(max(0, -iy_base), min(HPH, p.IH - iy_base));
    };
    auto col_words = [&]() {
      const int c0 = ccol * TW, ix_base = c0 * S - p.pad;
      dv_c = (unsigned)span(0, min(TW, p.OW - c0)) << TH;
      hv_c = span(max(0, -ix_base), min(HPW, p.IW - ix_base)) << HPH;
    };
    auto to_start = [&]() {
      crow = trow_s; ccol = tcol_s;
      od = d_at(b_s, trow_s, tcol_s); od_r = d_at(b_s, trow_s, 0); od_i = d_at(b_s, 0, 0);
      ox = x_at(b_s, trow_s, tcol_s); ox_r = x_at(b_s, trow_s, 0); ox_i = x_at(b_s, 0, 0);
      row_words();
    };
    to_start();
    col_words();
    bptr nx_d = zero, nx_x = zero;      // origins and validity words of the item being issued
    unsigned nx_dv = 0;
    hmask_t nx_hv = 0;
    auto next_item = [&](const bool have) {      // have = false: no validity bit, every lane reads the zero page (into the free buffer)
      nx_d = od + ((HPM && cpass == 1) ? 128 : 0);      // lo plane of dz' / of x
      nx_x = ox + ((HPM && cpass == 0) ? 128 : 0);
      nx_dv = have ? dv_r | dv_c : 0u;
      nx_hv = have ? hv_r | hv_c : (hmask_t)0;
      ++ccol; od += d_col; ox += x_col;
      if (ccol == tiles_w) {
        ccol = 0; ++crow; od_r += d_row; ox_r += x_row;
        if (crow == tiles_h) { crow = 0; od_i += d_img; ox_i += x_img; od_r = od_i; ox_r = ox_i; }
        od = od_r; ox = ox_r;
        row_words();
      }
      if constexpr (HPM) { if (--cleft == 0) { cleft = nt; ++cpass; to_start(); } }
      col_words();
    };
    unsigned ldst = lds0 + wave * 1024;      // LDS byte address of this wave's first dz piece in the buffer being filled
    auto dma = [&](const int k) __attribute__((always_inline)) {      // piece k: dz pieces first, then the halo's
#ifndef PH_ABL_WG_NODMA   // timing ablation only (garbage results): no operand traffic
      if (k < NDP) {
        const unsigned char* src = (d_pos[k] & nx_dv) == d_pos[k] ? nx_d + d_off[k] : zero;
        lds_dma16(src, ldst + k * 4096);
      } else if (k < NPC) {
        const int e = k - NDP;
        if (H_TAIL && e == NHP - 1 && wave * 64 + 256 * e >= C::HPP * 8) return;      // (wave-uniform)
        const unsigned char* src = (h_pos[e] & nx_hv) == h_pos[e] ? nx_x + h_off[e] : zero;
        lds_dma16(src, ldst + C::D_BYTES + e * 4096);
      }
#endif
    };
    if (nitems > 0) {
      next_item(true);
#pragma unroll
      for (int k = 0; k < NPC; ++k) dma(k);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (int it = 0; it < nitems; ++it) {
      next_item(it + 1 < nitems);
      ldst = lds0 + (buf ^ 1) * BUF + wave * 1024;
      if constexpr (HPM) {
        if (!hi1 && it == 2 * nt) {      // the cross terms are complete: weight them before the leading products accumulate
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              if constexpr (PIPE) {      // (one register at a time, as above)
                float tmp_;
                asm volatile("v_accvgpr_read_b32 %1, %0\n\ts_nop 4\n\tv_mul_f32 %1, %2, %1\n\ts_nop 4\n\tv_accvgpr_write_b32 %0, %1\n\ts_nop 4"
                             : "+a"(acc[t][q]), "=&v"(tmp_) : "v"(PH_HP_LO_INV));
              } else {
                acc[t][q] *= PH_HP_LO_INV;
              }
            }
        }
      }
      // Buffer discipline (unchanged): the pieces of item it + 1 go to buffer buf ^ 1, whose last reads - the fragment reads of item
      // it - 1 - every wave completed before it passed the barrier that ended iteration it - 1 (each read was waited for by the MFMA
      // that consumed it, and all MFMAs precede the barrier).  The fragment reads of item it address bytes [buf * BUF, buf * BUF +
      // BUF) only and the pieces bytes of the other buffer only, so no read of the current buffer can see a piece of the next item,
      // wherever in the MFMA stream it is issued; nobody reads buffer buf ^ 1 before the vmcnt(0) + barrier below.
      if constexpr (PIPE) {
        compute_l(buf * PBUF, dma);
      } else {
        if (it + 1 < nitems) {
#pragma unroll
          for (int k = 0; k < NPC; ++k) dma(k);
        }
        compute(smem + buf * BUF, smem + buf * BUF + C::D_BYTES);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the next item have landed
      __syncthreads();                                    // ... and everybody's; buffer buf is free again
      buf ^= 1;
    }
  }
  // ---- partial slab: acc[t][q] -> row (cout) = (q&3)+8*(q>>2)+4*khalf, col (cin) = lane&31
  float* slab = p.slab + (size_t)chunk * NT * p.Cout * p.Cin;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = co0 + cf * 32 + (q & 3) + 8 * (q >> 2) + 4 * khalf;
      const int col = ci0 + kf * 32 + (lane & 31);
#ifdef PH_ABL_WG_NOSLAB   // timing ablation only
      asm volatile("" ::"v"(acc[t][q]), "v"(row + col));
#else
      if constexpr (PIPE) {      // straight from the accumulation register (copied through vector registers the 144 values cost the
        float* dst = slab + ((size_t)t * p.Cout + row) * p.Cin + col;      // kernel its second wave per SIMD)
        asm volatile("global_store_dword %0, %1, off" : : "v"(dst), "a"(acc[t][q]) : "memory");
      } else {
        slab[((size_t)t * p.Cout + row) * p.Cin + col] = acc[t][q];
      }
#endif
      // (accumulators pinned to AGPRs: one tap's 16 values at a time through the vector registers - hoisted together the 144
      // reads cost the second workgroup of the CU its registers)
      if (PIPE && q == 15) __builtin_amdgcn_sched_barrier(0);
    }
}

// the lean loop keeps a piece's source offset from its tile origin in 32 bits (unsigned): true of every tensor whose rows are
// shorter than ~200 MB; anything else keeps the loop with the 64-bit address arithmetic per piece
template <typename T, int S, int TH, int KS>
bool wg_lean_fits(const PhWgrad& p) {
  using C = WgCfg<T, S, TH, KS>;
  const long EW = C::HPM ? 2 : 1;
  const long xpix = (p.x_pix_stride ? p.x_pix_stride : p.Cin) * EW;
  const long xrow = (p.x_row_stride ? p.x_row_stride : (long)p.IW * p.Cin) * EW;
  const long xmax = ((long)C::HPH * xrow + (long)C::HPW * xpix + 128) * 2;
  const long dmax = (((long)TH * p.OW + C::TW) * p.Cout * EW + 128) * 2;
  return xrow >= 0 && xpix >= 0 && xmax < (1L << 32) && dmax < (1L << 32);
}

template <typename T, int S, int TH, int KS, bool LEAN>
int launch_wg_k(const PhWgrad& p, hipStream_t st) {
  using C = WgCfg<T, S, TH, KS>;
  auto kern = wgrad_kernel<T, S, TH, KS, LEAN>;
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            C::LDS_BYTES) != hipSuccess)
      return PH_ELAUNCH;
    attr_done = true;
  }
  dim3 grid((p.Cout / 64) * (p.Cin / 64), p.nchunks);
  void* tok = nullptr;
  if (ph_prof_on())
    ph_prof_begin2(PH_CLS_WGRAD, 2.0 * p.B * p.OH * p.OW * (double)p.Cout * p.KS * p.KS * p.Cin,
                   ((double)p.B * p.IH * p.IW * p.Cin + (double)p.B * p.OH * p.OW * p.Cout) * sizeof(T) +
                       (double)p.nchunks * p.KS * p.KS * p.Cout * p.Cin * 4.0, st, &tok);   // x + dy once, the fp32 slab
  hipLaunchKernelGGL(kern, grid, dim3(256), C::LDS_BYTES, st, p);
  ph_prof_end(tok, st);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

template <typename T, int S, int TH, int KS>
int launch_wg(const PhWgrad& p, hipStream_t st) {
  if constexpr (!is_f32<T>::value) {
    if (ph_wg_lean_switch(-1) && wg_lean_fits<T, S, TH, KS>(p)) return launch_wg_k<T, S, TH, KS, true>(p, st);
  }
  return launch_wg_k<T, S, TH, KS, false>(p, st);
}

template <typename T>
int launch_wg_T(const PhWgrad& p, hipStream_t st) {
  if (p.S == 1 && p.KS == 3) return launch_wg<T, 1, 8, 3>(p, st);
  if (p.S == 2 && p.KS == 3) return launch_wg<T, 2, 4, 3>(p, st);
  if (p.S == 2 && p.KS == 1) return launch_wg<T, 2, 4, 1>(p, st);
  if (p.S == 1 && p.KS == 1) return launch_wg<T, 1, 8, 1>(p, st);
  return PH_EINVAL;
}

// slab[nchunks][NT][Cout][Cin] -> OIHW.  64 outputs x 4 chunk-lanes per block, 4 independent partial sums per
// thread (loads in flight), fixed summation order (bitwise reproducible)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                           int nchunks, int NT, int Cout, int Cin,
                                                           const float* __restrict__ unscale) {
  const size_t n = (size_t)NT * Cout * Cin;
  const int e = threadIdx.x & 63, cl = threadIdx.x >> 6;
  const size_t i = (size_t)blockIdx.x * 64 + e;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n) {
    int c = cl;
    for (; c + 12 < nchunks; c += 16) {
      s0 += slab[(size_t)c * n + i];
      s1 += slab[(size_t)(c + 4) * n + i];
      s2 += slab[(size_t)(c + 8) * n + i];
      s3 += slab[(size_t)(c + 12) * n + i];
    }
    for (; c < nchunks; c += 4) s0 += slab[(size_t)c * n + i];
  }
  __shared__ float sh[4][64];
  sh[cl][e] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (cl == 0 && i < n) {
    float s = (sh[0][e] + sh[1][e]) + (sh[2][e] + sh[3][e]);
    if (unscale) s *= unscale[1];      // (power of two: exact)
    const int ci = i % Cin;
    const int co = (i / Cin) % Cout;
    const int t = i / ((size_t)Cin * Cout);
    dw[((size_t)co * Cin + ci) * NT + t] = s;
  }
}

}  // namespace

int ph_wgrad_tile_h(int S) { return S == 1 ? 8 : 4; }

int ph_wgrad_launch(const PhWgrad* p, int prec, hipStream_t st) {
  if (p->Cin % 64 || p->Cout % 64 || p->nchunks < 1) return PH_EINVAL;
  if (prec == PH_PREC_BF16) { ph_dispatch_note(PH_DK_WGRAD_BF16); return launch_wg_T<bf16>(*p, st); }
  if (prec == PH_PREC_FP16X3 || prec == PH_PREC_FP16X1) {
    PhWgrad q = *p;
    q.hp_hi_only = prec == PH_PREC_FP16X1;
    ph_dispatch_note(PH_DK_WGRAD_HP16);
    return launch_wg_T<hp16>(q, st);
  }
  if (PH_IS_SPLIT_PREC(prec)) {
    PhWgrad q = *p;
    q.prod6 = prec == PH_PREC_BF16X6;
    ph_dispatch_note(PH_DK_WGRAD_F32);
    return launch_wg_T<float>(q, st);
  }
  return PH_EINVAL;
}

int ph_wgrad_reduce_launch(const float* slab, float* dw, int nchunks, int KS, int Cout, int Cin, const float* unscale,
                           hipStream_t st) {
  const size_t n = (size_t)KS * KS * Cout * Cin;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, slab, dw, nchunks,
                     KS * KS, Cout, Cin, unscale);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

// The nine-set weight window of the register-window kernels (conv_tap6.hip, conv_tap6b.hip, conv_tap7.hip): the fragment registers,
// the MFMA / LDS-read / weight-load macros, the MFMA group and the groups of a tap that are the same in all three.  A kernel file
// keeps what differs: its Cfg and tables, the waits and their skip conditions, the piece-mask bookkeeping, the hand-over condition
// and its PHn_DMA.  (conv_tap5.hip's window has another shape - fb[SET][KS][N], three taps ahead, a scalar base - and keeps its own.)
//
// The including file names two things first:
//   #define PHW_MFMA v_mfma_f32_16x16x32_bf16      the MFMA mnemonic
//   #define PHW_DBG PH7_DBG                        its ablation flag (timing builds): 2 = no image pieces (the kernel's PHn_DMA tests
//                                                  it), 4 = no weight loads inside the taps
// The macros name the kernel's locals: smem, C::ROW_BYTES, NN, acc[NM][NN], the per-lane fragment bases ab0 / ab1[buffer][dx] (k-step
// 0 / its k-step-1 twin), and inside a tap `first` (the tap opens a tile: its first k-step writes the accumulators).
#pragma once
#include "tap_common.h"
#if !defined(PHW_MFMA) || !defined(PHW_DBG)
#error "define PHW_MFMA and PHW_DBG before including tap_window.h"
#endif
#define PHW_STR_(X) #X
#define PHW_STR(X) PHW_STR_(X)

// Fragment registers: A ring of 4; B NINE k-step sets (4 N tiles each) - k-step j of the stream multiplies set j % 9 (54 k-steps
// per group in conv_tap6.hip, 18 per slice in the other two - multiples of 9: the assignment is the same in every group or slice)
// while the fragments of k-step j + 8 are loaded into set (j + 8) % 9, the one k-step j - 1 has just used: weights run FOUR taps ahead
// of the MFMAs.  That distance is what lets image pieces stay in flight: loads return in order, so a piece must have landed when a
// weight load issued after it is waited for - with a window of three taps (conv_tap5.hip) that is 2.5 taps after its issue, and
// conv_tap6.hip moves 2.6 x the image bytes per MFMA of the dense kernel (its first version: 1.6 us per tap, all of it waiting for
// pieces); in conv_tap7.hip a piece may stay in flight for 4.5 taps.  Sets 0..5 live in accumulation registers, 6..8 in vector registers.
#define PHW_FRAGMENTS u32x4 fa[4], fba[6][NN], fbv[3][NN]
// sets of tap S (stream position; two k-steps KS = 0, 1 per tap): the one its MFMAs read, the one loaded meanwhile (tap S + 4, same k-step)
#define PHW_SET(S, KS) ((2 * (S) + (KS)) % 9)
#define PHW_SET_LD(S, KS) ((2 * (S) + (KS) + 8) % 9)

#define PHW_MM(M, N, AI, Q, FIRST)                                                                                                                 \
  do {                                                                                                                                             \
    if ((Q) < 6) {                                                                                                                                 \
      if (FIRST) asm volatile(PHW_STR(PHW_MFMA) " %0, %1, %2, 0" : "=&a"(acc[M][N]) : "v"(fa[AI]), "a"(fba[(Q) < 6 ? (Q) : 0][N]));                \
      else asm volatile(PHW_STR(PHW_MFMA) " %0, %1, %2, %0" : "+a"(acc[M][N]) : "v"(fa[AI]), "a"(fba[(Q) < 6 ? (Q) : 0][N]));                      \
    } else {                                                                                                                                       \
      if (FIRST) asm volatile(PHW_STR(PHW_MFMA) " %0, %1, %2, 0" : "=&a"(acc[M][N]) : "v"(fa[AI]), "v"(fbv[(Q) >= 6 ? (Q) - 6 : 0][N]));           \
      else asm volatile(PHW_STR(PHW_MFMA) " %0, %1, %2, %0" : "+a"(acc[M][N]) : "v"(fa[AI]), "v"(fbv[(Q) >= 6 ? (Q) - 6 : 0][N]));                 \
    }                                                                                                                                              \
  } while (0)
#define PHW_LD(ADDR, IMM) (*reinterpret_cast<const u32x4*>(smem + (ADDR) + (IMM)))
#define PHW_LDA(AB, AOFF, MT) PHW_LD(AB, (AOFF) + (MT) * C::ROW_BYTES)
// weight fragment N of a k-step -> set Q.  WB: the lane's address of its 16 bytes of the tap's fragment (0, 0), + 4 KiB; OFF: literal
// byte offset (4 ks + N) KiB - 4 KiB, so the eight fragments of a tap are the immediates -4096 .. 3072.
// (WB is a per-lane 64-bit address, no scalar operand: a scalar base restored by v_readlane right in front of inline assembly needs
// wait states the hazard recognizer does not insert - conv_tap5.hip copies it with s_mov_b64 in front of every load; here ONE vector
// add per tap makes the address and the eight loads carry nothing but an immediate)
#define PHW_BLD(Q, N, WB, OFF)                                                                                             \
  do {                                                                                                                     \
    if ((Q) < 6) asm volatile("global_load_dwordx4 %0, %1, off offset:" #OFF : "=a"(fba[(Q) < 6 ? (Q) : 0][N]) : "v"(WB) : "memory");     \
    else asm volatile("global_load_dwordx4 %0, %1, off offset:" #OFF : "=v"(fbv[(Q) >= 6 ? (Q) - 6 : 0][N]) : "v"(WB) : "memory");       \
  } while (0)
// fragment N (= the MFMA group that issues it) of k-step KS of the tap at WB
#define PHW_BLD_KN(Q, KS, N, WB)                                     \
  do {                                                               \
    if (PHW_DBG & 4) break;                                          \
    if ((KS) == 0) {                                                 \
      if ((N) == 0) PHW_BLD(Q, 0, WB, -4096);                        \
      else if ((N) == 1) PHW_BLD(Q, 1, WB, -3072);                   \
      else if ((N) == 2) PHW_BLD(Q, 2, WB, -2048);                   \
      else PHW_BLD(Q, 3, WB, -1024);                                 \
    } else {                                                         \
      if ((N) == 0) PHW_BLD(Q, 0, WB, 0);                            \
      else if ((N) == 1) PHW_BLD(Q, 1, WB, 1024);                    \
      else if ((N) == 2) PHW_BLD(Q, 2, WB, 2048);                    \
      else PHW_BLD(Q, 3, WB, 3072);                                  \
    }                                                                \
  } while (0)
// prologue: the eight fragments of stream taps 0..3 into sets 0..7 (set 8 is first loaded by tap 0's k-step 0)
#define PHW_BLD_TAP(Q, WB)                                                                                               \
  PHW_BLD(Q, 0, WB, -4096); PHW_BLD(Q, 1, WB, -3072); PHW_BLD(Q, 2, WB, -2048); PHW_BLD(Q, 3, WB, -1024);               \
  PHW_BLD((Q) + 1, 0, WB, 0); PHW_BLD((Q) + 1, 1, WB, 1024); PHW_BLD((Q) + 1, 2, WB, 2048); PHW_BLD((Q) + 1, 3, WB, 3072)
#define PHW_PROLOGUE_LOADS(WB0, WB1, WB2, WB3) \
  PHW_BLD_TAP(0, WB0); PHW_BLD_TAP(2, WB1); PHW_BLD_TAP(4, WB2); PHW_BLD_TAP(6, WB3)

// One MFMA group: the four MFMAs of M tile M (A fragment fa[M & 3]) against set Q, each followed by one issue slot - RA: the LDS read
// of the A fragment three groups ahead, X1: a weight load, X2: an image piece - and a scheduling barrier that keeps the slot where it is.
#define PHW_GROUP(M, Q, KS, RA, X1, X2)                            \
  PHW_MM(M, 0, (M) & 3, Q, first && (KS) == 0); RA; PH_SB();       \
  PHW_MM(M, 1, (M) & 3, Q, first && (KS) == 0); X1; PH_SB();       \
  PHW_MM(M, 2, (M) & 3, Q, first && (KS) == 0); PH_SB();           \
  PHW_MM(M, 3, (M) & 3, Q, first && (KS) == 0); X2; PH_SB()

// ---- the groups of tap S that are the same in every kernel.  BUF, DX, AOFF: the tap's image buffer, its column shift and the byte
// offset of its row shift; WB: PHW_BLD's base for stream tap S + 4.  Between these three a kernel places its waits, its mask
// bookkeeping and its hand-over.
// k-step 0 (chunks lg): A tile m + 3 is read by group m, the last three groups read tiles 0..2 of k-step 1 (chunks lg + 4: ab1);
// groups 0..3 load the four fragments of tap S + 4's k-step 0
#define PHW_TAP_K0(S, BUF, DX, AOFF, WB)                                                                                       \
  PHW_GROUP(0, PHW_SET(S, 0), 0, fa[3] = PHW_LDA(ab0[BUF][DX], AOFF, 3), PHW_BLD_KN(PHW_SET_LD(S, 0), 0, 0, WB), PH_NOP);      \
  PHW_GROUP(1, PHW_SET(S, 0), 0, fa[0] = PHW_LDA(ab0[BUF][DX], AOFF, 4), PHW_BLD_KN(PHW_SET_LD(S, 0), 0, 1, WB), PH_NOP);      \
  PHW_GROUP(2, PHW_SET(S, 0), 0, fa[1] = PHW_LDA(ab0[BUF][DX], AOFF, 5), PHW_BLD_KN(PHW_SET_LD(S, 0), 0, 2, WB), PH_NOP);      \
  PHW_GROUP(3, PHW_SET(S, 0), 0, fa[2] = PHW_LDA(ab0[BUF][DX], AOFF, 6), PHW_BLD_KN(PHW_SET_LD(S, 0), 0, 3, WB), PH_NOP);      \
  PHW_GROUP(4, PHW_SET(S, 0), 0, fa[3] = PHW_LDA(ab0[BUF][DX], AOFF, 7), PH_NOP, PH_NOP);                                      \
  PHW_GROUP(5, PHW_SET(S, 0), 0, fa[0] = PHW_LDA(ab1[BUF][DX], AOFF, 0), PH_NOP, PH_NOP);                                      \
  PHW_GROUP(6, PHW_SET(S, 0), 0, fa[1] = PHW_LDA(ab1[BUF][DX], AOFF, 1), PH_NOP, PH_NOP);                                      \
  PHW_GROUP(7, PHW_SET(S, 0), 0, fa[2] = PHW_LDA(ab1[BUF][DX], AOFF, 2), PH_NOP, PH_NOP)
// k-step 1, groups 0..4: the four fragments of tap S + 4's k-step 1; D0..D4: the kernel's image-piece slots (PHn_DMA(i) or PH_NOP)
#define PHW_TAP_K1(S, BUF, DX, AOFF, WB, D0, D1, D2, D3, D4)                                                                   \
  PHW_GROUP(0, PHW_SET(S, 1), 1, fa[3] = PHW_LDA(ab1[BUF][DX], AOFF, 3), PHW_BLD_KN(PHW_SET_LD(S, 1), 1, 0, WB), D0);          \
  PHW_GROUP(1, PHW_SET(S, 1), 1, fa[0] = PHW_LDA(ab1[BUF][DX], AOFF, 4), PHW_BLD_KN(PHW_SET_LD(S, 1), 1, 1, WB), D1);          \
  PHW_GROUP(2, PHW_SET(S, 1), 1, fa[1] = PHW_LDA(ab1[BUF][DX], AOFF, 5), PHW_BLD_KN(PHW_SET_LD(S, 1), 1, 2, WB), D2);          \
  PHW_GROUP(3, PHW_SET(S, 1), 1, fa[2] = PHW_LDA(ab1[BUF][DX], AOFF, 6), PHW_BLD_KN(PHW_SET_LD(S, 1), 1, 3, WB), D3);          \
  PHW_GROUP(4, PHW_SET(S, 1), 1, fa[3] = PHW_LDA(ab1[BUF][DX], AOFF, 7), PH_NOP, D4)
// k-step 1, groups 5..7, behind the hand-over: they read A tiles 0..2 of the NEXT tap (BUFN, DXN, AOFFN: possibly the next image)
#define PHW_TAP_K1_NEXT(S, BUFN, DXN, AOFFN)                                                                                   \
  PHW_GROUP(5, PHW_SET(S, 1), 1, fa[0] = PHW_LDA(ab0[BUFN][DXN], AOFFN, 0), PH_NOP, PH_NOP);                                   \
  PHW_GROUP(6, PHW_SET(S, 1), 1, fa[1] = PHW_LDA(ab0[BUFN][DXN], AOFFN, 1), PH_NOP, PH_NOP);                                   \
  PHW_GROUP(7, PHW_SET(S, 1), 1, fa[2] = PHW_LDA(ab0[BUFN][DXN], AOFFN, 2), PH_NOP, PH_NOP)

// The stem's dz - the gradient at the 7x7 / stride-2 conv output, through max-pool, ReLU and BatchNorm (training statistics) -
// per ELEMENT: one expression for the pass that writes the tensor (stem_bwd_kernel, bn_act.hip) and for the weight-gradient
// kernel that forms its dz tile in LDS (stem_wgrad_kernel<bf16, true>, conv_stem.hip).  Both call these helpers, so the compiler sees
// the same operations with the same contraction in both and the two paths give bitwise the same values.
#pragma once
#include "ph_common.h"

// Pixel (h, w) of the conv output lies in up to four 3x3 / stride-2 / pad-1 pooling windows, q = a * 2 + c with pooled row
// a ? (h + 1) >> 1 : h >> 1 and pooled column c ? (w + 1) >> 1 : w >> 1.  g[q]: that window's gradient, hit[q]: the window
// exists (distinct, inside the pooled image) and its arg-max code names this pixel.  Sum in the order q = 0 .. 3, then the
// ReLU mask re-derived from the conv output y.
__device__ __forceinline__ float stem_dz_masked(const float (&g)[4], const bool (&hit)[4], float y, float sc, float sf) {
  float dz = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) dz += hit[q] ? g[q] : 0.f;
  return (y * sc + sf) > 0.f ? dz : 0.f;
}

__device__ __forceinline__ float stem_xhat(float y, float mu, float is) { return (y - mu) * is; }

// ... and BatchNorm backward: ga = gamma * invstd, k1 / k2 = the two batch means of bn_bwd_finalize, dsc = the power-of-two
// scale of a half-pair dz tensor (1 elsewhere: exact)
__device__ __forceinline__ float stem_dz_value(const float (&g)[4], const bool (&hit)[4], float y, float sc, float sf, float mu,
                                               float is, float ga, float k1, float k2, float dsc) {
  const float dz = stem_dz_masked(g, hit, y, sc, sf);
  const float xh = stem_xhat(y, mu, is);
  return ga * (dz - k1 - xh * k2) * dsc;
}

// the arg code window (ph, pw) stores for pixel (h, w): row-major position inside the 3 x 3 window whose origin is (2 ph - 1, 2 pw - 1)
__device__ __forceinline__ unsigned stem_arg_code(int h, int w, int ph, int pw) {
  return (unsigned)((h - (2 * ph - 1)) * 3 + (w - (2 * pw - 1)));
}

// Host side of the tap convolutions (no device code): the kernel selector every caller reads, the A/B switches it alone consults,
// and the descriptor builders shared by the convolution entry points (c_api.hip) and the ResNet plan (resnet_plan.hip).
#include <algorithm>
#include "ph_common.h"
#include "ph_kernels.h"

// A/B and test switches between kernel generations (same-box A/B; the tests use them as second opinions).  Off = the family
// falls back: PH_TAP3 -> conv_tap2.hip <2,2,4> (half-pair: first generation), PH_TAP4 -> tapconv2_l1_kernel, PH_TAP7 -> conv_tap3.hip,
// PH_TAP6B -> the masked grid, PH_TAP5 / PH_TAP6 -> row-major weights and the first generation (read when the weights are packed)
PH_SWITCH(tap3, "PH_TAP3")
PH_SWITCH(tap4, "PH_TAP4")
PH_SWITCH(tap5, "PH_TAP5")
PH_SWITCH(tap6, "PH_TAP6")
PH_SWITCH(tap6b, "PH_TAP6B")
PH_SWITCH(tap7, "PH_TAP7")

namespace {
// rows of the first-generation kernel: one per (image, tile); tile heights of launch_T's configurations (conv_tap.hip)
int gen1_parts(const PhTapConv* p, int S, int prec) {
  const bool split = PH_IS_SPLIT_PREC(prec);
  const int TH = S == 1 ? ((split && p->Cout % 128 == 0) ? 8 : 16) : (split ? 2 : 8);
  return p->B * cdiv(p->OHt, TH) * cdiv(p->OWt, 16);
}
}  // namespace

PhConvChoice ph_tapconv_select(const PhTapConv* p, int S, int prec) {
  const PhConvChoice reject{PH_CK_REJECT, 0, PH_WFRAG_ROW};
  if (p->Cin % 64 || p->Cout % 64 || p->ntaps < 1 || p->ntaps > 9 || (S != 1 && S != 2)) return reject;
  const bool hp = prec == PH_PREC_FP16X3 || prec == PH_PREC_FP16X1;
  if (prec != PH_PREC_BF16 && !hp && !PH_IS_SPLIT_PREC(prec)) return reject;
  // perf mode, 3x3 / stride 2 forward over the un-masked descriptor: conv_tap6b.hip
  if (S == 2 && prec == PH_PREC_BF16 && !p->no_tap6b && ph_tap6b_switch(-1) && ph_tapconv6b_eligible(p))
    return {PH_CK_TAP6B, ph_tapconv6b_stat_parts(p), PH_WFRAG_ROW};
  // perf mode, 3x3 stride-1 grids: the persistent kernels, one row per workgroup
  if (ph_tapconv2_tile_h(p, S, prec)) {
    if (p->in_scale && (!p->in_shift || p->Cin > 512)) return reject;
    int k;
    if (p->m_groups) {
      if (p->Cout % 128 || p->in_scale) return reject;
      k = PH_CK_TAP2_MASKED;
    } else if (p->Cout % 128 == 0) {
      // (conv_tap7.hip: every form but the in-LDS input BatchNorm, Cin = Cout; same outputs as conv_tap3.hip)
      if (ph_tap3_switch(-1) && ph_tapconv3_eligible(p)) k = ph_tap7_switch(-1) && ph_tapconv7_eligible(p) ? PH_CK_TAP7 : PH_CK_TAP3;
      else k = PH_CK_TAP2;
    } else {
      k = ph_tap4_switch(-1) && ph_tapconv4_eligible(p) ? PH_CK_TAP4 : PH_CK_TAP2_L1;
    }
    // (the fused BatchNorm-backward sums exist in conv_tap3.hip / conv_tap4.hip / conv_tap7.hip only)
    if (p->bst_y && (k == PH_CK_TAP2 || k == PH_CK_TAP2_L1)) return reject;
    return {k, ph_tapconv2_stat_parts(p), PH_WFRAG_ROW};
  }
  if (p->in_scale || p->m_groups) return reject;   // in-LDS BatchNorm + ReLU / masked tap grids: those kernels only
  if (hp) {
    // the fragment-major layouts: their kernels alone read them, and read nothing else
    if (p->w_frag == PH_WFRAG_TAP5)   // dense 3x3 stride-1, Cin = Cout = 64 (layer 1)
      return S == 1 && ph_tapconv5_eligible(p) ? PhConvChoice{PH_CK_TAP5, ph_tapconv5_stat_parts(p), PH_WFRAG_TAP5} : reject;
    if (p->w_frag == PH_WFRAG_TAP6)   // 3x3 / stride 2 forward (layers 2-4 conv1)
      return S == 2 && prec == PH_PREC_FP16X3 && ph_tapconv6_eligible(p) ? PhConvChoice{PH_CK_TAP6, ph_tapconv6_stat_parts(p), PH_WFRAG_TAP6}
                                                                         : reject;
    if (p->w_frag != PH_WFRAG_ROW) return reject;
    // dense 3x3 stride-1, Cout % 128 == 0: the third-generation kernel's half-pair form
    if (S == 1 && ph_tap3_switch(-1) && ph_tapconv3_eligible(p)) return {PH_CK_TAP3_HP, ph_tapconv2_stat_parts(p), PH_WFRAG_ROW};
  }
  // first generation.  Stride 2: 128-wide channel tiles only; merged output-parity classes: stride 1, no statistics
  if (S == 2 && p->Cout % 128) return reject;
  if (p->ncls && (S != 1 || p->ncls < 2 || p->ncls > 4 || p->stats)) return reject;
  return {prec == PH_PREC_BF16 ? PH_CK_GEN1_BF16 : (hp ? PH_CK_GEN1_HP16 : PH_CK_GEN1_F32), gen1_parts(p, S, prec), PH_WFRAG_ROW};
}

int ph_tapconv_stat_parts_bound(int B, int OH, int OW, int Cout, int S, int prec) {
  PhTapConv t{};      // (the row counts need B / OHt / OWt / Cout only)
  t.B = B; t.OHt = OH; t.OWt = OW; t.Cout = Cout;
  const bool hp = prec == PH_PREC_FP16X3 || prec == PH_PREC_FP16X1;
  int n = gen1_parts(&t, S, prec);
  if (S == 1 && (prec == PH_PREC_BF16 || hp) && Cout <= 512 && (Cout % 128 == 0 || (Cout == 64 && !hp)))
    n = std::max(n, ph_tapconv2_stat_parts(&t));      // conv_tap2 / 3 / 4 / 7
  if (S == 1 && hp && Cout == 64) n = std::max(n, ph_tapconv5_stat_parts(&t));
  // (two rows per workgroup; not while switched off - buffers are sized as before, so do not switch them on under a live plan)
  if (S == 2 && prec == PH_PREC_BF16 && Cout % 128 == 0 && ph_tap6b_switch(-1)) n = std::max(n, ph_tapconv6b_stat_parts(&t));
  if (S == 2 && prec == PH_PREC_FP16X3 && Cout % 128 == 0 && ph_tap6_switch(-1)) n = std::max(n, ph_tapconv6_stat_parts(&t));
  return n;
}

int ph_tapconv_hp_wfrag(const PhTapConv* p, int S, int prec) {
  if (prec != PH_PREC_FP16X3 && prec != PH_PREC_FP16X1) return PH_WFRAG_ROW;
  PhTapConv q = *p;
  q.w_frag = S == 1 ? PH_WFRAG_TAP5 : PH_WFRAG_TAP6;
  if (!(S == 1 ? ph_tap5_switch(-1) : ph_tap6_switch(-1))) return PH_WFRAG_ROW;
  return ph_tapconv_select(&q, S, prec).kernel != PH_CK_REJECT ? q.w_frag : PH_WFRAG_ROW;
}

bool ph_tapconv_needs_frag_copy(const PhTapConv* p, int S, int prec) {
  const int k = ph_tapconv_select(p, S, prec).kernel;
  return k == PH_CK_TAP7 || k == PH_CK_TAP6B;
}

// ---- descriptor builders

void ph_conv_fwd_geometry(PhTapConv* t, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad) {
  t->IH = IH; t->IW = IW; t->Cin = Cin; t->Cout = Cout;
  t->OH = (IH + 2 * pad - KS) / stride + 1; t->OW = (IW + 2 * pad - KS) / stride + 1;
  t->OHt = t->OH; t->OWt = t->OW; t->os = 1; t->oa_h = 0; t->oa_w = 0;
  t->iy0 = -pad; t->ix0 = -pad; t->ntaps = KS * KS;
  for (int k = 0; k < t->ntaps; ++k) { t->dy[k] = k / KS; t->dx[k] = k % KS; t->wtap[k] = k; }
}

int ph_conv_fwd_route(PhTapConv* t, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad, int prec, int no_masked) {
  t->no_tap6b = no_masked;
  if (KS == 1 && stride == 2) {   // 1x1 / stride 2 == 1x1 / stride 1 over the even-pixel view of the input (no wasted halo pixels)
    t->in_pix_stride = 2L * Cin; t->in_row_stride = 2L * IW * Cin; t->in_img_stride = (long)IH * IW * Cin;
    t->IH = t->OH; t->IW = t->OW;
    return 1;
  }
  if (KS == 3 && stride == 2 && pad == 1 && !no_masked && ph_tapconv_select(t, 2, prec).kernel != PH_CK_TAP6B &&
      ph_tapconv2_setup_s2_fwd(t, Cin, Cout, IH, IW, prec))
    return 1;      // a stride-1 MASKED tap grid over the four pixel-parity planes of the input
  return stride;
}

void ph_conv_dgrad_s1_geometry(PhTapConv* t, int Cin, int IH, int IW, int Cout, int KS, int pad) {
  t->IH = (IH + 2 * pad - KS) + 1; t->IW = (IW + 2 * pad - KS) + 1; t->Cin = Cout; t->Cout = Cin;
  t->OH = IH; t->OW = IW; t->OHt = IH; t->OWt = IW; t->os = 1; t->oa_h = 0; t->oa_w = 0;
  t->iy0 = -(KS - 1 - pad); t->ix0 = t->iy0; t->ntaps = KS * KS;
  for (int k = 0; k < t->ntaps; ++k) { t->dy[k] = k / KS; t->dx[k] = k % KS; t->wtap[k] = (KS - 1 - k / KS) * KS + (KS - 1 - k % KS); }
}

int ph_conv_dgrad_s2_classes(const PhTapConv* t, int Cin, int IH, int IW, int Cout, int KS, int pad, PhTapConv cls[4], int* ncls,
                             bool* tapless) {
  *ncls = 0; *tapless = false;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      int nk = 0, khs[3], dhs[3], nw = 0, kws[3], dws[3];
      for (int kh = 0; kh < KS; ++kh)
        if (((a + pad - kh) & 1) == 0) { khs[nk] = kh; dhs[nk] = (a + pad - kh) / 2; ++nk; }
      for (int kw = 0; kw < KS; ++kw)
        if (((b + pad - kw) & 1) == 0) { kws[nw] = kw; dws[nw] = (b + pad - kw) / 2; ++nw; }
      PhTapConv c = *t;
      c.IH = (IH + 2 * pad - KS) / 2 + 1; c.IW = (IW + 2 * pad - KS) / 2 + 1; c.Cin = Cout; c.Cout = Cin; c.OH = IH; c.OW = IW;
      c.OHt = (IH - a + 1) / 2; c.OWt = (IW - b + 1) / 2;
      if (c.OHt <= 0 || c.OWt <= 0) continue;
      c.os = 2; c.oa_h = a; c.oa_w = b; c.iy0 = 0; c.ix0 = 0; c.ntaps = nk * nw;
      if (c.ntaps == 0) { *tapless = true; continue; }      // (1x1: the gradient is zero there)
      int q = 0;
      for (int i = 0; i < nk; ++i)
        for (int j = 0; j < nw; ++j) {
          if (dhs[i] < 0 || dws[j] < 0 || dhs[i] > 2 || dws[j] > 2) return PH_EINVAL;
          c.dy[q] = dhs[i]; c.dx[q] = dws[j]; c.wtap[q] = khs[i] * KS + kws[j]; ++q;
        }
      cls[(*ncls)++] = c;
    }
  return PH_OK;
}

int ph_conv_dgrad_s2_merge(const PhTapConv cls[4], int ncls, int KS, PhTapConv* m, bool taken[4]) {
  PhTapConv& mt = *m;
  mt = cls[0];
  mt.ncls = 0;
  for (int i = 0; i < ncls; ++i) {
    const PhTapConv& q = cls[i];
    taken[i] = KS == 3 && q.ntaps <= 4 && mt.ncls < 4;
    if (!taken[i]) continue;
    const int k = mt.ncls++;
    mt.c_ntaps[k] = q.ntaps; mt.c_oa_h[k] = q.oa_h; mt.c_oa_w[k] = q.oa_w; mt.c_OHt[k] = q.OHt; mt.c_OWt[k] = q.OWt;
    for (int e = 0; e < q.ntaps; ++e) { mt.c_dy[k][e] = q.dy[e]; mt.c_dx[k][e] = q.dx[e]; mt.c_wtap[k][e] = q.wtap[e]; }
    for (int e = q.ntaps; e < 4; ++e) { mt.c_dy[k][e] = 0; mt.c_dx[k][e] = 0; mt.c_wtap[k][e] = 0; }
    // the descriptor's own fields: the largest class (grid extent; profiler)
    if (k == 0 || q.OHt * q.OWt > mt.OHt * mt.OWt) { mt.OHt = q.OHt; mt.OWt = q.OWt; }
    if (k == 0 || q.ntaps > mt.ntaps) {
      mt.ntaps = q.ntaps;
      for (int e = 0; e < q.ntaps; ++e) { mt.dy[e] = q.dy[e]; mt.dx[e] = q.dx[e]; mt.wtap[e] = q.wtap[e]; }
    }
    mt.os = 2; mt.oa_h = 0; mt.oa_w = 0; mt.iy0 = 0; mt.ix0 = 0;
  }
  if (mt.ncls == 1) {      // (a single class that qualified: an ordinary launch)
    mt.ncls = 0;
    mt.ntaps = mt.c_ntaps[0]; mt.oa_h = mt.c_oa_h[0]; mt.oa_w = mt.c_oa_w[0]; mt.OHt = mt.c_OHt[0]; mt.OWt = mt.c_OWt[0];
    for (int e = 0; e < mt.ntaps; ++e) { mt.dy[e] = mt.c_dy[0][e]; mt.dx[e] = mt.c_dx[0][e]; mt.wtap[e] = mt.c_wtap[0][e]; }
    return 1;
  }
  return mt.ncls;
}

void ph_conv_wgrad_geometry(PhWgrad* w, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad) {
  w->IH = IH; w->IW = IW; w->Cin = Cin; w->Cout = Cout;
  w->OH = (IH + 2 * pad - KS) / stride + 1; w->OW = (IW + 2 * pad - KS) / stride + 1;
  w->S = stride; w->pad = pad; w->KS = KS;
  if (KS == 1 && stride == 2) {   // strided view, as in ph_conv_fwd_route
    w->x_pix_stride = 2L * Cin; w->x_row_stride = 2L * IW * Cin; w->x_img_stride = (long)IH * IW * Cin;
    w->IH = w->OH; w->IW = w->OW; w->S = 1;
  }
}

int ph_wgrad_chunks(const PhWgrad* w, int B, int wg_want, int* tiles_per_chunk) {
  const int th = ph_wgrad_tile_h(w->S);
  const int ntiles = B * cdiv(w->OH, th) * cdiv(w->OW, 16);
  const int blocks = (w->Cout / 64) * (w->Cin / 64);
  int want = cdiv(wg_want, blocks);
  if (want > ntiles) want = ntiles;
  if (want < 1) want = 1;
  *tiles_per_chunk = cdiv(ntiles, want);
  return cdiv(ntiles, *tiles_per_chunk);
}

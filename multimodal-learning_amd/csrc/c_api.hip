// Fine-grained convolution entry points of the C-ABI (used by the parity tests to pin each MFMA kernel
// against the oracle's F.conv2d) + ABI version.
#include <algorithm>
#include "ph_common.h"
#include "ph_kernels.h"
#include "ph_dense.h"

namespace {
constexpr size_t AL = 256;
inline size_t up(size_t x) { return (x + AL - 1) / AL * AL; }

__global__ void parts_sum_kernel(const float* __restrict__ parts, int nparts, int C, float* s1, float* s2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < nparts; ++p) { a += parts[((size_t)p * 2) * C + c]; b += parts[((size_t)p * 2 + 1) * C + c]; }
  if (s1) s1[c] = (float)a;
  if (s2) s2[c] = (float)b;
}

__global__ void parts3_sum_kernel(const float* __restrict__ parts, int nparts, int C, float* __restrict__ sums) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a[3] = {0.0, 0.0, 0.0};
  for (int p = 0; p < nparts; ++p)
    for (int k = 0; k < 3; ++k) a[k] += parts[((size_t)p * 3 + k) * C + c];
  for (int k = 0; k < 3; ++k) sums[(size_t)k * C + c] = (float)a[k];
}

// fp32 <-> half-pair tensors (ph_common.h), 8 channels per thread
__global__ void hp_pack_kernel(const float* __restrict__ src, hp16* __restrict__ dst, size_t n8, float scale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float v[8];
  load8(src + i * 8, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] *= scale;
  store8(dst + i * 8, v);
}
__global__ void hp_unpack_kernel(const hp16* __restrict__ src, float* __restrict__ dst, size_t n8) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float v[8];
  load8(src + i * 8, v);
  store8(dst + i * 8, v);
}

// the geometries the convolution entry points accept: KS 3 at pad 1 (stride 1 or 2) or pad 0 (stride 1 only: a stride-2 dgrad
// at pad 0 would need taps before the first dy row), KS 1 at pad 0 (stride 1 or 2: the stride-2 view starts at pixel 0),
// channel counts multiples of 64, a non-empty output.  Everything else is PH_EINVAL before anything is written.
bool geometry_ok(int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad) {
  if (B < 1 || Cin < 64 || Cout < 64 || Cin % 64 || Cout % 64 || (stride != 1 && stride != 2)) return false;
  if (KS == 1 ? pad != 0 : (KS != 3 || !(pad == 1 || (pad == 0 && stride == 1)))) return false;
  return IH + 2 * pad >= KS && IW + 2 * pad >= KS;
}

struct Conv { int B, Cin, IH, IW, Cout, KS, stride, pad; };

// the weight-gradient launch of convolution v: geometry and chunking of descriptor g (tensors are the caller's); returns the chunks
int plan_wgrad(const Conv& v, PhWgrad* g) {
  g->B = v.B;
  ph_conv_wgrad_geometry(g, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.stride, v.pad);
  return g->nchunks = ph_wgrad_chunks(g, v.B, PH_WG_WANT_ALONE, &g->tiles_per_chunk);
}
}  // namespace

int ph_abi_version(void) { return 1; }

size_t ph_conv2d_workspace_bytes(int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad) {
  const int OH = (IH + 2 * pad - KS) / stride + 1, OW = (IW + 2 * pad - KS) / stride + 1;
  const size_t wbytes = up((size_t)PH_NPLANES * KS * KS * Cin * Cout * sizeof(bf16));
  // BatchNorm partial rows: the largest count of any arithmetic, at the convolution's stride or (the routes of ph_conv_fwd_route) 1;
  // never fewer than one per CU (the size this call has always returned for small maps, kept for its callers)
  int nparts = ph_num_cus();
  for (int prec = PH_PREC_BF16; prec <= PH_PREC_FP16X3; ++prec)
    for (int S = 1; S <= stride; ++S) nparts = std::max(nparts, ph_tapconv_stat_parts_bound(B, OH, OW, Cout, S, prec));
  const size_t parts = up((size_t)nparts * 2 * Cout * sizeof(float));
  // slab: the chunks ph_conv2d_wgrad launches with - and never fewer than a launch at the convolution's own stride would take, which
  // is how the 1x1 / stride-2 view used to be sized (that count can be the smaller or the larger one)
  PhWgrad g{};
  int nc = plan_wgrad(Conv{B, Cin, IH, IW, Cout, KS, stride, pad}, &g);
  g.S = stride;
  nc = std::max(nc, ph_wgrad_chunks(&g, B, PH_WG_WANT_ALONE, &g.tiles_per_chunk));
  const size_t slab = up((size_t)nc * KS * KS * Cin * Cout * sizeof(float));
  return wbytes + (parts > slab ? parts : slab) + 256;
}

namespace {
// the forward launch of convolution v: geometry, route and weight layout of descriptor t (tensors are the caller's), *S = the stride
// it is launched with.  PH_EINVAL before anything is written.
int plan_fwd(const Conv& v, int prec, PhTapConv* t, int* S) {
  // (PH_PREC_FP16X1 is a backward arithmetic)
  if (!geometry_ok(v.B, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.stride, v.pad) || prec < PH_PREC_BF16 || prec > PH_PREC_FP16X3) return PH_EINVAL;
  t->B = v.B; t->wplane = (size_t)v.KS * v.KS * v.Cin * v.Cout;
  ph_conv_fwd_geometry(t, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.stride, v.pad);
  *S = ph_conv_fwd_route(t, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.stride, v.pad, prec, 0);
  t->w_frag = ph_tapconv_hp_wfrag(t, *S, prec);
  return ph_tapconv_select(t, *S, prec).kernel == PH_CK_REJECT ? PH_EINVAL : PH_OK;
}

// the dgrad launches of convolution v over descriptor t (tensors are the caller's): the stride-1 launch, or one launch per output
// parity class of a stride-2 convolution (row-major weights).  Every class is planned, and the call checked, before anything is written.
int plan_dgrad(const Conv& v, int prec, PhTapConv* t, PhTapConv cls[4], int* ncls, bool* tapless) {
  if (!geometry_ok(v.B, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.stride, v.pad) || prec < PH_PREC_BF16 || prec > PH_PREC_FP16X1) return PH_EINVAL;
  t->B = v.B; t->wplane = (size_t)v.KS * v.KS * v.Cin * v.Cout;
  *tapless = false;
  if (v.stride == 1) {
    ph_conv_dgrad_s1_geometry(t, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.pad);
    t->w_frag = ph_tapconv_hp_wfrag(t, 1, prec);
    cls[0] = *t; *ncls = 1;
  } else {
    t->w_frag = PH_WFRAG_ROW;
    const int rc = ph_conv_dgrad_s2_classes(t, v.Cin, v.IH, v.IW, v.Cout, v.KS, v.pad, cls, ncls, tapless);
    if (rc) return rc;
  }
  for (int k = 0; k < *ncls; ++k)
    if (ph_tapconv_select(&cls[k], 1, prec).kernel == PH_CK_REJECT) return PH_EINVAL;
  return PH_OK;
}

// the weights of convolution v at `hi` in the orientation and layout launch t (stride S) reads: the half-pair layout t->w_frag, the
// split planes, or perf-mode plane 0 with the plane-1 fragment copy when the launch's kernel reads it
int pack_one(const float* w, bf16* hi, const PhTapConv* t, int S, const Conv& v, int dgrad, int prec, hipStream_t st) {
  const bool hp = prec == PH_PREC_FP16X3 || prec == PH_PREC_FP16X1;
  const int frag = hp ? t->w_frag : (ph_tapconv_needs_frag_copy(t, S, prec) ? PH_WFRAG_COPY : PH_WFRAG_ROW);
  return ph_pack_w_launch(w, hi, v.Cout, v.Cin, v.KS, dgrad, hp ? -3 : (prec == PH_PREC_BF16 ? 1 : 3), frag, st);
}
}  // namespace

int ph_conv2d_fwd(const void* x, const float* w, void* y, float* ch_sum, float* ch_sumsq, int B, int Cin, int IH,
                  int IW, int Cout, int KS, int stride, int pad, int prec, void* ws_, hipStream_t st) {
  if (!x || !w || !y || !ws_) return PH_EINVAL;
  unsigned char* ws = reinterpret_cast<unsigned char*>(ws_);
  bf16* hi = reinterpret_cast<bf16*>(ws);
  PhTapConv t{};
  int S;
  t.in = x; t.w = hi; t.out = y;
  int rc = plan_fwd(Conv{B, Cin, IH, IW, Cout, KS, stride, pad}, prec, &t, &S);
  if (rc) return rc;
  t.stats = reinterpret_cast<float*>(ws + up(PH_NPLANES * t.wplane * sizeof(bf16)));
  if ((rc = pack_one(w, hi, &t, S, Conv{B, Cin, IH, IW, Cout, KS, stride, pad}, 0, prec, st))) return rc;
  if ((rc = ph_tapconv_launch(&t, S, prec, st))) return rc;
  if (ch_sum || ch_sumsq) {
    hipLaunchKernelGGL(parts_sum_kernel, dim3(cdiv(Cout, 64)), dim3(64), 0, st, t.stats,
                       ph_tapconv_stat_parts(&t, S, prec), Cout, ch_sum, ch_sumsq);
    PH_LAUNCH_CHECK();
  }
  return PH_OK;
}

namespace {
// dgrad (+ residual) of a stride-1 or stride-2 convolution.  Stride 2: one launch per output parity class; a class no tap
// reaches (1x1) receives res_g in place (res_g == dx, no res_a), zeros (no residual), or the call is PH_EINVAL
int dgrad_common(const void* dy, const float* w, void* dx, const void* res_g, const void* res_a, int B, int Cin, int IH, int IW,
                 int Cout, int KS, int stride, int pad, int prec, void* ws_, hipStream_t st) {
  if (!dy || !w || !dx || !ws_) return PH_EINVAL;
  const Conv v{B, Cin, IH, IW, Cout, KS, stride, pad};
  bf16* hi = reinterpret_cast<bf16*>(ws_);
  PhTapConv t{}, cls[4];
  int ncls;
  bool tapless;
  t.in = dy; t.w = hi; t.out = dx; t.res_g = res_g; t.res_a = res_a;
  int rc = plan_dgrad(v, prec, &t, cls, &ncls, &tapless);
  if (rc) return rc;
  if (tapless && res_g && (res_g != dx || res_a)) return PH_EINVAL;
  if ((rc = pack_one(w, hi, &cls[0], 1, v, 1, prec, st))) return rc;
  if (tapless && !res_g) {
    const size_t es = prec == PH_PREC_BF16 ? 2 : 4;
    if (hipMemsetAsync(dx, 0, (size_t)B * IH * IW * Cin * es, st) != hipSuccess) return PH_ELAUNCH;
  }
  for (int k = 0; k < ncls; ++k)
    if ((rc = ph_tapconv_launch(&cls[k], 1, prec, st))) return rc;
  return PH_OK;
}
}  // namespace

// host-only test access to the selection (not part of the public C-ABI): the OR of the family bits (1u << PH_CK_*) the launches of
// ph_conv2d_fwd (op 0) / ph_conv2d_dgrad (op 1) would reach, or PH_EINVAL; *stat_parts / *w_frag (optional) of the first launch.
// Builds the descriptors as those entry points do and makes no HIP call.
extern "C" int ph_debug_conv2d_select(int op, int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad, int prec,
                                      int* stat_parts, int* w_frag) {
  const Conv v{B, Cin, IH, IW, Cout, KS, stride, pad};
  PhTapConv cls[4] = {}, t{};
  int ncls = 1, S = 1;
  bool tapless;
  const int rc = op == 0 ? plan_fwd(v, prec, &cls[0], &S) : (op == 1 ? plan_dgrad(v, prec, &t, cls, &ncls, &tapless) : PH_EINVAL);
  if (rc) return rc;
  int mask = 0;
  for (int k = ncls - 1; k >= 0; --k) {
    const PhConvChoice c = ph_tapconv_select(&cls[k], S, prec);
    mask |= 1 << c.kernel;
    if (stat_parts) *stat_parts = c.stat_parts;
    if (w_frag) *w_frag = c.w_frag;
  }
  return mask;
}

int ph_conv2d_dgrad_res(const void* dy, const float* w, void* dx, const void* res_g, const void* res_a, int B, int Cin,
                        int IH, int IW, int Cout, int KS, int stride, int pad, int prec, void* ws_, hipStream_t st) {
  return dgrad_common(dy, w, dx, res_g, res_a, B, Cin, IH, IW, Cout, KS, stride, pad, prec, ws_, st);
}

// test access to the in-LDS BatchNorm + ReLU of a 3x3 stride-1 perf-mode forward launch (PhTapConv::in_scale): y = conv(relu(x *
// in_scale[c] + in_shift[c]) rounded to bf16, w), bitwise what ph_bn_apply_launch + ph_conv2d_fwd give
int ph_conv2d_fwd_fused_in(const void* x, const float* in_scale, const float* in_shift, const float* w, void* y, float* ch_sum,
                           float* ch_sumsq, int B, int Cin, int IH, int IW, int Cout, void* ws_, hipStream_t st) {
  if (Cin % 64 || Cout % 64 || !in_scale || !in_shift) return PH_EINVAL;
  unsigned char* ws = reinterpret_cast<unsigned char*>(ws_);
  const size_t plane = (size_t)9 * Cin * Cout;
  bf16* hi = reinterpret_cast<bf16*>(ws);
  PhTapConv t{};
  t.in = x; t.w = hi; t.wplane = plane; t.out = y; t.in_scale = in_scale; t.in_shift = in_shift;
  t.stats = reinterpret_cast<float*>(ws + up(PH_NPLANES * plane * sizeof(bf16)));
  t.B = B;
  ph_conv_fwd_geometry(&t, Cin, IH, IW, Cout, 3, 1, 1);
  int rc = pack_one(w, hi, &t, 1, Conv{B, Cin, IH, IW, Cout, 3, 1, 1}, 0, PH_PREC_BF16, st);
  if (rc) return rc;
  if ((rc = ph_tapconv_launch(&t, 1, PH_PREC_BF16, st))) return rc;
  if (ch_sum || ch_sumsq) {
    hipLaunchKernelGGL(parts_sum_kernel, dim3(cdiv(Cout, 64)), dim3(64), 0, st, t.stats, ph_tapconv_stat_parts(&t, 1, PH_PREC_BF16), Cout,
                       ch_sum, ch_sumsq);
    PH_LAUNCH_CHECK();
  }
  return PH_OK;
}

// test access to the fused BatchNorm-backward sums of a 3x3 stride-1 perf-mode dgrad launch (PhTapConv::bst_y, conv_tap4.hip):
// dx = dgrad(dy, w) (+ res_g * (res_a > 0 | 1)) and sums[3][Cin] = sum dz | sum dz (bst_y - bst_mean) | sum dz (bst_y2 - bst_mean2)
// with dz = dx * (bst_a ? bst_a > 0 : bst_y * bst_scale + bst_shift > 0), combined in double from the per-workgroup rows
int ph_conv2d_dgrad_bnstat(const void* dy, const float* w, void* dx, const void* res_g, const void* res_a, const void* bst_y,
                           const void* bst_a, const void* bst_y2, const float* bst_scale, const float* bst_shift,
                           const float* bst_mean, const float* bst_mean2, float* sums, int B, int Cin, int IH, int IW, int Cout,
                           void* ws_, hipStream_t st) {
  if (Cin % 64 || Cout % 64 || !bst_y || !bst_mean || !sums) return PH_EINVAL;
  unsigned char* ws = reinterpret_cast<unsigned char*>(ws_);
  const size_t plane = (size_t)9 * Cin * Cout;
  bf16* hi = reinterpret_cast<bf16*>(ws);
  PhTapConv t{};
  t.in = dy; t.w = hi; t.wplane = plane; t.out = dx; t.res_g = res_g; t.res_a = res_a;
  t.B = B;
  ph_conv_dgrad_s1_geometry(&t, Cin, IH, IW, Cout, 3, 1);
  t.bst_y = bst_y; t.bst_a = bst_a; t.bst_y2 = bst_y2; t.bst_scale = bst_scale; t.bst_shift = bst_shift;
  t.bst_mean = bst_mean; t.bst_mean2 = bst_mean2;
  t.stats = reinterpret_cast<float*>(ws + up(PH_NPLANES * plane * sizeof(bf16)));
  int rc = pack_one(w, hi, &t, 1, Conv{B, Cin, IH, IW, Cout, 3, 1, 1}, 1, PH_PREC_BF16, st);
  if (rc) return rc;
  if ((rc = ph_tapconv_launch(&t, 1, PH_PREC_BF16, st))) return rc;
  const int nparts = ph_tapconv_stat_parts(&t, 1, PH_PREC_BF16);
  hipLaunchKernelGGL(parts3_sum_kernel, dim3(cdiv(Cin, 64)), dim3(64), 0, st, t.stats, nparts, Cin, sums);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

int ph_conv2d_dgrad(const void* dy, const float* w, void* dx, int B, int Cin, int IH, int IW, int Cout, int KS,
                    int stride, int pad, int prec, void* ws_, hipStream_t st) {
  return dgrad_common(dy, w, dx, nullptr, nullptr, B, Cin, IH, IW, Cout, KS, stride, pad, prec, ws_, st);
}

int ph_conv2d_wgrad(const void* x, const void* dy, float* dw, int B, int Cin, int IH, int IW, int Cout, int KS,
                    int stride, int pad, int prec, void* ws_, hipStream_t st) {
  if (!geometry_ok(B, Cin, IH, IW, Cout, KS, stride, pad) || prec < PH_PREC_BF16 || prec > PH_PREC_FP16X1 || !x || !dy || !dw || !ws_)
    return PH_EINVAL;
  unsigned char* ws = reinterpret_cast<unsigned char*>(ws_);
  PhWgrad g{};
  // layout: [256 B zero page][slab]
  if (hipMemsetAsync(ws, 0, 256, st) != hipSuccess) return PH_ELAUNCH;
  g.zeros = ws;
  g.x = x; g.dy = dy; g.slab = reinterpret_cast<float*>(ws + 256);
  plan_wgrad(Conv{B, Cin, IH, IW, Cout, KS, stride, pad}, &g);
  int rc = ph_wgrad_launch(&g, prec, st);
  if (rc) return rc;
  return ph_wgrad_reduce_launch(g.slab, dw, g.nchunks, KS, Cout, Cin, nullptr, st);
}

// host-only test access (not part of the public C-ABI): the chunk count - slab planes of KS * KS * Cin * Cout floats behind the
// 256-byte zero page - ph_conv2d_wgrad launches with, or PH_EINVAL.  Makes no HIP call.
extern "C" int ph_debug_conv2d_wgrad_chunks(int B, int Cin, int IH, int IW, int Cout, int KS, int stride, int pad) {
  if (!geometry_ok(B, Cin, IH, IW, Cout, KS, stride, pad)) return PH_EINVAL;
  PhWgrad g{};
  return plan_wgrad(Conv{B, Cin, IH, IW, Cout, KS, stride, pad}, &g);
}

int ph_stem_dgrad(const void* dy_nhwc, const float* w_oihw, float* dx_nchw, int B, int H, int W, int prec, hipStream_t st) {
  if (!dy_nhwc || !w_oihw || !dx_nchw || B < 1 || H < 2 || W < 2 || (prec != PH_PREC_BF16 && !PH_IS_SPLIT_PREC(prec)))
    return PH_EINVAL;
  return ph_stem_dgrad_launch(dy_nhwc, w_oihw, dx_nchw, B, H, W, prec, st);
}

// PH_PREC_FP16X3 storage of a tensor whose innermost extent is a multiple of 64 (NHWC activations, C % 64 == 0): fp32 -> the
// half-pair layout [..][C / 64][2][64] fp16 (x * scale ~= hi + lo * 2^-11; `scale` a power of two, 1 for activations) and
// back.  n = number of elements (multiple of 64), both pointers 256-B aligned, same byte size either way.
int ph_hp_pack(const float* src, void* dst, size_t n, float scale, hipStream_t st) {
  if (!src || !dst || (n & 63) || ((uintptr_t)dst & 255)) return PH_EINVAL;
  hipLaunchKernelGGL(hp_pack_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, src, reinterpret_cast<hp16*>(dst), n / 8, scale);
  PH_LAUNCH_CHECK();
  return PH_OK;
}
int ph_hp_unpack(const void* src, float* dst, size_t n, hipStream_t st) {
  if (!src || !dst || (n & 63) || ((uintptr_t)src & 255)) return PH_EINVAL;
  hipLaunchKernelGGL(hp_unpack_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const hp16*>(src), dst, n / 8);
  PH_LAUNCH_CHECK();
  return PH_OK;
}

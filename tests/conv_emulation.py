"""Emulated-arithmetic reference of the convolution entry points (ph_conv2d_fwd / _dgrad / _dgrad_res / _wgrad).

Each arithmetic is reproduced product by product on the CPU: the operands are split exactly as the kernels split them
(ph_common.h: split3_bf16, hp_split) and every plane pair the kernels multiply is convolved separately, in float64, then summed
with its scale.  Every product of bf16 or fp16 planes is exact in fp32, so a correct kernel differs from this reference by its
fp32 accumulation order alone; a kernel that leaves out (or doubles) one product differs by that product.

    arithmetic  operand planes                          products (plane of operand A, plane of operand B, scale)
    bf16   (0)  bf16(x)                                 (0, 0, 1); the stored result rounded to bf16 (RNE) where it is bf16
    bf16x6 (1)  split3_bf16: p0 + p1 + p2 = x           PH_SPLIT_PAIRS: (2,0) (0,2) (1,1) (1,0) (0,1) (0,0)
    bf16x3 (2)  split3_bf16                             PH_SPLIT_PAIRS_HI: (1,0) (0,1) (0,0)
    fp16x3 (3)  hp_split: hi + lo 2^-11 = x (saturated) (0,0,1) (0,1,2^-11) (1,0,2^-11)
    fp16x1 (4)  hp_split                                (0,0,1)   (dgrad / wgrad only: the hi planes of the half-pair tensors)

Operand A / B: x / w (forward), dy / w (dgrad), x / dy (wgrad).  The product sets are the kernels' own: conv_tap.hip's
PH_SPLIT_PAIRS_LO under prod6 and the hp slice walk (hi 2^11 | lo | hi weight blocks against hi, hi, lo activations),
conv_wgrad.hip's `pl < 2 || prod6` planes and its three / one (hi1) passes.
"""
import torch
import torch.nn.functional as F

BF16, BF16X6, BF16X3, FP16X3, FP16X1 = 0, 1, 2, 3, 4
NAMES = {BF16: "bf16", BF16X6: "bf16x6", BF16X3: "bf16x3", FP16X3: "fp16x3", FP16X1: "fp16x1"}
HP_LO = 2.0 ** -11

PRODUCTS = {
    BF16: [(0, 0, 1.0)],
    BF16X6: [(2, 0, 1.0), (0, 2, 1.0), (1, 1, 1.0), (1, 0, 1.0), (0, 1, 1.0), (0, 0, 1.0)],
    BF16X3: [(1, 0, 1.0), (0, 1, 1.0), (0, 0, 1.0)],
    FP16X3: [(0, 0, 1.0), (0, 1, HP_LO), (1, 0, HP_LO)],
    FP16X1: [(0, 0, 1.0)],
}


def split3_bf16(x):
    """ph_common.h split3_bf16 on fp32 values: three bf16 planes (as fp32 tensors) whose sum is x exactly."""
    x = x.float()
    p0 = x.bfloat16().float()
    r1 = x - p0
    p1 = r1.bfloat16().float()
    p2 = (r1 - p1).bfloat16().float()
    return [p0, p1, p2]


def hp_split(x):
    """ph_common.h hp_split: saturate to +-65504 (a NaN stays NaN), hi = fp16(x), lo = fp16((x - hi) * 2^11)."""
    x = x.float()
    x = torch.where(torch.isnan(x), x, x.clamp(-65504.0, 65504.0))
    hi = x.half().float()
    lo = ((x - hi) * 2048.0).half().float()
    return [hi, lo]


def planes(x, prec):
    if prec == BF16:
        return [x.float().bfloat16().float()]
    if prec in (BF16X6, BF16X3):
        return split3_bf16(x)
    return hp_split(x)


def _op(kind, a, b, geom, dtype):
    """One product: a, b are plane tensors (NCHW / OIHW), geom = (stride, pad, x_shape, w_shape)."""
    S, pad, xs, ws = geom
    a, b = a.to(dtype), b.to(dtype)
    # (the im2col + GEMM path, not oneDNN's: plain dot-product accumulation, no Winograd transforms in float32)
    with torch.backends.mkldnn.flags(enabled=False):
        if kind == "fwd":
            return F.conv2d(a, b, None, S, pad)
        if kind == "dgrad":
            return torch.nn.grad.conv2d_input(xs, b, a, S, pad)
        return torch.nn.grad.conv2d_weight(a, ws, b, S, pad)


def emulate(kind, prec, a, b, geom, acc=torch.float64, drop=None, round_out=False):
    """The sum of the arithmetic's products (minus product `drop`, an index into PRODUCTS[prec]), each product convolved in
    `acc` (float64: the reference; float32: a stand-in for a kernel's fp32 accumulation) and summed in `acc`.  round_out:
    round the result to bf16 as the perf-mode stores do.  Returns float64."""
    pa, pb = planes(a, prec), planes(b, prec)
    out = None
    for k, (i, j, s) in enumerate(PRODUCTS[prec]):
        if k == drop:
            continue
        t = _op(kind, pa[i], pb[j], geom, acc) * s
        out = t if out is None else out + t
    if round_out:
        out = out.float().bfloat16()
    return out.double()


def bf16_half_ulp(v):
    """Half a bf16 ulp of |v| (per element, float64; 2^-134 for zero)."""
    m = v.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 8.0)


def excess(ref, got, perf, allow=None):
    """The error measure the tolerances apply to: max over elements of |got - ref| (less half a bf16 ulp of the larger of the
    two in perf mode, where the kernel stores a bf16 rounding of its fp32 sum, and less `allow`, a per-element allowance for
    a rounding point inside the operation) relative to max |ref|."""
    ref, got = ref.double(), got.double()
    d = (got - ref).abs()
    if perf:
        d = d - bf16_half_ulp(torch.maximum(ref.abs(), got.abs()))
    if allow is not None:
        d = d - allow
    d = d.clamp_min(0.0)
    return (d.max() / ref.abs().max().clamp_min(1e-300)).item()


# tau per arithmetic (relative to max |ref|): the window that accepts fp32 accumulation noise and rejects any one missing product
# (tests/test_conv_emulation.py shows both with a margin of 4 at every shape class of the sweep)
TAU = {BF16: 4e-7, BF16X6: 6e-7, BF16X3: 2e-6, FP16X3: 2e-6, FP16X1: 2e-6}


def operands(B, Cin, IH, IW, Cout, KS, S, pad, seed):
    """Test operands of one sweep case, all fp32: x [B][Cin][IH][IW], w [Cout][Cin][KS][KS], dy [B][Cout][OH][OW] (the dgrad
    operand) and dy_w (the same tensor made sparse: the wgrad operand).  One operand of every product is sparse (random support) -
    w for the forward and dgrad, dy_w for wgrad - so that an output sums at most ~24 non-zero products (a 3x3 forward output 24,
    a dgrad output 24 * Cout / max(Cin, Cout), fewer at the border and in the stride-2 parity classes): the fp32 accumulation noise
    of a dense sum of hundreds would swamp the 2^-17-relative products of bf16x6 that the tolerance must resolve."""
    g = torch.Generator().manual_seed(seed)
    OH = (IH + 2 * pad - KS) // S + 1
    OW = (IW + 2 * pad - KS) // S + 1
    x = torch.randn(B, Cin, IH, IW, generator=g)
    w = torch.randn(Cout, Cin, KS, KS, generator=g) * (2.0 / (Cin * KS * KS)) ** 0.5
    kw = max(Cin, Cout) * KS * KS
    w = w * (torch.rand(w.shape, generator=g) < min(1.0, 24.0 / kw))
    dy = torch.randn(B, Cout, OH, OW, generator=g)
    kd = B * OH * OW
    dy_w = dy * (torch.rand(dy.shape, generator=g) < min(1.0, 24.0 / kd))
    return x, w, dy, dy_w, (S, pad, (B, Cin, IH, IW), (Cout, Cin, KS, KS))

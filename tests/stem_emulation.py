"""Plain CPU restatement of the stem convolution kernels (csrc/conv_stem.hip) for tests/test_gpu_stem.py: the 7x7 / stride 2 / pad 3
convolution of a three-channel image in every arithmetic (tests/conv_emulation.py: plane splits, product sets, `emulate`, `excess`),
and the bookkeeping the four kernels promise, read from the code:

  forward       8 x 16 output tiles in image-major order (t = (b * tiles_h + tile row) * tiles_w + tile column); statistics row vb =
                the VALID pixels (r < OH, c < OW) of tiles 8 vb .. 8 vb + 7: [sum, sum of squares] per channel, over the fp32 values
                (in PH_PREC_BF16 too: the sums are taken before the output is rounded to bf16).  The rows do not depend on the grid
                (PhStem::vblocks: a workgroup that walks several blocks resets its sums between them).
  pooled        strips of 14 conv columns, cut into nsplit pieces of per = ceil(tiles_h / nsplit) tile rows; statistics row
                (b * ncs + cs) * nsplit + split = the pixels of image b, columns 14 cs .. 14 cs + 13, tile rows split * per ..: every conv
                pixel in exactly one row (the tile column a strip shares with its left neighbour and the tile row a cut strip recomputes
                belong to the neighbour).  Pooled value: per channel the 3 x 3 / stride 2 / pad 1 window's maximum of the bf16-rounded
                conv output where gamma >= 0 (-0.0 included), its minimum where gamma < 0.
  weight grad   chunk k = tiles k tpc .. k tpc + tpc - 1 of the same tile order (chunks cross images); slab [chunk][kh][cout][kw * 4 + ch]:
                kw = 7 is the correlation with the halo column past the kernel (computed, never reduced), ch = 3 is zero.  dw = the
                chunks' sum over kw < 7, ch < 3, times unscale[1].

Two operand classes.  Integer: image in -2 .. 2, weights in {-1, 0, 1} with at most 24 of the 147 non-zero per output channel, dy in
-2 .. 2 - every product and sum is an integer below 2^24 whatever the order, every conv output an integer bf16 holds (|y| <= 48), in
every arithmetic (the low planes of an integer are zero), so the device must give the float64 VALUES (`mismatches`; zeros of either
sign are equal: the pooled kernel's sign flip leaves -0).  Random: Gaussian with the same sparsity, for the arithmetics' product sets
(`within`, TAU).

TAU is conv_emulation.TAU except for bf16x6 (below): tests/test_stem_emulation_cpu.py shows, on the operands and shapes of the GPU
test, the float32 stand-in a factor 4 inside it and the smallest single dropped product a factor 4 outside; STAND_IN records both.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_emulation as E

BF16, BF16X6, BF16X3, FP16X3, FP16X1 = E.BF16, E.BF16X6, E.BF16X3, E.FP16X3, E.FP16X1
NAMES = E.NAMES
TH, TW, TPW, PCOLS = 8, 16, 8, 14
MARGIN = 4.0
# (largest float32 stand-in excess, smallest single dropped product) per arithmetic, relative to max |ref|, over the random cases of
# the GPU test - tests/test_stem_emulation_cpu.py prints them (test_tau_*); None: the arithmetic has one product
STAND_IN = {"fwd": {BF16: (0.0, None), BF16X6: (1.032e-7, 1.932e-6), BF16X3: (1.052e-7, 1.109e-3), FP16X3: (1.663e-7, 1.947e-4)},
            "wgrad": {BF16: (6.375e-8, None), BF16X6: (9.849e-8, 2.625e-6), BF16X3: (1.042e-7, 1.771e-3),
                      FP16X3: (1.122e-7, 2.191e-4), FP16X1: (7.965e-8, None)}}
# conv_emulation.TAU, but for bf16x6: at (1, 3, 5) - 384 outputs - the smallest dropped product (x plane 2 against w plane 0) is
# 1.932e-6 of max |ref|, less than 4 x 6e-7.  The stem's own value by the same rule: at least 4 x the stand-in's 1.032e-7 = 4.13e-7, at
# most 1.932e-6 / 4 = 4.83e-7.
TAU = dict(E.TAU)
TAU[BF16X6] = 4.5e-7

# ---- the cases of tests/test_gpu_stem.py (B, IH, IW)
FWD_PRECS = (BF16, BF16X6, BF16X3, FP16X3)
FWD_SHAPES = ((1, 16, 32), (1, 14, 30), (1, 17, 35), (1, 3, 5), (3, 34, 66))
FWD_RANDOM = (FWD_SHAPES[1], FWD_SHAPES[3])
WALK_SHAPE, WALK_CAPS, WALK_PRECS = (5, 34, 66), (0, 4, 1), (BF16, FP16X3)
# OW = 14, 15, 16, 29 (IW = 2 OW); odd OH (IH 18 -> 9) and odd OW (15, 29); cut strips: nsplit 2 (9 tile rows: 5 + 4), nsplit 4
POOL_SHAPES = ((1, 16, 28), (2, 18, 30), (1, 20, 32), (1, 18, 58), (1, 130, 20), (2, 256, 12))
POOL_RANDOM, POOL_TINY = (2, 18, 30), (1, 18, 58)
WG_PRECS = (BF16, BF16X6, BF16X3, FP16X3, FP16X1)
WG_SHAPES = ((1, 16, 32), (1, 17, 35), (3, 34, 66))
WG_TPC = (1, 2, 4, 7, 27, 0)
WG_MANY = ((5, 34, 66), 1)
WG_RANDOM = (3, 34, 66)
FUSED_SHAPES = ((3, 34, 66), (2, 18, 38))

vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
# the test entry points at the end of csrc/conv_stem.hip (not part of include/pathomic_hip.h): name -> (restype, argtypes)
SIGNATURES = {
    "ph_debug_stem_weight_bytes": (sz, []),
    "ph_debug_stem_pack_weights": (i32, [vp, vp, i32, vp]),
    "ph_debug_stem_stat_parts": (i32, [i32, i32, i32]),
    "ph_debug_stem_pool_stat_parts": (i32, [i32, i32, i32]),
    "ph_debug_stem_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ph_debug_stem_fwd_pool": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ph_debug_stem_wgrad_slab_bytes": (sz, [i32, i32, i32, i32]),
    "ph_debug_stem_wgrad": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "ph_debug_stem_wgrad_fused": (i32, [vp] * 13 + [i32, i32, i32, i32, i32, vp, vp]),
}


def bind(L):
    """Declare the ph_debug_stem_* entries of the loaded library L (AttributeError if one is missing)."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def case_seed(shape):
    """The operand seed of a (B, IH, IW) case: the GPU test and the CPU self-test draw the same operands."""
    return 7919 * shape[0] + 131 * shape[1] + shape[2]


def cdiv(a, b):
    return -(-a // b)


def conv_map(i):
    return (i - 1) // 2 + 1


def geom(B, IH, IW):
    return 2, 3, (B, 3, IH, IW), (64, 3, 7, 7)


def tiles(B, IH, IW):
    """(tiles_h, tiles_w, ntiles) of the 8 x 16 output tiling."""
    th, tw = cdiv(conv_map(IH), TH), cdiv(conv_map(IW), TW)
    return th, tw, B * th * tw


def stat_parts(B, IH, IW):
    return cdiv(tiles(B, IH, IW)[2], TPW)


def pool_nsplit(B, OH, OW):
    ncs, th, ns = cdiv(OW, PCOLS), cdiv(OH, TH), 1
    while B * ncs * ns < 2048 and th // (ns * 2) >= 4:
        ns *= 2
    return ns


def pool_stat_parts(B, IH, IW):
    OH, OW = conv_map(IH), conv_map(IW)
    return B * cdiv(OW, PCOLS) * pool_nsplit(B, OH, OW)


def plan_chunks(ntiles):
    """resnet_plan.hip stem_chunks: (chunks, tiles per chunk)."""
    tpc = cdiv(ntiles, min(ntiles, 1024))
    return cdiv(ntiles, tpc), tpc


# ------------------------------------------------------------------------------------------------ operands
def _support(g, shape, k, per):
    """0 / 1 mask with about k of every `per` elements set."""
    return (torch.rand(shape, generator=g) < min(1.0, k / per)).float()


def operands_int(B, IH, IW, seed, xmax=2):
    """x [B][3][IH][IW] in -xmax .. xmax, w [64][3][7][7] in {-1, 0, 1} (at most 24 non-zero per output channel), dy [B][64][OH][OW] in
    -2 .. 2.  The bounds the exact class rests on are checked here."""
    g = torch.Generator().manual_seed(seed)
    OH, OW = conv_map(IH), conv_map(IW)
    x = torch.randint(-xmax, xmax + 1, (B, 3, IH, IW), generator=g).float()
    w = torch.randint(0, 2, (64, 3, 7, 7), generator=g).float() * 2 - 1
    w = w * _support(g, w.shape, 20.0, 147)
    for co in range(64):                                   # at most 24 non-zero per output channel
        nz = w[co].flatten().nonzero().flatten()
        if len(nz) > 24:
            w[co].view(-1)[nz[24:]] = 0
    dy = torch.randint(-2, 3, (B, 64, OH, OW), generator=g).float()
    nzmax = int((w != 0).flatten(1).sum(1).max())
    assert nzmax <= 24 and nzmax * xmax <= 256, "a conv output bf16 may not hold"
    npix = B * OH * OW
    assert npix * (nzmax * xmax) ** 2 < 2 ** 24, "a sum of squares float32 may not hold"
    assert npix * 2 * xmax < 2 ** 24 and nzmax * xmax * 2048 < 2 ** 24       # (dw sums; the half-pair forward's 2^11-scaled sums)
    return x, w, dy


def operands_rand(B, IH, IW, seed):
    """Gaussian x, w (about 24 of 147 non-zero per output), dy and dy_w (dy made sparse: about 24 non-zero per weight-gradient sum)."""
    g = torch.Generator().manual_seed(seed)
    OH, OW = conv_map(IH), conv_map(IW)
    x = torch.randn(B, 3, IH, IW, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    w = w * _support(g, w.shape, 24.0, 147)
    dy = torch.randn(B, 64, OH, OW, generator=g)
    dy_w = dy * _support(g, dy.shape, 24.0, B * OH * OW)
    return x, w, dy, dy_w


def nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ forward
def fwd(x, w, prec, acc=torch.float64, drop=None, defect=None):
    """The conv output [B][OH][OW][64] float64 (not rounded).  defect "halo_neighbour": the rows above / below an image are not zero
    but the neighbouring image's (what an unchecked row index reads)."""
    B, _, IH, IW = x.shape
    if defect == "halo_neighbour":
        z = torch.zeros(1, 3, 3, IW)
        up = torch.cat([z, x[:-1, :, IH - 3:]], 0)
        dn = torch.cat([x[1:, :, :3], z], 0)
        xt = torch.cat([up, x, dn], 2)
        return nhwc(E.emulate("fwd", prec, F.pad(xt, (3, 3, 0, 0)), w, (2, 0, None, None), acc, drop))
    return nhwc(E.emulate("fwd", prec, x, w, geom(B, IH, IW), acc, drop))


def fwd_extended(x, w, prec=BF16):
    """The accumulators of whole tiles, [B][tiles_h * 8][tiles_w * 16][64]: the conv map continued past OH / OW (zeros beyond the image)."""
    B, _, IH, IW = x.shape
    th, tw, _ = tiles(B, IH, IW)
    xe = F.pad(x, (0, 2 * tw * TW - IW, 0, 2 * th * TH - IH))
    y = nhwc(E.emulate("fwd", prec, xe, w, geom(B, 2 * th * TH, 2 * tw * TW)))
    assert y.shape[1:3] == (th * TH, tw * TW)
    return y


def fwd_stats(ye, OH, OW, defect=None, grid=0):
    """Statistics rows [blocks][2][64] float64 from the extended map.  defects: "oob_counted" (r < OH + 1), "no_reset" (a workgroup of a
    grid of `grid` does not reset its sums between its blocks)."""
    B, HE, WE, _ = ye.shape
    r, c = torch.arange(HE)[:, None], torch.arange(WE)[None, :]
    valid = ((r < OH + (1 if defect == "oob_counted" else 0)) & (c < OW)).double()[None, :, :, None]
    v = ye.double() * valid
    rows = []
    for q in (v, v * v):
        t = q.view(B, HE // TH, TH, WE // TW, TW, 64).sum((2, 4)).reshape(-1, 64)          # per tile, image-major
        nb = cdiv(t.shape[0], TPW)
        t = torch.cat([t, torch.zeros(nb * TPW - t.shape[0], 64, dtype=t.dtype)], 0)
        rows.append(t.view(nb, TPW, 64).sum(1))
    out = torch.stack(rows, 1)
    if defect == "no_reset":
        assert grid > 0
        for vb in range(grid, out.shape[0]):
            out[vb] = out[vb] + out[vb - grid]
    return out


# ------------------------------------------------------------------------------------------------ pooled forward
def pool_stats(y, defect=None):
    """Rows [(b, cs, split)][2][64] float64 of the conv output y [B][OH][OW][64].  defects: "shared_column_twice" (a strip counts the
    column left of its own), "cut_row_twice" (a cut strip counts the tile row it recomputes)."""
    B, OH, OW, _ = y.shape
    ncs, th, ns = cdiv(OW, PCOLS), cdiv(OH, TH), pool_nsplit(B, OH, OW)
    per = cdiv(th, ns)
    y = y.double()
    out = torch.zeros(B * ncs * ns, 2, 64, dtype=torch.float64)
    for b in range(B):
        for cs in range(ncs):
            c0 = cs * PCOLS - (1 if defect == "shared_column_twice" and cs > 0 else 0)
            for sp in range(ns):
                t0, t1 = sp * per, min(th, sp * per + per)
                if defect == "cut_row_twice" and sp > 0:
                    t0 -= 1
                if t0 >= t1:
                    continue
                v = y[b, t0 * TH:min(OH, t1 * TH), c0:min(OW, cs * PCOLS + PCOLS)]
                out[(b * ncs + cs) * ns + sp, 0] = v.sum((0, 1))
                out[(b * ncs + cs) * ns + sp, 1] = (v * v).sum((0, 1))
    return out


def pooled(yr, gamma, defect=None):
    """[B][PH][PW][64] float64 from the (bf16-rounded) conv output yr: window maximum where gamma >= 0, minimum where gamma < 0.
    defects: "max_everywhere", "last_window_dropped" (odd OH / OW: the last pooled row / column is never produced)."""
    v = yr.double().permute(0, 3, 1, 2)
    mx = F.max_pool2d(v, 3, 2, 1)
    mn = -F.max_pool2d(-v, 3, 2, 1)
    neg = (torch.as_tensor(gamma) < 0)[None, :, None, None]
    if defect == "max_everywhere":
        neg = neg & False
    out = nhwc(torch.where(neg, mn, mx))
    if defect == "last_window_dropped":
        if yr.shape[1] % 2:
            out[:, -1] = float("nan")
        if yr.shape[2] % 2:
            out[:, :, -1] = float("nan")
    return out


def pool_gamma():
    """gamma [64] float32 of the pooled cases: mixed signs (every third channel negative), one zero and one -0.0 (both: maximum)."""
    g = np.where(np.arange(64) % 3 == 1, -1.0, 1.0) * (0.5 + np.arange(64) / 64.0)
    g[6], g[9] = 0.0, -0.0
    return g.astype(np.float32)


def bf16r(y):
    return y.float().bfloat16().double()


def pooled_bounds(y, gamma, e):
    """(lo, hi) of the pooled tensor when every fp32 conv sum lies within e of the float64 y: bf16 rounding and the window
    extremum are monotone, so the device's value lies between the pooled roundings of y - e and y + e - one bf16 step apart where
    a sum is that close to a rounding boundary, equal elsewhere."""
    return pooled(bf16r(y - e), gamma), pooled(bf16r(y + e), gamma)


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_tiles(x, dy):
    """Per tile [ntiles][7][64][8][4] float64: sum over the tile's pixels of dy[co] x[ch][2 r - 3 + kh][2 c - 3 + kw], kw = 0 .. 7 (zeros
    outside the image), ch = 3 zero.  Exact on integer operands."""
    B, _, IH, IW = x.shape
    OH, OW = conv_map(IH), conv_map(IW)
    th, tw, nt = tiles(B, IH, IW)
    xp = F.pad(x.double(), (3, 2 * OW + 6 - IW - 3, 3, 2 * OH + 5 - IH - 3))          # 2 (OW - 1) + 8 columns, 2 (OH - 1) + 7 rows
    P = F.unfold(xp, (7, 8), stride=2).view(B, 3, 7, 8, OH, OW)
    d = dy.double()
    out = torch.zeros(nt, 7, 64, 8, 4, dtype=torch.float64)
    for b in range(B):
        for tr in range(th):
            for tc in range(tw):
                rs, cs = slice(tr * TH, min(OH, tr * TH + TH)), slice(tc * TW, min(OW, tc * TW + TW))
                out[(b * th + tr) * tw + tc, :, :, :, :3] = torch.einsum("orc,ihwrc->hoiw", d[b, :, rs, cs], P[b, :, :, :, rs, cs]).permute(0, 1, 3, 2)
    return out


def slab(tl, tpc):
    """[chunks][7][64][32] from the per-tile sums; tpc 0 = the plan's rule."""
    nt = tl.shape[0]
    if tpc == 0:
        tpc = plan_chunks(nt)[1]
    return torch.stack([tl[k:k + tpc].sum(0) for k in range(0, nt, tpc)]).reshape(-1, 7, 64, 32)


def dw_of_slab(sl, unscale=1.0, defect=None):
    """dw [64][3][7][7] as the reduce kernel sums the slab: chunk-lane cl walks cl, cl + 4, .. (four at a time, then a tail).  defects:
    "kh6_missing", "last_chunk_dropped", "lane_tail_dropped" (chunk-lane 3 loses the chunks its tail loop owns)."""
    n = sl.shape[0]
    keep = torch.ones(n, dtype=torch.bool)
    if defect == "last_chunk_dropped":
        keep[-1] = False
    if defect == "lane_tail_dropped":
        c = 3
        while c + 12 < n:
            c += 16
        keep[c::4] = False
    s = sl[keep].sum(0).view(7, 64, 8, 4)[:, :, :7, :3].permute(1, 3, 0, 2).contiguous() * unscale       # [co][ch][kh][kw]
    if defect == "kh6_missing":
        s[:, :, 6] = 0
    return s


def wgrad(x, dy, prec, acc=torch.float64, drop=None):
    """dw [64][3][7][7] float64 of the arithmetic (random class)."""
    B, _, IH, IW = x.shape
    return E.emulate("wgrad", prec, x, dy, geom(B, IH, IW), acc, drop)


# ------------------------------------------------------------------------------------------------ the comparisons of the GPU test
def mismatches(ref, got):
    """Elements of `got` that do not hold the VALUE of the float64 `ref` as float32 holds it (+0 == -0; a NaN never matches)."""
    ref = torch.as_tensor(ref).double().float()
    got = torch.as_tensor(got).float().reshape(ref.shape)
    return int((~(ref == got)).sum())


def within(ref, got, prec, perf=False):
    """(ok, excess): conv_emulation.excess of `got` against the float64 `ref` within TAU of the arithmetic."""
    ex = E.excess(torch.as_tensor(ref), torch.as_tensor(got).reshape(torch.as_tensor(ref).shape), perf)
    return (ex <= TAU[prec]), ex


def sum_bound(x, dz):
    """Per element of dw, the worst case of ANY float32 summation of its B OH OW exact products (bf16 x bf16): (n - 1) 2^-24 sum |t|.
    The allowance of the dense dz of the fused case, whose accumulation noise no sparse operand keeps below TAU; the defects it must
    reject (a kernel row, a chunk, a lane's tail missing) are whole terms of the sum."""
    B, _, IH, IW = x.shape
    n = dz.shape[0] * dz.shape[2] * dz.shape[3]
    with torch.backends.mkldnn.flags(enabled=False):
        s = torch.nn.grad.conv2d_weight(x.float().bfloat16().double().abs(), (64, 3, 7, 7), dz.double().abs(), 2, 3)
    return s * ((n - 1) * 2.0 ** -24)


def outside(ref, got, allow):
    """Elements of `got` further than `allow` from the float64 `ref` (a NaN is outside)."""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    return int((~((got - ref).abs() <= allow)).sum())


def between(lo, hi, got):
    """Elements of `got` outside [lo, hi] (a NaN is outside)."""
    got = torch.as_tensor(got).double().reshape(lo.shape)
    return int((~((got >= lo) & (got <= hi))).sum())

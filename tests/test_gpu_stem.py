"""Sweep of the stem convolution kernels (csrc/conv_stem.hip: stem_fwd_kernel, stem_fwd_pool_kernel, stem_wgrad_kernel with and
without the fused dz, stem_wgrad_reduce_kernel) through their test entry points (ph_debug_stem_*, at the end of that file) against
tests/stem_emulation.py, at the tile, strip, cut and chunk edges.

  integer class  image, weights and dy small integers: every product and sum is exact in float32, so the conv output, EVERY statistics
                 row (sum and sum of squares), the pooled tensor, every slab plane and dw must hold the float64 values (zeros of either
                 sign are equal), in every arithmetic, at every grid and every chunking.
  random class   Gaussian operands, one of them sparse: within stem_emulation.TAU of the emulated arithmetic (the excess is printed per
                 arithmetic); the pooled tensor between the pooled roundings of the reference moved by the forward's TAU either way.

Every output, every statistics buffer and the slab (sized exactly by its query) lie between sentinel guard bands and are filled with
NaN first: after each call the return code is PH_OK, the guards are intact and no NaN is left.

Shapes are (B, IH, IW); the launchers accepted every shape of the list, none had to move.

Measured on the MI355X, the largest excess seen relative to max |ref| (tolerance): forward bf16 0 (4e-7), bf16x6 2.33e-7 (4.5e-7),
bf16x3 1.83e-7 (2e-6), fp16x3 2.12e-7 (2e-6); weight gradient bf16 4.3e-8 (4e-7), bf16x6 1.30e-7 (4.5e-7), bf16x3 1.17e-7 (2e-6),
fp16x3 1.11e-7 (2e-6), fp16x1 7.9e-8 (2e-6); the dz-fed weight gradient of the fused case 1.7e-7 of max |ref| (worst-case allowance
up to 4.6e-4).  9 of the 5120 pooled values of the random case lay at a rounding boundary.  Every test prints its `excess[...]`;
re-measure after a change of the kernels or of the toolchain.  The pooled comparison holds below the fp16 normal range (outputs
k 2^-124): the packed maximum keeps fp16 denormals, as the kernel's comment says.
With scratch copies of conv_stem.hip, one change each: the bf16 forward statistics counting r < OH + 1 failed test_forward_integer at
every shape with a partial tile, test_forward_strided_block_walk[bf16] and the summed-rows comparison of test_pooled_integer; the
strip starting at cs * PCOLS failed every test_pooled_*; the block walk without its sum reset failed both
test_forward_strided_block_walk; the reduce kernel without its tail loop failed every test_wgrad_*.  The sweep found no kernel wrong."""
import numpy as np
import pytest
import torch

from tests import bn_emulation as BN
from tests import stem_emulation as S
from tests.gpu_util import Guarded, hp_pack

pytestmark = pytest.mark.gpu

OK = 0
EXCESS = {}


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return S.bind(BN.bind(lib())), ptr, stream()


def _check(what, rc, outs):
    assert rc == OK, f"{what}: returned {rc}"
    torch.cuda.synchronize()
    for k, G in outs.items():
        assert G.guards_intact(), f"{what} {k}: guard band overwritten"
        n = int(torch.isnan(G.t.float()).sum())
        assert n == 0, f"{what} {k}: {n} of {G.t.numel()} elements never written (or NaN)"


def _note(key, ex, tau):
    EXCESS[key] = max(EXCESS.get(key, 0.0), ex)
    print(f"   excess[{key}] = {ex:.3e} of max |ref| (tau {tau:.1e})")


def _act_dtype(prec):
    return torch.bfloat16 if prec == S.BF16 else torch.float32


def _pack_x(L, ptr, st, x, prec):
    """x [B][3][IH][IW] cpu fp32 -> the packed image of the arithmetic (ph_debug_bn_pack_input)."""
    B, _, IH, IW = x.shape
    xd = x.contiguous().cuda()
    hp = prec in (S.FP16X3, S.FP16X1)
    x4 = torch.zeros(B * IH * IW * 4 * (2 if hp else 1), dtype=torch.float16 if hp else _act_dtype(prec), device="cuda")
    assert x4.data_ptr() % 256 == 0
    rc = L.ph_debug_bn_pack_input(ptr(xd), ptr(x4), B, IH, IW, S.FP16X3 if hp else prec, st)
    assert rc == OK
    torch.cuda.synchronize()
    return x4


def _pack_w(L, ptr, st, w, prec):
    wd = w.contiguous().cuda()
    pk = Guarded((L.ph_debug_stem_weight_bytes(),), torch.uint8, 0)
    _check("pack_weights", L.ph_debug_stem_pack_weights(ptr(wd), ptr(pk.t), prec, st), {})
    assert pk.guards_intact()
    return pk


def _grad(dy, prec, scale=1.0):
    """dy [B][64][OH][OW] cpu fp32 -> the gradient tensor the weight-gradient kernel reads."""
    t = S.nhwc(dy).cuda()
    if prec == S.BF16:
        return t.bfloat16()
    if prec in (S.FP16X3, S.FP16X1):
        return hp_pack(t, scale)
    return t


_REF = {}


def _ints(shape, xmax=2):
    """Integer operands of a shape and their float64 results: computed once, shared, never modified."""
    key = (shape, xmax)
    if key not in _REF:
        x, w, dy = S.operands_int(*shape, seed=S.case_seed(shape), xmax=xmax)
        _REF[key] = dict(x=x, w=w, dy=dy, y=S.fwd(x, w, S.BF16))
    return _REF[key]


def _fwd_stats_ref(r, shape):
    if "stats" not in r:
        r["stats"] = S.fwd_stats(S.fwd_extended(r["x"], r["w"]), S.conv_map(shape[1]), S.conv_map(shape[2]))
    return r["stats"]


def _run_fwd(L, ptr, st, x4, pk, shape, prec, cap=0):
    B, IH, IW = shape
    OH, OW = S.conv_map(IH), S.conv_map(IW)
    nb = L.ph_debug_stem_stat_parts(B, OH, OW)
    assert nb == S.stat_parts(*shape)
    out, stats = Guarded((B, OH, OW, 64), _act_dtype(prec)), Guarded((nb, 2, 64), torch.float32)
    rc = L.ph_debug_stem_fwd(ptr(x4), ptr(pk.t), ptr(out.t), ptr(stats.t), B, IH, IW, prec, cap, st)
    _check(f"stem_fwd {shape} {S.NAMES[prec]} cap {cap}", rc, {"out": out, "stats": stats})
    return out, stats


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape", S.FWD_SHAPES)
def test_forward_integer(shape):
    L, ptr, st = _api()
    r = _ints(shape)
    for prec in S.FWD_PRECS:
        x4, pk = _pack_x(L, ptr, st, r["x"], prec), _pack_w(L, ptr, st, r["w"], prec)
        out, stats = _run_fwd(L, ptr, st, x4, pk, shape, prec)
        what = f"{shape} {S.NAMES[prec]}"
        assert S.mismatches(r["y"], out.t.float().cpu()) == 0, what
        assert S.mismatches(_fwd_stats_ref(r, shape), stats.t.cpu()) == 0, what


@pytest.mark.parametrize("shape", S.FWD_RANDOM)
def test_forward_random(shape):
    L, ptr, st = _api()
    x, w, _, _ = S.operands_rand(*shape, seed=S.case_seed(shape))
    bad = []
    for prec in S.FWD_PRECS:
        x4, pk = _pack_x(L, ptr, st, x, prec), _pack_w(L, ptr, st, w, prec)
        out, _ = _run_fwd(L, ptr, st, x4, pk, shape, prec)
        ok, ex = S.within(S.fwd(x, w, prec), out.t.float().cpu(), prec, perf=prec == S.BF16)
        _note(f"fwd {S.NAMES[prec]}", ex, S.TAU[prec])
        if not ok:
            bad.append((S.NAMES[prec], ex))
    assert not bad, bad


@pytest.mark.parametrize("prec", S.WALK_PRECS)
def test_forward_strided_block_walk(prec):
    """45 tiles = 6 blocks walked by 6 (grid_cap 0), 4 and 1 workgroups: output and every statistics row bitwise the same - on random
    operands, whose sums depend on their order - and the uncapped run against float64 in both classes."""
    L, ptr, st = _api()
    shape = S.WALK_SHAPE
    r = _ints(shape)
    x, w, _, _ = S.operands_rand(*shape, seed=S.case_seed(shape))
    for cls, (xx, ww) in (("integer", (r["x"], r["w"])), ("random", (x, w))):
        x4, pk = _pack_x(L, ptr, st, xx, prec), _pack_w(L, ptr, st, ww, prec)
        base = None
        for cap in S.WALK_CAPS:
            out, stats = _run_fwd(L, ptr, st, x4, pk, shape, prec, cap)
            got = (out.buf.clone(), stats.buf.clone())
            if cap == 0:
                base = got
                o = out.t.float().cpu()
                if cls == "integer":
                    assert S.mismatches(r["y"], o) == 0
                    assert S.mismatches(_fwd_stats_ref(r, shape), stats.t.cpu()) == 0
                else:
                    ok, ex = S.within(S.fwd(xx, ww, prec), o, prec, perf=prec == S.BF16)
                    _note(f"fwd walk {S.NAMES[prec]}", ex, S.TAU[prec])
                    assert ok, ex
            else:
                assert torch.equal(got[0], base[0]), f"{cls} cap {cap}: the output differs from the uncapped run's"
                assert torch.equal(got[1], base[1]), f"{cls} cap {cap}: statistics rows differ from the uncapped run's"


# ------------------------------------------------------------------------------------------------ pooled forward
def _run_pool(L, ptr, st, x, w, shape, gamma):
    B, IH, IW = shape
    OH, OW = S.conv_map(IH), S.conv_map(IW)
    nb = L.ph_debug_stem_pool_stat_parts(B, OH, OW)
    assert nb == S.pool_stat_parts(*shape)
    x4, pk = _pack_x(L, ptr, st, x, S.BF16), _pack_w(L, ptr, st, w, S.BF16)
    g = torch.from_numpy(gamma).cuda()
    out, stats = Guarded((B, (OH + 1) // 2, (OW + 1) // 2, 64), torch.bfloat16), Guarded((nb, 2, 64), torch.float32)
    rc = L.ph_debug_stem_fwd_pool(ptr(x4), ptr(pk.t), ptr(out.t), ptr(stats.t), ptr(g), B, IH, IW, S.BF16, st)
    _check(f"stem_fwd_pool {shape}", rc, {"pooled": out, "stats": stats})
    return out, stats, x4, pk


@pytest.mark.parametrize("shape", S.POOL_SHAPES)
def test_pooled_integer(shape):
    L, ptr, st = _api()
    r, gamma = _ints(shape), S.pool_gamma()
    out, stats, x4, pk = _run_pool(L, ptr, st, r["x"], r["w"], shape, gamma)
    assert S.mismatches(S.pooled(r["y"], gamma), out.t.float().cpu()) == 0
    rows = stats.t.cpu()
    assert S.mismatches(S.pool_stats(r["y"]), rows) == 0
    # the forward kernel's rows on the same operands: the same whole-tensor sums (integers: exact)
    _, fstats = _run_fwd(L, ptr, st, x4, pk, shape, S.BF16)
    assert torch.equal(rows.double().sum(0), fstats.t.cpu().double().sum(0))


def test_pooled_random():
    """The pooled value is the window's extremum of the bf16-rounded reference; where an fp32 sum lies within the forward's tolerance
    (TAU of max |y|) of a rounding boundary, either neighbour."""
    L, ptr, st = _api()
    shape, gamma = S.POOL_RANDOM, S.pool_gamma()
    x, w, _, _ = S.operands_rand(*shape, seed=S.case_seed(shape))
    out, _, _, _ = _run_pool(L, ptr, st, x, w, shape, gamma)
    y = S.fwd(x, w, S.BF16)
    lo, hi = S.pooled_bounds(y, gamma, S.TAU[S.BF16] * y.abs().max())
    print(f"   pooled random: {int((lo != hi).sum())} of {lo.numel()} values may take either neighbour")
    assert S.between(lo, hi, out.t.float().cpu()) == 0


def test_pooled_below_the_fp16_normal_range():
    """Weights in {-1, 0, 1} 2^-124, image in -1 .. 1: every conv output is k 2^-124 with |k| <= 24 - a bf16 magnitude below 2^-119,
    whose bit pattern the packed fp16 maximum reads as a denormal."""
    L, ptr, st = _api()
    shape, gamma = S.POOL_TINY, S.pool_gamma()
    r = _ints(shape, xmax=1)
    y = r["y"] * 2.0 ** -124
    assert 0 < y.abs().max() < 2.0 ** -119 and torch.equal(y.float().bfloat16().double(), y)
    out, stats, _, _ = _run_pool(L, ptr, st, r["x"], r["w"] * 2.0 ** -124, shape, gamma)
    assert S.mismatches(S.pooled(y, gamma), out.t.float().cpu()) == 0
    assert S.mismatches(S.pool_stats(y), stats.t.cpu()) == 0


# ------------------------------------------------------------------------------------------------ weight gradient
def _run_wgrad(L, ptr, st, x4, g, shape, prec, tpc, unscale=None):
    B, IH, IW = shape
    nbytes = L.ph_debug_stem_wgrad_slab_bytes(B, IH, IW, tpc)
    nt = S.tiles(*shape)[2]
    assert nbytes == (S.plan_chunks(nt)[0] if tpc == 0 else S.cdiv(nt, tpc)) * 7 * 64 * 32 * 4
    slab, dw = Guarded((nbytes // 4,), torch.float32), Guarded((64, 3, 7, 7), torch.float32)
    us = None if unscale is None else torch.tensor(unscale, dtype=torch.float32, device="cuda")
    rc = L.ph_debug_stem_wgrad(ptr(x4), ptr(g), ptr(slab.t), ptr(dw.t), B, IH, IW, prec, tpc, ptr(us), st)
    _check(f"stem_wgrad {shape} {S.NAMES[prec]} tpc {tpc}", rc, {"slab": slab, "dw": dw})
    return slab, dw


def _wgrad_integer(shape, tpcs, precs=S.WG_PRECS):
    L, ptr, st = _api()
    r = _ints(shape)
    if "tiles" not in r:
        r["tiles"] = S.wgrad_tiles(r["x"], r["dy"])
    for prec in precs:
        x4, g = _pack_x(L, ptr, st, r["x"], prec), _grad(r["dy"], prec)
        for tpc in tpcs:
            slab, dw = _run_wgrad(L, ptr, st, x4, g, shape, prec, tpc)
            sl = S.slab(r["tiles"], tpc)
            what = f"{shape} {S.NAMES[prec]} tiles_per_chunk {tpc}"
            assert S.mismatches(sl, slab.t.cpu()) == 0, what + ": slab"
            assert S.mismatches(S.dw_of_slab(sl), dw.t.cpu()) == 0, what + ": dw"


@pytest.mark.parametrize("shape", S.WG_SHAPES)
def test_wgrad_integer(shape):
    """(3, 34, 66): 27 tiles in chunks of 1, 2, 4, 7, 27 tiles and by the plan's rule (27, 14, 7, 4, 1 chunks): one float64 dw."""
    _wgrad_integer(shape, S.WG_TPC if shape == S.WG_SHAPES[2] else (0, 2))


def test_wgrad_integer_45_chunks():
    _wgrad_integer(*S.WG_MANY[:1], (S.WG_MANY[1],))


def test_wgrad_random():
    L, ptr, st = _api()
    shape = S.WG_RANDOM
    x, _, _, dy_w = S.operands_rand(*shape, seed=S.case_seed(shape))
    bad = []
    for prec in S.WG_PRECS:
        x4, g = _pack_x(L, ptr, st, x, prec), _grad(dy_w, prec)
        ref = S.wgrad(x, dy_w, prec)
        for tpc in (0, 4):
            _, dw = _run_wgrad(L, ptr, st, x4, g, shape, prec, tpc)
            ok, ex = S.within(ref, dw.t.cpu(), prec)
            _note(f"wgrad {S.NAMES[prec]}", ex, S.TAU[prec])
            if not ok:
                bad.append((S.NAMES[prec], tpc, ex))
    assert not bad, bad


def test_wgrad_unscale():
    """dw = the float64 gradient of the tensor the kernel read, times unscale[1]: bf16 (integers, exact) and the half-pair mode, whose dz
    is stored under the power-of-two scale unscale[0]."""
    L, ptr, st = _api()
    shape = S.WG_SHAPES[1]
    r = _ints(shape)
    x4 = _pack_x(L, ptr, st, r["x"], S.BF16)
    _, dw = _run_wgrad(L, ptr, st, x4, _grad(r["dy"], S.BF16), shape, S.BF16, 2, (4.0, 0.25))
    ref = S.dw_of_slab(S.slab(S.wgrad_tiles(r["x"], r["dy"]), 2))
    assert S.mismatches(ref * 0.25, dw.t.cpu()) == 0
    x, _, _, dy_w = S.operands_rand(*shape, seed=S.case_seed(shape))
    x4 = _pack_x(L, ptr, st, x, S.FP16X3)
    _, dw = _run_wgrad(L, ptr, st, x4, _grad(dy_w, S.FP16X3, 256.0), shape, S.FP16X3, 0, (256.0, 1.0 / 256))
    ok, ex = S.within(S.wgrad(x, dy_w * 256.0, S.FP16X3) / 256.0, dw.t.cpu(), S.FP16X3)
    _note("wgrad fp16x3 unscale", ex, S.TAU[S.FP16X3])
    assert ok, ex


# ------------------------------------------------------------------------------------------------ fused weight gradient
def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("shape", S.FUSED_SHAPES)
@pytest.mark.parametrize("cls", ["exact", "real"])
def test_wgrad_fused(shape, cls):
    """dpool, idx, y0 and the constants as the stem-backward entries take them (c1 / c2 of the real class from the reduce and finalize
    entries); dz by the separate apply entry.  The fused dw is bitwise the unfused kernel's fed that dz, slab included; the dz-fed dw
    against float64 on the same dz: equal values in the exact class (gamma invstd = 1, c1 = c2 = 0, integer image: dz is the masked
    scatter, multiples of 1 / 8), within the worst case of a float32 sum in the real class."""
    L, ptr, st = _api()
    B, IH, IW = shape
    OH, OW = S.conv_map(IH), S.conv_map(IW)
    i = BN._stem_inp(BN.BF16, B, OH, OW, "pixel", cls == "exact", S.case_seed(shape))
    if cls == "exact":
        i.update(gamma=np.ones(64, np.float32), invstd=np.ones(64, np.float32), c1=np.zeros(64, np.float32), c2=np.zeros(64, np.float32))
        x = _ints(shape)["x"]
    else:
        x = S.operands_rand(*shape, seed=S.case_seed(shape))[0]
    dpool, idx, y0 = _d(i["dpool"], torch.bfloat16), _d(i["idx"].astype(np.uint8)), _d(i["y"], torch.bfloat16)
    cst = {k: _d(i[k]) for k in ("mean", "invstd", "scale", "shift", "gamma", "c1", "c2")}
    if cls == "real":
        nb = L.ph_debug_bn_stem_bwd_parts(B, OH)
        parts, c1, c2 = Guarded((nb, 2, 64), torch.float32), Guarded((64,), torch.float32), Guarded((64,), torch.float32)
        rc = L.ph_debug_bn_stem_bwd_reduce(ptr(dpool), ptr(idx), ptr(y0), None, ptr(cst["mean"]), ptr(cst["invstd"]), ptr(cst["scale"]),
                                           ptr(cst["shift"]), ptr(parts.t), B, OH, OW, 64, S.BF16, None, 0, st)
        _check("stem_bwd_reduce", rc, {"parts": parts})
        rc = L.ph_debug_bn_bwd_finalize(ptr(parts.t), nb, 64, float(B * OH * OW), None, None, ptr(c1.t), ptr(c2.t), None, 0, None, None,
                                        None, st)
        _check("bn_bwd_finalize", rc, {"c1": c1, "c2": c2})
        cst["c1"], cst["c2"] = c1.t, c2.t
    dz = Guarded((B, OH, OW, 64), torch.bfloat16)
    rc = L.ph_debug_bn_stem_bwd_apply(ptr(dpool), ptr(idx), ptr(y0), ptr(cst["mean"]), ptr(cst["invstd"]), ptr(cst["scale"]), ptr(cst["shift"]),
                                      ptr(cst["gamma"]), ptr(cst["c1"]), ptr(cst["c2"]), ptr(dz.t), B, OH, OW, 64, S.BF16, None, st)
    _check("stem_bwd_apply", rc, {"dz": dz})
    x4 = _pack_x(L, ptr, st, x, S.BF16)
    dzc = dz.t.float().cpu().permute(0, 3, 1, 2).contiguous()
    assert dzc.abs().max() > 0
    if cls == "exact":
        assert S.mismatches(BN.stem_bwd_apply(i, BN.F64)["dy"], dz.t.float().cpu()) == 0
        ref = S.dw_of_slab(S.slab(S.wgrad_tiles(x, dzc), 0))
    else:
        ref, allow = S.wgrad(x, dzc, S.BF16), S.sum_bound(x, dzc)
    for tpc in (0, 4):
        slab_u, dw_u = _run_wgrad(L, ptr, st, x4, dz.t, shape, S.BF16, tpc)
        nbytes = L.ph_debug_stem_wgrad_slab_bytes(B, IH, IW, tpc)
        slab_f, dw_f = Guarded((nbytes // 4,), torch.float32), Guarded((64, 3, 7, 7), torch.float32)
        rc = L.ph_debug_stem_wgrad_fused(ptr(x4), ptr(y0), ptr(dpool), ptr(idx), ptr(cst["mean"]), ptr(cst["invstd"]), ptr(cst["scale"]),
                                         ptr(cst["shift"]), ptr(cst["gamma"]), ptr(cst["c1"]), ptr(cst["c2"]), ptr(slab_f.t), ptr(dw_f.t),
                                         B, IH, IW, S.BF16, tpc, None, st)
        _check(f"stem_wgrad_fused {shape} tpc {tpc}", rc, {"slab": slab_f, "dw": dw_f})
        assert torch.equal(slab_f.buf, slab_u.buf), f"tpc {tpc}: the fused slab is not bitwise the dz-fed one"
        assert torch.equal(dw_f.buf, dw_u.buf), f"tpc {tpc}: the fused dw is not bitwise the dz-fed one"
        if cls == "exact":
            assert S.mismatches(ref, dw_u.t.cpu()) == 0
        else:
            err = ((dw_u.t.cpu().double() - ref).abs().max() / ref.abs().max()).item()
            print(f"   fused {shape} tpc {tpc}: dz-fed dw against float64 {err:.3e} of max |ref| (allowance up to {(allow / ref.abs().max()).max().item():.1e})")
            assert S.outside(ref, dw_u.t.cpu(), allow) == 0

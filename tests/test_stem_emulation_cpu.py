"""CPU self-test of tests/stem_emulation.py, on the operands and shapes of tests/test_gpu_stem.py:

  - the restatement agrees with torch float64 (F.conv2d, autograd's weight gradient, F.max_pool2d) and with itself (every statistics
    row set sums to the whole tensor's sums; the integer class gives the same values in every arithmetic and in float32);
  - conv_emulation.TAU holds for the stem: the float32 stand-in stays a factor 4 inside it and every single dropped product a factor 4
    outside, in every arithmetic, forward and weight gradient (the figures are printed and recorded in stem_emulation.STAND_IN);
  - every injected defect is rejected by the very comparison the GPU test calls (`mismatches`, `within`, `between`)."""
import pytest
import torch
import torch.nn.functional as F

from tests import stem_emulation as S

torch.set_num_threads(min(16, torch.get_num_threads()))


def _int(shape, **kw):
    return S.operands_int(*shape, seed=S.case_seed(shape), **kw)


def _rand(shape):
    return S.operands_rand(*shape, seed=S.case_seed(shape))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shape", S.FWD_SHAPES + (S.WALK_SHAPE,))
def test_forward_restatement_on_integer_operands(shape):
    B, IH, IW = shape
    OH, OW = S.conv_map(IH), S.conv_map(IW)
    x, w, _ = _int(shape)
    y = S.fwd(x, w, S.BF16)
    assert torch.equal(y, S.nhwc(F.conv2d(x.double(), w.double(), None, 2, 3)))
    assert torch.equal(y, y.round()) and y.abs().max() <= 48
    for prec in S.FWD_PRECS:                                   # integers: the low planes are zero, every order gives the same sums
        assert torch.equal(S.fwd(x, w, prec), y)
        assert S.mismatches(y, S.fwd(x, w, prec, acc=torch.float32)) == 0
    ye = S.fwd_extended(x, w)
    assert torch.equal(ye[:, :OH, :OW], y)
    rows = S.fwd_stats(ye, OH, OW)
    assert rows.shape[0] == S.stat_parts(*shape)
    assert torch.equal(rows.sum(0), torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))]))
    assert rows[:, 1].max() < 2 ** 24


@pytest.mark.parametrize("shape", S.POOL_SHAPES)
def test_pooled_restatement_on_integer_operands(shape):
    B, IH, IW = shape
    x, w, _ = _int(shape)
    y = S.fwd(x, w, S.BF16)
    OH, OW = y.shape[1:3]
    rows = S.pool_stats(y)
    assert rows.shape[0] == S.pool_stat_parts(*shape)
    assert torch.equal(rows.sum(0), S.fwd_stats(S.fwd_extended(x, w), OH, OW).sum(0))
    gamma = S.pool_gamma()
    p = S.pooled(y, gamma)
    assert p.shape[1:3] == ((OH + 1) // 2, (OW + 1) // 2)
    for b, ph, pw, c in ((0, 0, 0, 0), (B - 1, p.shape[1] - 1, p.shape[2] - 1, 1), (0, p.shape[1] // 2, p.shape[2] - 1, 5), (0, p.shape[1] - 1, 0, 2)):
        win = y[b, max(0, 2 * ph - 1):2 * ph + 2, max(0, 2 * pw - 1):2 * pw + 2, c]
        assert p[b, ph, pw, c] == (win.min() if gamma[c] < 0 else win.max())


def test_cut_strips_are_cut():
    assert S.pool_nsplit(1, 65, 10) == 2 and S.pool_nsplit(2, 128, 6) == 4 and S.pool_nsplit(1, 9, 29) == 1
    assert [S.conv_map(s[2]) for s in S.POOL_SHAPES[:4]] == [14, 15, 16, 29]


@pytest.mark.parametrize("shape", S.WG_SHAPES + (S.WG_MANY[0],))
def test_weight_gradient_restatement_on_integer_operands(shape):
    x, w, dy = _int(shape)
    tl = S.wgrad_tiles(x, dy)
    wv = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wv, None, 2, 3).backward(dy.double())
    for tpc in S.WG_TPC:
        sl = S.slab(tl, tpc)
        assert torch.equal(S.dw_of_slab(sl), wv.grad)
    assert [S.slab(tl, t).shape[0] for t in (1, 2, 4, 7, 27)] == [S.cdiv(tl.shape[0], t) for t in (1, 2, 4, 7, 27)]
    for prec in S.WG_PRECS:
        assert torch.equal(S.wgrad(x, dy, prec), wv.grad)
    assert tl.abs().max() < 2 ** 24 and tl[..., 7, :3].abs().max() > 0 and tl[..., 3].abs().max() == 0


# ------------------------------------------------------------------------------------------------ TAU on the stem's operands
def _tau_rows(kind, a, b, precs, perf_prec):
    rows, bad = [], []
    for prec in precs:
        perf = prec == perf_prec
        fn = S.fwd if kind == "fwd" else S.wgrad
        ref = fn(a, b, prec)
        noisy = fn(a, b, prec, acc=torch.float32)
        if perf:
            noisy = S.bf16r(noisy)
        ok, ex = S.within(ref, noisy, prec, perf)
        rows.append((kind, S.NAMES[prec], "fp32", ex))
        if ex * S.MARGIN > S.TAU[prec]:
            bad.append((kind, S.NAMES[prec], "accepts", ex))
        if len(S.E.PRODUCTS[prec]) > 1:
            for k in range(len(S.E.PRODUCTS[prec])):
                ok, rej = S.within(ref, fn(a, b, prec, acc=torch.float32, drop=k), prec, perf)
                rows.append((kind, S.NAMES[prec], f"-{S.E.PRODUCTS[prec][k][:2]}", rej))
                if ok or rej < S.MARGIN * S.TAU[prec]:
                    bad.append((kind, S.NAMES[prec], f"rejects {S.E.PRODUCTS[prec][k][:2]}", rej))
    for r in rows:
        print("  %-6s %-7s %-10s excess %.3e" % r, " tau %.1e" % S.TAU[[k for k, v in S.NAMES.items() if v == r[1]][0]])
    return bad


@pytest.mark.parametrize("shape", S.FWD_RANDOM)
def test_tau_forward(shape):
    x, w, _, _ = _rand(shape)
    assert not _tau_rows("fwd", x, w, S.FWD_PRECS, S.BF16)


def test_tau_weight_gradient():
    x, _, _, dy_w = _rand(S.WG_RANDOM)
    assert not _tau_rows("wgrad", x, dy_w, S.WG_PRECS, None)


# ------------------------------------------------------------------------------------------------ injected defects
def test_forward_defects_are_rejected():
    shape = S.FWD_SHAPES[1]                                     # (1, 14, 30): a partial tile in both directions
    x, w, _ = _int(shape)
    OH, OW = S.conv_map(shape[1]), S.conv_map(shape[2])
    ye = S.fwd_extended(x, w)
    assert S.mismatches(S.fwd_stats(ye, OH, OW), S.fwd_stats(ye, OH, OW, "oob_counted")) > 0
    shape = S.WALK_SHAPE
    x, w, _ = _int(shape)
    OH, OW = S.conv_map(shape[1]), S.conv_map(shape[2])
    ye = S.fwd_extended(x, w)
    for grid in (4, 1):
        assert S.mismatches(S.fwd_stats(ye, OH, OW), S.fwd_stats(ye, OH, OW, "no_reset", grid)) > 0
    shape = S.FWD_SHAPES[4]                                     # three images
    x, w, _ = _int(shape)
    assert S.mismatches(S.fwd(x, w, S.BF16), S.fwd(x, w, S.BF16, defect="halo_neighbour")) > 0


def test_pooled_defects_are_rejected():
    gamma = S.pool_gamma()
    for shape in S.POOL_SHAPES:
        x, w, _ = _int(shape)
        y = S.fwd(x, w, S.BF16)
        B, OH, OW, _ = y.shape
        if OW > S.PCOLS:
            assert S.mismatches(S.pool_stats(y), S.pool_stats(y, "shared_column_twice")) > 0
        if S.pool_nsplit(B, OH, OW) > 1:
            assert S.mismatches(S.pool_stats(y), S.pool_stats(y, "cut_row_twice")) > 0
        assert S.mismatches(S.pooled(y, gamma), S.pooled(y, gamma, "max_everywhere")) > 0
        if OH % 2 or OW % 2:
            assert S.mismatches(S.pooled(y, gamma), S.pooled(y, gamma, "last_window_dropped")) > 0
    assert any(S.conv_map(s[1]) % 2 for s in S.POOL_SHAPES) and any(S.conv_map(s[2]) % 2 for s in S.POOL_SHAPES)
    # the random class: the bounds reject the same defects, and accept the float32 stand-in
    x, w, _, _ = _rand(S.POOL_RANDOM)
    y = S.fwd(x, w, S.BF16)
    lo, hi = S.pooled_bounds(y, gamma, S.TAU[S.BF16] * y.abs().max())
    assert S.between(lo, hi, S.pooled(S.bf16r(S.fwd(x, w, S.BF16, acc=torch.float32)), gamma)) == 0
    assert (lo != hi).sum() < 0.01 * lo.numel()
    for d in ("max_everywhere", "last_window_dropped"):
        assert S.between(lo, hi, S.pooled(S.bf16r(y), gamma, d)) > 0


def test_weight_gradient_defects_are_rejected():
    for shape, tpcs in ((S.WG_SHAPES[2], S.WG_TPC), (S.WG_MANY[0], (S.WG_MANY[1],))):
        x, _, dy = _int(shape)
        tl = S.wgrad_tiles(x, dy)
        for tpc in tpcs:
            sl = S.slab(tl, tpc)
            ref = S.dw_of_slab(sl)
            assert S.mismatches(ref, S.dw_of_slab(sl, defect="kh6_missing")) > 0
            if sl.shape[0] > 1:
                assert S.mismatches(ref, S.dw_of_slab(sl, defect="last_chunk_dropped")) > 0
            if sl.shape[0] > 3:
                assert S.mismatches(ref, S.dw_of_slab(sl, defect="lane_tail_dropped")) > 0
    x, _, dy, dy_w = _rand(S.WG_RANDOM)
    dz = dy.bfloat16().float()                                  # the fused case's class: a dense bf16 dz
    ref = S.wgrad(x, dz, S.BF16)
    allow = S.sum_bound(x, dz)
    assert S.outside(ref, S.wgrad(x, dz, S.BF16, acc=torch.float32), allow) == 0
    assert (allow / ref.abs().max()).max() < 1e-2
    tl = S.wgrad_tiles(x.bfloat16().float(), dz)
    for tpc in (0, 4):
        sl = S.slab(tl, tpc)
        assert S.outside(ref, S.dw_of_slab(sl), allow) == 0
        for d in ("kh6_missing", "last_chunk_dropped", "lane_tail_dropped"):
            assert S.outside(ref, S.dw_of_slab(sl, defect=d), allow) > 0
    for prec in S.WG_PRECS:
        ref = S.wgrad(x, dy_w, prec)
        bad = ref.clone()
        bad[:, :, 6] = 0
        assert not S.within(ref, bad, prec)[0]

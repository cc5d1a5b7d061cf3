"""CPU self-test of tests/bn_emulation.py: the tolerances of the BatchNorm / pooling / stem-backward sweep (tests/test_gpu_bn_act.py)
accept the float32 restatement of every operator on every case and reject each injected defect by a factor of MARGIN (4) or more (an
array of the exact class rejects by not being equal); the exact class is what it claims (the float64 reference, cast to the output
type, is the float32 restatement bit for bit); the float64 references agree with torch float64 (F.batch_norm, F.max_pool2d with
return_indices, F.adaptive_avg_pool2d and autograd), so the implementation is not its own oracle; the case tables reach every value
the sweep is meant to cross."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_emulation as E

F64 = np.float64
DEFECTS = {"drop_last_block": "the last partial vector block dropped", "drop_ragged": "the ragged last iteration of a reduce block dropped",
           "drop_tail_iter": "the tail iteration of the grid-stride loop dropped",
           "neighbour_cg": "per-channel constants of the neighbouring channel group", "relu_ge": "a ReLU mask with >= 0",
           "mask_from_a": "the mask taken from a where mscale / mshift was asked for", "last_max": "arg-max where the last maximum wins",
           "code_kw_kh": "arg-max code kw * 3 + kh", "pad_counted": "padding taps counted into the maximum", "oh_floor": "OH = H / 2",
           "window_missing": "one of the four windows missing from the stem scatter on odd rows",
           "amax_no_4": "the stem amax without the factor 4", "dzs_exp_off": "the dzs exponent off by one",
           "dzs_not_reciprocal": "dzs not the reciprocal pair", "s2_no_invstd": "the fused form's s2 without invstd",
           "row2_swapped": "row2 1 and 2 swapped", "biased_running": "the biased variance written to the running statistics",
           "var_unclamped": "variance not clamped at 0", "momentum_swapped": "momentum applied to the wrong term",
           "nbt_per_channel": "num_batches_tracked advanced once per channel",
           "lane_rounded_count": "average pool dividing by the lane-rounded pixel count",
           "no_accumulate": "accumulate ignored in the average-pool backward",
           "shortcut_unrounded": "the relu & 2 shortcut term not rounded to the activation type", "out32_differs": "out32 differing from out",
           "ch3_nonzero": "the 4th channel of the packed input not zero", "planes_swapped": "the hi and lo planes of the packed input swapped"}


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float16 or b.dtype == np.float16:
        return bool((a.astype(np.float16).view(np.uint16) == b.astype(np.float16).view(np.uint16)).all())
    if a.dtype.kind == "f":
        return bool((a.astype(np.float32).view(np.int32) == b.astype(np.float32).view(np.int32)).all())
    return bool((a == b).all())


def defect_ratio(e, outs):
    """How far the outputs `outs` of suite entry e lie outside: inf if an exact array differs, else the largest error / tolerance."""
    r = 0.0
    for k, ref in e["ref"].items():
        if k in e["exact"]:
            if not _same_bits(e["rest"][k], outs[k]):
                return np.inf
            continue
        tol, er = E.entry_tolerance(e, k), E.err(ref, outs[k])
        r = max(r, er / tol if tol > 0 else (np.inf if er > 0 else 0.0))
    return r


@pytest.mark.parametrize("op", E.OPS)
def test_restatement_inside_and_defects_outside_the_tolerance(op):
    worst_rest, worst_tol, ratios, bad = 0.0, 0.0, {}, []
    for e in E.suite(op):
        for k, ref in e["ref"].items():
            if k in e["exact"]:
                if not _same_bits(E.cast(e, k), e["rest"][k]):
                    bad.append(f"{e['name']} {k}: the float32 restatement is not the float64 reference cast to the output type")
                if ref.dtype.kind == "f" and ref.dtype != np.float16 and k != "x4":
                    if not np.array_equal(ref.astype(np.float32).astype(F64), ref, equal_nan=True):
                        bad.append(f"{e['name']} {k}: the exact result is no float32")
                continue
            tol, er, sc = E.entry_tolerance(e, k), E.err(ref, e["rest"][k]), max(E.scale(ref), 1e-300)
            worst_rest, worst_tol = max(worst_rest, er / sc), max(worst_tol, tol / sc)
            if not er <= tol:
                bad.append(f"{e['name']} {k}: restatement {er:.3e} > tol {tol:.3e}")
        for d, outs in e["defects"].items():
            r = defect_ratio(e, outs)
            ratios[d] = min(ratios.get(d, np.inf), r)
            if not r >= E.MARGIN:
                bad.append(f"{e['name']}: defect {d} only {r:.2f} x the tolerance")
    print(f"\n{op:<22s} restatement {worst_rest:.2e}  tolerance {worst_tol:.2e} (of max |ref|)  smallest defect ratio: "
          + (", ".join(f"{d} {r:.3g}" for d, r in ratios.items()) or "-"))
    assert not bad, "\n".join(bad[:40])


def test_every_listed_defect_is_injected_somewhere():
    seen = {}
    for op in E.OPS:
        for e in E.suite(op):
            for d in e["defects"]:
                seen.setdefault(d, set()).add(E.base_op(op))
    assert set(seen) == set(DEFECTS), set(seen) ^ set(DEFECTS)
    assert seen["drop_tail_iter"] == {"bn_apply", "bn_bwd_apply"} and seen["drop_last_block"] == {"bn_apply", "bn_bwd_apply"}
    assert seen["neighbour_cg"] == {"bn_apply", "bn_bwd_reduce", "bn_bwd_apply"}
    assert seen["relu_ge"] == seen["mask_from_a"] == {"bn_bwd_reduce", "bn_bwd_apply"}
    assert seen["window_missing"] == {"stem_bwd_reduce", "stem_bwd_apply"}


# ------------------------------------------------------------------------------------------------ the references against torch float64
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64))


def _close(a, b, what, tol=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = np.abs(a - b).max() if a.size else 0.0
    assert d <= tol * max(1.0, np.abs(b).max()), (what, d)


def test_batchnorm_forward_reference_is_torch_batch_norm():
    rng = np.random.default_rng(0)
    for nparts, n, C in ((1, 1, 8), (3, 7, 16), (5, 64, 8)):
        x = rng.standard_normal((nparts, n, C)) * rng.uniform(0.5, 3, C) + rng.standard_normal(C)
        x[:, :, 1] = 1.7                                                         # a constant channel
        inp = dict(parts=np.stack([x.sum(1), (x * x).sum(1)], 1), count=float(nparts * n), eps=1e-5, momentum=0.1,
                   gamma=rng.standard_normal(C), beta=rng.standard_normal(C), running=(rng.standard_normal(C), rng.uniform(0.5, 2, C)), nbt=3)
        ref = E.bn_finalize(inp, F64)
        rm, rv = _t(inp["running"][0]).clone(), _t(inp["running"][1]).clone()
        if nparts * n > 1:
            xt = _t(x.reshape(-1, C))
            y = F.batch_norm(xt, rm, rv, _t(inp["gamma"]), _t(inp["beta"]), True, float(np.float32(0.1)), float(np.float32(1e-5)))
            _close(x.reshape(-1, C) * ref["scale"] + ref["shift"], y.numpy(), "bn output", 1e-9)
            _close(ref["running_mean"], rm.numpy(), "running_mean")
            _close(ref["running_var"], rv.numpy(), "running_var", 1e-9)
            _close(ref["mean"], x.reshape(-1, C).mean(0), "mean")
            _close(ref["invstd"], 1 / np.sqrt(x.reshape(-1, C).var(0) + F64(np.float32(1e-5))), "invstd", 1e-9)
        assert ref["nbt"][0] == 4
        # the apply pass and the eval parameters
        a = dict(prec=E.BF16X6, npix=nparts * n, C=C, relu=1, out32=0, res_as_t=0, res=rng.standard_normal((nparts * n, C)), y_r=None,
                 y=x.reshape(-1, C), scale=ref["scale"], shift=ref["shift"])
        if nparts * n > 1:
            want = F.relu(F.batch_norm(_t(a["y"]), None, None, _t(inp["gamma"]), _t(inp["beta"]), True, 0.0, float(np.float32(1e-5))) + _t(a["res"]))
            _close(E.bn_apply(a, F64)["out"], want.numpy(), "bn_apply", 1e-9)
        u = dict(C=C, gamma=inp["gamma"], beta=inp["beta"], running_mean=inp["running"][0], running_var=inp["running"][1])
        ev = E.bn_eval_params(dict(units=[u], eps=1e-5, n=1), F64)
        want = F.batch_norm(_t(x.reshape(-1, C)), _t(u["running_mean"]), _t(u["running_var"]), _t(u["gamma"]), _t(u["beta"]), False, 0.0,
                            float(np.float32(1e-5)))
        _close(x.reshape(-1, C) * ev["scale"] + ev["shift"], want.numpy(), "eval", 1e-9)


def test_batchnorm_backward_reference_is_torch_autograd():
    """relu(batch_norm(y)) backward: reduce (one block's rows added up), finalize and apply against autograd."""
    rng = np.random.default_rng(1)
    for npix, C in ((33, 64), (300, 128)):
        y, g = rng.standard_normal((npix, C)), rng.standard_normal((npix, C))
        gamma, beta = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C), rng.standard_normal(C)
        yt, gt, bt = _t(y).requires_grad_(), _t(gamma).requires_grad_(), _t(beta).requires_grad_()
        out = F.relu(F.batch_norm(yt, None, None, gt, bt, True, 0.0, 1e-5))
        out.backward(_t(g))
        mean, var = y.mean(0), y.var(0)
        istd = 1 / np.sqrt(var + 1e-5)
        i = dict(prec=E.BF16X6, npix=npix, C=C, a=None, mscale=gamma * istd, mshift=beta - mean * gamma * istd, amax=False, g=g, y=y,
                 mean=mean, invstd=istd, gamma=gamma, dzs=None)
        parts = E.bn_bwd_reduce(i, F64)["parts"]
        assert parts.shape == (E.bn_bwd_parts(npix, C), 2, C)
        fin = E.bn_bwd_finalize(dict(parts=parts, row2=1, fused=False, count=float(npix), dgb=1, amax=None), F64)
        _close(fin["dbeta"], bt.grad.numpy(), "dbeta", 1e-10)
        _close(fin["dgamma"], gt.grad.numpy(), "dgamma", 1e-10)
        _close(E.bn_bwd_apply(dict(i, c1=fin["c1"], c2=fin["c2"]), F64)["dy"], yt.grad.numpy(), "dy", 1e-9)
        # the same with the mask taken from the activation, and the fused rows (sum dz (y - mean), scaled by invstd in the finalize)
        ia = dict(i, a=out.detach().numpy(), mscale=None, mshift=None)
        _close(E.bn_bwd_reduce(ia, F64)["parts"], parts, "mask from a")
        fused = np.stack([parts[:, 0], parts[:, 1] * 7, parts[:, 1] / istd], 1)
        f2 = E.bn_bwd_finalize(dict(parts=fused, row2=2, fused=True, count=float(npix), dgb=1, amax=None, invstd=istd), F64)
        _close(f2["dgamma"], gt.grad.numpy(), "fused dgamma", 1e-10)


def test_pooling_references_are_torch():
    rng = np.random.default_rng(2)
    for B, H, W in E.POOL_SHAPES + E.STEM_SHAPES:
        y = rng.integers(-8, 9, (B, H, W, 64)) / 4.0                           # ties on purpose
        sc, sf = rng.choice([0.5, 1.0, 2.0], 64) * rng.choice([-1.0, 1.0], 64), rng.integers(-4, 5, 64) / 4.0
        sf[::8] = -8
        ref = E.bn_relu_maxpool(dict(prec=E.BF16X6, y=y, scale=sc, shift=sf, idx=1, raw=1), F64)
        a = _t(np.maximum(y * sc + sf, 0).transpose(0, 3, 1, 2)).requires_grad_()
        out, ind = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        _close(ref["out"].transpose(0, 3, 1, 2), out.detach().numpy(), "max pool", 0)
        OH, OW = out.shape[2:]
        ih, iw = (ind // W).numpy(), (ind % W).numpy()
        code = (ih - (2 * np.arange(OH)[:, None] - 1)) * 3 + (iw - (2 * np.arange(OW)[None, :] - 1))
        assert np.array_equal(ref["idx"].transpose(0, 3, 1, 2), code), (B, H, W)
        assert np.array_equal(ref["raw"], np.take_along_axis(y.reshape(B, H * W, 64), ind.numpy().transpose(0, 2, 3, 1).reshape(B, -1, 64), 1)
                              .reshape(B, OH, OW, 64))
        assert (ref["out"][..., 0] == 0).all() and ref["idx"][0, 0, 0, 0] == 4          # a window of zeros: its first tap inside the image
        # the scatter of the stem backward is autograd's max-pool backward
        dp = rng.standard_normal(out.shape)
        out.backward(_t(dp))
        _close(E.stem_scatter(dp.transpose(0, 2, 3, 1), ref["idx"], H, W), a.grad.numpy().transpose(0, 2, 3, 1), "scatter", 1e-14)
        _close(E._stem_gather(dp.transpose(0, 2, 3, 1), ref["idx"], H, W), a.grad.numpy().transpose(0, 2, 3, 1), "gather", 1e-14)
    for B, HW, C in ((1, 1, 64), (3, 49, 64), (2, 33, 128)):
        x = rng.standard_normal((B, HW, C))
        xt = _t(x.transpose(0, 2, 1).reshape(B, C, HW, 1)).requires_grad_()
        out = F.adaptive_avg_pool2d(xt, 1)
        _close(E.avgpool(dict(x=x), F64)["out"], out.detach().numpy().reshape(B, C), "avgpool")
        g, dx = rng.standard_normal((B, C)), rng.standard_normal((B, HW, C))
        out.backward(_t(g.reshape(B, C, 1, 1)))
        for acc in (0, 1):
            got = E.avgpool_bwd(dict(prec=E.BF16X6, B=B, HW=HW, C=C, accumulate=acc, g=g, dx=dx), F64)["dx"]
            _close(got, xt.grad.numpy().reshape(B, C, HW).transpose(0, 2, 1) + acc * dx, "avgpool_bwd")


def test_stem_backward_reference_is_torch_autograd():
    rng = np.random.default_rng(3)
    for B, H, W in E.STEM_SHAPES:
        y = rng.standard_normal((B, H, W, 64))
        gamma, beta = rng.uniform(0.5, 1.5, 64) * rng.choice([-1.0, 1.0], 64), rng.standard_normal(64) * 0.5
        yt, gt, bt = _t(y.transpose(0, 3, 1, 2)).requires_grad_(), _t(gamma).requires_grad_(), _t(beta).requires_grad_()
        act = F.relu(F.batch_norm(yt, None, None, gt, bt, True, 0.0, 1e-5))
        out, ind = F.max_pool2d(act, 3, 2, 1, return_indices=True)
        dp = rng.standard_normal(out.shape)
        out.backward(_t(dp))
        mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2))
        istd = 1 / np.sqrt(var + 1e-5)
        sc, sf = gamma * istd, beta - mean * gamma * istd
        fwd = E.bn_relu_maxpool(dict(prec=E.BF16X6, y=y, scale=sc, shift=sf, idx=1, raw=1), F64)
        i = dict(prec=E.BF16X6, B=B, H=H, W=W, y=y, scale=sc, shift=sf, idx=fwd["idx"], raw=fwd["raw"], amax=False, dpool=dp.transpose(0, 2, 3, 1),
                 mean=mean, invstd=istd, gamma=gamma, dzs=None)
        sums = {f: E.stem_bwd_reduce(dict(i, form=f), F64)["sums"] for f in (("pixel",) if H % 2 else ("pixel", "raw"))}
        for f, s in sums.items():
            _close(s[0], bt.grad.numpy(), f + " dbeta", 1e-10)
            _close(s[1], gt.grad.numpy(), f + " dgamma", 1e-10)
        n = float(B * H * W)
        dy = E.stem_bwd_apply(dict(i, c1=sums["pixel"][0] / n, c2=sums["pixel"][1] / n), F64)["dy"]
        _close(dy, yt.grad.numpy().transpose(0, 2, 3, 1), "dy0", 1e-9)


# ------------------------------------------------------------------------------------------------ the tables
def test_tables_reach_every_listed_value():
    inp = {op: [e["inp"] for e in E.suite(op)] for op in E.OPS if not op.endswith("_stride") and not op.endswith("_clamp")}
    for op in ("bn_apply_exact", "bn_apply"):
        a = inp[op]
        assert {(c["C"], c["npix"]) for c in a} == {(x, y) for x in (64, 128, 256, 512) for y in (1, 3, 33)}
        assert {c["prec"] for c in a} == set(E.PRECS) and {c["relu"] for c in a} == {0, 1, 3}
        hp = [c for c in a if c["prec"] == E.FP16X3]
        assert {(c["out32"], c["res_as_t"]) for c in hp if c["res"] is not None} == {(0, 0), (1, 0), (0, 1), (1, 1)}
        assert any(c["y_r"] is not None and c["relu"] == 1 for c in a) and any(c["res"] is None and c["y_r"] is None and c["relu"] == 0 for c in a)
    assert 33 * 8 == 256 + 8                                           # C = 64, npix = 33: one block plus eight vectors
    assert [E.ew_grid(n) for n in E.STRIDE_N8] == [2048, 2048, 2049] and E.ew_grid(2048 * 256) == 2048
    for C in (64, 512):
        for n8 in E.STRIDE_N8:
            m8 = E.stride_npix(n8, C) * C // 8                          # a whole number of pixels: the same grid, the same last block
            assert 0 <= m8 - n8 < C // 8 and E.ew_grid(m8) == E.ew_grid(n8) and (m8 + 255) // 256 == (n8 + 255) // 256
    for op in ("bn_relu_maxpool_exact", "bn_relu_maxpool"):
        assert {(c["B"], c["H"], c["W"]) for c in inp[op]} == set(E.POOL_SHAPES) and {c["prec"] for c in inp[op]} == set(E.PRECS)
    assert {(c["idx"], c["raw"]) for c in inp["bn_relu_maxpool_exact"]} == {(0, 0), (1, 0), (1, 1)}
    ties = 0
    for e in E.suite("bn_relu_maxpool_exact"):                         # all-zero windows and ties between positive taps
        if e["inp"]["idx"]:
            assert (e["ref"]["out"][..., ::8] == 0).all()
            ties += int(((e["defects"]["last_max"]["idx"] != e["ref"]["idx"]) & (e["ref"]["out"] > 0)).sum())
    assert ties > 100
    for op in ("avgpool", "avgpool_t", "avgpool_bwd"):
        assert {(c["B"], c["HW"], c["C"]) for c in inp[op]} == {(b, h, c) for b in (1, 3) for h in (1, 31, 32, 33, 49, 256) for c in (64, 512)}
    assert {c["accumulate"] for c in inp["avgpool_bwd"]} == {0, 1}
    f = inp["bn_finalize"]
    assert {(c["nparts"], c["C"]) for c in f if c["count"] > 1} == {(n, c) for n in (1, 255, 257, 1000) for c in (64, 512)}
    assert any(c["count"] == 1 for c in f) and {c["running"] is None for c in f} == {False, True}
    for c in f:
        if c["count"] > 1:                                              # the constant channel: negative in double before the clamp
            s1, s2 = c["parts"][:, 0, 1].astype(F64).sum(), c["parts"][:, 1, 1].astype(F64).sum()
            assert s2 / c["count"] - (s1 / c["count"]) ** 2 < 0
    ev = inp["bn_eval_params"]
    assert {c["n"] for c in ev} == {1, 20} and {u["C"] for u in ev[1]["units"]} == {64, 128, 256, 512}
    for op in ("bn_bwd_reduce_exact", "bn_bwd_reduce", "bn_bwd_apply"):
        b = inp[op]
        assert {(c["C"], c["npix"]) for c in b} == {(x, y) for x in (64, 128, 256, 512) for y in (5, 33, 300, 1000)}
        assert {c["mask"] for c in b} == {"a", "m", "none"} and {c["prec"] for c in b} == set(E.PRECS)
    assert all(c["dzs"] is not None for c in inp["bn_bwd_apply"] if c["prec"] == E.FP16X3)
    per = {(C, n): -(-n // E.bn_bwd_parts(n, C)) for C in E.BWD_C for n in E.BWD_NPIX}
    assert any(p < 256 // (C // 8) for (C, n), p in per.items()) and any(n % p for (C, n), p in per.items())
    assert E.bn_bwd_parts(E.BWD_CLAMP_NPIX, 64) == 1024 and E.bn_bwd_parts(262144, 64) == 1024 and E.bn_bwd_parts(262143, 64) == 1024
    assert E.bn_bwd_parts(1, 64) == 1 and E.bn_bwd_parts(257, 64) == 2
    bf = inp["bn_bwd_finalize"]
    assert {c["nparts"] for c in bf} == {1, 3, 256, 257, 1024} and {(c["fused"], c["row2"]) for c in bf} == {(0, 1), (1, 1), (1, 2)}
    for e in E.suite("dzs"):
        j, d = e["inp"]["j"], e["ref"]["dzs"]
        assert d[0] * d[1] == 1 and np.frexp(d[0])[0] == 0.5
        if j in ("zero", "inf"):
            assert d[0] == 1
        elif -91 <= j <= 109:
            assert 2.0 ** 9 <= np.ldexp(1.5, j) * F64(d[0]) < 2.0 ** 10
        else:
            assert d[0] == np.ldexp(1.0, 100 if j < 0 else -100)
    for op in ("stem_bwd_reduce_exact", "stem_bwd_reduce", "stem_bwd_apply_exact", "stem_bwd_apply"):
        assert {(c["B"], c["H"], c["W"]) for c in inp[op]} == set(E.STEM_SHAPES) and {c["prec"] for c in inp[op]} == set(E.PRECS)
    assert {(c["H"] % 2, c["form"]) for c in inp["stem_bwd_reduce"]} == {(1, "pixel"), (0, "pixel"), (0, "raw"), (0, "pooled")}
    assert any(c["amax"] for c in inp["stem_bwd_reduce"]) and any(c["dzs"] is not None for c in inp["stem_bwd_apply"])
    assert {(c["B"], c["H"], c["W"]) for c in inp["pack_input"]} == set(E.PACK_SHAPES) and {c["prec"] for c in inp["pack_input"]} == set(E.PRECS)

"""CPU self-test of tests/dscd_emulation.py: the restatement reproduces the reference-run fixture tests/golden/dscd_forward.npz
(both criteria, both weight settings, host-drawn ranks, the three widths, two consecutive calls each); the rank by counting equals
the stable argsort on every case of the device sweep; the tolerances accept the float32 restatement on every case of the chain;
and each injected defect of dscd_emulation.DEFECTS misses by a printed factor of at least DEFECT_MARGIN (100) x the tolerance on
every case it applies to."""
import os

import numpy as np
import pytest

from tests import dscd_emulation as DE

F32, F64 = np.float32, np.float64
SEEN = {}


def _fixture_setup(g, name):
    from oracle import weights as W
    from oracle.losses import CRDState
    D = int(g[name + ".dims"][0])
    s_dim = int(g["s_dim"])
    es = W.make_state_dict(W.embed_shapes(s_dim, D), 10)
    et = W.make_state_dict(W.embed_shapes(s_dim, D), 11)
    st = CRDState(int(g["n_data"]), feat_dim=D, seed=int(g["bank_seed"]))
    mono = str(g[name + ".crit"]) == "CRDLoss_v2"
    return ((es["linear.weight"].numpy(), es["linear.bias"].numpy()),
            None if mono else (et["linear.weight"].numpy(), et["linear.bias"].numpy()),
            (st.memory_v1.numpy(), st.memory_v2.numpy()))


@pytest.mark.parametrize("name", ["v4_rw_hard", "v4_plain_hard", "v4_rw_mid", "mono_hard", "v4_rw_hard_d64", "mono_hard_d256"])
def test_restatement_reproduces_the_reference_fixture(golden_dir, name):
    """float64 chain against the reference's float64 run: 2e-6 of max |ref| (T is float32(0.07) in the package's buffer, 0.07 in the
    reference's float64 run: 1.1e-8 relative in s / T, times |s / T| <= 14.3); float32 restatement against the reference's
    float32 run: within the sum of both runs' distances from the float64 run plus 1e-6."""
    g = np.load(os.path.join(golden_dir, "dscd_forward.npz"))
    assert name in list(g["cases"])
    es, et, banks = _fixture_setup(g, name)
    r64 = DE.criterion_calls(g, name, es, et, banks, F64)
    r32 = DE.criterion_calls(g, name, es, et, banks, F32)
    keys = ["loss", "g_fs", "g_ws", "g_bs", "bank_v1_rows", "bank_v2_rows"] + (["g_wt"] if et is not None else [])
    bad = []
    for it in range(2):
        gold_sel = g["%s.sel%d" % (name, it)]
        P2 = gold_sel.shape[1]
        for r in (r64, r32):
            if not np.array_equal(r[it]["sel"][:, :P2], gold_sel):
                bad.append("%s call %d: selected columns differ" % (name, it))
        for k in keys:
            ref64, ref32 = g["%s.%s%d_f64" % (name, k, it)], g["%s.%s%d" % (name, k, it)]
            sc = DE.scale(ref64)
            e64, e32 = DE.err(ref64, r64[it][k]), DE.err(ref32, r32[it][k])
            bound32 = DE.err(ref64, ref32) + DE.err(ref64, r32[it][k]) + 1e-6 * sc
            print("%-16s call %d %-13s f64 %.2e  f32 %.2e (bound %.2e) of max |ref| %.3e" % (name, it, k, e64 / sc, e32 / sc, bound32 / sc, sc))
            if not e64 <= 2e-6 * sc:
                bad.append("%s call %d %s: float64 chain %.3e of max |ref|" % (name, it, k, e64 / sc))
            if not (e32 <= bound32 and DE.err(ref64, r32[it][k]) <= 1e-4 * sc):
                bad.append("%s call %d %s: float32 chain %.3e of max |ref|" % (name, it, k, e32 / sc))
        par64 = g["%s.params%d_f64" % (name, it)]
        zs = [("Z2", 3)] + ([("Z1", 2)] if et is not None else [])
        for zk, zi in zs:
            if not abs(float(r64[it][zk]) - par64[zi]) <= 2e-6 * par64[zi]:
                bad.append("%s call %d %s: %r against %r" % (name, it, zk, float(r64[it][zk]), par64[zi]))
            if it == 0 and F32(r32[it][zk]) != g["%s.params%d" % (name, it)][zi]:      # (the issue's probe: Z to the last bit)
                print("%s %s: float32 Z %r against the reference's %r" % (name, zk, F32(r32[it][zk]), g["%s.params%d" % (name, it)][zi]))
    sd = list(g[name + ".state_dict"])
    assert sd[-3:] == ["contrast.params:%d" % (5 if et is None else 6), "contrast.memory_v1:%dx%d" % (int(g["n_data"]), int(g[name + ".dims"][0])),
                       "contrast.memory_v2:%dx%d" % (int(g["n_data"]), int(g[name + ".dims"][0]))]
    assert not bad, "\n".join(bad)


def test_rank_by_counting_equals_the_stable_argsort():
    n_tie = 0
    for c in DE.select_cases():
        i = DE.select_inputs(c)
        ref = DE.select_ref(i["diff"], i["out1"], i["out2"], i["ranks"], c["P"], c["K"], c["P2"], c["asc"], c["rw"])
        cnt = DE.select_count(i["diff"], c["P"], i["ranks"], c["P2"], c["asc"])
        assert np.array_equal(ref["sel"][:, :c["P2"]], cnt), c
        assert (ref["sel"][:, 0] == 0).all() and np.array_equal(ref["sel"][:, c["P2"]:], np.tile(c["P"] + np.arange(c["K"]), (c["B"], 1)))
        if c["rw"]:      # the product is float32 out * (1 + diff), weights at or below zero included
            w = F32(1) + i["diff"][:, c["P"]:]
            assert np.array_equal(ref["xs"][:, c["P2"]:], i["out1"][:, c["P"]:] * w)
            n_tie += int((w <= 0).sum())
        rev = DE.select_ref(i["diff"], i["out1"], i["out2"], i["ranks"], c["P"], c["K"], c["P2"], c["asc"], c["rw"], "tie_higher")
        if c["P"] >= 100 and c["ranks"] is None:
            assert (rev["sel"] != ref["sel"]).any(), c      # ties decide on every list long enough to hold some
    assert n_tie > 0
    shapes = {(c["P"], c["K"], c["P2"]) for c in DE.select_cases()}
    assert shapes == set(DE.SELECT_SHAPES) and 2 * 8200 * 4 > 64 * 1024


def test_tolerances_accept_the_restatement_and_every_defect_misses():
    bad, ratios = [], {}
    for n, case in enumerate(DE.CHAIN_CASES):
        c = DE.chain_inputs(case, n)
        ref, rest = DE.chain(c, F64), DE.chain(c, F32)
        tol = DE.chain_tolerances(ref, rest)
        assert np.array_equal(ref["sel"], rest["sel"])
        for k, t in tol.items():
            if not np.isfinite(np.asarray(ref[k], dtype=F64)).all():
                bad.append("%r %s: the reference is not finite" % (case, k))
            if not DE.err(np.asarray(ref[k], F64), np.asarray(rest[k], F64)) <= t:
                bad.append("%r %s: the restatement misses its own tolerance" % (case, k))
        for d in DE.defects_of(case):
            out = DE.chain(c, F32, d)
            r = max(DE.err(np.asarray(ref[k], F64), np.asarray(out[k], F64)) / t for k, t in tol.items())
            ratios[d] = min(ratios.get(d, np.inf), r)
            if not r >= DE.DEFECT_MARGIN:
                bad.append("%r: defect %s only %.2f x the tolerance" % (case, d, r))
    print("\nsmallest defect factor over the cases it applies to:")
    for d, r in sorted(ratios.items(), key=lambda kv: kv[1]):
        print("   %-18s %10.3g   %s" % (d, r, DE.DEFECTS[d]))
    SEEN.update(ratios)
    assert set(ratios) == set(DE.DEFECTS) and len(ratios) >= 10
    assert not bad, "\n".join(bad)


def test_one_directional_half_restatement():
    """dv of the half is the dv2 of the two-directional restatement bit for bit; the loss is the xt terms alone."""
    from tests import crd_width_emulation as W
    for c in DE.LG_ONE_CASES:
        two, one = DE.lg_one_inputs(c)
        for dt in (F64, F32):
            a, b = W.loss_grad(two, dt, c["D"]), DE.loss_grad_one(one, dt, c["D"])
            assert np.array_equal(a["dv2"], b["dv"]), c
            assert np.isfinite(b["lossp"]).all() and (np.abs(b["lossp"]) < np.abs(a["lossp"])).all(), c
    assert {c["D"] for c in DE.LG_ONE_CASES} == {64, 128, 256}
    assert {DE.E.lg_splits(c["S2"], c["S2"] >= 1024) for c in DE.LG_ONE_CASES} >= {1, 2, 5}

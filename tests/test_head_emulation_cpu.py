"""CPU self-test of tests/head_emulation.py: the tolerances of the head sweep (tests/test_gpu_head.py) accept the float32 restatement
of every operator on every case and reject each injected defect by a factor of MARGIN (4) or more (an array of the exact class
rejects by not being equal); the exact class is what it claims (integers below 2^24, float64 and float32 forms bit-identical); the
case tables reach every value the sweep is meant to cross."""
import numpy as np
import pytest

from tests import head_emulation as E

DEFECTS = {"drop_tail": "a dropped tail element (ph_gram with n % 1024 != 0, ph_l1_sum, ph_sqdiff_sum)",
           "ext_internal": "scale_ext left in internal order", "mom_first": "momentum applied on the first call",
           "ge_thresh": ">= in place of > at thresh", "no_mult": "mult omitted", "no_area": "a superpixel sum not divided by its area",
           "tie_high": "a tie given to the higher index", "clamp_label": "an out-of-range label clamped instead of skipped",
           "gt_kth": "> in place of >= at the K-th value of the top-k mask", "bc2_nosqrt": "Adam's bc2 without the square root",
           "wd_after": "weight decay added after the moments", "ema_old_p": "the EMA taken from the old p",
           "eps_in_sqrt": "Adagrad's eps inside the square root", "sign0_plus": "sign(0) = +1",
           "no_range": "range missing from the sigmoid backward", "no_shift": "shift missing from the sigmoid forward",
           "no_sub": "x * mask instead of x * (1 - mask)", "swap_rate": "EMA rate and complement exchanged",
           "no_alpha": "alpha missing from ph_scaled_diff", "max_init0": "a maximum that starts from 0 instead of -inf"}


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        a, b = a.astype(np.float32).view(np.int32), b.astype(np.float32).view(np.int32)
    return a.shape == b.shape and bool((a == b).all())


def defect_ratio(e, outs):
    """How far the outputs `outs` of suite entry e lie outside: inf if an exact array differs, else the largest error / tolerance."""
    r = 0.0
    for k, ref in e["ref"].items():
        if k in e["exact"]:
            if not _same_bits(ref, outs[k]):
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
                if not _same_bits(ref, e["rest"][k]):
                    bad.append(f"{e['name']} {k}: the float32 restatement is not the exact result")
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
    print(f"\n{op:<20s} restatement {worst_rest:.2e}  tolerance {worst_tol:.2e} (of max |ref|)  smallest defect ratio: "
          + (", ".join(f"{d} {r:.3g}" for d, r in ratios.items()) or "-"))
    assert not bad, "\n".join(bad)


def test_every_listed_defect_is_injected_somewhere():
    seen = {}
    for op in E.OPS:
        for e in E.suite(op):
            for d in e["defects"]:
                seen.setdefault(d, set()).add(op)
    assert set(seen) == set(DEFECTS), set(seen) ^ set(DEFECTS)
    assert seen["drop_tail"] >= {"gram_exact", "gram", "l1_sum_exact", "sqdiff_sum"}
    assert seen["mom_first"] == seen["ge_thresh"] == {"gk_scale_momentum", "gk_finish_momentum"}
    assert seen["no_mult"] >= {"gk_scale", "gk_finish", "gk_finish_momentum"} and seen["ext_internal"] == {"gk_finish", "gk_finish_momentum"}
    assert seen["ema_old_p"] == {"adam", "adagrad"}


def test_exact_class_is_exact():
    for e in E.suite("gram_exact"):
        G = e["inp"]["G"].astype(np.int64)
        assert (G != 0).all() and np.abs(G).max() <= 3 and (np.abs(G) @ np.abs(G).T).max() < 2 ** 24
        assert np.array_equal(e["ref"]["gram"], G @ G.T)
    for op in ("gram_exact", "gram"):                  # no two rows can be exchanged unseen
        for e in E.suite(op):
            g, ng = e["ref"]["gram"], e["inp"]["ng"]
            for i in range(ng):
                for j in range(i + 1, ng):
                    p = np.arange(ng)
                    p[[i, j]] = p[[j, i]]
                    d = np.abs(g[p][:, p] - g).max()
                    assert d > (0 if op == "gram_exact" else 1e-3 * np.abs(g).max()), (op, e["name"], i, j)
    for e in E.suite("l1_sum_exact"):
        w = e["inp"]["w"].astype(np.int64)
        assert (w != 0).all() and np.abs(w).max() <= 3
        want = np.abs(w).sum() + (5 if e["inp"]["accumulate"] else 0)
        assert want < 2 ** 24 and e["ref"]["out"][0] == want
    # the cosines of the thresholded GK cases: exact ties with 0 and 1, or at least 1e-3 away from every threshold in use
    R = E._TROWS.astype(np.float64)
    c = (R @ R.T) / np.sqrt(np.outer((R * R).sum(1), (R * R).sum(1)))
    assert all(float(np.sqrt((r * r).sum())).is_integer() for r in R)
    for t in E.THRESHES:
        assert ((c == t) | (np.abs(c - t) >= 1e-3)).all()
    assert (c == 0).sum() >= 8 and (c == 1).sum() >= 7 and not (c == 0.5).any()
    for op in ("gk_scale_momentum", "gk_finish_momentum"):
        for e in E.suite(op):
            i = e["inp"]
            if i["use_thresh"]:
                assert "mo0" in e["exact"] and all(float(v).is_integer() for v in e["ref"]["mo0"])
                if i["thresh"] == 1.0:             # nothing exceeds a cosine of 1: the strict rule gives all zeros
                    assert not e["ref"]["mo0"].any()
            if op == "gk_finish_momentum":
                assert all(e["ref"]["wce%d" % c][0] == np.float32(i["lam"]) for c in range(3))
    for e in E.suite("superpixel"):
        i = e["inp"]
        gap = E.sp_gap(E._sp_means64(i["grad"], i["lab"], i["N"]), i["K"])
        assert gap > E.SP_GAP or (gap == 0 and i["kind"] in ("tie", "zero")), (e["name"], gap)
        assert not np.isnan(i["grad"]).any()


def test_tables_reach_every_listed_value():
    g = [e["inp"] for e in E.suite("gram_exact")]
    assert {(c["ng"], c["n"]) for c in g} == {(a, b) for a in (2, 3, 4, 5) for b in (1, 63, 64, 65, 1023, 1024, 1025, 4099, 16384)}
    s = [e["inp"] for e in E.suite("gk_scale")]
    assert {(c["ng"], c["nl"], c["mult"]) for c in s} == {(a, b, m) for a in (3, 5) for b in (0, a - 1) for m in (1.0, 4.0)}
    assert all((c["losses"] is None) == (c["nl"] == 0) for c in s)
    for op, ngs in (("gk_scale_momentum", {3, 5}), ("gk_finish_momentum", {5})):
        m = [e["inp"] for e in E.suite(op)]
        assert {c["ng"] for c in m} == ngs and all(len(c["grams"]) == 3 for c in m)
        assert {(c["mo_init"], c["use_thresh"], c["momentum"]) for c in m} == {(a, b, d) for a in (0, None) for b in (0, 1) for d in (0.0, 0.9)}
        assert {c["thresh"] for c in m if c["use_thresh"]} == {0.0, 1.0, 0.5}
        if op == "gk_finish_momentum":
            assert {(c["e_dev"], c["mult"]) for c in m} == {(None, 1.0), (None, 4.0), (0.37, 1.0), (0.37, 4.0)}
    sp = [e["inp"] for e in E.suite("superpixel")]
    assert {c["B"] for c in sp} == {1, 3} and {c["C"] for c in sp} == {1, 3}
    assert {c["H"] * c["W"] for c in sp} == {1, 1023, 1024, 1025, 48 * 40} and {c["N"] for c in sp} >= {1, 2, 1024, 1025, 2048}
    assert {c["kind"] for c in sp} == {"real", "oob", "empty", "tie", "zero"} and {c["scale2"] for c in sp} == {0, -100, 100}
    assert {c["want_mean"] for c in sp} == {False, True}
    assert any(c["K"] == 1 and c["N"] > 1 for c in sp) and any(c["K"] == c["N"] > 1 for c in sp) and any(1 < c["K"] < c["N"] for c in sp)
    assert any(c["N"] > 1024 and 1 < c["K"] < c["N"] for c in sp)                    # the arg-max loop strides
    for c in sp:
        if c["kind"] == "oob":
            assert (c["lab"] == -1).any() and (c["lab"] == c["N"]).any()
        if c["kind"] == "empty":
            assert (c["grad"] < 0).all() and len(np.unique(c["lab"])) < c["N"]
    tk = [e["inp"] for e in E.suite("topk_mask")]
    assert {c["B"] for c in tk} == {1, 3} and {c["D"] for c in tk} == {1, 2, 255, 256, 257, 16384}
    for D in (255, 256, 257, 16384):
        ks = {c["K"] for c in tk if c["D"] == D}
        assert 1 in ks and D in ks and any(1 < k < D for k in ks)
    for e in E.suite("topk_mask"):
        c = e["inp"]
        kth = -np.sort(-c["x"], axis=1)[:, c["K"] - 1]
        if c["kind"] == "ties" and 1 < c["K"] < c["D"]:          # a run of equal values straddles the K-th place and is kept whole
            assert (e["ref"]["mask"].sum(1) > c["K"]).all()
        if c["kind"] == "zero":
            assert (kth == 0).all() and np.signbit(c["x"][c["x"] == 0]).any() and not np.signbit(c["x"][c["x"] == 0]).all()
            assert (e["ref"]["mask"][c["x"] == 0] == 1).all()
        if c["kind"] == "inf":
            assert np.isposinf(c["x"]).any() and np.isneginf(c["x"]).any()
    assert {(c["B"], c["C"], c["P"]) for c in (e["inp"] for e in E.suite("apply_mask"))} == {(1, 1, 1), (2, 3, 85), (3, 1, 257)}
    assert any(((c["mask"] != 0) & (c["mask"] != 1)).any() for c in (e["inp"] for e in E.suite("apply_mask")))
    for op in ("adam", "adagrad"):
        u = [e["inp"] for e in E.suite(op)]
        assert {c["n"] for c in u} == {1, 2, 3, 4, 5, 1023, 1024, 1025, 1027}
        for n in E.UPD_N:
            assert {c["use_ema"] for c in u if c["n"] == n} == {False, True}
        assert {(c["wd"], c["step"]) for c in u} == {(a, b) for a in (0.0, 4e-4) for b in (1, 1000)}
        assert any((c["g"] == 0).any() and (c["v"][c["g"] == 0] == 0).all() and (c["m"][c["g"] == 0] == 0).all() for c in u)
    for op in ("ema_update", "ema_update_dev", "scaled_diff", "l1_sign_axpy"):
        assert {e["inp"]["n"] for e in E.suite(op)} == {1, 255, 256, 257, 1025}
    ax = [e["inp"] for e in E.suite("l1_sign_axpy")]
    assert {c["coef_dev"] for c in ax} == {None, 0.5}
    assert any(((c["w"] == 0) & np.signbit(c["w"])).any() for c in ax) and any(((c["w"] == 0) & ~np.signbit(c["w"])).any() for c in ax)
    l1 = [e["inp"] for e in E.suite("l1_sum_exact")]
    assert {c["n"] for c in l1} == {1, 255, 256, 2047, 2048, 2049, 2097152, 2097153} and {c["accumulate"] for c in l1} == {0, 1}
    assert E.l1_blocks(2097152) == 1024 and E.l1_blocks(2097153) == 1024 and E.l1_blocks(2049) == 2 and E.l1_blocks(1) == 1
    for op in ("sqdiff_sum", "maxnorm_mix"):
        assert {e["inp"]["n"] for e in E.suite(op)} == {1, 1023, 1024, 1025, 5000}
    assert any(c["neg"] and c["b"].max() < 0 for c in (e["inp"] for e in E.suite("maxnorm_mix")))
    for op in ("sigmoid_range_fwd", "sigmoid_range_bwd"):
        assert {e["inp"]["n"] for e in E.suite(op)} == {1, 255, 256, 257}
        for e in E.suite(op):
            if e["inp"]["n"] >= 5:
                assert set(e["inp"]["h"][:5]) == {0.0, 20.0, -20.0, 100.0, -100.0}
    for e in E.suite("sigmoid_range_fwd"):
        assert np.isfinite(e["rest"]["pred"]).all() and np.isfinite(e["rest"]["sigma"]).all()
    for e in E.suite("sigmoid_range_bwd"):
        assert len(e["ref"]["dh_sat"]) >= 1 and not e["ref"]["dh_sat"].any()

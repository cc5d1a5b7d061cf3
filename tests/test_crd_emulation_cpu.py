"""CPU self-test of tests/crd_emulation.py: the tolerances of the CRD sweep (tests/test_gpu_crd.py) accept the float32 restatement
of every real-class operator on every case (so the inputs alone keep the tolerance meaningful), the counting selection equals the
stable argsort, and each injected defect misses by a printed factor: DEFECT_MARGIN (100) x the tolerance or more in the real class,
at least one differing element in every case it applies to in the exact class.  The case tables reach every value of every axis
the sweep is meant to cross."""
import numpy as np
import pytest

from tests import crd_emulation as E

# the defects the sweep must reject
DEFECTS = {"drop_last_col": "the last column dropped when PK % 64 != 0", "tie_reversed": "the tie-break reversed",
           "shift_p3": "the sixteen-byte negative path used at P % 4 != 0 (list shifted by P & 3)",
           "drop_last_split": "the last split's partial left out of the reduce", "hist_edge": "the histogram chunk boundary off by one row",
           "scan_tail": "the scan chunk tail dropped", "uniform_posw": "uniform 1/P2 used where posw is given",
           "swap_z": "Z1 and Z2 swapped", "no_idx2": "idx_bank2 ignored", "mpn_k2": "mPn taken from K2 instead of m_neg",
           "mean_max_rows": "a class mean divided by max_class_rows", "no_renorm": "the momentum update without renormalisation"}
SEEN = {}          # defect -> smallest factor (real class) or smallest number of differing elements (exact class)


@pytest.mark.parametrize("op", E.REAL_OPS)
def test_restatement_inside_and_defects_outside_the_tolerance(op):
    worst_rest, worst_tol, ratios, bad = 0.0, 0.0, {}, []
    for e in E.suite(op):
        for k, ref in e["ref"].items():
            tol, er, sc = E.entry_tolerance(e, k), E.err(ref, e["rest"][k]), max(E.scale(ref), 1e-300)
            worst_rest, worst_tol = max(worst_rest, er / sc), max(worst_tol, tol / sc)
            if not er <= tol:
                bad.append(f"{e['name']} {k}: restatement {er:.3e} > tol {tol:.3e}")
            if not np.isfinite(np.asarray(ref)).all():
                bad.append(f"{e['name']} {k}: the reference is not finite")
        for d, outs in e["defects"].items():
            r = max((E.err(ref, outs[k]) / E.entry_tolerance(e, k)) if E.entry_tolerance(e, k) > 0
                    else (np.inf if E.err(ref, outs[k]) > 0 else 0.0) for k, ref in e["ref"].items())
            ratios[d] = min(ratios.get(d, np.inf), r)
            if not r >= E.DEFECT_MARGIN:
                bad.append(f"{e['name']}: defect {d} only {r:.2f} x the tolerance")
    for d, r in ratios.items():
        SEEN[d] = min(SEEN.get(d, np.inf), r)
    print(f"\n{op:<18s} restatement {worst_rest:.2e}  tolerance {worst_tol:.2e} (of max |ref|)  smallest defect factor: "
          + (", ".join(f"{d} {r:.3g}" for d, r in ratios.items()) or "-"))
    assert not bad, "\n".join(bad)


def _differ(a, b):
    return int(sum((np.asarray(a[k]) != np.asarray(b[k])).sum() for k in a))


def test_select_counting_equals_stable_argsort_and_its_defects_show():
    bad, n_rev, n_shift = [], np.inf, np.inf
    for n, c in enumerate(E.SELECT_CASES):
        i = E.select_inputs(c, n)
        a = (i["diff"], i["out1"], i["out2"], i["ranks"], c["P"], c["K"], c["P2"], c["K2"], c["sn"], c["sp"])
        ref = E.select_ref(*a)
        if _differ(ref, E.select_count(*a)):
            bad.append(f"{c}: rank by counting differs from the stable argsort")
        if not c["ties"]:
            assert all(np.unique(r).size == r.size for r in i["diff"]), c
        assert ref["sel"].min() >= 0 and (ref["sel"][:, 0] == 0).all()
        if c["ties"]:
            k = _differ(ref, E.select_count(*a, defect="tie_reversed"))
            n_rev = min(n_rev, k)
            if not k:
                bad.append(f"{c}: the reversed tie-break is not visible")
        if c["sn"] and c["P"] & 3 and c["K"] >= 4:
            k = _differ(ref, E.select_count(*a, defect="shift_p3"))
            n_shift = min(n_shift, k)
            if not k:
                bad.append(f"{c}: the shifted sixteen-byte path is not visible")
    SEEN["tie_reversed"], SEEN["shift_p3"] = n_rev, n_shift
    print(f"\nselect (exact): tie_reversed changes >= {n_rev} elements of every tie case, shift_p3 >= {n_shift} of every ranked case with "
          "P % 4 != 0 and K >= 4")
    assert np.isfinite(n_rev) and np.isfinite(n_shift)
    assert not bad, "\n".join(bad)
    # the big cases use the argsort reference alone; here only that their inputs have no ties and fit the documented LDS sizes
    c = E.SELECT_BIG_LDS_CASE
    assert 64 * 1024 < (c["P"] + c["K"]) * 4 + c["P"] * 4 <= 160 * 1024 and c["sn"] == 1 and c["K2"] == 8 and c["B"] == 1
    c = E.SELECT_COPY_CASE
    assert (c["P"], c["K"], c["B"], c["sp"], c["sn"]) == (4, 70000, 1, 0, 0) and (c["P"] + c["K"]) * 4 > 160 * 1024


def test_exact_class_defects_show():
    ks = []
    for c in E.HIST_CASES:
        idx, stride = E.hist_inputs(c)
        assert stride > c["col0"] + c["K"] and idx.max() >= c["n_data"] or c["K"] < 3
        good, broken = E.neg_hist(idx, c["col0"], c["K"], c["n_data"]), E.neg_hist(idx, c["col0"], c["K"], c["n_data"], "hist_edge")
        assert good.sum(1).max() <= c["K"]
        ks.append(int((good != broken).sum()))
    SEEN["hist_edge"] = min(ks)
    bank, members, offsets = E.class_inputs()
    good = E.class_centers(bank, members, offsets)
    kc = [int((good != E.class_centers(bank, members, offsets, defect_rows=m)).sum()) for m in E.CLASS_MAX_ROWS]
    SEEN["mean_max_rows"] = min(kc)
    print(f"\nneg_hist (exact): hist_edge changes >= {min(ks)} elements of every case; class_centers (exact): mean_max_rows changes "
          f">= {min(kc)} elements")
    assert min(ks) > 0 and min(kc) > 0
    # integer inputs of the exact sums stay exact in float32
    for n in E.ZSUM_N:
        xs, xt = E.zsum_inputs(n)
        assert xs.sum(dtype=np.float64) < 2 ** 24 and xt.sum(dtype=np.float64) < 2 ** 24
    assert np.abs(bank).max() <= 4 and np.array_equal(bank, np.round(bank))


def test_every_listed_defect_is_injected_somewhere():
    seen = {"tie_reversed", "shift_p3", "hist_edge", "mean_max_rows"}
    for op in E.REAL_OPS:
        for e in E.suite(op):
            seen |= set(e["defects"])
    assert seen == set(DEFECTS), seen ^ set(DEFECTS)


def test_tables_reach_every_axis_value():
    sc = [e["inp"] for e in E.suite("score")]
    assert {i["PK"] for i in sc} == {1, 7, 8, 9, 63, 64, 65, 129, 200} and {i["B"] for i in sc} == {1, 3}
    assert {i["idx2"] is None for i in sc} == {True, False} and {i["T"] for i in sc} == {0.07, 1.0}
    free = [c for c in E.SELECT_CASES if not c["ties"]]
    assert {c["P"] for c in free} >= {1, 2, 3, 4, 5, 7, 8, 101, 1030} and {c["K"] for c in free} >= {1, 3, 4, 5, 37, 1025, 2051}
    assert {(c["sp"], c["sn"]) for c in free} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ranked_neg = [c for c in free if c["sn"]]
    assert {bool(c["P"] & 3) for c in ranked_neg} == {True, False} and {c["K"] for c in ranked_neg} >= {1, 3, 4, 5, 37, 1025, 2051}
    assert any(c["P2"] == 1 for c in free) and any(c["P2"] == c["P"] > 1 for c in free) and any(1 < c["P2"] < c["P"] for c in free)
    assert any(c["K2"] == 1 for c in free) and any(c["K2"] == c["K"] > 1 for c in free) and any(1 < c["K2"] < c["K"] for c in free)
    assert any(c["ranks"] for c in free) and any(c["sp"] and not c["ranks"] for c in free)
    for n, c in enumerate(E.SELECT_CASES):
        if c["ranks"] and c["P2"] > 1:
            assert c["P"] - 1 in E.select_inputs(c, n)["ranks"]
    assert any(c["ties"] and c["ranks"] for c in E.SELECT_CASES) and any(c["ties"] and not c["ranks"] for c in E.SELECT_CASES)
    lg = [e["inp"] for e in E.suite("loss_grad")]
    assert {i["P2"] + i["K2"] for i in lg} >= {5, 31, 32, 33, 511, 512, 1023, 1024, 1025, 1537, 4096, 4608, 5000}
    assert {i["P2"] for i in lg} == {1, 6, 20} and {i["B"] for i in lg} == {1, 3} and {i["ns"] for i in lg} == {1, 2, 3, 5, 7, 8}
    assert {(i["posw_s"] is None, i["idx2"] is None) for i in lg} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(i["P2"] + i["K2"] == 1537 and not i["ws"] and i["ns"] == 1 for i in lg)
    assert all(not np.array_equal(i["sel"][0], np.arange(i["sel"].shape[1])) for i in lg)
    assert all(i["params"][2] != i["params"][3] and i["params"][2] > 0 and i["params"][3] > 0 for i in lg)
    assert all(i["idx"].min() == 0 and i["idx"].max() == E.N_DATA - 1 for i in lg)
    lp = [e["inp"] for e in E.suite("loss_grad_pos")]
    assert {(i["P2"], i["m_neg"]) for i in lp} == {(P, m) for P in (1, 6, 8) for m in (1, 4096)}
    h = E.HIST_CASES
    assert {c["n_data"] for c in h} == {1, 100, 32767, 32768, 32769, 65541} and {c["K"] for c in h} == {1, 1023, 1024, 1025, 3000}
    assert {c["col0"] for c in h} == {0, 1, 7} and {c["B"] for c in h} == {1, 3}
    s = E.SCAN_CASES
    assert {c["n_data"] for c in s if c["B"] == 3} == {1, 255, 256, 257, 2047, 2048, 2049, 4097}
    assert {c["B"] for c in s if c["n_data"] == 257} == {1, 3, 64, 65}
    for e in E.suite("scan_neg"):
        m = e["inp"]["mult"]
        assert m.max() > 1 and (m.min() == 0 or m.shape[1] < 3)
    assert {(c["B"], c["mom"]) for c in E.UPDATE_CASES} == {(B, m) for B in (1, 2, 3, 5) for m in (0.5, 0.0)}
    assert set(E.CLASS_SIZES) == {0, 1, 2, 255, 256, 257, 513} and E.CLASS_MAX_ROWS == (513, 1026)
    assert set(E.OUTPUTS_S2) == {1, 7, 8, 9, 17} and {c["S2"] for c in E.OUTPUTS_BWD_CASES} == {1, 7, 8, 9, 100}
    assert {(c["g1"], c["g2"]) for c in E.OUTPUTS_BWD_CASES} == {(1, 1), (1, 0), (0, 1)}
    assert {c["S"] for c in E.CL2_CASES} == {2, 255, 256, 257, 1000}
    for S in (255, 256, 257, 1000):
        assert {c["P"] for c in E.CL2_CASES if c["S"] == S} == {1, S // 2, S - 1}
    assert E.ZSUM_N == (1, 63, 64, 1023, 1024, 1025, 5000) and len(E.SETZ_CASES) == 4

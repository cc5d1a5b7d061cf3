"""tests/epoch_emulation.py against sklearn and numpy, without a GPU: the float64 reference of the
similarity audit is sklearn's cosine_similarity plus the reference's three formulas; the float32 restatement of the kernel sits
inside the tolerances that tests/test_gpu_epoch.py applies to the device; every injected defect falls outside them by a
factor of 4 or more on at least one of the GPU cases' shapes."""
import math

import numpy as np
import pytest

from tests import epoch_emulation as E


def _case(n, Df, Dp, classes, seed, zero_rows=()):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, Df)).astype(np.float32)
    P = (0.5 * F[:, :1] + rng.standard_normal((n, Dp))).astype(np.float32)
    for r in zero_rows:
        F[r] = 0.0
        P[(r + 1) % n] = 0.0
    return F, P, rng.integers(0, classes, size=n).astype(np.int64)


def test_reference_is_sklearn_plus_the_three_formulas():
    sk = pytest.importorskip("sklearn.metrics.pairwise")
    F, P, lab = _case(129, 33, 7, 3, 1, zero_rows=(5,))
    ref, counts = E.audit_reference(F, P, lab)
    Sf, Sp = sk.cosine_similarity(F.astype(np.float64)), sk.cosine_similarity(P.astype(np.float64))
    n = lab.shape[0]
    ind = 1.0 * np.equal(np.tile(lab.reshape(-1, 1), (1, n)), np.tile(lab.reshape(1, -1), (n, 1)))
    got = E.means(ref, counts)
    for name, S in (("teacher", Sf), ("student", Sp)):
        assert got[name + "_intra"] == pytest.approx(S[ind == 1].mean(), rel=1e-13)
        assert got[name + "_inter"] == pytest.approx(S[ind == 0].mean(), rel=1e-13, abs=1e-15)
    assert got["similarity_diff"] == pytest.approx(np.mean(np.abs(Sf - Sp)), rel=1e-13)
    assert counts == (int(ind.sum()), n * n - int(ind.sum()))
    assert Sf[5].max() == 0.0                                 # a zero row: similarity 0 with everything, itself included


def test_single_class_gives_nan_inter_means():
    F, P, _ = _case(20, 5, 5, 1, 2)
    ref, counts = E.audit_reference(F, P, np.zeros(20, dtype=np.int64))
    got = E.means(ref, counts)
    assert counts == (400, 0) and math.isnan(got["teacher_inter"]) and math.isnan(got["student_inter"])
    assert math.isfinite(got["teacher_intra"]) and math.isfinite(got["similarity_diff"])


@pytest.mark.parametrize("n,Df,Dp", [(1, 3, 3), (65, 31, 33), (129, 128, 3), (200, 33, 256)])
def test_restatement_within_tolerance_and_planted_case_exact(n, Df, Dp):
    F, P, lab = _case(n, Df, Dp, 3, n)
    ref, counts, tol = E.audit_tolerance(F, P, lab)
    for order in ("seq", "pair", "matmul"):
        got, c = E.audit_emulate(F, P, lab, order=order)
        assert c == counts
        for k in E.SUMS:
            assert abs(got[k] - ref[k]) <= tol[k], (order, k, got[k], ref[k], tol[k])
    F, P, lab = E.planted_exact(n, Df, Dp)
    ref, counts = E.audit_reference(F, P, lab)
    got, c = E.audit_emulate(F, P, lab, order="pair")
    assert c == counts and all(got[k] == ref[k] for k in E.SUMS), (got, ref)


@pytest.mark.parametrize("defect,n,Df,Dp", [("no_diagonal", 65, 33, 31), ("drop_last_row_tile", 65, 33, 31),
                                             ("drop_last_row_tile", 200, 3, 3), ("drop_last_chunk", 129, 33, 31),
                                             ("transposed_class_test", 129, 32, 32), ("transposed_class_test", 200, 31, 128)])
def test_audit_defects_fall_outside_the_tolerance(defect, n, Df, Dp):
    F, P, lab = _case(n, Df, Dp, 3, 7)
    ref, counts, tol = E.audit_tolerance(F, P, lab)
    got, c = E.audit_emulate(F, P, lab, defect=defect)
    worst = max(abs(got[k] - ref[k]) / tol[k] for k in E.SUMS)
    assert worst >= 4.0 or c != counts, (defect, worst, c, counts)
    # the planted case sees it bitwise as well (where the defect touches it at all)
    Fp, Pp, labp = E.planted_exact(n, Df, Dp)
    refp, cp = E.audit_reference(Fp, Pp, labp)
    gotp, cgp = E.audit_emulate(Fp, Pp, labp, defect=defect)
    if defect != "drop_last_chunk":
        assert cgp != cp or any(gotp[k] != refp[k] for k in E.SUMS)


def _record_calls():
    nan = float("nan")
    vals = [0.5, 0.0, -0.0, -1.25, nan, 3.0e-3, 7.0]
    calls = []
    for s, v in enumerate(vals):
        pred = np.array([[0.1, 0.7, 0.7], [0.3, 0.3, 0.1], [0.2, 0.1, 0.9], [0.5, 0.5, 0.5]], dtype=np.float32)
        grade = np.array([1, 0, -1, 3 if s == 2 else 0], dtype=np.int64)
        calls.append(dict(scalars=[1.0 + s, v, v], modes=[E.REC_ADD, E.REC_ADD_POSITIVE, E.REC_ADD], wvec=[0.25 * s, 1.0],
                          pred=pred, grade=grade, rows=[np.full(5, 1.0 + s, np.float32), np.arange(5, dtype=np.float32)]))
    return calls


def test_record_restatement_is_the_python_accumulation():
    calls = _record_calls()
    r = E.record_emulate(calls)
    acc = 0.0
    for c in calls:
        acc += float(np.float32(c["scalars"][0]))
    assert r["sums"][0] == acc and r["added"][0] == len(calls)
    assert r["sums"][1] == float(np.float32(0.5)) + float(np.float32(3.0e-3)) + 7.0 and r["added"][1] == 3   # > 0.0 only
    assert math.isnan(r["sums"][2]) and r["added"][2] == len(calls)                                       # plain add: NaN stays
    # tied maxima: the first wins - rows 0 (tie 1, 2 -> 1 == grade), 1 (tie 0, 1 -> 0 == grade), 3 (all equal -> 0)
    assert r["correct"] == 3 * len(calls) - 1 and r["bad"] == len(calls) + 1 and r["rows"] == 4 * len(calls)
    assert r["rowmeans"][1] == 2.0 * len(calls) and r["steps"] == len(calls)


def test_record_and_store_defects_are_visible():
    calls = _record_calls()
    good = E.record_emulate(calls)
    ge = E.record_emulate(calls, defect="ge_zero")
    assert ge["added"][1] == good["added"][1] + 2            # 0.0 and -0.0 pass `>= 0`; the sum alone cannot show it
    assert ge["sums"][1] == good["sums"][1]
    assert E.record_emulate(calls, defect="last_max")["correct"] != good["correct"]
    store = np.zeros((6, 3), dtype=np.float32)
    rows = np.arange(12, dtype=np.float32).reshape(4, 3)
    index = [2, 7, 2, -1]
    out, skipped = E.store_emulate(store, index, rows)
    ref = store.copy()
    ref[[2, 2]] = rows[[0, 2]]                                # numpy's a[index] = rows over the in-range entries
    assert skipped == 2 and np.array_equal(out, ref) and np.array_equal(out[2], rows[2])
    bad, _ = E.store_emulate(store, index, rows, defect="first_writer")
    assert not np.array_equal(bad, ref)


def test_softmax_restatement_within_tolerance():
    rng = np.random.default_rng(3)
    for D in (3, 33, 256):
        x = (4.0 * rng.standard_normal((17, D))).astype(np.float32)
        ref, rest = E.softmax_rows(x, np.float64), E.softmax_rows(x, np.float32)
        tol = E.softmax_tolerance(ref, rest)
        assert tol < 2e-6 and np.abs(rest - ref).max() <= tol
        y = x.copy()
        y[:, 0] += 1e-3                                         # (one logit moved by 1e-3: a softmax of the wrong row is seen)
        assert np.abs(E.softmax_rows(y, np.float64) - ref).max() > 4 * tol

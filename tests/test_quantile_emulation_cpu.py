"""tests/quantile_emulation.py (the numpy restatement of ph_group_quantile) against numpy and pandas on
float64 input: np.float32(np.percentile(x64, 100 q)) and, for q = 0.5, pandas.Series(x64).median().  Bound: one float32 ulp
(both sides round a float64 result that may differ in its last bits - numpy's lerp is two-sided); the number of cases that
are not bit-equal is printed.  numpy on float32 INPUT does its arithmetic in float32 and is not the yardstick.

Every named defect of quantile_emulation.DEFECTS, injected into the restatement, fails the same battery."""
import numpy as np
import pytest

from tests import quantile_emulation as E

NS = (1, 2, 3, 4, 9, 10, 63, 64, 65, 255, 256, 257, 4096)
QS = (0.0, 0.009, 0.25, 0.5, 0.75, 0.9, 1.0)
KINDS = ("neg", "int3", "unif")


def _seeds(n):
    return 20 if n <= 10 else (5 if n <= 257 else 1)


def _close(got, want):
    """Both NaN, or within one float32 ulp of `want` (float32)."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    if np.isinf(want) or np.isinf(got):
        return bool(got == want)
    return bool(abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.abs(want))))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def battery(defect=None, ns=NS, report=None):
    """Every check of this file on the restatement with `defect` injected; AssertionError (or IndexError) on the first miss."""
    import pandas as pd
    cases = differ = pd_cases = pd_differ = 0
    for n in ns:
        for kind in KINDS:
            for seed in range(_seeds(n)):
                v = E.values(kind, n, 1, 1000 * n + seed)[:, 0]
                v64 = v.astype(np.float64)
                rk = E.stable_ranks(v, defect)
                if defect is None:
                    assert sorted(rk.tolist()) == list(range(n)), (n, kind, seed)
                    assert np.array_equal(rk, E.stable_ranks_by_argsort(v)), (n, kind, seed)
                for q in QS:
                    want = np.float32(np.percentile(v64, 100 * q))
                    by_sort = E.quantile_sorted(v, q, defect)
                    by_rank = E.quantile_ranked(v, q, defect, ranks=lambda _v: rk)
                    assert _close(by_sort, want), ("sorted", n, kind, seed, q, by_sort, want)
                    assert _close(by_rank, want), ("ranked", n, kind, seed, q, by_rank, want)
                    assert _bits(by_sort) == _bits(by_rank), (n, kind, seed, q)
                    cases += 1
                    differ += int(_bits(by_rank) != _bits(want))
                    if q == 0.5:
                        med = np.float32(pd.Series(v64).median())
                        assert _close(by_rank, med), ("median", n, kind, seed, by_rank, med)
                        pd_cases += 1
                        pd_differ += int(_bits(by_rank) != _bits(med))
    # by hand
    four = np.array([3.0, -1.0, 2.0, 0.5], dtype=np.float32)                # sorted: -1, 0.5, 2, 3
    for q, want in ((0.0, -1.0), (1.0, 3.0), (0.5, 1.25), (0.25, 0.125), (1.0 / 3.0, 0.5)):
        for fn in (E.quantile_sorted, E.quantile_ranked):
            assert _close(fn(four, q, defect), np.float32(want)), (fn.__name__, q, fn(four, q, defect), want)
    # a NaN anywhere gives NaN (as numpy does)
    for n in (1, 3, 65):
        v = E.values("neg", n, 1, 7)[:, 0]
        v[n // 2] = np.nan
        for q in (0.0, 0.5, 1.0):
            assert np.isnan(np.percentile(v.astype(np.float64), 100 * q))
            assert np.isnan(E.quantile_sorted(v, q, defect)) and np.isnan(E.quantile_ranked(v, q, defect)), (n, q)
    # +-inf are ordinary values: t == 0 returns a without touching b; otherwise what IEEE gives for a + (b - a) t
    inf = np.float32(np.inf)
    up, down = np.array([1.0, inf, 0.0], dtype=np.float32), np.array([0.0, -inf, 1.0], dtype=np.float32)
    for fn in (E.quantile_sorted, E.quantile_ranked):
        assert fn(up, 0.5, defect) == np.float32(1.0) and fn(up, 0.0, defect) == np.float32(0.0), fn.__name__
        assert fn(up, 1.0, defect) == inf and fn(up, 0.75, defect) == inf, fn.__name__
        assert fn(down, 0.0, defect) == -inf and fn(down, 0.5, defect) == np.float32(0.0), fn.__name__
        assert np.isnan(fn(down, 0.25, defect)), fn.__name__                # -inf + (0 - -inf) / 2
        assert fn(np.array([inf, inf, 1.0], dtype=np.float32), 0.75, defect) == inf, fn.__name__      # a == b
    # the CSR: two groups interleaved in x, three columns
    gid = np.array([0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1], dtype=np.int64)
    x = E.values("neg", gid.shape[0], 3, 99)
    off, order = E.csr(gid, 2)
    for q in (0.0, 0.5, 0.9):
        got = E.group_quantile(x, off, order, q, defect)
        want = np.array([[E.quantile_sorted(x[gid == g, c], q) for c in range(3)] for g in range(2)], dtype=np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (q, got, want)
        assert np.array_equal(_bits(E.group_quantile(x[:, 1], off, order, q, defect)), _bits(want[:, 1]))
    if report is not None:
        report.update(cases=cases, differ=differ, pd_cases=pd_cases, pd_differ=pd_differ)


def test_restatement_against_numpy_and_pandas():
    rep = {}
    battery(None, report=rep)
    print("not bit-equal: %(differ)d of %(cases)d against numpy, %(pd_differ)d of %(pd_cases)d against pandas" % rep)
    assert rep["cases"] == sum(_seeds(n) for n in NS) * len(KINDS) * len(QS)


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_every_named_defect_fails_a_check(defect):
    with pytest.raises((AssertionError, IndexError)):
        battery(defect, ns=(1, 2, 3, 4, 9, 10, 63, 64, 65))


def test_select_by_hand():
    assert E.select(1, 0.5) == (0, 0, 0.0) and E.select(4, 1.0) == (3, 3, 0.0) and E.select(4, 0.0) == (0, 1, 0.0)
    assert E.select(9, 0.5) == (4, 5, 0.0) and E.select(2, 0.5) == (0, 1, 0.5)
    lo, hi, t = E.select(9, 0.009)
    assert (lo, hi) == (0, 1) and t == 8 * 0.009

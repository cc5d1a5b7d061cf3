"""ph_surv_strata, ph_surv_table and ph_surv_logrank_km through the C ABI against their numpy restatements
(tests/survstrata_emulation.py, itself held to numpy and scipy by tests/test_survstrata_emulation_cpu.py), and
evaluate.survival_strata_device against the restatement and against the committed scipy answers
(tests/golden/survstrata_scipy.npz) - DESIGN.md section 29.

Bitwise: cuts, groups, sizes, bad, the table and npoints.  stat within 2 M 2^-53 sum|term| of the restatement (which adds in
the kernels' order), survival[k] within (k + 1) 2^-52 relative; p-values against scipy 1e-12 relative.  Every output and the
workspaces - exactly as long as the workspace queries say - lie between sentinel guard bands (gpu_util.Guarded); the rows of
the table and of `surv` past npoints[0] keep their fill value.  Two runs agree bitwise, and so do the tables, sums and
curves of a row permutation."""
import os

import numpy as np
import pytest
import torch

from tests import survstrata_emulation as E
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

I32, F32, F64, U8 = torch.int32, torch.float32, torch.float64, torch.uint8
EPS = 2.0 ** -52
FILL_I, FILL_F = -7, -12345.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "survstrata_scipy.npz")


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def _strata(hazard, q):
    """ph_surv_strata on guarded buffers -> (cuts, group, sizes, bad)."""
    L, ptr, st = _api()
    N, K = hazard.shape[0], len(q)
    qh = np.asarray(q, dtype=np.float64)
    nbytes = L.ph_surv_strata_workspace_bytes(N, K)
    assert nbytes == 64
    dh = torch.from_numpy(hazard).cuda()
    cuts, group, sizes = Guarded((K,), F64), Guarded((N,), I32, fill=FILL_I), Guarded((K + 1,), I32, fill=FILL_I)
    bad, ws = Guarded((1,), I32, fill=FILL_I), Guarded((nbytes,), U8, fill=0x33)
    assert L.ph_surv_strata(ptr(dh), N, qh.ctypes.data, K, ptr(cuts.t), ptr(group.t), ptr(sizes.t), ptr(bad.t), ptr(ws.t), st) == E.OK
    torch.cuda.synchronize()
    for g in (cuts, group, sizes, bad, ws):
        assert g.guards_intact()
    return cuts.t.cpu().numpy().copy(), group.t.cpu().numpy().copy(), sizes.t.cpu().numpy().copy(), int(bad.t.cpu()[0])


def _table(survtime, event, group, G):
    """ph_surv_table on guarded buffers -> (times, at_risk, observed, censored of the npoints[0] slots, npoints, the device
    tensors for the next stage); asserts the guards and that the tails keep their fill value."""
    L, ptr, st = _api()
    N = survtime.shape[0]
    nbytes = L.ph_surv_table_workspace_bytes(N, G)
    assert nbytes == 4 * N
    dt, de, dg = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (survtime, event, group.astype(np.int32)))
    times = Guarded((N,), F32, fill=FILL_F)
    tabs = [Guarded((N, G), I32, fill=FILL_I) for _ in range(3)]
    npts, ws = Guarded((2,), I32, fill=FILL_I), Guarded((nbytes,), U8, fill=0x33)
    assert L.ph_surv_table(ptr(dt), ptr(de), ptr(dg), N, G, ptr(times.t), ptr(tabs[0].t), ptr(tabs[1].t), ptr(tabs[2].t), ptr(npts.t),
                           ptr(ws.t), st) == E.OK
    torch.cuda.synchronize()
    for g in [times, npts, ws] + tabs:
        assert g.guards_intact()
    M, left_out = npts.t.cpu().tolist()
    assert 0 <= M <= N
    th = times.t.cpu().numpy()
    assert (th[M:] == np.float32(FILL_F)).all(), "times past npoints[0] were written"
    out = [th[:M].copy()]
    for g in tabs:
        h = g.t.cpu().numpy()
        assert (h[M:] == FILL_I).all(), "table rows past npoints[0] were written"
        out.append(h[:M].copy())
    return out + [np.array([M, left_out], dtype=np.int32), (tabs[0], tabs[1], npts)]


def _logrank_km(dev, N, G, pairs):
    """ph_surv_logrank_km on the device table of `_table` -> (stat [P, 2], surv [M, G])."""
    L, ptr, st = _api()
    at_risk, observed, npts = dev
    ph = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = ph.shape[0]
    nbytes = L.ph_surv_logrank_km_workspace_bytes(N, G, P)
    assert nbytes == 8 * (-(-N // E.TILE)) * (2 * P + 2 * G)
    stat, surv, ws = Guarded((max(P, 1), 2), F64), Guarded((N, G), F64, fill=FILL_F), Guarded((nbytes,), U8, fill=0x33)
    assert L.ph_surv_logrank_km(ptr(at_risk.t), ptr(observed.t), ptr(npts.t), N, G, ph.ctypes.data if P else None, P,
                                ptr(stat.t) if P else None, ptr(surv.t), ptr(ws.t), st) == E.OK
    torch.cuda.synchronize()
    for g in (stat, surv, ws, at_risk, observed, npts):
        assert g.guards_intact()
    M = int(npts.t.cpu()[0])
    sh = surv.t.cpu().numpy()
    assert (sh[M:] == FILL_F).all(), "surv rows past npoints[0] were written"
    return stat.t.cpu().numpy()[:P].copy(), sh[:M].copy()


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _check_table_stage(survtime, event, group, G, pairs, runs=2):
    """Table, sums and curves of the device against the restatement; returns the device results of the first run."""
    N = survtime.shape[0]
    ref = E.table_ref(survtime, event, group, G)
    ref_stat, ref_surv = E.logrank_km_ref(ref[1], ref[2], pairs)
    oe, var = E.logrank_terms(ref[1], ref[2], pairs)
    M = ref[0].shape[0]
    first = None
    for _ in range(runs):
        got = _table(survtime, event, group, G)
        for name, a, b in zip(("times", "at_risk", "observed", "censored", "npoints"), got[:5], ref):
            _same(a, b, name)
        stat, surv = _logrank_km(got[5], N, G, pairs)
        if len(pairs):
            bound = 2 * M * 2.0 ** -53 * np.stack([np.abs(oe).sum(axis=1), np.abs(var).sum(axis=1)], axis=1)
            assert np.all(np.abs(stat - ref_stat) <= bound), (stat, ref_stat)
        k1 = np.arange(1, M + 1, dtype=np.float64)[:, None]
        assert surv.shape == ref_surv.shape and np.all(np.abs(surv - ref_surv) <= k1 * EPS * np.abs(ref_surv))
        if first is None:
            first = got[:5] + [stat, surv]
        else:
            for a, b in zip(first, got[:5] + [stat, surv]):
                _same(a, b, "two runs differ")
    return first


def _check_chain(hazard, survtime, event, q, runs=2):
    ref = E.strata_ref(hazard, q)
    K = len(q)
    for _ in range(runs):
        cuts, group, sizes, bad = _strata(hazard, q)
        _same(cuts, ref[0], "cuts"); _same(group, ref[1], "group"); _same(sizes, ref[2], "sizes")
        assert bad == ref[3]
    pairs = [(g, g + 1) for g in range(K)]
    return (cuts, group, sizes, bad), _check_table_stage(survtime, event, group, K + 1, pairs, runs)


@pytest.mark.parametrize("N", (2, 3, 255, 256, 257, 511, 513, 4097))
def test_kernels_vs_restatement(N):
    """N at the smallest sizes and at the tile edges 256 and 512 from both sides; 4097: 17 tiles of slots."""
    for k, K in enumerate((1, 2, 3, 7)):
        q = {1: (50,), 2: (33, 66), 3: (26, 51, 76), 7: (10, 20, 35, 50, 65, 80, 90)}[K]
        for j, kind in enumerate(("continuous", "tied_times", "tied_hazards")):
            hazard, survtime, event = E.case(kind, N, seed=100 * k + j)
            strata, table = _check_chain(hazard, survtime, event, q, runs=2 if N <= 513 else 1)
            assert int(strata[2].sum()) == N and strata[3] == 0 and table[4][1] == 0
            assert (table[1][0] == strata[2]).all()                     # everybody is at risk at the first time


def test_grid_stride_wrap():
    """N = 262 145 = 1024 workgroups of 256 rows and one row more: every grid-stride loop takes a second trip."""
    N = E.MAX_BLOCKS * E.TILE + 1
    hazard, survtime, event = E.case("continuous", N, seed=5)
    survtime = np.round(survtime * np.float32(64.0)) / np.float32(64.0)            # a few thousand distinct times, many ties
    strata, table = _check_chain(hazard, survtime, event, (33, 66), runs=1)
    assert int(strata[2].sum()) == N and table[0].shape[0] == np.unique(survtime).shape[0]
    hazard2, survtime2, event2 = E.case("continuous", N, seed=6)                    # (nearly) every row its own slot
    grp = E.strata_ref(hazard2, (50,))[1]
    _check_table_stage(survtime2, event2, grp, 2, [(0, 1)], runs=1)


def test_group_argument_form_G3():
    """The per-grade table: group given directly, G = 3, a pair that is not adjacent, P = 0, and rows outside [0, G)."""
    N = 700
    hazard, survtime, event = E.case("tied_times", N, seed=9)
    grade = np.random.RandomState(1).randint(0, 3, size=N).astype(np.int32)
    _check_table_stage(survtime, event, grade, 3, [(0, 1), (1, 2), (2, 0)])
    _check_table_stage(survtime, event, grade, 3, [])
    grade[::7] = 3; grade[5] = -1; grade[6] = 1 << 30
    t2 = survtime.copy(); t2[11] = np.nan
    out = _check_table_stage(t2, event, grade, 3, [(0, 1), (1, 2)])
    assert out[4][1] == int(((grade < 0) | (grade >= 3) | np.isnan(t2)).sum()) > 100
    _check_table_stage(survtime, event, np.zeros(N, dtype=np.int32), 1, [])        # one group: the plain Kaplan-Meier fit
    _check_table_stage(survtime, event, grade % 8, 8, [(a, b) for a in range(8) for b in range(a + 1, 8)])   # G = 8, P = 28


def test_special_inputs():
    N = 300
    # all times equal: one slot
    hazard, survtime, event = E.case("equal_times", N, 1)
    strata, table = _check_chain(hazard, survtime, event, (33, 66))
    assert table[0].tolist() == [7.0] and (table[1][0] == strata[2]).all()
    # no event: V = 0 for every pair, curves at 1
    hazard, survtime, event = E.case("no_event", N, 2)
    strata, table = _check_chain(hazard, survtime, event, (33, 66))
    assert not table[5].any() and (table[6] == 1.0).all() and not table[2].any()
    # all hazards equal with K = 2: the patch, one stratum holds everything, the other two are empty
    hazard, survtime, event = E.case("equal_hazards", N, 3)
    strata, table = _check_chain(hazard, survtime, event, (33, 66))
    assert strata[0].tolist() == [2.99997, -0.75] and strata[2].tolist() == [N, 0, 0] and not table[5][:, 1].any()
    strata, _ = _check_chain(hazard, survtime, event, (25, 50, 75))                # K = 3: no patch
    assert strata[2].tolist() == [0, 0, 0, N]
    # tied hazards that straddle the cuts
    hazard, survtime, event = E.case("tied_hazards", N, 4)
    strata, _ = _check_chain(hazard, survtime, event, (33, 66))
    assert (hazard.astype(np.float64) == strata[0][0]).any() or (hazard.astype(np.float64) == strata[0][1]).any()
    # a NaN hazard: every cut NaN, every row in stratum K; +-inf are ordinary values
    hazard, survtime, event = E.case("nan_inf", N, 5)
    strata, _ = _check_chain(hazard, survtime, event, (33, 66))
    assert np.isnan(strata[0]).all() and strata[2].tolist() == [0, 0, N] and strata[3] == 3
    hazard[N // 2] = 0.0
    strata, _ = _check_chain(hazard, survtime, event, (33, 66))
    assert np.isfinite(strata[0]).all() and strata[3] == 2 and strata[1][0] == 2 and strata[1][N - 1] == 0
    # (t == 0 returns the order statistic itself: the one divergence from np.percentile, which gives NaN for an infinite one)
    strata, _ = _check_chain(hazard, survtime, event, (0, 100))
    assert strata[0].tolist() == [-np.inf, np.inf] and strata[2].tolist() == [0, N - 1, 1]


def test_row_permutation_leaves_tables_sums_and_curves_bitwise_equal():
    N = 1000
    hazard, survtime, event = E.case("tied_times", N, 6)
    strata, table = _check_chain(hazard, survtime, event, (33, 66), runs=1)
    perm = np.random.RandomState(3).permutation(N)
    strata_p, table_p = _check_chain(hazard[perm], survtime[perm], event[perm], (33, 66), runs=1)
    _same(strata[0], strata_p[0], "cuts"); _same(strata[1][perm], strata_p[1], "group"); _same(strata[2], strata_p[2], "sizes")
    for a, b in zip(table, table_p):
        _same(a, b, "a row permutation changed the table stage")


def _device_dict(hazard, survtime, event, q, **kw):
    import multimodal_learning_amd as m
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()      # noqa: E731
    return m.evaluate.survival_strata_device(d(hazard), d(survtime), d(event), q, **kw)


def test_wrapper_vs_restatement_one_copy_and_refusals(monkeypatch):
    import multimodal_learning_amd as m
    N = 777
    hazard, survtime, event = E.case("tied_times", N, 8)
    copies = {"n": 0}
    for name in ("cpu", "item", "tolist"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            copies["n"] += 1 if self.is_cuda else 0
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    dh, dt, de = (torch.from_numpy(a).cuda() for a in (hazard, survtime, event))
    for q in ((33, 66), (50,), [25, 50, 75]):
        copies["n"] = 0
        got = m.evaluate.survival_strata_device(dh, dt, de, q)
        assert copies["n"] == 1, "more than one device-to-host copy"
        ref = E.chain_ref(hazard, survtime, event, q)
        assert set(got) == set(ref)
        for key in ("cuts", "group", "sizes", "times", "at_risk", "observed", "censored"):
            _same(got[key], ref[key], key)
        assert got["bad"] == ref["bad"] == 0 and got["stat"].shape == ref["stat"].shape == (len(q), 2)
        oe, var = E.logrank_terms(ref["at_risk"], ref["observed"], [(g, g + 1) for g in range(len(q))])
        M = ref["times"].shape[0]
        bound = 2 * M * 2.0 ** -53 * np.stack([np.abs(oe).sum(axis=1), np.abs(var).sum(axis=1)], axis=1)
        assert np.all(np.abs(got["stat"] - ref["stat"]) <= bound)
        assert np.all(np.abs(got["pvalues"] - ref["pvalues"]) <= 1e-12 * ref["pvalues"])
        k1 = np.arange(1, M + 1, dtype=np.float64)[:, None]
        assert np.all(np.abs(got["survival"] - ref["survival"]) <= k1 * EPS * np.abs(ref["survival"]))
    assert m.evaluate.survival_strata_device(dh, dt, de)["cuts"].shape == (2,)            # the default is (33, 66)
    # group=: the percentile stage replaced
    grade = np.random.RandomState(2).randint(0, 3, size=N)
    copies["n"] = 0
    got = m.evaluate.survival_strata_device(None, dt, de, group=torch.from_numpy(grade).cuda(), G=3)
    assert copies["n"] == 1
    ref = E.chain_ref(None, survtime, event, group=grade, G=3)
    for key in ("group", "sizes", "times", "at_risk", "observed", "censored"):
        _same(got[key], ref[key], key)
    assert got["cuts"].shape == (0,) and got["sizes"].tolist() == np.bincount(grade, minlength=3).tolist()
    assert np.all(np.abs(got["pvalues"] - ref["pvalues"]) <= 1e-12 * ref["pvalues"]) and got["pvalues"].shape == (2,)
    # the curve helper on a device column: lifelines' layout
    tl, s = m.evaluate.km_step_function(got["times"], got["survival"][:, 1], got["at_risk"][:, 1])
    keep = got["at_risk"][:, 1] > 0
    assert tl[0] == 0.0 and s[0] == 1.0 and np.array_equal(tl[1:], got["times"][keep].astype(np.float64))
    assert np.array_equal(s[1:], got["survival"][keep, 1]) and (np.diff(s) <= 0).all()
    # no event, an empty stratum: NaN p-values, no exception
    got = m.evaluate.survival_strata_device(dh, dt, torch.zeros_like(de), (33, 66))
    assert np.isnan(got["pvalues"]).all()
    got = _device_dict(np.full(N, 0.5, dtype=np.float32), survtime, event, (33, 66))
    assert got["sizes"].tolist() == [N, 0, 0] and np.isnan(got["pvalues"]).all() and got["cuts"].tolist() == [2.99997, 0.5]
    for bad in ((), tuple(range(8)), (66, 33), (-1, 50), (50, 101), (float("nan"),), 50, None, ("33",), (True,)):
        with pytest.raises(ValueError, match="percentile"):
            m.evaluate.survival_strata_device(dh, dt, de, bad)
    with pytest.raises(ValueError):
        m.evaluate.survival_strata_device(dh[:1], dt[:1], de[:1])
    with pytest.raises(ValueError):
        m.evaluate.survival_strata_device(dh, dt, de[:5])
    for G in (None, 0, 9):
        with pytest.raises(ValueError, match="G="):
            m.evaluate.survival_strata_device(None, dt, de, group=torch.from_numpy(grade).cuda(), G=G)


def test_fixture_scipy_answers():
    g = np.load(GOLDEN)
    names = sorted({k.split("_")[0] for k in g.files})
    assert len(names) >= 5
    for n in names:
        hazard, survtime, event, q = (g["%s_%s" % (n, k)] for k in ("hazard", "survtime", "event", "q"))
        got = _device_dict(hazard, survtime, event, tuple(q.tolist()))
        _same(got["cuts"], g[n + "_cuts"], "cuts"); _same(got["group"], g[n + "_group"], "group")
        _same(got["times"], g[n + "_times"], "times")
        want_p, want_s = g[n + "_pvalues"], g[n + "_survival"]
        print(n, "p device", got["pvalues"], "scipy", want_p)
        assert np.all(np.abs(got["pvalues"] - want_p) <= 1e-12 * want_p)
        k1 = np.arange(1, want_s.shape[0] + 1, dtype=np.float64)[:, None]
        assert np.all(np.abs(got["survival"] - want_s) <= k1 * EPS * np.abs(want_s))

"""The rank-window rule of ph_crd_bank_topk for num_pos > 8 on the CPU (tests/knn_np_emulation.py), and the host checks of the entry
and of ph_crd_bank_topk_workspace_bytes_np.

The emulation is exact on the uint64 keys, so it is held to a stable sort with no tolerance: on the cases of
tests/test_gpu_knn_np.py, and on (5000, 100, 16) and (4000, 8, 64), which the GPU file leaves out because no seed separates their
float32 similarities from the float64 reference's - here both sides sort the same float32 values and ties are ordered by row on
both.  Each of the four injected defects is run on ALL ten cases and must change at least one row of every case it applies to - and
none where it does not:

  ub_inclusive          `<=` instead of `<` at ub: the eighth key of a window is found again by the next.  Every case.
  thr_of_first_window   thr[p] from the eighth group maximum for every p.  The window rule needs min(num_pos, n_data) keys at or above
                        its thresholds; with thr[0] everywhere a query is short of them exactly when fewer than that many of its keys
                        reach thr[0] (`_short_of_keys`, counted from the keys, not from a run of the defect).  That holds for some query
                        of seven cases.  It does not for (33, 33, 24) and (12, 4, 24): 4 and 2 groups, fewer than eight, so every thr is
                        0 with and without the defect.  And it does not for (65536, 8, 16): there the sample is 256 groups of 16 rows out
                        of 65 536, the eighth largest group maximum is so loose a bound that at least 16 keys of every query reach it,
                        and a wrong thr[p] changes only how many elements take the rare path, never a row.  So these three cases - on
                        the CPU and in tests/test_gpu_knn_np.py - cannot see a wrong thr[p]; the other seven do.
  no_exhausted_state    ub = 0 read as "no bound": the windows behind an exhausted bank start over.  Banks of fewer than
                        8 (npass - 1) rows: (12, 4, 24) alone.
  rank_offset_zero      every window written at rank 0.  Every case."""
import numpy as np
import pytest

from tests import crd_width_emulation as W
from tests import knn_np_emulation as K

TABLE = ((33, 33, 24), (257, 65, 9), (300, 5, 64), (2000, 33, 17), (1500, 40, 16), (5000, 100, 9), (65536, 8, 16))
UNSEPARATED = ((5000, 100, 16), (4000, 8, 64))
EXHAUSTED = (12, 4, 24)
_CACHE = {}


def _case(n, B, NP, D=128):
    key = (n, B, NP, D)
    if key not in _CACHE:
        if (n, B, NP) in TABLE:
            i, ref, gap = W.knn_seed(n, B, NP, D)
        else:
            i = W.knn_inputs(n, B, NP, D, 0)
            ref = None
        _CACHE[key] = (i, ref, K.stable_sort_f32(i, NP), K.knn_windows(i, NP))
    return _CACHE[key]


def _groups(n):
    return 2 * min((n + 31) // 32, K.SAMPLE_TILES)


@pytest.mark.parametrize("case", TABLE + UNSEPARATED + (EXHAUSTED,))
def test_windows_equal_the_stable_sort(case):
    n, B, NP = case
    i, ref, sort32, got = _case(n, B, NP)
    for bank in range(2):
        assert np.array_equal(got[bank][0], sort32[bank]), (case, bank)
        if ref is not None:      # a separated seed: the float64 sort of the GPU test orders the same rows
            assert np.array_equal(got[bank][0], ref[bank][0]), (case, bank)
            assert np.abs(got[bank][1].astype(np.float64) - ref[bank][1]).max() < 1e-6
    if case == EXHAUSTED:
        for bank in range(2):
            assert (got[bank][0][:, n:] == K.EMPTY_ROW).all() and np.isneginf(got[bank][1][:, n:]).all()
            assert np.array_equal(np.sort(got[bank][0][:, :n], axis=1), np.tile(np.arange(n), (B, 1)))


@pytest.mark.parametrize("D", (64, 256))
def test_windows_equal_the_stable_sort_at_the_other_widths(D):
    for (n, B, NP) in ((33, 33, 24), (300, 5, 64)):
        i, ref, sort32, got = _case(n, B, NP, D)
        for bank in range(2):
            assert np.array_equal(got[bank][0], ref[bank][0]), (D, n, B, NP, bank)


ALL_CASES = TABLE + UNSEPARATED + (EXHAUSTED,)


def _short_of_keys(i, n, NP):
    """True when, for some query and bank, fewer than min(NP, n) keys reach the eighth largest group maximum (0 when there are fewer
    than eight groups: every key reaches it)."""
    for sim in K.masked_cosine(i):
        for s_ in sim:
            keys = K.keys_of(s_.astype(np.float32))
            thr0 = K.thresholds(K.group_maxima(keys), 1)[0]
            if int((keys >= thr0).sum()) < min(NP, n):
                return True
    return False


def _applies(defect, i, n, NP):
    npass = (NP + K.W - 1) // K.W
    if defect == "thr_of_first_window":
        return _short_of_keys(i, n, NP)
    if defect == "no_exhausted_state":
        return n < K.W * (npass - 1)
    return npass > 1


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_injected_defects_are_seen(defect):
    seen = {}
    for (n, B, NP) in ALL_CASES:
        i, ref, sort32, good = _case(n, B, NP)
        bad = K.knn_windows(i, NP, defect)
        changed = any(not np.array_equal(bad[bank][0], good[bank][0]) for bank in range(2))
        seen[(n, B, NP)] = changed
        assert changed == _applies(defect, i, n, NP), (defect, n, B, NP, changed)
    if defect == "thr_of_first_window":
        assert [c for c, ch in seen.items() if not ch] == [(33, 33, 24), (65536, 8, 16), EXHAUSTED]
    elif defect == "no_exhausted_state":
        assert [c for c, ch in seen.items() if ch] == [EXHAUSTED]
    else:
        assert all(seen.values())


def test_group_maxima_bound_the_ranks():
    """thr[p] is a lower bound of the 8 (p + 1)-th best key: the groups are disjoint row sets."""
    n, B, NP = 2000, 33, 17
    i = _case(n, B, NP)[0]
    sim = K.masked_cosine(i)[0]
    for s in sim[:8]:
        keys = K.keys_of(s.astype(np.float32))
        g = K.group_maxima(keys)
        assert g.size == _groups(n) and np.unique(g).size == g.size
        thr = K.thresholds(g, 3)
        best = np.sort(keys)[::-1]
        for p in range(3):
            assert thr[p] != 0 and thr[p] <= best[K.W * (p + 1) - 1]


def test_host_checks_without_a_device():
    """num_pos outside 1 .. 64 is PH_EINVAL before any HIP call; the size function equals the old one up to 8, grows by one
    window record per further window, and is 0 outside the range."""
    import multimodal_learning_amd as m
    L = m.lib()
    N4, N5 = [None] * 4, [None] * 5
    one = 1      # a non-null workspace pointer that nothing dereferences
    for NP in (0, -1, 65, 1 << 20):
        assert L.ph_crd_bank_topk(*N4, 5, None, 4, 100, NP, 128, *N4, one, None) == -22, NP
        assert L.ph_crd_bank_topk_workspace_bytes_np(4, 100, NP) == 0, NP
    for D in (0, 96, 512):
        assert L.ph_crd_bank_topk(*N4, 5, None, 4, 100, 16, D, *N4, one, None) == -22, D
    assert L.ph_crd_bank_topk(*N4, 5, None, 4, 100, 16, 128, *N5, None) == -22      # no workspace
    for (B, n) in ((1, 1), (5, 300), (64, 65536), (65, 257), (256, 5000)):
        old = L.ph_crd_bank_topk_workspace_bytes(B, n)
        prev = 0
        for NP in range(1, 65):
            got = L.ph_crd_bank_topk_workspace_bytes_np(B, n, NP)
            assert got == K.workspace_bytes(old, B, NP), (B, n, NP)
            assert got == old if NP <= 8 else got > old
            assert got >= prev
            prev = got


def test_neighbor_count_is_checked_at_construction():
    from types import SimpleNamespace
    from multimodal_learning_amd.CL_utils.CRD_criterion_v10 import CRDLoss
    cls = [np.arange(0, 40), np.arange(40, 80)]
    opt = lambda p, extra="neighbors": SimpleNamespace(s_dim=8, t_dim=8, feat_dim=128, nce_k=4, nce_t=0.07, nce_m=0.5, nce_p=p,
                                                        pos_extra=extra)
    for p in (0, 65, -3, 300):
        with pytest.raises(ValueError, match=r"1 \.\. 64"):
            CRDLoss(opt(p), 80, cls)
    for p in (1, 6, 9, 64):
        assert CRDLoss(opt(p), 80, cls).num_pos == p
    # more neighbours than bank rows would leave empty KNN slots in the column lists
    with pytest.raises(ValueError, match="n_data"):
        CRDLoss(opt(24), 20, [np.arange(0, 10), np.arange(10, 20)])
    assert CRDLoss(opt(20), 20, [np.arange(0, 10), np.arange(10, 20)]).num_pos == 20

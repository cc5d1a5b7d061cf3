"""The numpy restatements of the evaluation-tail kernels (tests/eval_emulation.py) against sklearn and
pandas, without a GPU - the two identities the kernels rest on:

    micro roc_auc_score           = (concordant + tied / 2) / (P Q)
    micro average_precision_score = (1 / P) sum over the positives of ge_pos_i / ge_all_i

within M * 2^-52 absolute (both sides are float64 sums of at most M terms in [0, 1]), the confusion matrix against f1_score
exactly, the group aggregation against pandas' groupby (max bit for bit; mean within one float32 ulp: the two float64
summation orders differ by far less, so only a rounding boundary can flip), and the patch geometry.  Each injected defect of
eval_emulation.DEFECTS must fail at least one of these checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_emulation as E  # noqa: E402

KINDS = ("random", "distinct", "ties", "equal", "logprob")
SHAPES = ((300, 3), (77, 3), (341, 3), (257, 1))


def _onehot(grade, C):
    y = np.zeros((grade.shape[0], C), dtype=np.int64)
    y[np.arange(grade.shape[0]), grade] = 1
    return y


def check_rank(defect=None):
    from sklearn import metrics as skm
    worst = 0.0
    for kind in KINDS:
        for k, (N, C) in enumerate(SHAPES):
            pred, grade = E.scores(kind, N, C, seed=10 * k + 1)
            if C == 1:                      # one column: label = (grade == 0) must have both values
                grade = (np.arange(N) % 3 != 0).astype(np.int64)
            M = N * C
            s, l = E.pairs(pred, grade)
            P, conc, tied, bad, ap_sum = E.rank_counts_ref(pred, grade, defect)
            assert bad == int((grade >= C).sum())      # (C = 1: the rows that are not class 0 are flagged, and still counted)
            auc, ap = E.rank_metrics(P, conc, tied, ap_sum, M, defect)
            y = l.astype(np.int64)
            ref_auc, ref_ap = skm.roc_auc_score(y, s.astype(np.float64)), skm.average_precision_score(y, s.astype(np.float64))
            if C > 1:                       # the micro average IS the flattened problem: hold sklearn to that too
                assert ref_auc == skm.roc_auc_score(_onehot(grade, C), pred, average="micro")
                assert ref_ap == skm.average_precision_score(_onehot(grade, C), pred, average="micro")
            tol = M * 2.0 ** -52
            worst = max(worst, abs(auc - ref_auc) / tol, abs(ap - ref_ap) / tol)
            assert P == int(y.sum())
            assert abs(auc - ref_auc) <= tol, (kind, N, C, auc, ref_auc)
            assert abs(ap - ref_ap) <= tol, (kind, N, C, ap, ref_ap)
    return worst


def check_confusion(defect=None):
    from sklearn import metrics as skm
    for kind in ("random", "ties", "logprob"):
        for N in (300, 77):
            pred, grade = E.scores(kind, N, 3, seed=N)
            conf = E.confusion_ref(pred, grade, defect)
            micro, per = E.f1_from_confusion(conf)
            arg = np.argmax(pred, axis=1)
            assert set(grade) == {0, 1, 2}
            assert np.array_equal(conf, skm.confusion_matrix(grade, arg, labels=[0, 1, 2])), (kind, N)
            assert micro == skm.f1_score(grade, arg, average="micro"), (kind, N)
            assert np.array_equal(per, skm.f1_score(grade, arg, average=None, labels=[0, 1, 2], zero_division=0)), (kind, N)
            # the reference passes (prediction, label): F1 is symmetric in the two
            assert micro == skm.f1_score(arg, grade, average="micro")


def _groups(N, G, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, G, N)
    g[:G] = rng.permutation(G)          # no empty group; interleaved, not contiguous
    return g


def check_group_agg(defect=None):
    import pandas as pd
    for N, G, seed in ((257, 7, 0), (9, 3, 1), (36, 36, 2), (40, 1, 3)):
        pred, _ = E.scores("logprob", N, 3, seed=seed)
        pred = pred - np.float32(0.125)                     # all strictly negative
        g = _groups(N, G, seed) if 1 < G < N else (np.arange(N) if G == N else np.zeros(N, dtype=np.int64))
        offsets, order = E.csr(g, G)
        df = pd.DataFrame(pred)
        ref_max = df.groupby(g).agg("max").to_numpy()
        ref_mean = df.astype(np.float64).groupby(g).agg("mean").to_numpy().astype(np.float32)
        got_max = E.group_agg_ref(pred, offsets, order, "max", defect)
        got_mean = E.group_agg_ref(pred, offsets, order, "mean", defect)
        assert got_max.dtype == np.float32 and np.array_equal(got_max.view(np.int32), ref_max.astype(np.float32).view(np.int32)), (N, G)
        ulp = np.spacing(np.abs(ref_mean))
        assert np.all(np.abs(got_mean.astype(np.float64) - ref_mean.astype(np.float64)) <= ulp), (N, G)


CHECKS = (check_rank, check_confusion, check_group_agg)


def test_rank_counts_give_sklearns_micro_auc_and_ap():
    worst = check_rank()
    print("largest |metric - sklearn| / (M 2^-52): %.3g" % worst)


def test_confusion_matrix_gives_sklearns_f1():
    check_confusion()


def test_group_agg_gives_pandas_groupby():
    check_group_agg()


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_each_injected_defect_fails_a_check(defect):
    failed = []
    for chk in CHECKS:
        try:
            chk(defect)
        except AssertionError:
            failed.append(chk.__name__)
    print(defect, "->", failed)
    assert failed, "no check notices the defect %r" % defect


def test_summation_tree_is_the_stated_order():
    v = np.arange(E.TILE, dtype=np.float64) * 2.0 ** -30 + 1.0
    ref = v.copy()
    o = E.TILE // 2
    while o:
        for t in range(o):
            ref[t] += ref[t + o]
        o //= 2
    assert E.tree_sum(v) == ref[0]


def test_patch_geometry_1024_512_grid3():
    assert E.patch_offsets(1024, 512, 3) == [0, 256, 512]
    rows = E.patch_rows(2, 1024, 1024, 512, 3)
    assert len(rows) == 18 and [r[0] for r in rows] == [0] * 9 + [1] * 9
    assert rows[:9] == [(0, t, l) for t in (0, 256, 512) for l in (0, 256, 512)]
    assert E.patch_offsets(96, 64, 1) == [16]
    with pytest.raises(ValueError):
        E.patch_offsets(1024, 511, 3)            # stride 513 / 2
    with pytest.raises(ValueError):
        E.patch_offsets(512, 1024, 3)


def test_package_geometry_is_the_restatement():
    import multimodal_learning_amd as m
    for extent, S, grid in ((1024, 512, 3), (96, 64, 3), (96, 64, 1), (100, 40, 4), (64, 64, 1)):
        assert m.augment.patch_offsets(extent, S, grid) == E.patch_offsets(extent, S, grid)
    for bad in ((1024, 511, 3), (512, 1024, 3), (96, 64, 0)):
        with pytest.raises(ValueError):
            m.augment.patch_offsets(*bad)


def test_metrics_from_counts_is_the_restatement():
    """evaluate.metrics_from_counts (the host arithmetic behind grading_metrics_device) on the restatement's counts."""
    import multimodal_learning_amd as m
    from sklearn import metrics as skm
    pred, grade = E.scores("logprob", 300, 3, seed=5)
    P, conc, tied, bad, ap_sum = E.rank_counts_ref(pred, grade)
    conf = E.confusion_ref(pred, grade)
    auc, ap, f1, f1_iv = m.evaluate.metrics_from_counts((P, conc, tied, bad), ap_sum, conf)
    assert (auc, ap) == E.rank_metrics(P, conc, tied, ap_sum, 900)
    arg = pred.argmax(axis=1)
    assert f1 == skm.f1_score(grade, arg, average="micro") and f1_iv == skm.f1_score(grade, arg, average=None)[2]
    with pytest.raises(ValueError):
        m.evaluate.metrics_from_counts((P, conc, tied, 1), ap_sum, conf)
    with pytest.raises(ValueError):
        m.evaluate.metrics_from_counts((0, 0, 0, 0), 0.0, conf)

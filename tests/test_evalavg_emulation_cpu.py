"""The numpy restatements of ph_rank_counts_classes, ph_roc_points and the host formulas behind them
(tests/evalavg_emulation.py) against sklearn, without a GPU:

    roc_auc_score / average_precision_score / f1_score with average = None | "macro" | "weighted"
    roc_curve(drop_intermediate = True | False) per class and over the flattened (micro) problem, and auc(fpr, tpr)

Floats compare under the rule of tests/test_eval_emulation_cpu.py: within M * 2^-52 absolute, M = the number of elements of
the problem (both sides are float64 sums of at most M terms in [0, 1]) - M = N for one class, and M = N * C for an average
over the classes (a sum of C per-class values, each within N * 2^-52).  The curves compare as arrays that must be equal:
the points are integers, the divisions the same two operands.  Each injected defect of evalavg_emulation.DEFECTS must fail
at least one check."""
import numpy as np
import pytest

from tests import eval_emulation as E0
from tests import evalavg_emulation as E

EPS = 2.0 ** -52


def _onehot(grade, C):
    y = np.zeros((grade.shape[0], C), dtype=np.int64)
    y[np.arange(grade.shape[0]), grade] = 1
    return y


def cases():
    """(name, pred, grade): continuous, one decimal (heavy ties), a constant column, one positive / one negative in a class."""
    out = []
    for k, (kind, N, C) in enumerate((("continuous", 300, 3), ("decimal", 300, 3), ("constant", 77, 3), ("decimal", 41, 4),
                                      ("continuous", 257, 3), ("decimal", 513, 2))):
        pred, grade = E.scores(kind, N, C, seed=20 + k)
        out.append(("%s %dx%d" % (kind, N, C), pred, grade))
    pred, _ = E.scores("decimal", 12, 3, seed=3)
    out.append(("one positive in classes 1 and 2", pred, np.array([0] * 10 + [1, 2], dtype=np.int64)))
    pred, _ = E.scores("continuous", 9, 2, seed=4)
    out.append(("one negative in class 0", pred, np.array([0] * 8 + [1], dtype=np.int64)))
    return out


CASES = cases()


def check_class_metrics(defect=None):
    from sklearn import metrics as skm
    worst = 0.0
    for name, pred, grade in CASES:
        N, C = pred.shape
        y, s64 = _onehot(grade, C), pred.astype(np.float64)
        arg = np.argmax(pred, axis=1)
        labels = list(range(C))
        counts, ap_sum = E.rank_counts_classes_ref(pred, grade, defect)
        conf = E0.confusion_ref(pred, grade)
        assert counts[:, 0].tolist() == y.sum(axis=0).tolist() and not counts[:, 3].any(), name
        for avg in (None, "macro", "weighted"):
            got = E.class_metrics(counts, ap_sum, conf, avg, defect)
            ref = (skm.roc_auc_score(y, s64, average=avg), skm.average_precision_score(y, s64, average=avg),
                   skm.f1_score(grade, arg, average=avg, labels=labels, zero_division=0))
            tol = (N if avg is None else N * C) * EPS
            for what, a, b in zip(("auc", "ap", "f1"), got, ref):
                err = float(np.abs(np.asarray(a) - np.asarray(b)).max())
                worst = max(worst, err / tol)
                assert err <= tol, (name, avg, what, a, b)
    return worst


def check_brute_force(defect=None):
    """The definitions, pair by pair, on inputs with ties, a NaN in column 1 and labels out of range."""
    pred, grade = E.scores("decimal", 61, 3, seed=9)
    pred[7, 1] = np.nan
    grade = grade.copy(); grade[3] = 3; grade[20] = -1
    counts, ap_sum = E.rank_counts_classes_ref(pred, grade, defect)
    assert counts[:, 3].tolist() == [2, 1, 0]
    for c in range(3):
        s, l = pred[:, c], grade == c
        with np.errstate(invalid="ignore"):
            ge = s[None, :] >= s[:, None]                  # [i, j]: s_j >= s_i
            lt, eq = s[None, :] < s[:, None], s[None, :] == s[:, None]
        conc, tied = int(lt[l][:, ~l].sum()), int(eq[l][:, ~l].sum())
        assert counts[c, :3].tolist() == [int(l.sum()), conc, tied], c
        live = l & ~np.isnan(s)
        terms = ge[live][:, l].sum(axis=1) / ge[live].sum(axis=1)
        assert abs(ap_sum[c] - terms.sum()) <= 61 * EPS, c
    for cls in (-1, 0, 1, 2):
        s, l = (pred[:, cls], grade == cls) if cls >= 0 else (pred.reshape(-1), (grade[:, None] == np.arange(3)[None, :]).reshape(-1))
        fps, tps, thr, bad = E.roc_points_ref(pred, grade, cls, defect)
        assert bad == 2 + (1 if cls in (-1, 1) else 0), cls
        t = np.array(sorted(set(s[~np.isnan(s)].tolist()), reverse=True), dtype=np.float32)
        assert np.array_equal(thr, t), cls
        with np.errstate(invalid="ignore"):
            assert tps.tolist() == [int((l & (s >= v)).sum()) for v in t], cls
            assert fps.tolist() == [int((~l & (s >= v)).sum()) for v in t], cls
        assert fps.dtype == np.int32 and tps.dtype == np.int32 and thr.dtype == np.float32


def check_curves(defect=None):
    from sklearn import metrics as skm
    for name, pred, grade in CASES:
        N, C = pred.shape
        counts, ap_sum = E.rank_counts_classes_ref(pred, grade)
        auc_c = E.class_metrics(counts, ap_sum, E0.confusion_ref(pred, grade), None)[0]
        for cls in list(range(C)) + [-1]:
            s, l = E.problem(pred, grade, cls)
            fps, tps, thr, bad = E.roc_points_ref(pred, grade, cls, defect)
            assert bad == 0 and thr.shape[0] == np.unique(s).shape[0], (name, cls)
            for drop in (True, False):
                fpr, tpr, th = E.roc_curve_ref(fps, tps, thr, drop, defect)
                ref = skm.roc_curve(l.astype(np.int64), s, drop_intermediate=drop)
                for what, a, b in zip(("fpr", "tpr", "thresholds"), (fpr, tpr, th), ref):
                    assert a.shape == b.shape and np.array_equal(a, b), (name, cls, drop, what)
                area = E.trapezoid(fpr, tpr)
                assert area == skm.auc(ref[0], ref[1]), (name, cls, drop)
                M = s.shape[0]
                want = auc_c[cls] if cls >= 0 else skm.roc_auc_score(l.astype(np.int64), s.astype(np.float64))
                assert abs(area - want) <= M * EPS, (name, cls, drop, area, want)


CHECKS = (check_class_metrics, check_brute_force, check_curves)


def test_class_counts_give_sklearns_macro_weighted_and_per_class_values():
    worst = check_class_metrics()
    print("largest |metric - sklearn| / (M 2^-52): %.3g" % worst)


def test_counts_and_points_are_the_pairwise_definitions():
    check_brute_force()


def test_points_give_sklearns_roc_curve_and_auc():
    check_curves()


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


def test_ap_sum_is_added_in_the_stated_order():
    """Per block of TILE rows the tree, then the blocks t, t + TILE, .. per thread, then the tree - written out by hand."""
    rng = np.random.default_rng(0)
    term = rng.random(E.TILE * E.TILE + 300)
    nb = -(-term.shape[0] // E.TILE)
    padded = np.pad(term, (0, nb * E.TILE - term.shape[0])).reshape(nb, E.TILE)
    part = [float(E0.tree_sum(row)) for row in padded]
    acc = [0.0] * E.TILE
    for b, v in enumerate(part):
        acc[b % E.TILE] += v
    assert E.fixed_order_sum(term) == float(E0.tree_sum(np.array(acc)))


def test_package_host_arithmetic_is_the_restatement():
    """evaluate.metrics_from_class_counts, roc_curve_from_points and roc_auc_from_curve on the restatement's integers."""
    import multimodal_learning_amd as m
    from sklearn import metrics as skm
    EV = m.evaluate
    pred, grade = E.scores("decimal", 300, 3, seed=21)
    counts, ap_sum = E.rank_counts_classes_ref(pred, grade)
    conf = E0.confusion_ref(pred, grade)
    f1_iv = skm.f1_score(grade, pred.argmax(axis=1), average=None)[2]
    for avg in (None, "macro", "weighted"):
        got = EV.metrics_from_class_counts(counts, ap_sum, conf, avg)
        want = E.class_metrics(counts, ap_sum, conf, avg)
        assert len(got) == 4 and got[3] == f1_iv
        for a, b in zip(got[:3], want):
            assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 900 * EPS, avg
        if avg is None:
            assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (3,) for a in got[:3])
    bad = counts.copy(); bad[1, 3] = 1
    with pytest.raises(ValueError, match="non-finite"):
        EV.metrics_from_class_counts(bad, ap_sum, conf, "macro")
    with pytest.raises(ValueError, match="avg"):
        EV.metrics_from_class_counts(counts, ap_sum, conf, "samples")
    empty = counts.copy(); empty[1, :3] = 0
    conf1 = conf.copy(); conf1[0] += conf1[1]; conf1[1] = 0         # class 1 has no label
    with pytest.raises(ValueError, match="class 1"):
        EV.metrics_from_class_counts(empty, ap_sum, conf1, "macro")
    for cls in (0, 1, 2, -1):
        fps, tps, thr, _ = E.roc_points_ref(pred, grade, cls)
        for drop in (True, False):
            got, want = EV.roc_curve_from_points(fps, tps, thr, drop), E.roc_curve_ref(fps, tps, thr, drop)
            for a, b in zip(got, want):
                assert a.dtype == np.float64 and np.array_equal(a, b), (cls, drop)
            assert EV.roc_auc_from_curve(got[0], got[1]) == skm.auc(got[0], got[1])
    with pytest.raises(ValueError):
        EV.roc_curve_from_points([0, 0], [1, 5], [0.5, 0.25])           # no negative element

"""Numpy restatements of ph_rank_counts_classes and ph_roc_points (csrc/evalmetrics.hip) and of the host arithmetic behind
evaluate.grading_metrics_device(avg=...) and evaluate.roc_curve_device.  None of the project's code
runs here; tests/test_evalavg_emulation_cpu.py holds these to sklearn, tests/test_gpu_evalavg.py holds the kernels to these.

Every function takes `defect=`: a named wrong variant of the same computation.  The CPU self-test checks that each one fails
at least one of its checks."""
import numpy as np

from tests.eval_emulation import TILE, tree_sum

MAX_N = 1 << 20
MAX_C = 16
OK, EINVAL = 0, -22

DEFECTS = ("gt_for_ge", "ties_whole", "oor_every_class", "stride_one", "rep_last", "drop_after_origin", "weights_uniform",
           "weighted_f1_macro", "tps_strict")


def column(pred, grade, c, defect=None):
    """(scores f32 [N], labels bool [N]) of the one-vs-rest problem of class c: element n = (pred[n][c], grade[n] == c)."""
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    flat = pred.reshape(-1)
    stride = 1 if defect == "stride_one" else C
    s = flat[np.arange(N) * stride + c]
    return s, np.asarray(grade, dtype=np.int64).reshape(-1) == c


def problem(pred, grade, cls, defect=None):
    """The elements ph_roc_points ranks: cls >= 0 a column, cls == -1 the N * C pairs in pair order i = n * C + c."""
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    if cls >= 0:
        return column(pred, grade, cls, defect)
    lab = np.asarray(grade, dtype=np.int64).reshape(N, 1) == np.arange(C).reshape(1, C)
    return pred.reshape(-1), lab.reshape(-1)


def _ge_counts(s, l):
    """Per element i (NaN scores take part in nothing and get zeros): ge_all = #{j: s_j >= s_i}, ge_pos = the positives among
    them, below_neg = #{j negative: s_j < s_i}, equal_neg = #{j negative: s_j == s_i} - by rank over the sorted scores."""
    out = np.zeros((5, s.shape[0]), dtype=np.int64)
    ok = ~np.isnan(s)
    sf, lf = s[ok].astype(np.float64), l[ok]
    order = np.argsort(sf, kind="stable")
    ss, ls = sf[order], lf[order]
    cp = np.concatenate([[0], np.cumsum(ls)])
    cn = np.concatenate([[0], np.cumsum(~ls)])
    left = np.searchsorted(ss, sf, side="left")               # #{j: s_j < s_i}
    right = np.searchsorted(ss, sf, side="right")             # #{j: s_j <= s_i}
    out[0, ok] = ss.shape[0] - left
    out[1, ok] = int(ls.sum()) - cp[left]
    out[2, ok] = cn[left]
    out[3, ok] = cn[right] - cn[left]
    out[4, ok] = ss.shape[0] - right                          # #{j: s_j > s_i}: what the `gt_for_ge` defect divides by
    return tuple(out)


def fixed_order_sum(term):
    """The kernel's summation order over one value per ROW: per block of TILE rows the tree, then per thread t the blocks
    t, t + TILE, .. in order, then the tree."""
    N = term.shape[0]
    nb = -(-N // TILE)
    part = tree_sum(np.pad(term, (0, nb * TILE - N)).reshape(nb, TILE))
    k = -(-nb // TILE)
    lanes = np.pad(part, (0, k * TILE - nb)).reshape(k, TILE)
    acc = np.zeros(TILE, dtype=np.float64)
    for row in lanes:
        acc = acc + row
    return float(tree_sum(acc))


def rank_counts_classes_ref(pred, grade, defect=None):
    """(counts int64 [C, 4] = P_c, concordant_c, tied_c, bad_c; ap_sum float64 [C]) of ph_rank_counts_classes."""
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    g = np.asarray(grade, dtype=np.int64).reshape(-1)
    counts = np.zeros((C, 4), dtype=np.int64)
    ap_sum = np.zeros(C, dtype=np.float64)
    oor = int(((g < 0) | (g >= C)).sum())
    for c in range(C):
        s, l = column(pred, grade, c, defect)
        ge_all, ge_pos, below, equal, gt = _ge_counts(s, l)
        if defect == "gt_for_ge":
            ge_all = gt
        term = np.zeros(N, dtype=np.float64)
        live = l & (ge_all > 0)
        term[live] = ge_pos[live].astype(np.float64) / ge_all[live].astype(np.float64)
        counts[c] = (int(l.sum()), int(below[l].sum()), int(equal[l].sum()),
                     int((~np.isfinite(s)).sum()) + (oor if (c == 0 or defect == "oor_every_class") else 0))
        ap_sum[c] = fixed_order_sum(term)
    return counts, ap_sum


def roc_points_ref(pred, grade, cls, defect=None):
    """(fps int32 [K], tps int32 [K], thr f32 [K], bad) of ph_roc_points: K distinct non-NaN scores, descending."""
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    g = np.asarray(grade, dtype=np.int64).reshape(-1)
    s, l = problem(pred, grade, cls, defect)
    bad = int((~np.isfinite(s)).sum()) + int(((g < 0) | (g >= C)).sum())
    ok = ~np.isnan(s)
    sf, lf = s[ok], l[ok]
    if defect == "rep_last":
        # representative = the LAST equal element, slot = the number of ELEMENTS (not representatives) with a larger score
        t = np.unique(sf)[::-1]
        slot = np.array([int((sf > v).sum()) for v in t], dtype=np.int64)
        K = int(slot.max()) + 1 if t.size else 0
        fps, tps, thr = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.float32)
        for v, k in zip(t, slot):
            thr[k] = v
            tps[k] = int((lf & (sf >= v)).sum())
            fps[k] = int((~lf & (sf >= v)).sum())
        return fps, tps, thr, bad
    _, first = np.unique(sf, return_index=True)                # the FIRST element of each distinct score, ascending
    t = sf[first][::-1].astype(np.float32)                     # the thresholds, descending
    asc = np.sort(sf)
    order = np.argsort(sf, kind="stable")
    cp = np.concatenate([[0], np.cumsum(lf[order])])
    side = "right" if defect == "tps_strict" else "left"
    lo = np.searchsorted(asc, t, side=side)                    # elements below t_k
    tps = (int(lf.sum()) - cp[lo]).astype(np.int32)
    fps = ((asc.shape[0] - lo) - (int(lf.sum()) - cp[lo])).astype(np.int32)
    return fps, tps, t, bad


def f1_per_class(conf):
    conf = np.asarray(conf, dtype=np.int64)
    tp = np.diag(conf).astype(np.float64)
    denom = (conf.sum(axis=1) + conf.sum(axis=0)).astype(np.float64)
    return np.divide(2.0 * tp, denom, out=np.zeros(conf.shape[0]), where=denom > 0)


def class_metrics(counts, ap_sum, conf, avg, defect=None):
    """(auc, ap, f1) under avg = "macro" | "weighted" | None from the per-class counts and the confusion matrix."""
    counts = np.asarray(counts, dtype=np.int64)
    C = counts.shape[0]
    N = int(np.asarray(conf).sum())
    P = counts[:, 0].astype(np.float64)
    Q = N - P
    half = 1.0 if defect == "ties_whole" else 2.0
    auc = (counts[:, 1] + counts[:, 2] / half) / (P * Q)
    ap = np.asarray(ap_sum, dtype=np.float64) / P
    f1 = f1_per_class(conf)
    if avg is None:
        return auc, ap, f1
    if avg == "macro":
        w = np.full(C, 1.0 / C)
    elif avg == "weighted":
        w = np.full(C, 1.0 / C) if defect == "weights_uniform" else P / N
    else:
        raise ValueError(avg)
    wf = np.full(C, 1.0 / C) if defect == "weighted_f1_macro" else w
    return float((auc * w).sum()), float((ap * w).sum()), float((f1 * wf).sum())


def roc_curve_ref(fps, tps, thr, drop_intermediate=True, defect=None):
    """sklearn's roc_curve from the integer points: drop the points whose second differences of fps and tps are both zero
    (the ends stay; more than two points), THEN prepend the origin with threshold inf, then divide by the last counts."""
    fps, tps, thr = (np.asarray(a, dtype=np.float64) for a in (fps, tps, thr))

    def drop(f, t, h):
        if not drop_intermediate or f.shape[0] <= 2:
            return f, t, h
        d2 = lambda a: a[2:] - 2.0 * a[1:-1] + a[:-2]
        keep = np.concatenate([[True], (d2(f) != 0) | (d2(t) != 0), [True]])
        return f[keep], t[keep], h[keep]

    def origin(f, t, h):
        return np.concatenate([[0.0], f]), np.concatenate([[0.0], t]), np.concatenate([[np.inf], h])

    if defect == "drop_after_origin":
        fps, tps, thr = drop(*origin(fps, tps, thr))
    else:
        fps, tps, thr = origin(*drop(fps, tps, thr))
    return fps / fps[-1], tps / tps[-1], thr


def trapezoid(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0).sum())


def scores(kind, N, C, seed):
    """The input families of these tests: pred f32 [N, C], grade int64 [N] (every class occurs when N >= C)."""
    rng = np.random.default_rng(seed)
    grade = rng.integers(0, C, N).astype(np.int64)
    if N >= C:
        grade[rng.permutation(N)[:C]] = np.arange(C)
    if kind == "continuous":
        pred = rng.standard_normal((N, C)).astype(np.float32)
    elif kind == "decimal":                                   # rounded to one decimal: heavy ties
        pred = (np.round(rng.standard_normal((N, C)) * 10) / 10).astype(np.float32)
    elif kind == "constant":                                  # one constant column, the others continuous
        pred = rng.standard_normal((N, C)).astype(np.float32)
        pred[:, seed % C] = np.float32(-0.75)
    elif kind == "equal":
        pred = np.full((N, C), -1.25, dtype=np.float32)
    elif kind == "increasing":                                # strictly increasing in pair order: all distinct
        pred = (np.arange(N * C, dtype=np.float32) / np.float32(4) - np.float32(N)).reshape(N, C)
    else:
        raise ValueError(kind)
    return pred, grade

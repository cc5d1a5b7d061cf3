"""Evaluation loop of the stage-2 trainer, reference MICCAI-2022/train_test_path_multi_distill.py:
`test()` (:409-501), `grading_metrics` (:516-526); and of the stage-1 teacher (`test_teacher`, train_test_MT.py:340-458)
for the grading and the survival task.

Both networks run their eval-mode forward through the C-ABI (running-statistics BatchNorm, dropout off, no tape).  The
reference copies logits, features and a loss scalar to the host after EVERY batch (three `.cpu()` / `.item()` syncs per
batch); here the per-batch results stay on the device and leave it once, after the last batch.  The ranking metrics
(ROC-AUC, average precision, F1) are host-side sklearn calls on ~N x 3 numbers, exactly as in the reference.

`test_patches` is the protocol the results are reported under: the same pass over the nine-patch
test loader (`augment.ResidentPatchLoader`), the predictions aggregated per patient (`aggregate_by_patient`), and the four
numbers taken from count kernels on the device (`grading_metrics_device`) instead of sklearn on copied rows.
`test_teacher_patches` is the same protocol for the stage-1 teacher under both tasks (per-patient hazards, C-indices, log-rank
p-value under survival), and `sync=` on either pass shards whole batches over data-parallel replicas behind one all-gather
(DESIGN.md section 24).  `grading_metrics_device(avg=)` and `roc_curve_device` are the reference's `avg` argument and the
curves of its `makeAUROCPlot` on the device; `avg=` / `curves=` carry them through both patch passes.
`survival_strata_device` is the survival side of the same analysis (risk strata at the percentile cuts, log-rank p-values
between adjacent strata, Kaplan-Meier tables; `km_step_function` for a curve's layout), and `strata=` carries it through
`test_teacher_patches`."""
import numbers

import numpy as np
import torch

from . import ops
from .networks_new import define_reg


def grading_metrics(y_label, y_pred, avg="micro"):
    """The reference's four ranking numbers of the grading task (train_test_path_multi_distill.py:516-526): ROC-AUC and
    average precision of the one-hot labels against the predicted scores, the F1 of the arg-max grades, and the F1 of the
    third class (grade IV) alone.  (Its per-batch `compute_accuracy` helper, :504-513, has no counterpart: `test()` below keeps
    the per-batch predictions on the device and counts once.)"""
    from sklearn import metrics as skm
    true_grade, pred_grade = np.argmax(y_label, axis=1), np.argmax(y_pred, axis=1)
    per_class_f1 = skm.f1_score(true_grade, pred_grade, average=None)
    return (skm.roc_auc_score(y_label, y_pred, average=avg), skm.average_precision_score(y_label, y_pred, average=avg),
            skm.f1_score(true_grade, pred_grade, average=avg), per_class_f1[2])


def test_model(opt, model, test_loader, device):
    """:530-611 - `test()` for the student alone (no frozen teacher): same 9-tuple, `probs_all` is None."""
    return test(opt, None, model, test_loader, device)


def test(opt, fix_model, model, test_loader, device):
    """:409-501 for the grading task.  Returns the reference's 9-tuple
    (loss_test, cindex_path, pvalue_test, surv_acc_test, grad_path_test, all_grad_metrics, pred_test, grads_test,
    feats_test); the survival entries are None.  `fix_model=None` gives `test_model()` (:530-611)."""
    if opt.task != "grad":
        raise NotImplementedError("evaluation of the survival (Cox) task is out of scope")
    from sklearn.preprocessing import LabelBinarizer
    outs, losses = _run(opt, (model, fix_model), test_loader, device, None,
                        lambda loss_reg, dev: _student_batch(opt, model, fix_model, loss_reg, dev, True))
    return _student_result(test_loader, outs[0], outs[2] if fix_model is not None else None, outs[1], outs[-1], losses,
                           _host_metric(lambda gt_all: LabelBinarizer().fit(gt_all).transform(gt_all)))    # :476-478


def test_teacher(opt, model, test_loader, device):
    """The stage-1 trainer's `test()` (MICCAI-2022/train_test_MT.py:340-458) for both tasks, with its 16-tuple
    (loss_test, loss_fuse_test, loss_path_test, loss_omic_test, cindex_test, cindex_path, cindex_omic, pvalue_test,
    surv_acc_test, grad_acc_test, grad_path_test, grad_omic_test, all_grad_metrics, pred_test, grads_test, feats_test).
    Per-batch losses and outputs stay on the device and leave it once, after the last batch; the survival batch losses are the
    forward-only fused Cox kernel, the three C-indices one concordance-count launch (utils.CIndex_lifeline's rule)."""
    if opt.task not in ("grad", "surv"):
        raise NotImplementedError("task %r" % opt.task)
    surv = opt.task == "surv"
    outs, losses = _run(opt, (model,), test_loader, device, None,
                        lambda loss_reg, dev: _teacher_batch(opt, model, loss_reg, dev, surv, True))
    return _teacher_result(test_loader, outs[:3], outs[3:6], outs[6], (outs[8], outs[7]) if surv else None, losses,
                           _host_metric(lambda gt_all: _one_hot(gt_all.astype(np.int64), opt.label_dim)))[0]    # :452


def metrics_from_counts(counts, ap_sum, conf):
    """Host arithmetic on the integers of ph_rank_counts (counts = P, concordant, tied, bad over M = conf.sum() * C pairs)
    and ph_confusion_counts: (rocauc, ap, f1_micro, f1_gradeIV) as sklearn computes them -
    AUC = (concordant + tied / 2) / (P Q), AP = ap_sum / P, F1 = 2 tp / (true + predicted) (0 where that is empty)."""
    conf = np.asarray(conf, dtype=np.int64)
    C = conf.shape[0]
    P, conc, tied, bad = (int(v) for v in counts)
    Q = int(conf.sum()) * C - P
    if bad:
        raise ValueError("%d non-finite scores or labels outside [0, %d)" % (bad, C))
    if P == 0 or Q == 0:
        raise ValueError("ROC-AUC and average precision need a positive and a negative pair (P = %d, Q = %d)" % (P, Q))
    if C < 3:
        raise ValueError("the F1 of grade IV is the F1 of class 2: label_dim >= 3")
    tp = np.diag(conf).astype(np.float64)
    denom = (conf.sum(axis=1) + conf.sum(axis=0)).astype(np.float64)
    f1 = np.divide(2.0 * tp, denom, out=np.zeros(C), where=denom > 0)
    n = float(conf.sum())
    return ((conc + tied / 2.0) / (float(P) * float(Q)), float(ap_sum) / P, float(2.0 * tp.sum() / (2.0 * n)), float(f1[2]))


AVERAGES = ("micro", "macro", "weighted", None)


def _check_avg(avg):
    if not (avg is None or (isinstance(avg, str) and avg in AVERAGES)):
        raise ValueError('avg must be "micro", "macro", "weighted" or None (per class), got %r' % (avg,))


def metrics_from_class_counts(counts, ap_sum, conf, avg="macro"):
    """Host arithmetic on the integers of ph_rank_counts_classes (counts [C, 4] = P_c, concordant_c, tied_c, bad_c over the
    N = conf.sum() elements of each one-vs-rest column; ap_sum [C]) and ph_confusion_counts, as sklearn's
    average="macro" | "weighted" | None computes them -
    AUC_c = (concordant_c + tied_c / 2) / (P_c Q_c) with Q_c = N - P_c, AP_c = ap_sum_c / P_c, F1_c = 2 tp / (true + predicted);
    "macro" the plain mean over the classes, "weighted" the mean with the supports P_c as weights (F1 too), None the three
    float64 [C] arrays.  Returns (rocauc, ap, f1, f1_gradeIV); f1_gradeIV is the F1 of class 2 in every form."""
    _check_avg(avg)
    if avg == "micro":
        raise ValueError('the micro average comes from the pair counts: metrics_from_counts')
    conf = np.asarray(conf, dtype=np.int64)
    C = conf.shape[0]
    counts = np.asarray(counts, dtype=np.int64).reshape(C, 4)
    ap_sum = np.asarray(ap_sum, dtype=np.float64).reshape(C)
    bad = int(counts[:, 3].sum())
    if bad:
        raise ValueError("%d non-finite scores or labels outside [0, %d)" % (bad, C))
    if C < 3:
        raise ValueError("the F1 of grade IV is the F1 of class 2: label_dim >= 3")
    n = int(conf.sum())
    P = counts[:, 0]
    Q = n - P
    for c in range(C):
        if P[c] == 0 or Q[c] == 0:
            raise ValueError("class %d: ROC-AUC and average precision need a positive and a negative element "
                             "(P = %d, Q = %d)" % (c, P[c], Q[c]))
    Pf, Qf = P.astype(np.float64), Q.astype(np.float64)
    auc = (counts[:, 1].astype(np.float64) + counts[:, 2].astype(np.float64) / 2.0) / (Pf * Qf)
    ap = ap_sum / Pf
    tp = np.diag(conf).astype(np.float64)
    denom = (conf.sum(axis=1) + conf.sum(axis=0)).astype(np.float64)
    f1 = np.divide(2.0 * tp, denom, out=np.zeros(C), where=denom > 0)
    if avg is None:
        return auc, ap, f1, float(f1[2])
    w = Pf if avg == "weighted" else None
    return float(np.average(auc, weights=w)), float(np.average(ap, weights=w)), float(np.average(f1, weights=w)), float(f1[2])


def grading_metrics_device(pred, grade, avg="micro"):
    """`grading_metrics` without sklearn and without copying the rows: pred f32 [N, C] and grade [N] stay on the device,
    two count kernels fill a few words, and ONE host read of those gives (rocauc, ap, f1, f1_gradeIV) - sklearn's values,
    ties included.  avg = "micro": ph_rank_counts and ph_confusion_counts, 5 + C * C words.
    avg = "macro" | "weighted" | None: ph_rank_counts_classes and ph_confusion_counts, 5 C + C * C words, the averages of
    `metrics_from_class_counts` (None: three float64 [C] arrays and f1_gradeIV) - DESIGN.md section 26.

    Raises ValueError for an unknown avg, for a non-finite score or a label outside [0, C), and when there is no positive or
    no negative pair - per class, naming the class, under the other averages (sklearn raises in those cases).  Every column
    of pred takes part whether or not its class occurs among the labels; the reference's LabelBinarizer would drop an absent
    class and then fail on the shape mismatch with pred.  Likewise f1_gradeIV is the F1 of class 2 (0.0 if it is neither a
    label nor a prediction), where sklearn's `average=None` indexes the classes that occur."""
    _check_avg(avg)
    C = pred.shape[1]
    if avg == "micro":
        buf = torch.empty(5 + C * C, device=pred.device, dtype=torch.int64)
        ops.rank_counts(pred, grade, out=buf[:5])
        ops.confusion_counts(pred, grade, out=buf[5:].view(C, C))
        host = buf.cpu()
        return metrics_from_counts(host[:4].tolist(), float(host[4:5].view(torch.float64)[0]), host[5:].view(C, C).numpy())
    buf = torch.empty(5 * C + C * C, device=pred.device, dtype=torch.int64)
    ops.rank_counts_classes(pred, grade, out=buf[:5 * C])
    ops.confusion_counts(pred, grade, out=buf[5 * C:].view(C, C))
    host = buf.cpu()
    return metrics_from_class_counts(host[:4 * C].view(C, 4).numpy(), host[4 * C:5 * C].view(torch.float64).numpy(),
                                     host[5 * C:].view(C, C).numpy(), avg)


def roc_curve_from_points(fps, tps, thr, drop_intermediate=True):
    """sklearn's roc_curve from the integer points of ph_roc_points (descending thresholds): with `drop_intermediate` (and
    more than two points) keep the points where the second difference of fps or of tps is not zero, and both ends - applied
    BEFORE the origin is prepended; then prepend (0, 0, inf) and divide by the last fps / tps.  -> (fpr, tpr, thresholds),
    float64."""
    fps, tps = np.asarray(fps, dtype=np.float64), np.asarray(tps, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    if drop_intermediate and fps.shape[0] > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    fps, tps, thr = np.r_[0.0, fps], np.r_[0.0, tps], np.r_[np.inf, thr]
    if fps[-1] <= 0 or tps[-1] <= 0:
        raise ValueError("a ROC curve needs a positive and a negative element (P = %d, Q = %d)" % (tps[-1], fps[-1]))
    return fps / fps[-1], tps / tps[-1], thr


def roc_curve_device(pred, grade, cls="micro", drop_intermediate=True):
    """sklearn's roc_curve(label, score, drop_intermediate=...) of column `cls` of pred [N, C] one-vs-rest, or with
    cls = "micro" of all N * C (score, label) pairs (the curves makeAUROCPlot draws, core/utils_analysis.py:172-215), the
    points counted on the device (ph_roc_points) and read in ONE host copy: (fpr, tpr, thresholds), float64, thresholds
    descending from inf.  Raises ValueError for a non-finite score or a label outside [0, C), and when the problem has no
    positive or no negative element."""
    buf = ops.roc_points(pred, grade, cls)
    M = (buf.shape[0] - 2) // 3
    host = buf.cpu()
    npts, bad = int(host[0]), int(host[1])
    if bad:
        raise ValueError("%d non-finite scores or labels outside [0, %d)" % (bad, pred.shape[1]))
    h = host.numpy()
    try:
        return roc_curve_from_points(h[2:2 + npts], h[2 + M:2 + M + npts], h[2 + 2 * M:2 + 2 * M + npts].view(np.float32),
                                     drop_intermediate)
    except ValueError as e:
        raise ValueError("class %r: %s" % (cls, e)) from None


def roc_auc_from_curve(fpr, tpr):
    """The area under a curve by the trapezoid rule, as sklearn.metrics.auc(fpr, tpr) computes it for an increasing fpr."""
    fpr, tpr = np.asarray(fpr, dtype=np.float64), np.asarray(tpr, dtype=np.float64)
    if fpr.shape[0] < 2 or fpr.shape != tpr.shape:
        raise ValueError("at least two points, as many fpr as tpr")
    return float((np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0).sum())


def check_percentile(percentile):
    """The tuple of 1 to 7 ascending percents in [0, 100] that `survival_strata_device` accepts; ValueError otherwise."""
    ok = isinstance(percentile, (tuple, list)) and 1 <= len(percentile) <= ops.SURV_MAX_K
    ok = ok and all(isinstance(v, numbers.Real) and not isinstance(v, bool) and 0.0 <= float(v) <= 100.0 for v in percentile)
    ok = ok and all(float(a) <= float(b) for a, b in zip(percentile[:-1], percentile[1:]))
    if not ok:
        raise ValueError("percentile must be 1 to %d ascending percents in [0, 100], got %r" % (ops.SURV_MAX_K, percentile))
    return tuple(float(v) for v in percentile)


def logrank_pvalue(o_minus_e, var):
    """p = erfc(sqrt(chi2 / 2)) of the one-degree-of-freedom log-rank statistic chi2 = (O - E)^2 / V; NaN where V <= 0 (an empty
    stratum, no event, one risk time) - the rule of utils.cox_log_rank."""
    import math
    if not var > 0.0:
        return float("nan")
    return math.erfc(math.sqrt(o_minus_e * o_minus_e / var / 2.0))


def _strata_layout(N, K, Gn, P):
    """The one buffer of `survival_strata_device`: (name, numpy dtype, entries) in storage order, the float64 fields first
    so that every field is aligned.  It drives the device views and the host views alike."""
    return (("cuts", np.float64, K), ("stat", np.float64, 2 * P), ("survival", np.float64, N * Gn),
            ("npoints", np.int32, 2), ("bad", np.int32, 1), ("sizes", np.int32, K + 1), ("group", np.int32, N),
            ("times", np.float32, N), ("at_risk", np.int32, N * Gn), ("observed", np.int32, N * Gn),
            ("censored", np.int32, N * Gn))


_TORCH_OF = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32}


def survival_strata_device(hazard, survtime, censor, percentile=(33, 66), group=None, G=None):
    """The survival analysis of core/utils_analysis.py on the device: the risk strata of the hazards at
    the percentile cuts (the first-i rule on np.percentile(hazard, percentile), with the reference's 2.99997 patch), lifelines'
    event table per stratum, the log-rank p-values between adjacent strata (getPValAggSurv_GBMLGG_Binary / _Multi) and the
    Kaplan-Meier estimate per stratum (makeKaplanMeierPlot).  hazard, survtime, censor: device tensors [N] (an event is
    censor > 0).  `group=` (an int device tensor [N]) with `G=` (its number of groups, 1 .. 8) replaces the percentile stage:
    the per-grade curves of makeKaplanMeierPlot; rows whose group lies outside [0, G) take part in nothing.

    Returns a dict of host arrays: cuts float64 [K] (empty with group=), group int32 [N], sizes int64 [K + 1] (or [G]),
    pvalues float64 [groups - 1] (the adjacent pairs (0, 1), (1, 2), .. in that order; NaN where V <= 0), stat float64
    [groups - 1, 2] = (O - E, V), times float32 [npoints], at_risk / observed / censored int32 [npoints, groups], survival
    float64 [npoints, groups], bad (non-finite hazards + rows left out of the table).

    Device work whatever N is: seven kernel launches and four memsets of the three C entries (2 + 2 + 3 launches, 3 + 1 + 0
    memsets) and no torch kernel; with group= five launches and one memset of the entries plus ONE torch copy (the groups,
    converted to int32, into the buffer).  ONE device-to-host copy, of the whole buffer at its capacity of N slots."""
    hazard = ops._f32(hazard).reshape(-1) if hazard is not None else None
    survtime, censor = ops._f32(survtime).reshape(-1), ops._f32(censor).reshape(-1)
    N = survtime.shape[0]
    if group is None:
        q = check_percentile(percentile)
        K, Gn = len(q), len(q) + 1
        if hazard is None or hazard.shape[0] != N or censor.shape[0] != N:
            raise ValueError("hazard, survtime and censor are [N] device tensors")
    else:
        if G is None or not 1 <= int(G) <= ops.SURV_MAX_G or group.numel() != N or censor.shape[0] != N:
            raise ValueError("group= needs one group per row and G= in 1 .. %d" % ops.SURV_MAX_G)
        K, Gn = 0, int(G)
    if not 2 <= N <= ops.SURV_MAX_N:
        raise ValueError("the survival strata need 2 <= N <= %d rows, got %d" % (ops.SURV_MAX_N, N))
    P = Gn - 1
    layout = _strata_layout(N, K, Gn, P)
    buf = torch.empty(sum(np.dtype(dt).itemsize * n for _, dt, n in layout), device=survtime.device, dtype=torch.uint8)

    def views(raw, view):
        out, at = {}, 0
        for name, dt, n in layout:
            nbytes = np.dtype(dt).itemsize * n
            out[name] = view(raw[at:at + nbytes], dt)
            at += nbytes
        return out
    d = views(buf, lambda b, dt: b.view(_TORCH_OF[dt]))
    if group is None:
        ops.surv_strata(hazard, q, d["cuts"], d["group"], d["sizes"], d["bad"])
    else:
        d["group"].copy_(ops.require_cuda(group, "group").reshape(-1))
    ops.surv_table(survtime, censor, d["group"], Gn, d["times"], d["at_risk"], d["observed"], d["censored"], d["npoints"])
    ops.surv_logrank_km(d["at_risk"], d["observed"], d["npoints"], Gn, [(g, g + 1) for g in range(P)], d["stat"], d["survival"])
    h = views(buf.cpu().numpy(), lambda b, dt: b.view(dt))
    npts, left_out = int(h["npoints"][0]), int(h["npoints"][1])
    out = {name: h[name][:npts * Gn].reshape(npts, Gn).copy() for name in ("at_risk", "observed", "censored", "survival")}
    stat = h["stat"].reshape(P, 2).copy()
    grp = h["group"].copy()
    if group is None:                                   # (with group= the entry that fills sizes and bad did not run)
        sizes, bad = h["sizes"].astype(np.int64), int(h["bad"][0])
    else:
        sizes, bad = np.bincount(grp[(grp >= 0) & (grp < Gn)], minlength=Gn).astype(np.int64), 0
    out.update(cuts=h["cuts"].copy(), group=grp, sizes=sizes, stat=stat, times=h["times"][:npts].copy(), bad=bad + left_out,
               pvalues=np.array([logrank_pvalue(float(v[0]), float(v[1])) for v in stat], dtype=np.float64))
    return out


def km_step_function(times, survival_column, at_risk_column):
    """One group's Kaplan-Meier curve as lifelines' `survival_function_` lays it out, from a column of the `survival` and
    `at_risk` arrays of `survival_strata_device`: (timeline, S) float64, the timeline starting at 0 with S = 1, the slots
    at which the group is no longer at risk dropped.  (A first time of 0 is the timeline's first entry, not a second one.)"""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    s = np.asarray(survival_column, dtype=np.float64).reshape(-1)
    keep = np.asarray(at_risk_column).reshape(-1) > 0
    if not (times.shape == s.shape == keep.shape):
        raise ValueError("times, survival_column and at_risk_column have one entry per slot")
    t, s = times[keep], s[keep]
    if t.shape[0] and t[0] == 0.0:
        return t, s
    return np.r_[0.0, t], np.r_[1.0, s]


def agg_spec(agg):
    """("mean" | "max", None) or ("quantile", q) for the aggregation names of `aggregate_by_patient`; ValueError otherwise."""
    if isinstance(agg, str) and agg in ops.AGG_FUN:
        return agg, None
    if isinstance(agg, str) and agg == "median":
        return "quantile", 0.5
    if isinstance(agg, (tuple, list)) and len(agg) == 2 and isinstance(agg[0], str) and agg[0] == "quantile" \
            and isinstance(agg[1], numbers.Real) and not isinstance(agg[1], bool) and 0.0 <= float(agg[1]) <= 1.0:
        return "quantile", float(agg[1])
    note = ""
    if agg == "p0.75":
        note = ('; the reference evaluates the name "p0.75" as np.percentile(x, 0.90), a percent - here that is '
                '("quantile", 0.009)')
    raise ValueError('agg must be "mean" or "max", or "median" or ("quantile", q) with q a fraction in [0, 1], got %r%s'
                     % (agg, note))


def aggregate_by_patient(loader, pred, agg="max"):
    """groupby('TCGA ID').agg(...) of the patch rows (core/utils_analysis.py:79-135, called with agg_type 'max' by
    evaluation_GBMLGG.py:55-61; :467 for the hazards of the survival task): pred f32 [rows, C] or [rows] on the device, in
    the row order of `loader` (a ResidentPatchLoader) -> device [G, C] or [G], patient g = loader.patients[g].

    agg: "mean", "max" (ph_group_agg), "median" (= quantile 0.5, pandas' median) or ("quantile", q) with q a FRACTION in
    [0, 1] (ph_group_quantile: numpy's percentile, method "linear"; at most 4096 rows per patient).  The reference's
    percentile form, agg_type 'p0.75', evaluates np.percentile(x, 0.90) - a percent: ("quantile", 0.009)."""
    fun, q = agg_spec(agg)
    if pred.shape[0] != loader.n_rows:
        raise ValueError("pred has %d rows, the loader %d" % (pred.shape[0], loader.n_rows))
    if pred.dim() not in (1, 2):
        raise ValueError("pred is [rows, C] or [rows]")
    x = pred.reshape(pred.shape[0], -1)
    if fun == "quantile":
        out = ops.group_quantile(x, loader.group_offsets, loader.group_order, loader.group_offsets_host, q)
    else:
        out = ops.group_agg(x, loader.group_offsets, loader.group_order, loader.group_offsets_host, fun)
    return out.reshape(-1) if pred.dim() == 1 else out


# ---- rows sharded over replicas.  The loader's batches stay the single-process batches; batch b is run
# by replica b % W.  The four functions below are index arithmetic and tensor reshapes only (no device call of their own):
# tests/test_eval_shard_cpu.py drives them on CPU tensors.
def shard_batches(n_rows, batch_size, rank, world_size):
    """The batches replica `rank` runs: [(b, lo, hi)] with b = rank, rank + W, .. and rows lo .. hi - 1 of batch b."""
    nb = -(-n_rows // batch_size)
    return [(b, b * batch_size, min((b + 1) * batch_size, n_rows)) for b in range(rank, nb, world_size)]


def shard_slots(n_rows, batch_size, world_size):
    """(number of batches, batch slots per replica = ceil(batches / W))."""
    nb = -(-n_rows // batch_size)
    return nb, -(-nb // world_size)


def pack_shard(rows, losses, n_rows, batch_size, world_size, like=None):
    """One replica's float32 send buffer: `slots` batch slots of batch_size rows each, then `slots` loss rows; unused
    slots, and the rows a partial batch leaves free, are zero.  rows: per batch run (in the order of `shard_batches`) a
    [rows of the batch, width] tensor; losses: per batch a [k] tensor.  `like`: a tensor whose device the buffer takes when
    the replica ran no batch (width and k then come from `like` = (width, k, device))."""
    _, slots = shard_slots(n_rows, batch_size, world_size)
    if rows:
        width, k, dev = rows[0].shape[1], losses[0].numel(), rows[0].device
    else:
        width, k, dev = like
    buf = torch.zeros(slots * batch_size * width + slots * k, device=dev, dtype=torch.float32)
    body = buf[:slots * batch_size * width].view(slots, batch_size, width)
    tail = buf[slots * batch_size * width:].view(slots, k)
    for s, (r, l) in enumerate(zip(rows, losses)):
        body[s, :r.shape[0]] = r
        tail[s] = l.reshape(-1)
    return buf


def undeal_shards(gathered, n_rows, batch_size, world_size, width, k):
    """The rank-ordered concatenation of every replica's `pack_shard` buffer -> (rows [n_rows, width], losses [batches, k])
    in the single-process order: slot s of replica r is batch s * W + r."""
    nb, slots = shard_slots(n_rows, batch_size, world_size)
    per = slots * batch_size * width + slots * k
    g = gathered.reshape(world_size, per)
    body = g[:, :slots * batch_size * width].reshape(world_size, slots, batch_size, width)
    tail = g[:, slots * batch_size * width:].reshape(world_size, slots, k)
    rows = body.permute(1, 0, 2, 3).reshape(slots * world_size * batch_size, width)[:n_rows].contiguous()
    losses = tail.permute(1, 0, 2).reshape(slots * world_size, k)[:nb].contiguous()
    return rows, losses


def _sync_buffers(sync, modules):
    """Rank 0's buffers (BatchNorm running statistics, num_batches_tracked) on every replica."""
    bufs = [b for m in modules if m is not None for b in m.buffers()]
    if bufs:
        sync.broadcast_from0(bufs)


def _collect(loader, sync, one_batch):
    """Run `one_batch(batch) -> (per-row outputs, loss vector [k])` over the loader; returns (outputs concatenated over
    the rows, losses [batches, k]).  With `sync`, replica r runs the batches r, r + W, .. and ONE all-gather returns
    every replica's rows and losses, which `undeal_shards` puts back into row order."""
    if sync is None:                    # any iterable loader with __len__ and .dataset
        outs, losses = [], []
        for batch in loader:
            o, l = one_batch(batch)
            outs.append(o); losses.append(l)
        return [torch.cat([o[j] for o in outs]) for j in range(len(outs[0]))], torch.stack(losses)
    W, n_rows, B = sync.world_size, loader.n_rows, loader.batch_size
    packed, losses, meta = [], [], None
    for b, lo, hi in shard_batches(n_rows, B, sync.rank, W):
        o, l = one_batch(loader.rows(lo, hi))
        if meta is None:
            meta = [(tuple(t.shape[1:]), t.dtype) for t in o]
        packed.append(torch.cat([t.reshape(t.shape[0], -1).float() for t in o], dim=1))
        losses.append(l)
    if meta is None:                    # more replicas than batches: this one ran none; its shapes come from one row
        o, l = one_batch(loader.rows(0, 1))
        meta = [(tuple(t.shape[1:]), t.dtype) for t in o]
        like = (sum(t[0].numel() for t in o), l.numel(), o[0].device)
    else:
        like = None
    widths = [int(torch.Size(shape).numel()) for shape, _ in meta]
    k = l.numel()
    buf = pack_shard(packed, losses, n_rows, B, W, like=like)
    rows, loss = undeal_shards(sync.all_gather_cat(buf), n_rows, B, W, sum(widths), k)
    outs, at = [], 0
    for (shape, dtype), w in zip(meta, widths):
        outs.append(rows[:, at:at + w].reshape((n_rows,) + shape).to(dtype).contiguous())
        at += w
    return outs, loss


def _run(opt, nets, loader, device, sync, make_batch):
    """The one pass behind `test`, `test_teacher` and the patch forms: `nets` (the first one carries the regulariser; None
    entries are skipped) in eval mode, under `sync` rank 0's buffers on every replica, then `_collect` over
    `make_batch(loss_reg, dev)` without a tape."""
    for net in nets:
        if net is not None:
            net.eval()
    with torch.no_grad():
        if sync is not None:
            _sync_buffers(sync, nets)
        return _collect(loader, sync, make_batch(define_reg(opt, nets[0]), torch.device(device)))


def _student_batch(opt, model, fix_model, loss_reg, dev, labels):
    """one_batch of the stage-2 student (:427-441): outputs [pred_path, feat_path] + [the frozen teacher's fused pred, if
    there is one] + [grade, if `labels`]; loss [1]."""
    def one_batch(batch):
        x_path, x_grph, x_omic, censor, survtime, grade = batch
        x_path = x_path.to(dev, non_blocking=True)
        x_omic = x_omic.to(dev, non_blocking=True)
        grade = grade.to(dev, non_blocking=True)
        _, feat_path, _, pred_path, _ = model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)                 # :427
        outs = [pred_path, feat_path]
        if fix_model is not None:
            _, _, _, _, _, pred, _, _, _, _, _ = fix_model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)   # :431
            outs.append(pred)
        loss_nll = ops.NLLFn.apply(pred_path, grade, float(pred_path.shape[0]))                            # :439
        loss = (opt.lambda_nll * loss_nll + opt.lambda_reg * loss_reg).reshape(1)                          # :441
        return (outs + [grade.reshape(-1)]) if labels else outs, loss
    return one_batch


def _teacher_batch(opt, model, loss_reg, dev, surv, labels):
    """one_batch of the stage-1 teacher (train_test_MT.py:355-379): outputs [pred, pred_path, pred_omic, feat_fuse, feat_path,
    feat_omic] + [grade (, censor, survtime under `surv`), if `labels`]; loss [4] = (total, fuse, path, omic)."""
    def one_batch(batch):
        x_path, x_grph, x_omic, censor, survtime, grade = batch
        x_path = x_path.to(dev, non_blocking=True)
        x_omic = x_omic.to(dev, non_blocking=True)
        grade = grade.to(dev, non_blocking=True)
        feat_fuse, feat_path, feat_omic, _, _, pred, pred_path, pred_omic, _, _, _ = model(
            x_path=x_path, x_grph=x_grph, x_omic=x_omic)                                                  # :355-356
        own = [grade.reshape(-1)]
        if surv:
            censor = censor.to(dev, torch.float32, non_blocking=True)
            survtime = survtime.to(dev, torch.float32, non_blocking=True)
            branch = ops.surv_loss_terms(pred, pred_path, pred_omic, survtime, censor)                   # :366-369
            loss = opt.lambda_cox * branch.sum() + opt.lambda_reg * loss_reg                             # :379
            own += [censor.reshape(-1), survtime.reshape(-1)]
        else:
            bn = float(pred.shape[0])
            branch = torch.stack([ops.NLLFn.apply(p, grade, bn) for p in (pred, pred_path, pred_omic)])   # :374-377
            loss = opt.lambda_nll * branch.sum() + opt.lambda_reg * loss_reg
        outs = [pred, pred_path, pred_omic, feat_fuse, feat_path, feat_omic]
        return (outs + own) if labels else outs, torch.cat([loss.reshape(1), branch])
    return one_batch


def _one_hot(index, width):
    """float32 [len(index), width], a 1 at column index[i] of row i."""
    y = np.zeros((len(index), width), dtype=np.float32)
    y[np.arange(len(index)), index] = 1
    return y


def _host_metric(labels):
    """The builders' metric(pred, grade, probs, gt_all) of the plain forms: sklearn on the copied rows against
    labels(gt_all)."""
    return lambda pred, grade, probs, gt_all: grading_metrics(labels(gt_all), probs)


def _device_metric(avg="micro"):
    """The builders' metric of the patch forms: the count kernels on the device rows, under the average `avg`."""
    return lambda pred, grade, probs, gt_all: grading_metrics_device(pred, grade, avg)


def _student_result(loader, d_path, d_fuse, d_feat, d_grade, losses, metric):
    """The 9-tuple of `test` from the collected device tensors (d_fuse None without a teacher); each array leaves the
    device here, once."""
    loss_test = float(losses.reshape(-1).sum().item()) / len(loader)                                       # :442, :465
    probs_path = d_path.cpu().numpy()
    probs_all = d_fuse.cpu().numpy() if d_fuse is not None else None
    feat_path_all = d_feat.cpu().numpy()
    gt = d_grade.cpu().numpy().reshape(-1)
    gt_all = gt.astype(np.float64)                                     # np.concatenate onto np.array([]) (:444)
    grad_path_test = float((probs_path.argmax(axis=1) == gt).sum()) / len(loader.dataset)                  # :458, :472
    if d_fuse is not None:
        print("fixed fuse branch:", *metric(d_fuse, d_grade, probs_all, gt_all))                           # :481
    all_grad_metrics = list(metric(d_path, d_grade, probs_path, gt_all))
    print("Path branch:", *all_grad_metrics)
    e = np.array([])
    pred_test = [e, e, e, e, e, probs_all, probs_path, None, gt_all]                                       # :491-492
    return (loss_test, None, None, None, grad_path_test, all_grad_metrics, pred_test, [None, None, None],
            [None, feat_path_all, None, gt_all])


def _teacher_result(loader, d_preds, d_feats, d_grade, surv_cols, losses, metric, more_counts=None):
    """(the 16-tuple of `test_teacher`, host `more_counts`) from the collected device tensors: d_preds and d_feats in the
    order fuse, path, omic; surv_cols = the rows' (survtime, censor) under the survival task, None under grading.
    `more_counts`: further int64 [k, 3] concordance counts on the device, read in the one copy of the rows' three.  Each
    array leaves the device here, once."""
    from . import utils as U
    nb = len(loader)
    loss_test, loss_fuse_test, loss_path_test, loss_omic_test = (float(v) / nb for v in
                                                                 losses.sum(0).double().cpu().numpy())    # :432-435
    feat_fuse_all, feat_path_all, feat_omic_all = (f.cpu().numpy() for f in d_feats)
    gt_all = d_grade.cpu().numpy().reshape(-1).astype(np.float64)                                          # :384
    e = np.array([])
    cindex_test = cindex_path = cindex_omic = pvalue_test = surv_acc_test = None
    grad_acc_test = grad_path_test = grad_omic_test = all_grad_metrics = None
    if surv_cols is not None:
        risk = [p.reshape(-1) for p in d_preds]
        t_all, c_all = surv_cols
        counts = ops.cindex_counts(t_all, c_all, risk)                                                     # :436-438
        if more_counts is not None:
            counts = torch.cat([counts, more_counts])
        counts = counts.cpu().numpy()
        counts, more_counts = counts[:3], counts[3:]
        risk_pred_all, risk_path_all, risk_omic_all = (r.cpu().numpy().astype(np.float64) for r in risk)
        censor_all, survtime_all = c_all.cpu().numpy().astype(np.float64), t_all.cpu().numpy().astype(np.float64)
        cindex_test, cindex_path, cindex_omic = (U.cindex_from_counts(c) for c in counts)
        pvalue_test = U.cox_log_rank(risk_pred_all, censor_all, survtime_all)                              # :439
        surv_acc_test = U.accuracy_cox(risk_pred_all, censor_all)                                         # :440
        pred_test = [risk_pred_all, risk_path_all, risk_omic_all, survtime_all, censor_all, None, None, None, gt_all]
    else:
        probs = [p.cpu().numpy() for p in d_preds]
        n = len(loader.dataset)
        grad_acc_test, grad_path_test, grad_omic_test = (float((p.argmax(axis=1) == gt_all).sum()) / n
                                                         for p in probs)                                   # :389-391, :442-444
        all_grad_metrics = []
        for name, d, p in zip(("Fused", "Path", "Omic"), d_preds, probs):
            mtr = metric(d, d_grade, p, gt_all)
            print("%s branch:" % name, *mtr)
            all_grad_metrics.extend(mtr)
        pred_test = [e, e, e, e, e] + probs + [gt_all]
    grads_test = [None, None, None]
    feats_test = [feat_fuse_all, feat_path_all, feat_omic_all, gt_all]
    return (loss_test, loss_fuse_test, loss_path_test, loss_omic_test, cindex_test, cindex_path, cindex_omic, pvalue_test,
            surv_acc_test, grad_acc_test, grad_path_test, grad_omic_test, all_grad_metrics, pred_test, grads_test,
            feats_test), more_counts


def _patient_grading(loader, agg, branches, avg="micro", curves=False):
    """The patient level of the grading task (core/utils_analysis.py:79-135, :152-167) for branches = ((name, device pred
    [rows, C] or None), ..): dict(y_label one-hot [G, C], y_pred_<name> (`aggregate_by_patient`), metrics_<name> (the four
    numbers of calcAggGradMetrics, `grading_metrics_device` under `avg`)); both entries of a None branch are None.  With
    `avg` other than "micro" the dict carries it as `avg`; with `curves`, roc_<name> = {0: (fpr, tpr, thresholds), ..,
    C - 1: .., "micro": ..} (`roc_curve_device` on the aggregated rows: the data makeAUROCPlot plots, :172-215) for every
    branch that has predictions."""
    C = branches[0][1].shape[1]
    out = dict(y_label=_one_hot(loader.patient_grade_host, C))
    if avg != "micro":
        out["avg"] = avg
    for name, d in branches:
        out["metrics_" + name] = out["y_pred_" + name] = None
        if d is not None:
            a = aggregate_by_patient(loader, d, agg)
            out["metrics_" + name] = list(grading_metrics_device(a, loader.patient_grade, avg))
            out["y_pred_" + name] = a.cpu().numpy()
            if curves:
                out["roc_" + name] = {c: roc_curve_device(a, loader.patient_grade, c) for c in list(range(C)) + ["micro"]}
    return out


def test_patches(opt, fix_model, model, loader, device, agg="max", sync=None, avg="micro", curves=False):
    """The pass the reference's trainers take their final figures from: `test()` over `test_loader_patches`
    (train_test_path_multi_distill.py:360-366, train_test_MT.py:287-289), then the per-patient aggregation and `calcAggGradMetrics`
    (core/utils_analysis.py:79-135, :152-167) - here over a `augment.ResidentPatchLoader`, with the metric tail on the device.

    Returns (patch_result, patient_result).  patch_result is the 9-tuple `test()` returns for the same loader (the same
    forward calls in the same order; loss, accuracy, predictions and features bit for bit), its all_grad_metrics computed by
    `grading_metrics_device`.  patient_result: dict(patients, y_label one-hot [G, C], y_pred_path [G, C], y_pred_fuse (None
    without a teacher), metrics_path, metrics_fuse (None without a teacher), agg) - the four numbers of calcAggGradMetrics
    for one split.  `fix_model=None` is the student-only form.  The number of host reads does not depend on the number of
    batches.  `agg`: the names of `aggregate_by_patient`, echoed in patient_result["agg"].

    `sync` (a dist.ReplicaSync): the rows are sharded over the replicas, whole batches at a time (batch b on replica
    b % world_size), and every replica returns the single-process result of RANK 0's networks bit for bit.  Training keeps
    per-replica BatchNorm running statistics; the reference's nn.DataParallel keeps replica 0's.  An evaluation must use
    one set everywhere, or the replicas' rows do not belong to one model: the buffers of `model` and `fix_model` are
    first broadcast from rank 0, which OVERWRITES the other replicas' running statistics (train mode never reads them).
    Then one all-gather per pass returns the rows and the per-batch losses; the metric tail runs on every replica.

    `avg` ("micro", "macro", "weighted" or None = per class; the `avg` of the reference's grading_metrics and
    calcAggGradMetrics): the average of the patch-level and patient-level metric lists; other than "micro" it is echoed in
    patient_result["avg"].  `curves=True` adds patient_result["roc_path"] (and "roc_fuse" with a teacher): per class and
    "micro" the (fpr, tpr, thresholds) of `roc_curve_device` on the aggregated patient rows."""
    if opt.task != "grad":
        raise NotImplementedError("evaluation of the survival (Cox) task is out of scope")
    agg_spec(agg)
    _check_avg(avg)
    outs, losses = _run(opt, (model, fix_model), loader, device, sync,
                        lambda loss_reg, dev: _student_batch(opt, model, fix_model, loss_reg, dev, sync is None))
    d_path = outs[0].float().contiguous()
    d_fuse = outs[2].float().contiguous() if fix_model is not None else None
    d_grade = (outs[-1] if sync is None else loader.grade[loader.row_roi]).reshape(-1)
    patch_result = _student_result(loader, d_path, d_fuse, outs[1], d_grade, losses, _device_metric(avg))
    patient_result = dict(patients=list(loader.patients), agg=agg,
                          **_patient_grading(loader, agg, (("path", d_path), ("fuse", d_fuse)), avg, curves))
    print("Patient level (%s):" % (agg,), *patient_result["metrics_path"])
    return patch_result, patient_result


CINDEX_MAX_N = 1 << 20                   # ph_cindex_counts: 2 <= N <= 1048576


def test_teacher_patches(opt, model, loader, device, agg=None, sync=None, avg="micro", curves=False, strata=None,
                         grade_classes=None):
    """`test_patches` for the stage-1 teacher (a three-branch PathomicNet, both tasks): the reference's `test()` over
    `test_loader_patches` (train_test_MT.py:287-289, :340-458), then the per-patient aggregation
    (core/utils_analysis.py:425-480) - DESIGN.md section 24.  Returns (patch_result, patient_result).

    patch_result: the 16-tuple `test_teacher` returns for the same loader (the same forward calls in the same order: bit
    for bit), except that under the grading task its twelve all_grad_metrics come from `grading_metrics_device`.  The number
    of host reads does not depend on the number of batches.

    Grading (agg default "max"): patient_result = dict(patients, y_label one-hot [G, C], y_pred_fuse / _path / _omic [G, C],
    metrics_fuse / _path / _omic (the four numbers of calcAggGradMetrics each), agg).

    Survival (agg default "mean", the reference's Hazard_mean; "median" and "max" are its other two, utils_analysis.py:467):
    patient_result = dict(patients, hazard_fuse / _path / _omic (float32 [G], aggregated on the device), survtime, censor
    (per patient, float64), cindex_fuse / _path / _omic (one ph_cindex_counts launch on the three aggregated vectors,
    utils.cindex_from_counts), pvalue, surv_acc (the fused branch, utils.cox_log_rank / utils.accuracy_cox), agg).  The loader
    must carry `censor` and `survtime` (ValueError otherwise), and the number of patients must lie in 2 .. 1048576, the
    range ph_cindex_counts accepts (ValueError otherwise).

    `sync`: as `test_patches` - rank 0's buffers everywhere, whole batches dealt over the replicas, one all-gather.
    `avg`, `curves`: as `test_patches`, for the grading task (roc_fuse / roc_path / roc_omic); the survival task has no
    grading metrics and ignores both.

    `strata` (survival task only; ValueError under grading): a percentile tuple of `survival_strata_device`, e.g. (33, 66) or
    (50,).  Adds strata_fuse / _path / _omic - the dict of `survival_strata_device` on each aggregated hazard vector (cuts,
    strata, adjacent log-rank p-values, event table, Kaplan-Meier estimates) - and km_grade, the same table and curves with
    group = loader.patient_grade and G = `grade_classes`, the number of grade classes (1 .. 8; None: the largest patient grade
    of this loader + 1, which is narrower than the reference's table when the split has no patient of the top grade): the
    "ground truth" curves of makeKaplanMeierPlot.  None returns the dict of before.  With `sync`, every replica
    computes them on the gathered, aggregated hazards: no further collective."""
    from . import utils as U
    if opt.task not in ("grad", "surv"):
        raise NotImplementedError("task %r" % opt.task)
    surv = opt.task == "surv"
    if strata is not None:
        if not surv:
            raise ValueError("strata= belongs to the survival task; the grading task has no hazards to stratify")
        strata = check_percentile(strata)
    if agg is None:
        agg = "mean" if surv else "max"
    agg_spec(agg)
    _check_avg(avg)
    G = loader.num_patients
    if surv:
        if not getattr(loader, "has_survival", False):
            raise ValueError("the survival task needs a loader built with censor= and survtime=")
        if not 2 <= G <= CINDEX_MAX_N:
            raise ValueError("the patient-level C-index needs 2 <= patients <= %d (the range of ph_cindex_counts), got %d"
                             % (CINDEX_MAX_N, G))
        if strata is not None:                          # (at least two patients from here on)
            top = int(loader.patient_grade_host.max())
            n_grades = top + 1 if grade_classes is None else int(grade_classes)
            if int(loader.patient_grade_host.min()) < 0 or not 1 <= n_grades <= ops.SURV_MAX_G or top >= n_grades:
                raise ValueError("km_grade needs patient grades in [0, grade_classes) with 1 <= grade_classes <= %d, got "
                                 "grades %d .. %d and grade_classes=%r"
                                 % (ops.SURV_MAX_G, int(loader.patient_grade_host.min()), top, grade_classes))
    outs, losses = _run(opt, (model,), loader, device, sync,
                        lambda loss_reg, dev: _teacher_batch(opt, model, loss_reg, dev, surv, False))
    d_grade = loader.grade[loader.row_roi]
    patient_result = dict(patients=list(loader.patients), agg=agg)
    names = ("fuse", "path", "omic")
    if surv:
        risk = [outs[j].reshape(-1) for j in range(3)]
        hazard = aggregate_by_patient(loader, torch.stack([r.float() for r in risk], dim=1).contiguous(), agg)
        hz = [hazard[:, j].contiguous() for j in range(3)]
        patch_result, counts = _teacher_result(
            loader, outs[:3], outs[3:6], d_grade, (loader.survtime[loader.row_roi], loader.censor[loader.row_roi]), losses,
            _device_metric(avg), more_counts=ops.cindex_counts(loader.patient_survtime, loader.patient_censor, hz))
        hz_host = hazard.cpu().numpy()
        p_censor = loader.patient_censor_host.astype(np.float64)
        p_time = loader.patient_survtime_host.astype(np.float64)
        for j, name in enumerate(names):
            patient_result["hazard_" + name] = np.ascontiguousarray(hz_host[:, j])
            patient_result["cindex_" + name] = U.cindex_from_counts(counts[j])
        h64 = patient_result["hazard_fuse"].astype(np.float64)
        patient_result.update(survtime=p_time, censor=p_censor, pvalue=U.cox_log_rank(h64, p_censor, p_time),
                              surv_acc=U.accuracy_cox(h64, p_censor))
        print("Patient level (%s): C-index" % (agg,), *(patient_result["cindex_" + n] for n in names))
        if strata is not None:
            for j, name in enumerate(names):
                patient_result["strata_" + name] = survival_strata_device(hz[j], loader.patient_survtime, loader.patient_censor,
                                                                          strata)
            patient_result["km_grade"] = survival_strata_device(None, loader.patient_survtime, loader.patient_censor,
                                                                group=loader.patient_grade, G=n_grades)
    else:
        d = [outs[j].float().contiguous() for j in range(3)]
        patch_result, _ = _teacher_result(loader, d, outs[3:6], d_grade, None, losses, _device_metric(avg))
        patient_result.update(_patient_grading(loader, agg, tuple(zip(names, d)), avg, curves))
        print("Patient level (%s):" % (agg,), *patient_result["metrics_fuse"])
    return patch_result, patient_result


def feature_audit_device(fuse, path, labels):
    """`evaluate_feature` of the MIA-2023 trainer ("MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":172-188)
    over two device stores [n, Df] (teacher) and [n, Dp] (student) and the int labels [n]: the intra-class and inter-class
    mean cosine similarity of either, and the mean |S_f - S_p| - without an n x n matrix (ph_sim_audit, DESIGN.md section 30;
    one memset, three launches, one host read).  -> dict(teacher_intra, teacher_inter, student_intra, student_inter,
    similarity_diff, intra_pairs, inter_pairs); a single class gives NaN for the inter-class means, as numpy's mean of an
    empty selection.  1 <= n <= 65536, 1 <= D <= 512, else ValueError."""
    from . import epoch
    if labels is None:
        raise ValueError("feature_audit_device: labels [n]")
    labels = torch.as_tensor(labels)
    if labels.is_floating_point():
        raise ValueError("feature_audit_device: integer labels")
    return epoch.audit_means(epoch.sim_audit(fuse, path, labels.to(fuse.device)))


def logit_audit_device(fuse_pred, path_pred):
    """`evaluate_logits` (:191-196): the mean absolute difference of the two cosine similarity matrices of the prediction
    stores (the reference's third argument is unused there).  -> float."""
    from . import epoch
    return float(epoch.audit_means(epoch.sim_audit(fuse_pred, path_pred, None))["similarity_diff"])

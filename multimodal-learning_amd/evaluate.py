"""Evaluation loop of the stage-2 trainer, reference MICCAI-2022/train_test_path_multi_distill.py:
`test()` (:409-501), `grading_metrics` (:516-526); and of the stage-1 teacher (`test_teacher`, train_test_MT.py:340-458)
for the grading and the survival task.

Both networks run their eval-mode forward through the C-ABI (running-statistics BatchNorm, dropout off, no tape).  The
reference copies logits, features and a loss scalar to the host after EVERY batch (three `.cpu()` / `.item()` syncs per
batch); here the per-batch results stay on the device and leave it once, after the last batch.  The ranking metrics
(ROC-AUC, average precision, F1) are host-side sklearn calls on ~N x 3 numbers, exactly as in the reference.

`test_patches` is the protocol the results are reported under: the same pass over the nine-patch
test loader (`augment.ResidentPatchLoader`), the predictions aggregated per patient (`aggregate_by_patient`), and the four
numbers taken from count kernels on the device (`grading_metrics_device`) instead of sklearn on copied rows."""
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
    if fix_model is not None:
        fix_model.eval()
    model.eval()
    dev = torch.device(device)
    preds_path, preds_fuse, feats, grades, losses = [], [], [], [], []
    with torch.no_grad():
        loss_reg = define_reg(opt, model)
        for x_path, x_grph, x_omic, censor, survtime, grade in test_loader:
            x_path = x_path.to(dev, non_blocking=True)
            x_omic = x_omic.to(dev, non_blocking=True)
            grade = grade.to(dev, non_blocking=True)
            _, feat_path, _, pred_path, _ = model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)            # :427
            pred = None
            if fix_model is not None:
                _, _, _, _, _, pred, _, _, _, _, _ = fix_model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)  # :431
            loss_nll = ops.NLLFn.apply(pred_path, grade, float(pred_path.shape[0]))                        # :439
            losses.append((opt.lambda_nll * loss_nll + opt.lambda_reg * loss_reg).reshape(1))              # :441
            preds_path.append(pred_path); preds_fuse.append(pred); feats.append(feat_path); grades.append(grade)
    nb = len(losses)
    loss_test = float(torch.cat(losses).sum().item()) / len(test_loader)                                   # :442, :465
    probs_path = torch.cat(preds_path).cpu().numpy()
    probs_all = torch.cat(preds_fuse).cpu().numpy() if fix_model is not None else None
    feat_path_all = torch.cat(feats).cpu().numpy()
    gt = torch.cat(grades).cpu().numpy().reshape(-1)
    gt_all = gt.astype(np.float64)                                     # np.concatenate onto np.array([]) (:444)
    grad_path_test = float((probs_path.argmax(axis=1) == gt).sum()) / len(test_loader.dataset)             # :458, :472
    enc = LabelBinarizer()
    enc.fit(gt_all)
    grad_gt = enc.transform(gt_all)                                                                        # :476-478
    if fix_model is not None:
        rocauc_fuse, ap_fuse, f1_micro_fuse, f1_gradeIV_fuse = grading_metrics(grad_gt, probs_all)         # :481
        print("fixed fuse branch:", rocauc_fuse, ap_fuse, f1_micro_fuse, f1_gradeIV_fuse)
    rocauc_path, ap_path, f1_micro_path, f1_gradeIV_path = grading_metrics(grad_gt, probs_path)
    print("Path branch:", rocauc_path, ap_path, f1_micro_path, f1_gradeIV_path)
    all_grad_metrics = [rocauc_path, ap_path, f1_micro_path, f1_gradeIV_path]
    e = np.array([])
    pred_test = [e, e, e, e, e, probs_all, probs_path, None, gt_all]                                       # :491-492
    grads_test = [None, None, None]
    feats_test = [None, feat_path_all, None, gt_all]
    del nb
    return loss_test, None, None, None, grad_path_test, all_grad_metrics, pred_test, grads_test, feats_test


def test_teacher(opt, model, test_loader, device):
    """The stage-1 trainer's `test()` (MICCAI-2022/train_test_MT.py:340-458) for both tasks, with its 16-tuple
    (loss_test, loss_fuse_test, loss_path_test, loss_omic_test, cindex_test, cindex_path, cindex_omic, pvalue_test,
    surv_acc_test, grad_acc_test, grad_path_test, grad_omic_test, all_grad_metrics, pred_test, grads_test, feats_test).
    Per-batch losses and outputs stay on the device and leave it once, after the last batch; the survival batch losses are the
    forward-only fused Cox kernel, the three C-indices one concordance-count launch (utils.CIndex_lifeline's rule)."""
    from . import utils as U
    if opt.task not in ("grad", "surv"):
        raise NotImplementedError("task %r" % opt.task)
    surv = opt.task == "surv"
    model.eval()
    dev = torch.device(device)
    preds, feats, losses, censors, times, grades = [], [], [], [], [], []
    with torch.no_grad():
        loss_reg = define_reg(opt, model)
        for x_path, x_grph, x_omic, censor, survtime, grade in test_loader:
            x_path = x_path.to(dev, non_blocking=True)
            x_omic = x_omic.to(dev, non_blocking=True)
            grade = grade.to(dev, non_blocking=True)
            feat_fuse, feat_path, feat_omic, _, _, pred, pred_path, pred_omic, _, _, _ = model(
                x_path=x_path, x_grph=x_grph, x_omic=x_omic)                                                  # :355-356
            if surv:
                censor = censor.to(dev, torch.float32, non_blocking=True)
                survtime = survtime.to(dev, torch.float32, non_blocking=True)
                branch = ops.surv_loss_terms(pred, pred_path, pred_omic, survtime, censor)               # :366-369
                loss = opt.lambda_cox * branch.sum() + opt.lambda_reg * loss_reg                         # :379
                censors.append(censor.reshape(-1)); times.append(survtime.reshape(-1))
            else:
                bn = float(pred.shape[0])
                branch = torch.stack([ops.NLLFn.apply(p, grade, bn) for p in (pred, pred_path, pred_omic)])   # :374-377
                loss = opt.lambda_nll * branch.sum() + opt.lambda_reg * loss_reg
            grades.append(grade.reshape(-1))
            losses.append(torch.cat([loss.reshape(1), branch]))
            preds.append((pred, pred_path, pred_omic)); feats.append((feat_fuse, feat_path, feat_omic))
    nb = len(test_loader)
    loss_test, loss_fuse_test, loss_path_test, loss_omic_test = (float(v) / nb for v in
                                                                 torch.stack(losses).sum(0).double().cpu().numpy())   # :432-435
    feat_fuse_all, feat_path_all, feat_omic_all = (torch.cat([f[k] for f in feats]).cpu().numpy() for k in range(3))
    gt_all = torch.cat(grades).cpu().numpy().reshape(-1).astype(np.float64)                                # :384
    e = np.array([])
    cindex_test = cindex_path = cindex_omic = pvalue_test = surv_acc_test = None
    grad_acc_test = grad_path_test = grad_omic_test = all_grad_metrics = None
    if surv:
        risk = [torch.cat([p[k].reshape(-1) for p in preds]) for k in range(3)]
        t_all, c_all = torch.cat(times), torch.cat(censors)
        counts = ops.cindex_counts(t_all, c_all, risk).cpu().numpy()                                       # :436-438
        risk_pred_all, risk_path_all, risk_omic_all = (r.cpu().numpy().astype(np.float64) for r in risk)
        censor_all, survtime_all = c_all.cpu().numpy().astype(np.float64), t_all.cpu().numpy().astype(np.float64)
        cindex_test, cindex_path, cindex_omic = (U.cindex_from_counts(c) for c in counts)
        pvalue_test = U.cox_log_rank(risk_pred_all, censor_all, survtime_all)                              # :439
        surv_acc_test = U.accuracy_cox(risk_pred_all, censor_all)                                         # :440
        pred_test = [risk_pred_all, risk_path_all, risk_omic_all, survtime_all, censor_all, None, None, None, gt_all]
    else:
        probs_all, probs_path, probs_omic = (torch.cat([p[k] for p in preds]).cpu().numpy() for k in range(3))
        n = len(test_loader.dataset)
        grad_acc_test, grad_path_test, grad_omic_test = (float((p.argmax(axis=1) == gt_all).sum()) / n
                                                         for p in (probs_all, probs_path, probs_omic))       # :389-391, :442-444
        grad_gt = np.zeros((gt_all.shape[0], opt.label_dim), dtype=np.float32)                           # :452
        grad_gt[np.arange(gt_all.shape[0]), gt_all.astype(np.int64)] = 1
        all_grad_metrics = []
        for name, p in (("Fused", probs_all), ("Path", probs_path), ("Omic", probs_omic)):
            mtr = grading_metrics(grad_gt, p)
            print("%s branch:" % name, *mtr)
            all_grad_metrics.extend(mtr)
        pred_test = [e, e, e, e, e, probs_all, probs_path, probs_omic, gt_all]
    grads_test = [None, None, None]
    feats_test = [feat_fuse_all, feat_path_all, feat_omic_all, gt_all]
    return (loss_test, loss_fuse_test, loss_path_test, loss_omic_test, cindex_test, cindex_path, cindex_omic, pvalue_test,
            surv_acc_test, grad_acc_test, grad_path_test, grad_omic_test, all_grad_metrics, pred_test, grads_test, feats_test)


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


def grading_metrics_device(pred, grade):
    """`grading_metrics` (micro average only) without sklearn and without copying the rows: pred f32 [N, C] and grade [N]
    stay on the device, two count kernels (ph_rank_counts, ph_confusion_counts) fill 5 + C * C words, and ONE host read of
    those gives (rocauc, ap, f1_micro, f1_gradeIV) - sklearn's values, ties included.

    Raises ValueError for a non-finite score or a label outside [0, C), and when there is no positive or no negative pair
    (sklearn raises in those cases).  Every column of pred takes part whether or not its class occurs among the labels;
    the reference's LabelBinarizer would drop an absent class and then fail on the shape mismatch with pred.  Likewise
    f1_gradeIV is the F1 of class 2 (0.0 if it is neither a label nor a prediction), where sklearn's `average=None`
    indexes the classes that occur."""
    C = pred.shape[1]
    buf = torch.empty(5 + C * C, device=pred.device, dtype=torch.int64)
    ops.rank_counts(pred, grade, out=buf[:5])
    ops.confusion_counts(pred, grade, out=buf[5:].view(C, C))
    host = buf.cpu()
    return metrics_from_counts(host[:4].tolist(), float(host[4:5].view(torch.float64)[0]), host[5:].view(C, C).numpy())


def aggregate_by_patient(loader, pred, agg="max"):
    """groupby('TCGA ID').agg(max | mean) of the patch rows (core/utils_analysis.py:79-135, called with agg_type 'max' by
    evaluation_GBMLGG.py:55-61): pred f32 [rows, C] on the device, in the row order of `loader` (a ResidentPatchLoader) ->
    device [G, C], patient g = loader.patients[g].  The percentile form (agg_type 'p0.75', which the reference evaluates as
    np.percentile(x, 0.90)) is not built."""
    if agg not in ops.AGG_FUN:
        raise ValueError('agg must be "mean" or "max" (the percentile aggregation is not built), got %r' % (agg,))
    if pred.shape[0] != loader.n_rows:
        raise ValueError("pred has %d rows, the loader %d" % (pred.shape[0], loader.n_rows))
    return ops.group_agg(pred, loader.group_offsets, loader.group_order, loader.group_offsets_host, agg)


def test_patches(opt, fix_model, model, loader, device, agg="max"):
    """The pass the reference's trainers take their final figures from: `test()` over `test_loader_patches`
    (train_test_path_multi_distill.py:360-366, train_test_MT.py:287-289), then the per-patient aggregation and `calcAggGradMetrics`
    (core/utils_analysis.py:79-135, :152-167) - here over a `augment.ResidentPatchLoader`, with the metric tail on the device.

    Returns (patch_result, patient_result).  patch_result is the 9-tuple `test()` returns for the same loader (the same
    forward calls in the same order; loss, accuracy, predictions and features bit for bit), its all_grad_metrics computed by
    `grading_metrics_device`.  patient_result: dict(patients, y_label one-hot [G, C], y_pred_path [G, C], y_pred_fuse (None
    without a teacher), metrics_path, metrics_fuse (None without a teacher), agg) - the four numbers of calcAggGradMetrics
    for one split.  `fix_model=None` is the student-only form.  The number of host reads does not depend on the number of
    batches.  Rows are not sharded over replicas: data-parallel evaluation is out of scope."""
    if opt.task != "grad":
        raise NotImplementedError("evaluation of the survival (Cox) task is out of scope")
    if agg not in ops.AGG_FUN:
        raise ValueError('agg must be "mean" or "max" (the percentile aggregation is not built), got %r' % (agg,))
    if fix_model is not None:
        fix_model.eval()
    model.eval()
    dev = torch.device(device)
    preds_path, preds_fuse, feats, grades, losses = [], [], [], [], []
    with torch.no_grad():
        loss_reg = define_reg(opt, model)
        for x_path, x_grph, x_omic, censor, survtime, grade in loader:
            x_path = x_path.to(dev, non_blocking=True)
            x_omic = x_omic.to(dev, non_blocking=True)
            grade = grade.to(dev, non_blocking=True)
            _, feat_path, _, pred_path, _ = model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)
            pred = None
            if fix_model is not None:
                _, _, _, _, _, pred, _, _, _, _, _ = fix_model(x_path=x_path, x_grph=x_grph, x_omic=x_omic)
            loss_nll = ops.NLLFn.apply(pred_path, grade, float(pred_path.shape[0]))
            losses.append((opt.lambda_nll * loss_nll + opt.lambda_reg * loss_reg).reshape(1))
            preds_path.append(pred_path); preds_fuse.append(pred); feats.append(feat_path); grades.append(grade)
        d_path = torch.cat(preds_path).float().contiguous()
        d_fuse = torch.cat(preds_fuse).float().contiguous() if fix_model is not None else None
        d_grade = torch.cat(grades).reshape(-1)
        loss_test = float(torch.cat(losses).sum().item()) / len(loader)
        probs_path = d_path.cpu().numpy()
        probs_all = d_fuse.cpu().numpy() if d_fuse is not None else None
        feat_path_all = torch.cat(feats).cpu().numpy()
        gt = d_grade.cpu().numpy().reshape(-1)
        gt_all = gt.astype(np.float64)
        grad_path_test = float((probs_path.argmax(axis=1) == gt).sum()) / len(loader.dataset)
        metrics_fuse = None
        if d_fuse is not None:
            print("fixed fuse branch:", *grading_metrics_device(d_fuse, d_grade))
        all_grad_metrics = list(grading_metrics_device(d_path, d_grade))
        print("Path branch:", *all_grad_metrics)
        e = np.array([])
        patch_result = (loss_test, None, None, None, grad_path_test, all_grad_metrics,
                        [e, e, e, e, e, probs_all, probs_path, None, gt_all], [None, None, None],
                        [None, feat_path_all, None, gt_all])
        # per patient
        G, C = loader.num_patients, d_path.shape[1]
        y_label = np.zeros((G, C), dtype=np.float32)
        y_label[np.arange(G), loader.patient_grade_host] = 1
        agg_path = aggregate_by_patient(loader, d_path, agg)
        metrics_path = list(grading_metrics_device(agg_path, loader.patient_grade))
        y_pred_fuse = None
        if d_fuse is not None:
            agg_fuse = aggregate_by_patient(loader, d_fuse, agg)
            metrics_fuse = list(grading_metrics_device(agg_fuse, loader.patient_grade))
            y_pred_fuse = agg_fuse.cpu().numpy()
        patient_result = dict(patients=list(loader.patients), y_label=y_label, y_pred_path=agg_path.cpu().numpy(),
                              y_pred_fuse=y_pred_fuse, metrics_path=metrics_path, metrics_fuse=metrics_fuse, agg=agg)
        print("Patient level (%s):" % agg, *metrics_path)
    return patch_result, patient_result

"""Evaluation loop of the stage-2 trainer, reference MICCAI-2022/train_test_path_multi_distill.py:
`test()` (:409-501), `grading_metrics` (:516-526); and of the stage-1 teacher (`test_teacher`, train_test_MT.py:340-458)
for the grading and the survival task.

Both networks run their eval-mode forward through the C-ABI (running-statistics BatchNorm, dropout off, no tape).  The
reference copies logits, features and a loss scalar to the host after EVERY batch (three `.cpu()` / `.item()` syncs per
batch); here the per-batch results stay on the device and leave it once, after the last batch.  The ranking metrics
(ROC-AUC, average precision, F1) are host-side sklearn calls on ~N x 3 numbers, exactly as in the reference."""
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

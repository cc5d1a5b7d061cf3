"""train() of the three stage-2 trainers (MICCAI-2022/train_test_path_multi_distill.py:144-406,
"MIA 2022/train_test_path_multi_distill_v2.py":292-587, "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":
199-537) over DistillStep: the last of the five free functions of the drop-in boundary.

The batch body is the step (replayed from one HIP graph from the third batch on); what the reference reads back after every
batch - loss sums, correct predictions, GK-Refine weights, query weights, the MIA-2023 per-sample stores - stays on the
device in an `epoch.EpochRecord` / `epoch.FeatureStores`, and the training part of an epoch reads the host exactly once,
`record.read()`.  The epoch-end decisions are `train_step.epoch_end_plan`; the test pass is `evaluate.test`.
DESIGN.md section 30.

`train_teacher` is train() of the three stage-1 trainers over TeacherStage1Step with an `epoch.Stage1Record` - the function that
writes the checkpoint `train` loads."""
import os
import random

import numpy as np
import torch

from . import evaluate
from .epoch import EpochRecord, FeatureStores, Stage1Record
from .train_step import DistillStep, EPOCH_AVERAGE_OVER, TeacherStage1Step, epoch_end_plan, teacher_epoch_end_plan

ARITY = {"miccai2022": 4, "mia2022": 6, "mia2023": 6}


def teacher_checkpoint_path(opt, k):
    """Where the stage-1 trainer left the fused teacher of split k (:157)."""
    return os.path.join(opt.checkpoints_dir, opt.exp_name, opt.fixed_model, "%s_%d_best.pt" % (opt.fixed_model, k))


def best_checkpoint_path(opt, k):
    """The student's best checkpoint of split k (:391-392 | v2 :571-572 | MIA-2023 :521-522)."""
    return os.path.join(opt.checkpoints_dir, opt.exp_name, opt.model_name, "%s_%d_best.pt" % (opt.model_name, k))


def _is_resident(loader):
    from .augment import ResidentTileLoader
    return isinstance(loader, ResidentTileLoader)


def _rows_of(loader, n_data):
    """len(train_loader.dataset) (:357); a resident loader's rows are its label vector's."""
    if _is_resident(loader):
        return int(loader.grade.shape[0])
    ds = getattr(loader, "dataset", None)
    return len(ds) if ds is not None else int(n_data)


def train(opt, train_loader, n_data, test_loader, test_loader_patches, device, k, variant="miccai2022", train_class_idx=None,
          audit=False):
    """The reference's train() for `variant`.  `train_loader`: the reference's loader (an iterable of its 8-tuples) or an
    augment.ResidentTileLoader, which is stepped n_data // opt.batch_size times per epoch through step.step(None, epoch).
    Returns (fix_model, model, optimizer, metric_logger) for "miccai2022" and (.., best_metrics, avg_metrics) for the two MIA
    trainers; metric_logger carries the reference's keys (empty lists there as well) and "epochs": one dict per epoch, the
    `EpochRecord.read()` of its training part plus, on a measured epoch, the test pass' numbers.  `audit=True` (MIA-2023):
    the similarity audit of the stores at every measured epoch (the reference's commented-out call, :466-468).
    `step_graph=False` on opt keeps the step eager."""
    if variant not in ARITY:
        raise ValueError("variant must be 'miccai2022', 'mia2022' or 'mia2023'")
    if audit and variant != "mia2023":
        raise ValueError("audit=True belongs to variant 'mia2023' (its trainer keeps the per-sample stores)")
    torch.cuda.manual_seed_all(2019); torch.manual_seed(2019); random.seed(2019); np.random.seed(2019)     # :145-149

    # ---- the frozen teacher (:157-166), the step with its record (and stores)
    load_path = teacher_checkpoint_path(opt, k)
    model_state_dict = torch.load(load_path, map_location=device, weights_only=False)["model_state_dict"]
    if hasattr(model_state_dict, "_metadata"):
        del model_state_dict._metadata
    step = DistillStep(opt, n_data, device=device, k=k, variant=variant, train_class_idx=train_class_idx)
    step.fix_model.load_state_dict(model_state_dict)
    record = step.record = EpochRecord(step)
    stores = None
    if variant == "mia2023":
        stores = step.stores = FeatureStores(step, n_data)
    if getattr(opt, "step_graph", True):
        step.enable_graph()
    resident = _is_resident(train_loader)
    if resident:
        step.loader = train_loader
    n_rows = _rows_of(train_loader, n_data)
    class_of_row = None
    if audit:
        class_of_row = torch.zeros(n_data, dtype=torch.int64)
        for c, rows in enumerate(train_class_idx):
            class_of_row[torch.as_tensor(np.asarray(rows), dtype=torch.int64)] = c
        class_of_row = class_of_row.to(device)

    metric_logger = {"train": {"loss": [], "pvalue": [], "cindex": [], "surv_acc": [], "grad_acc": []},
                     "test": {"loss": [], "pvalue": [], "cindex": [], "surv_acc": [], "grad_acc": []},     # :220-221
                     "epochs": []}
    best_acc, best_metrics = 0.0, None
    avg_all_metrics = np.array([0.0, 0.0, 0.0, 0.0])                                                        # :225-226
    last = opt.niter + opt.niter_decay

    for epoch in range(opt.epoch_count, last + 1):                                                          # :228
        # ---- training part: no host read between reset() and read()
        record.reset()
        if resident:
            for _ in range(n_data // opt.batch_size):
                step.step(None, epoch)
        else:
            for batch in train_loader:
                step.step(batch, epoch)
        step.scheduler.step()                                                                               # :346
        ep = record.read()
        ep["epoch"] = epoch
        metric_logger["epochs"].append(ep)

        plan = epoch_end_plan(opt, epoch, variant)
        if not plan.measure:
            continue
        batches = max(ep["steps"], 1)
        ep["loss_cls_mean"] = ep["loss_cls_epoch"] / batches                                                # :349-351
        ep["loss_div_mean"] = ep["loss_div_epoch"] / batches
        ep["loss_kd_mean"] = ep["loss_kd_epoch"] / batches
        ep["grad_acc_epoch"] = ep["grad_path_epoch"] / n_rows if opt.task == "grad" else None               # :357
        if audit:
            ep["feature_audit"] = evaluate.feature_audit_device(stores.fuse_feat, stores.path_feat, class_of_row)
            ep["logit_audit"] = evaluate.logit_audit_device(stores.fuse_pred, stores.path_pred)
        loader = test_loader_patches if plan.use_patches else test_loader                                   # :360-366
        loss_test, _, _, _, grad_acc_test, all_grad_metrics, _, _, _ = evaluate.test(opt, step.fix_model, step.model, loader,
                                                                                     device)
        ep.update(loss_test=loss_test, grad_acc_test=grad_acc_test, all_grad_metrics=list(all_grad_metrics),
                  used_patches=plan.use_patches)
        if plan.add_to_average:
            avg_all_metrics += np.array(all_grad_metrics)                                                   # :368-369
        if opt.task == "grad" and ep["loss_epoch"] < opt.patience:                                          # :383 (the SUM)
            ep["early_stop"] = True
            break
        if plan.may_save:                                                                                   # :387-402
            avg_metric = np.mean(np.array(all_grad_metrics))
            if avg_metric > best_acc:
                best_metrics, best_acc = all_grad_metrics, avg_metric
                save_path = best_checkpoint_path(opt, k)
                os.makedirs(os.path.dirname(save_path), exist_ok=True)
                torch.save({"split": k, "opt": opt, "epoch": last, "model_state_dict": step.model.state_dict(),
                            "optimizer_state_dict": step.optimizer.state_dict(), "metrics": metric_logger}, save_path)
                ep["saved"] = save_path

    avg_metrics = avg_all_metrics / EPOCH_AVERAGE_OVER                                                      # :404
    if variant == "miccai2022":
        return step.fix_model, step.model, step.optimizer, metric_logger                                    # :406
    if best_metrics is None:
        # v2 :587 | MIA-2023 :537 return a name that only a saved checkpoint binds
        raise UnboundLocalError("local variable 'best_metrics' referenced before assignment (no epoch saved a checkpoint: "
                                "\"MIA 2022/train_test_path_multi_distill_v2.py\":569, :587)")
    return step.fix_model, step.model, step.optimizer, metric_logger, best_metrics, avg_metrics


def train_teacher(opt, train_loader, n_data, test_loader, test_loader_patches, device, k, variant="miccai2022"):
    """The reference's stage-1 train() for `variant` over TeacherStage1Step: MICCAI-2022/train_test_MT.py:
    42-337 | "MIA 2022/train_test_tSVD.py":99-592 | "MIA 2023/stage1_multi_modal_teacher/train_test_MT_SP_Masking.py":105-432.
    `train_loader`: any iterable of the reference's 8-tuples (the MIA-2023 6-view tuple included).  Returns the reference's
    (module_list, model, ema_model, optimizer, metric_logger); metric_logger carries the reference's keys and "epochs": one
    dict per epoch, the `Stage1Record.read()` of its training part plus, on a measured epoch, the means, the accuracies or
    C-indices and the test pass' numbers.  Between record.reset() and record.read() the loop reads the host not at all.
    "miccai2022" and "mia2022" write best_checkpoint_path(opt, k) - the file stage 2 loads through teacher_checkpoint_path -
    with the reference's dict (:297-307 | :542-554, the latter with ema_model_state_dict); "mia2023" only records the path,
    its save being commented out (:389-397).  `step_graph=False` on opt keeps the step eager; masking steps are eager anyway."""
    if variant not in ARITY:
        raise ValueError("variant must be 'miccai2022', 'mia2022' or 'mia2023'")
    tsvd_on, masking = getattr(opt, "tSVD_loss", "False") == "True", bool(getattr(opt, "masking", 0))
    if (tsvd_on and variant != "mia2022") or (masking and variant != "mia2023"):
        raise ValueError("tSVD_loss belongs to variant 'mia2022' and masking to 'mia2023' (got %r)" % (variant,))
    seed = 2019                                                                                   # :44-46 | :100-104 | :107-109
    torch.cuda.manual_seed_all(seed); torch.manual_seed(seed); random.seed(seed)
    opt.n_data = n_data                                                                           # :72 | :126
    step = TeacherStage1Step(opt, device=device, k=k)
    n_rows = _rows_of(train_loader, n_data)
    record = step.record = Stage1Record(step, n_rows)
    if getattr(opt, "step_graph", True):
        step.enable_graph()
    metric_logger = {"train": {"loss": [], "pvalue": [], "cindex": [], "surv_acc": [], "grad_acc": []},
                     "test": {"loss": [], "pvalue": [], "cindex": [], "surv_acc": [], "grad_acc": []},     # :99-100 | :155-156
                     "epochs": []}
    best_acc = 0.0
    last = opt.niter + opt.niter_decay
    onecycle = opt.lr_policy == "onecycle"

    for epoch in range(opt.epoch_count, last + 1):                                                # :104 | :182 | :168
        # ---- training part: no host read between reset() and read()
        record.reset()
        step.start_epoch()
        for batch in train_loader:
            step.step(batch, epoch)
            if onecycle:
                step.scheduler.step()                                                             # :244-245 | :475-476
        if not onecycle:
            step.scheduler.step()                                                                 # :266-267 | :506-507
        ep = record.read()
        ep["epoch"] = epoch
        metric_logger["epochs"].append(ep)

        plan = teacher_epoch_end_plan(opt, epoch, variant)
        if not plan.measure:
            continue
        batches = max(ep["steps"], 1)                                                             # len(train_loader)
        for name in Stage1Record.SCALARS:                                                         # :270-276 | :510-521
            key = name + "_epoch" if name.startswith("loss") else name
            ep[name + "_mean"] = ep[key] / batches
        if opt.task == "grad":                                                                    # :283-285 | :528-530
            for key in ("grad_acc_epoch", "grad_path_epoch", "grad_omic_epoch"):
                ep[key.replace("_epoch", "_train")] = ep[key] / n_rows
        else:                                                                                     # :278-280 | :523-525
            ep["cindex_epoch"], ep["cindex_path"], ep["cindex_omic"] = record.cindex()
        loader = test_loader_patches if plan.use_patches else test_loader                         # :288-289 | :533-534
        res = evaluate.test_teacher(opt, step.model, loader, device)
        names = ("loss_test", "loss_test_fuse", "loss_test_path", "loss_test_omic", "cindex_test", "cindex_test_path",
                 "cindex_test_omic", "pvalue_test", "surv_acc_test", "grad_acc_test", "grad_path_test", "grad_omic_test")
        ep.update(dict(zip(names, res[:12])), used_patches=plan.use_patches)
        grad_acc_test = res[4] if opt.task == "surv" else res[9]                                  # :294 | :539
        if plan.may_save and grad_acc_test > best_acc:                                            # :295 | :540 | :385
            best_acc = grad_acc_test
            save_path = best_checkpoint_path(opt, k)
            if variant != "mia2023":
                os.makedirs(os.path.dirname(save_path), exist_ok=True)
                ckpt = {"split": k, "opt": opt, "epoch": last, "model_state_dict": step.model.state_dict()}
                if variant == "mia2022":
                    ckpt["ema_model_state_dict"] = step.ema_model.state_dict()                    # :545, :551
                ckpt.update(optimizer_state_dict=step.optimizer.state_dict(), metrics=metric_logger)
                torch.save(ckpt, save_path)
            ep["saved"] = save_path
    return step.module_list, step.model, step.ema_model, step.optimizer, metric_logger

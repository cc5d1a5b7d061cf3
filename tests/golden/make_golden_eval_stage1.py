#!/usr/bin/env python3
"""Golden vectors for the stage-1 evaluation: the reference's own `test()` of MICCAI-2022/train_test_MT.py:340-458 (the
module imported under install_shims(): its lifelines calls come back as stubs), run on the reference's PathomicNet in eval
mode over a three-batch synthetic loader with an uneven last batch, for both tasks.  Recorded: loss_test, the per-branch
losses, surv_acc_test (surv) / the three grading accuracies (grad), and the pred_test / feats_test arrays.  The
lifelines-backed C-index and p-value are stubs and are not recorded.  Build container only.
Writes tests/golden/eval_stage1_b6_h64.npz."""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference/MICCAI-2022"

SIZES = (6, 6, 5)          # uneven last batch
H = 64
# the survival heads of the seeded weights saturate the sigmoid (every risk ~ +3): scaled down so that the risks spread
HEAD_KEYS = ("classifier.0.weight", "path_net.fc_new2.weight", "omic_net.classifier.0.weight")
HEAD_SCALE = 0.02


def state_dict(task):
    from oracle import weights as W
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1 if task == "surv" else 3), 3)
    if task == "surv":
        for k in HEAD_KEYS:
            sd[k] = sd[k] * HEAD_SCALE
    return sd


class Loader(list):
    """The two things test() asks of a DataLoader: iteration / len() over batches, and len(loader.dataset)."""
    dataset = None


def batches():
    """Deterministic loader (tests/test_gpu_survival.py builds the same one): synthetic images / omics, survival times
    with ties, a mix of events and censored rows."""
    from oracle.step import synthetic_batch
    out = Loader()
    for i, B in enumerate(SIZES):
        bt = synthetic_batch(B, H, seed=600 + i)
        g = torch.Generator().manual_seed(610 + i)
        censor = (torch.rand(B, generator=g) > 0.35).float()
        survtime = torch.randint(1, 12, (B,), generator=g).float()
        out.append((bt["x_path"], torch.zeros(B), bt["x_omic"], censor, survtime, bt["grade"]))
    out.dataset = range(sum(SIZES))
    return out


def run(task, rec):
    from make_golden import ref_opt
    extra = ["--task", "surv", "--act_type", "Sigmoid", "--label_dim", "1"] if task == "surv" else []
    opt = ref_opt(tempfile.mkdtemp(), extra=extra + ["--lambda_reg", "3e-4", "--reg_type", "omic"])
    opt.cut_fuse_grad = False
    with contextlib.redirect_stdout(io.StringIO()):
        import networks_new as NN
        import train_test_MT as T
        model = NN.define_net(opt, 1)
    model.load_state_dict(state_dict(task))
    model.__dict__["module"] = model     # define_reg unwraps DataParallel (`model.module`); on the CPU there is no wrapper
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        res = T.test(opt, torch.nn.ModuleList([model]), model, batches(), torch.device("cpu"))
    (loss_test, loss_fuse, loss_path, loss_omic, _cidx, _cpath, _comic, _pval, surv_acc, grad_acc, grad_path, grad_omic,
     metrics, pred_test, grads_test, feats_test) = res
    p = task + "_"
    rec.update({p + "loss_test": loss_test, p + "loss_fuse_test": loss_fuse, p + "loss_path_test": loss_path,
                p + "loss_omic_test": loss_omic, p + "lambda_reg": opt.lambda_reg, p + "lambda_cox": opt.lambda_cox,
                p + "lambda_nll": opt.lambda_nll, p + "feat_fuse_all": feats_test[0], p + "feat_path_all": feats_test[1],
                p + "feat_omic_all": feats_test[2], p + "gt_all": feats_test[3]})
    if task == "surv":
        rec.update({p + "surv_acc_test": surv_acc, p + "risk_pred_all": pred_test[0], p + "risk_path_all": pred_test[1],
                    p + "risk_omic_all": pred_test[2], p + "survtime_all": pred_test[3], p + "censor_all": pred_test[4]})
    else:
        rec.update({p + "grad_acc_test": grad_acc, p + "grad_path_test": grad_path, p + "grad_omic_test": grad_omic,
                    p + "metrics": np.asarray(metrics, dtype=np.float64), p + "probs_all": pred_test[5],
                    p + "probs_path": pred_test[6], p + "probs_omic": pred_test[7]})
    print(task, "loss_test", loss_test, "branches", loss_fuse, loss_path, loss_omic, "surv_acc", surv_acc, "grad_acc", grad_acc)


def main():
    from make_golden import install_shims, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    rec = dict(sizes=np.array(SIZES), H=H, weight_seed=3, head_scale=HEAD_SCALE)
    run("surv", rec)
    run("grad", rec)
    np.savez_compressed(os.path.join(HERE, "eval_stage1_b6_h64.npz"), **npz(rec))
    print("wrote eval_stage1_b6_h64.npz")


if __name__ == "__main__":
    main()

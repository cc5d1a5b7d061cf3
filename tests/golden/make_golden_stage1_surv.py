#!/usr/bin/env python3
"""Golden vectors for the stage-1 mean-teacher batch body under the survival task (--task surv --act_type Sigmoid
--label_dim 1), produced by running the reference's own modules (MICCAI-2022: networks_new.define_net / define_optimizer,
utils.CoxLoss, CL_utils.KD_losses.pred_KD_loss with opt.task "surv", CL_utils.CRD_criterion.CRDLoss,
CL_utils.orthogonal_loss.OrthLoss, train_test_MT.update_ema_variables) in the order of train_test_MT.py:121-230 for two
steps, B = 8, dropout 0.  Two option sets: (a) num_teachers 2, pred_distill on; (b) num_teachers 3 + CRD_distill 1 +
orth_loss True.  The student starts with output_range / output_shift 5 / -2.5, the EMA copy with 6 / -3, so the head reads
the parameters and the EMA update moves them.  Build container only.  Writes tests/golden/stage1_surv_b8_h64.npz."""
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

B, H = 8, 64
SURVTIME = [3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 4.0]      # ties at 1 and 4
CENSOR = [1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]
RANGE, SHIFT = 5.0, -2.5


def run(tag, extra, num_teachers, crd_orth, rec):
    from make_golden import ref_opt
    from make_golden_stage1_terms import embed2_state
    from oracle import weights as W
    from oracle.step import synthetic_batch
    from oracle.variants import CRDv3State
    opt = ref_opt(tempfile.mkdtemp(), extra=["--task", "surv", "--act_type", "Sigmoid", "--label_dim", "1"] + extra)
    opt.cut_fuse_grad = False          # the stage-1 trainer lets the fused loss train both encoders
    opt.num_teachers = num_teachers
    opt.pred_distill = 1
    with contextlib.redirect_stdout(io.StringIO()):
        import networks_new as NN
        from utils import CoxLoss
        from CL_utils.KD_losses import pred_KD_loss
        from CL_utils.CRD_criterion import CRDLoss
        from CL_utils.orthogonal_loss import OrthLoss
        model = NN.define_net(opt, 1)
        ema = NN.define_net(opt, 1)
        crds = [CRDLoss(opt) for _ in range(3)] if crd_orth else []       # path, omic, fuse (train_test_MT.py:74-76)
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    ema.load_state_dict(sd)
    sd["output_range"] = torch.tensor([RANGE]); sd["output_shift"] = torch.tensor([SHIFT])
    model.load_state_dict(sd)
    for p in ema.parameters():
        p.detach_()
    ml = torch.nn.ModuleList([model])
    for i, c in enumerate(crds):
        c.embed_s.load_state_dict(embed2_state(90 + 2 * i)); c.embed_t.load_state_dict(embed2_state(91 + 2 * i))
        st = CRDv3State(opt.n_data, K=opt.nce_k, seed=100 + i)
        c.contrast.memory_v1.copy_(st.memory_v1); c.contrast.memory_v2.copy_(st.memory_v2)
        ml.append(c.embed_s); ml.append(c.embed_t)                                       # :84-90
    optimizer = NN.define_optimizer(opt, ml if crd_orth else model)
    orth = OrthLoss()
    ml.train(); ema.train()

    def update_ema_variables(model, ema_model, alpha, global_step):     # train_test_MT.py:34-38
        alpha = min(1 - 1 / (global_step + 1), alpha)
        for ema_param, param in zip(ema_model.parameters(), model.parameters()):
            ema_param.data.mul_(alpha).add_(param.data, alpha=1 - alpha)

    def kd(p_s, p_t):
        return pred_KD_loss(opt, p_s, p_t)

    survtime, censor = torch.tensor(SURVTIME), torch.tensor(CENSOR)
    rec.update({f"{tag}_num_teachers": num_teachers, f"{tag}_crd_orth": int(crd_orth), f"{tag}_KD_weight": opt.KD_weight,
                f"{tag}_lambda_cox": opt.lambda_cox, f"{tag}_CRD_weight": opt.CRD_weight, f"{tag}_K": opt.nce_k,
                f"{tag}_n_data": opt.n_data, f"{tag}_lr": opt.lr, f"{tag}_weight_decay": opt.weight_decay,
                f"{tag}_ema_decay": opt.ema_decay})
    iter_num = 0
    for it in range(2):
        bt = synthetic_batch(B, H, n_data=opt.n_data, P=1, K=opt.nce_k, seed=70 + it)
        out = model(x_path=bt["x_path"], x_omic=bt["x_omic"])
        fuse_feat, path_feat, omic_feat, pred, pred_path, pred_omic = out[0], out[1], out[2], out[5], out[6], out[7]
        with torch.no_grad():
            eo = ema(x_path=bt["ema_x_path"], x_omic=bt["x_omic"])
        ema_fuse_feat, ema_pred, ema_pred_path, ema_pred_omic = eo[0], eo[5], eo[6], eo[7]
        cox_path = CoxLoss(survtime, censor, pred_path, "cpu")                          # :149-152
        cox_omic = CoxLoss(survtime, censor, pred_omic, "cpu")
        cox_fuse = CoxLoss(survtime, censor, pred, "cpu")
        loss_cox = cox_path + cox_omic + cox_fuse
        loss_CRD = 0.0
        if crd_orth:
            with contextlib.redirect_stdout(io.StringIO()):
                loss_CRD = opt.CRD_weight * crds[2](fuse_feat, ema_fuse_feat.detach(), bt["index"], bt["sample_idx"])
        kd_fuse = kd(pred, ema_pred)                                                     # :180-201
        if num_teachers == 2:
            kd_path = (kd(pred_path, ema_pred_path) + kd(pred_path, ema_pred)) / 2.0
            kd_omic = (kd(pred_omic, ema_pred_omic) + kd(pred_omic, ema_pred)) / 2.0
        else:
            kd_path = (kd(pred_path, ema_pred_path) + kd(pred_path, ema_pred) + kd(pred_path, ema_pred_omic)) / 3.0
            kd_omic = (kd(pred_omic, ema_pred_omic) + kd(pred_omic, ema_pred) + kd(pred_omic, ema_pred_path)) / 3.0
        loss_kd = opt.KD_weight * (kd_fuse + kd_path + kd_omic)
        loss = opt.lambda_cox * loss_cox + loss_CRD + loss_kd                              # :214-215 (reg_type none)
        loss_orth = torch.zeros(())
        if crd_orth:
            loss_orth = orth(path_feat, omic_feat)
            loss = loss + loss_orth
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        update_ema_variables(model, ema, opt.ema_decay, iter_num)
        iter_num += 1
        rec.update({f"{tag}_loss{it}": loss, f"{tag}_loss_cox{it}": loss_cox, f"{tag}_loss_cox_fuse{it}": cox_fuse,
                    f"{tag}_loss_cox_path{it}": cox_path, f"{tag}_loss_cox_omic{it}": cox_omic,
                    f"{tag}_loss_kd{it}": loss_kd, f"{tag}_kd_fuse{it}": kd_fuse, f"{tag}_kd_path{it}": kd_path,
                    f"{tag}_kd_omic{it}": kd_omic, f"{tag}_loss_CRD{it}": loss_CRD, f"{tag}_loss_orth{it}": loss_orth,
                    f"{tag}_pred{it}": pred, f"{tag}_pred_path{it}": pred_path, f"{tag}_pred_omic{it}": pred_omic})
        if it == 0:
            msd, esd = model.state_dict(), ema.state_dict()
            for k in ("omic_net.encoder.0.0.weight", "omic_net.classifier.0.weight", "fusion.linear_h1.0.weight",
                      "fusion.encoder2.0.weight", "classifier.0.weight", "path_net.fc_new2.weight",
                      "path_net.layer3.0.downsample.1.weight"):
                rec[f"{tag}_w0_{k}"] = msd[k].clone()
    esd = ema.state_dict()
    for k in ("output_range", "output_shift", "omic_net.output_range", "omic_net.output_shift", "path_net.output_range",
              "path_net.output_shift"):
        rec[f"{tag}_ema_{k}"] = esd[k].clone()
    print(tag, [round(float(rec[f"{tag}_loss{i}"]), 5) for i in range(2)])


def main():
    from make_golden import install_shims, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    rec = dict(B=B, H=H, weight_seed=3, survtime=np.array(SURVTIME, np.float32), censor=np.array(CENSOR, np.float32),
               output_range=RANGE, output_shift=SHIFT)
    run("a", [], 2, False, rec)
    run("b", ["--nce_k", "512", "--orth_loss", "True", "--CRD_distill", "1", "--n_data", "1024"], 3, True, rec)
    np.savez_compressed(os.path.join(HERE, "stage1_surv_b8_h64.npz"), **npz(rec))
    print("wrote stage1_surv_b8_h64.npz")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of the two batch bodies at feature width 64, produced by running the reference's own modules on the CPU (build
container only; shims and seeded weight recipes of make_golden.py / oracle.weights at path_dim = omic_dim = mmhid = 64):

  distill   MICCAI-2022 stage 2 (train_test_path_multi_distill.py:249-330, the calls of make_golden.py part iii) with
            --path_dim 64 --omic_dim 64 --mmhid 64 --s_dim 64 --t_dim 64 --feat_dim 64, B = 4, 64 x 64, n_data = 1024: the six loss
            terms, `scale`, the logits, Z and the updated bank rows after step 1, and the `mid` rank lists the reference drew.
  stage1    the stage-1 mean-teacher body (train_test_MT.py:121-230, as in make_golden_stage1.py) at the options of
            "MIA 2022/train.sh":15-17: --pred_distill 0 --CRD_distill 0 --tSVD_loss False --init_type max --beta1 0.5
            --fusion_type pofusion --path_dim 64 --omic_dim 64 --mmhid 64; B = 4, 64 x 64: losses and predictions of step 1,
            a few Adam-updated weights and their EMA copies.

Usage:  python tests/golden/make_golden_step_width.py        # writes tests/golden/step_dim64_b4_h64.npz
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference/MICCAI-2022"
DIMS = ["--path_dim", "64", "--omic_dim", "64", "--mmhid", "64"]


def main():
    from make_golden import install_shims, ref_opt, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    from oracle import weights as W
    from oracle.losses import CRDState
    from oracle.step import synthetic_batch
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    B, H, n_data, D = 4, 64, 1024, 64
    rec = dict(B=B, H=H, n_data=n_data, dim=D, seed=0)

    # ---------------------------------------------------------------- stage 2
    opt = ref_opt(tempfile.mkdtemp(), extra=DIMS + ["--s_dim", "64", "--t_dim", "64", "--feat_dim", "64"])
    with quiet():
        import networks_new as NN
        from CL_utils.CRD_loss import CRDLoss
        from KD_loss import DistillKL
        import train_test_path_multi_distill as TT
        student = NN.define_net(opt, 1, path_only=True)
        ema = NN.define_net(opt, 1, path_only=True)
        teacher = NN.define_net(opt, 1)
    student.load_state_dict(W.make_state_dict(W.student_shapes(D), 1))
    ema.load_state_dict(W.make_state_dict(W.student_shapes(D), 2))
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320, D, D, D), 3))
    for p in ema.parameters():
        p.detach_()
    for p in teacher.parameters():
        p.detach_(); p.requires_grad = False
    student.train(); teacher.train()
    kl = DistillKL(opt.kd_T)
    _choice = np.random.choice

    def make_crds():
        crds = []
        for i in range(2):
            torch.manual_seed(20 + i)
            with quiet():
                c = CRDLoss(opt, n_data)
            c.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(D, D), 10 + 2 * i))
            c.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(D, D), 11 + 2 * i))
            sti = CRDState(n_data, D, opt.nce_p, opt.nce_k, seed=20 + i)
            assert tuple(sti.memory_v1.shape) == (n_data, D)
            c.contrast.memory_v1.copy_(sti.memory_v1); c.contrast.memory_v2.copy_(sti.memory_v2)
            crds.append(c)
        return crds

    def crd_terms(crds, feats, bt, ranks_all):
        def rec_choice(*a, **k):
            r = _choice(*a, **k); ranks_all.append(np.asarray(r)); return r
        np.random.choice = rec_choice
        np.random.seed(2019)
        try:
            with quiet():
                k1 = crds[0](0.0, feats[0], feats[1].detach(), bt["index"], bt["sample_idx"])
                k2 = crds[1](0.0, feats[0], feats[2].detach(), bt["index"], bt["sample_idx"])
        finally:
            np.random.choice = _choice
        return k1, k2

    # The pair selection of ContrastMemory_v3 is a ranking of score differences over 1000 columns whose scores exp(. / 0.07) span
    # orders of magnitude: when two columns of very different score lie within the features' rounding of each other in that
    # ranking, the reference itself moves by 1e-3 .. 1e-2 in the CRD terms and Z when its features move by 2e-4 (measured here on
    # forty batches), and such a batch has no golden value at the step test's 1e-3.  The batch seed is the first whose CRD terms and
    # Z stay within 2e-4 relative (a fifth of that tolerance) under three draws of a perturbation OF THE REFERENCE's features of
    # standard deviation 5e-5 - the size by which two float32 evaluations of these features differ (largest element ~1.7e-4).
    for batch_seed in range(100, 260):
        bt = synthetic_batch(B, H, seed=batch_seed)
        with torch.no_grad():
            feats = (student(x_path=bt["x_path"])[1], teacher(x_path=bt["x_path"], x_omic=bt["x_omic"])[0], ema(x_path=bt["ema_x_path"])[1])
        base = make_crds()
        k0 = [float(v) for v in crd_terms(base, feats, bt, [])] + [float(c.contrast.params[j]) for c in base for j in (2, 3)]
        worst = 0.0
        for draw in range(3):
            gq = torch.Generator().manual_seed(1000 + draw)
            noisy = [f + 5e-5 * torch.randn(f.shape, generator=gq) for f in feats]
            cq = make_crds()
            kq = [float(v) for v in crd_terms(cq, noisy, bt, [])] + [float(c.contrast.params[j]) for c in cq for j in (2, 3)]
            worst = max(worst, max(abs(x - y) / abs(x) for x, y in zip(k0, kq)))
        print("batch seed", batch_seed, "relative change of the CRD terms / Z under a 5e-5 feature perturbation: %.2e" % worst)
        if worst <= 2e-4:
            break
    else:
        raise SystemExit("no stable batch seed")
    # (the running statistics moved in the search; reload so that the golden step is the first on the seeded state)
    student.load_state_dict(W.make_state_dict(W.student_shapes(D), 1))
    ema.load_state_dict(W.make_state_dict(W.student_shapes(D), 2))
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320, D, D, D), 3))
    for p in ema.parameters():
        p.detach_()
    for p in teacher.parameters():
        p.detach_(); p.requires_grad = False
    rec["d_batch_seed"] = batch_seed
    crds = make_crds()
    ml = torch.nn.ModuleList([student, crds[0].embed_s, crds[0].embed_t, crds[1].embed_s, crds[1].embed_t])
    optimizer = NN.define_optimizer(opt, ml)
    ranks_all = []
    _, path_feat, logit_path, pred_path, _ = student(x_path=bt["x_path"])
    with torch.no_grad():
        _, ema_path_feat, ema_logit_path, _, _ = ema(x_path=bt["ema_x_path"])
        fuse_feat, _, _, _, logits, pred, _, _, _, _, _ = teacher(x_path=bt["x_path"], x_omic=bt["x_omic"])
    assert tuple(path_feat.shape) == (B, D) and tuple(fuse_feat.shape) == (B, D)
    loss_cls = F.nll_loss(pred_path, bt["grade"])
    loss_div1 = kl(logit_path, logits[-1].detach())
    loss_div2 = kl(logit_path, ema_logit_path.detach())
    loss_kd1, loss_kd2 = crd_terms(crds, (path_feat, fuse_feat, ema_path_feat), bt, ranks_all)
    kd_list = [opt.alpha * loss_div1, opt.alpha * loss_div2, opt.beta * loss_kd1, opt.beta * loss_kd2]
    scale, loss_KD = TT.AEKD_loss(opt, optimizer, loss_cls, path_feat, kd_list)
    loss = opt.lambda_nll * loss_cls + loss_KD
    optimizer.zero_grad()
    loss.backward()
    rec.update(d_logit_path=logit_path, d_path_feat=path_feat, d_ema_logit=ema_logit_path, d_fuse_logit=logits[-1], d_loss_cls=loss_cls,
               d_loss_div1=loss_div1, d_loss_div2=loss_div2, d_loss_kd1=loss_kd1, d_loss_kd2=loss_kd2, d_scale=scale, d_loss_KD=loss_KD,
               d_loss=loss, d_beta=opt.beta, d_ranks=np.stack(ranks_all), d_g_fc2_w=student.fc_new2.weight.grad.clone(),
               d_g_embed_s0=crds[0].embed_s.linear.weight.grad.clone(), d_g_embed_t1=crds[1].embed_t.linear.weight.grad.clone(),
               d_params0=crds[0].contrast.params.clone(), d_params1=crds[1].contrast.params.clone(),
               d_bank0_v1_rows=crds[0].contrast.memory_v1[bt["index"]].clone(),
               d_bank1_v2_rows=crds[1].contrast.memory_v2[bt["index"]].clone())
    print("distill: loss", float(loss), "scale", scale.tolist())

    # ---------------------------------------------------------------- stage 1, "MIA 2022/train.sh":15-17
    opt = ref_opt(tempfile.mkdtemp(), extra=DIMS + ["--pred_distill", "0", "--CRD_distill", "0", "--tSVD_loss", "False", "--mode", "pathomic",
                                                   "--init_type", "max", "--beta1", "0.5", "--fusion_type", "pofusion"])
    opt.cut_fuse_grad = False
    with quiet():
        model = NN.define_net(opt, 1)
        ema = NN.define_net(opt, 1)
    sd0 = W.make_state_dict(W.teacher_shapes(320, D, D, D), 3)
    model.load_state_dict(sd0); ema.load_state_dict(sd0)
    for p in ema.parameters():
        p.detach_()
    optimizer = NN.define_optimizer(opt, model)
    model.train(); ema.train()
    bt = synthetic_batch(B, H, seed=20)
    out = model(x_path=bt["x_path"], x_omic=bt["x_omic"])
    pred, pred_path, pred_omic = out[5], out[6], out[7]
    assert tuple(out[0].shape) == (B, D)
    with torch.no_grad():
        ema(x_path=bt["ema_x_path"], x_omic=bt["x_omic"])
    g = bt["grade"]
    loss_nll = F.nll_loss(pred_path, g) + F.nll_loss(pred_omic, g) + F.nll_loss(pred, g)
    loss = opt.lambda_nll * loss_nll          # pred_distill 0, CRD_distill 0, SP off, reg_type none: train_test_MT.py:212-213
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    for ema_param, param in zip(ema.parameters(), model.parameters()):      # update_ema_variables at global_step 0: alpha = 0
        ema_param.data.mul_(0.0).add_(param.data, alpha=1.0)
    rec.update(s_loss=loss, s_loss_nll=loss_nll, s_pred=pred, s_pred_path=pred_path, s_pred_omic=pred_omic, s_lr=opt.lr,
               s_weight_decay=opt.weight_decay, s_ema_decay=opt.ema_decay, s_beta1=opt.beta1)
    msd, esd = model.state_dict(), ema.state_dict()
    for k in ("omic_net.encoder.0.0.weight", "fusion.linear_h1.0.weight", "fusion.encoder2.0.weight", "classifier.0.weight",
              "path_net.fc_new2.weight"):
        rec["s_w_" + k] = msd[k].clone()
        rec["s_e_" + k] = esd[k].clone()
    np.savez_compressed(os.path.join(HERE, "step_dim64_b4_h64.npz"), **npz(rec))
    print("stage1: loss", float(loss), "-> wrote step_dim64_b4_h64.npz")


if __name__ == "__main__":
    main()

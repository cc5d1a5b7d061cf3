"""The training steps at another feature width: path_dim = omic_dim = mmhid = s_dim = t_dim = 64 (the reference's shipped
`..._dim64` stage-1 command, "MIA 2022/train.sh":15-17) with feat_dim 64 and 256.

  DistillStep, all three variants   the fused loss head (loss_head.py: closed-form gradient rows, ph_gk_rows at width 64) against
                                    the eager composition of the same drop-in modules, in bf16x6, one step from one seeded
                                    initialisation: losses and weights within 1e-5 relative, every parameter gradient within 2e-4,
                                    the updated bank bitwise - the tolerances of the 128-wide tests of tests/test_gpu_step.py.
  DistillStep (miccai2022)          step 1 against the reference's own modules at dims 64 / feat_dim 64, B = 4, 64 x 64
                                    (tests/golden/make_golden_step_width.py -> step_dim64_b4_h64.npz): six loss terms, `scale`,
                                    logits, gradients, Z, bank rows at the tolerances of the 128-wide golden test.
  TeacherStage1Step                 step 1 against the reference at the options of the shipped 64-wide stage-1 command
                                    ("MIA 2022/train.sh":15-17) from the same golden file; and, with the CRD term on at dims 64,
                                    finite losses, the batch's bank rows replaced by unit rows, all other rows untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = dict(path_dim=64, omic_dim=64, mmhid=64, s_dim=64, t_dim=64)


def _tuple(bt):
    B = bt["x_path"].shape[0]
    return ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], torch.zeros(B), torch.zeros(B),
            bt["grade"], bt["index"], bt["sample_idx"])


def _one_step(variant, feat_dim, fused):
    import multimodal_learning_amd as m
    from oracle.step import default_opt, synthetic_batch
    n_data, B = 256, 8
    labels = torch.arange(n_data) % 3
    kw, skw, P, K = {}, {}, 1, 64
    if variant == "miccai2022":
        P, K = 40, 80
        opt = default_opt(nce_p=P, nce_k=K, nce_p2=10, nce_k2=48, select_pos_mode="hard", feat_dim=feat_dim, **DIMS)
    elif variant == "mia2022":
        opt = default_opt(nce_k=K, grads_m=0.9, grads_thresh="True", thresh=0.1, niter_decay=10, feat_dim=feat_dim, **DIMS)
        skw = dict(epoch=3)
    else:
        opt = default_opt(nce_k=K, nce_p=4, pos_extra="neighbors", neg_mode="all_others", start_reweight=0, discrep_scale=1,
                          max_discrep=2.0, use_grads_thresh="True", grads_thresh=0.1, loss_weighting="GK_refine", batch_size=B,
                          feat_dim=feat_dim, **DIMS)
        kw = dict(train_class_idx=[np.nonzero((labels == c).numpy())[0] for c in range(3)])
        skw = dict(epoch=2)
    opt.fused_loss_head = fused
    torch.manual_seed(7)
    if variant == "miccai2022":
        step = m.DistillStep(opt, n_data, device="cuda")
    else:
        step = m.DistillStep(opt, n_data, device="cuda", variant=variant, **kw)
    for crd in (step.criterion_kd, step.criterion_kd_path):
        crd.contrast.verbose = False
        assert crd.contrast.memory_v1.shape == (n_data, feat_dim)
    bt = synthetic_batch(B, 64, n_data=n_data, P=P, K=K, seed=600)
    if variant == "mia2023":
        bt["grade"] = labels[bt["index"]].long()
    out = step.step(_tuple(bt), **skw)
    assert step._fused_head_ok() == fused
    names = [k for k in ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2", "scale", "logit_path") if k in out]
    Pm = dict(step.module_list.named_parameters())
    return dict(out={k: out[k].detach().float().clone() for k in names},
                grads={k: p.grad.detach().clone() for k, p in Pm.items() if p.grad is not None},
                bank=step.criterion_kd.contrast.memory_v1.clone())


@pytest.mark.parametrize("feat_dim", [64, 256])
@pytest.mark.parametrize("variant", ["miccai2022", "mia2022", "mia2023"])
def test_fused_step_equals_eager_composition_at_dims_64(variant, feat_dim):
    import multimodal_learning_amd as m
    m.set_precision("bf16x6")
    try:
        a, b = _one_step(variant, feat_dim, True), _one_step(variant, feat_dim, False)
    finally:
        m.set_precision("bf16")
    assert {"loss", "loss_kd1", "scale"} <= set(a["out"])
    for k in a["out"]:
        assert torch.isfinite(a["out"][k]).all(), k
        d = (a["out"][k].reshape(-1) - b["out"][k].reshape(-1)).abs().max().item()
        assert d <= 1e-5 * max(1.0, b["out"][k].abs().max().item()), (k, d)
    assert set(a["grads"]) == set(b["grads"])
    for k in b["grads"]:
        ga, gb = a["grads"][k], b["grads"][k]
        d = max((ga - gb).abs().max().item() - 1e-6, 0.0) / (gb.abs().max().item() + 1e-12)
        assert d <= 2e-4, (k, d)
    assert torch.equal(a["bank"], b["bank"])


def test_teacher_stage1_step_at_dims_64_with_the_crd_term():
    """The CRD term of the stage-1 body at width 64 (--CRD_distill 1 on the fused features): finite losses, the bank rows of the
    batch replaced by unit rows, every other bank row bitwise untouched, Z set."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    B, n_data, K = 8, 256, 48
    opt = m.stage2_opt(dropout_rate=0.0, batch_size=B, cut_fuse_grad=True, num_teachers=2, nce_k=K, feat_dim=64, n_data=n_data, **DIMS)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 1, 1.0, 1, 0, "False", "False"
    torch.manual_seed(8)
    model, ema = m.define_net(opt, 1), m.define_net(opt, 1)
    st = m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()))
    mem = st.CRD_criterion_fuse.contrast          # the criterion the body runs (train_test_MT.py:163-164)
    mem.verbose = False
    assert mem.memory_v1.shape == (n_data, 64)
    before = [mem.memory_v1.clone(), mem.memory_v2.clone()]
    bt = synthetic_batch(B, 64, n_data=n_data, P=1, K=K, seed=601)
    z = torch.zeros(B)
    out = st.step(((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"]))
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
    idx = bt["index"].cuda()
    others = torch.ones(n_data, dtype=torch.bool, device="cuda")
    others[idx] = False
    for old, new in zip(before, (mem.memory_v1, mem.memory_v2)):
        assert torch.equal(old[others], new[others])
        assert (old[idx] != new[idx]).any(dim=1).all()
        assert (new[idx].norm(dim=1) - 1).abs().max().item() <= 1e-5
    assert bool((mem.params[2:4] > 0).all())


# ------------------------------------------------------------------------------------------------ reference-run goldens
def test_distill_step_vs_reference_golden_at_dims_64(golden_dir):
    """DistillStep (miccai2022) at path_dim = omic_dim = mmhid = s_dim = t_dim = feat_dim = 64, B = 4, 64 x 64, against the
    reference's own modules run on the same seeded weights (tests/golden/make_golden_step_width.py): the six loss terms, `scale`,
    the logits, three gradients, Z and the updated bank rows of step 1, at the step-0 tolerances of
    test_gpu_step.py::test_three_steps_vs_reference_golden."""
    import os
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.losses import CRDState
    from oracle.step import default_opt, synthetic_batch
    from tests.gpu_util import Report
    g = np.load(os.path.join(golden_dir, "step_dim64_b4_h64.npz"))
    D, n_data = int(g["dim"]), int(g["n_data"])
    assert D == 64
    m.set_precision("bf16x6")
    try:
        opt = default_opt(feat_dim=D, **DIMS)
        step = m.DistillStep(opt, n_data, device="cuda")
        step.model.load_state_dict(W.make_state_dict(W.student_shapes(D), 1))
        step.ema_model.load_state_dict(W.make_state_dict(W.student_shapes(D), 2))
        step.fix_model.load_state_dict(W.make_state_dict(W.teacher_shapes(320, D, D, D), 3))
        for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
            crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(D, D), 10 + 2 * i))
            crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(D, D), 11 + 2 * i))
            st = CRDState(n_data, D, opt.nce_p, opt.nce_k, seed=20 + i)
            crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
            crd.contrast.verbose = False
        bt = synthetic_batch(int(g["B"]), int(g["H"]), seed=int(g["d_batch_seed"]))
        out = step.step(_tuple(bt), epoch=0, ranks=[g["d_ranks"][0], g["d_ranks"][1]])
        R = Report("DistillStep at dims 64 vs REFERENCE golden (B = 4, 64 x 64)")
        tol, beta = 1e-3, float(g["d_beta"])
        for key, name in (("d_logit_path", "logit_path"), ("d_ema_logit", "ema_logit"), ("d_fuse_logit", "fuse_logit"),
                          ("d_path_feat", "path_feat"), ("d_loss_cls", "loss_cls"), ("d_loss", "loss"), ("d_loss_div1", "loss_div1"),
                          ("d_loss_div2", "loss_div2"), ("d_scale", "scale")):
            R.close(g[key], out[name], tol, 0, name)
        # (the golden stores the unscaled CRD losses; DistillStep returns the beta-scaled ones)
        R.close(float(g["d_loss_kd1"]) * beta, out["loss_kd1"], tol, 0, "loss_kd1")
        R.close(float(g["d_loss_kd2"]) * beta, out["loss_kd2"], tol, 0, "loss_kd2")
        P = dict(step.model.named_parameters())
        R.close(g["d_g_fc2_w"], P["fc_new2.weight"].grad, 1e-5, 1e-3, "grad fc2")
        R.close(g["d_g_embed_s0"], step.criterion_kd.embed_s.linear.weight.grad, 1e-7, 1e-3, "grad embed_s")
        R.close(g["d_g_embed_t1"], step.criterion_kd_path.embed_t.linear.weight.grad, 1e-7, 1e-3, "grad embed_t")
        idx = bt["index"].cuda()
        R.close(g["d_params0"], step.criterion_kd.contrast.params, 1e-2, 1e-5, "CRD params / Z, bank 0")
        R.close(g["d_params1"], step.criterion_kd_path.contrast.params, 1e-2, 1e-5, "CRD params / Z, bank 1")
        R.close(g["d_bank0_v1_rows"], step.criterion_kd.contrast.memory_v1[idx], 1e-4, 0, "bank0 rows")
        R.close(g["d_bank1_v2_rows"], step.criterion_kd_path.contrast.memory_v2[idx], 1e-4, 0, "bank1 rows")
        R.finish()
    finally:
        m.set_precision("bf16")


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3/x1"])
def test_stage1_teacher_step_vs_reference_golden_at_dims_64(golden_dir, pmode):
    """TeacherStage1Step at the options of the reference's shipped 64-wide stage-1 command ("MIA 2022/train.sh":15-17:
    --pred_distill 0 --CRD_distill 0 --tSVD_loss False --beta1 0.5 --path_dim 64 --omic_dim 64 --mmhid 64), B = 4, 64 x 64, step 1
    against the reference's modules, at the step-0 tolerances of test_gpu_step.py::test_stage1_teacher_step_vs_reference_golden."""
    import os
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch
    g = np.load(os.path.join(golden_dir, "step_dim64_b4_h64.npz"))
    D = int(g["dim"])
    m.set_precision(pmode)
    try:
        opt = m.stage2_opt(dropout_rate=0.0, batch_size=4, cut_fuse_grad=False, num_teachers=2, path_dim=D, omic_dim=D, mmhid=D)
        opt.pred_distill, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 0, 0, 0, "False", "False"
        opt.lr, opt.weight_decay, opt.ema_decay, opt.beta1 = float(g["s_lr"]), float(g["s_weight_decay"]), float(g["s_ema_decay"]), float(g["s_beta1"])
        model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
        sd = W.make_state_dict(W.teacher_shapes(320, D, D, D), 3)
        model.load_state_dict(sd); ema.load_state_dict(sd)
        st = m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()))
        bt = synthetic_batch(4, 64, seed=20)
        z = torch.zeros(4)
        out = st.step(((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"]))
        tol = 1e-3
        for k in ("loss", "loss_nll"):
            assert abs(out[k].item() - float(g["s_" + k])) <= tol * abs(float(g["s_" + k])), (k, out[k].item(), float(g["s_" + k]))
        for k in ("pred", "pred_path", "pred_omic"):
            assert np.abs(out[k].cpu().numpy() - g["s_" + k]).max() <= tol * 10, k
        msd, esd = st.model.state_dict(), st.ema_model.state_dict()
        names = [key[4:] for key in g.files if key.startswith("s_w_")]
        assert len(names) == 5
        for name in names:
            # Adam's first step moves every weight by ~lr * sign(g): compare the update, not the weight
            upd_ref = g["s_w_" + name] - sd[name].numpy()
            upd = msd[name].cpu().numpy() - sd[name].numpy()
            assert float((np.abs(upd - upd_ref) > 0.2 * float(g["s_lr"])).mean()) < 0.02, name
            assert float((np.abs(esd[name].cpu().numpy() - g["s_e_" + name]) > 0.2 * float(g["s_lr"])).mean()) < 0.02, name
            assert np.abs(esd[name].cpu().numpy() - msd[name].cpu().numpy()).max() <= 1e-7, name
    finally:
        m.set_precision("bf16")

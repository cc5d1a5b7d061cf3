"""The DSCD criteria of the MIA-2022 tree (CL_utils/CRD_loss_v2.py: CRDLoss over ContrastMemory_v4, CRDLoss_v2 over
ContrastMemory_mono) on the GPU against tests/golden/dscd_forward.npz - the reference classes run on the CPU by
tests/golden/make_golden_dscd.py - at the bounds tests/test_gpu_losses.py uses for the v3 criterion (test_crd_loss_golden: loss
1e-4 + 1e-5 |ref|, gradients 1e-6 + 1e-3 |ref|, Z 1e-2 + 1e-4 |ref|, bank rows 1e-6); the selected columns must be EQUAL."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["v4_rw_hard", "v4_plain_hard", "v4_rw_mid", "mono_hard", "v4_rw_hard_d64", "mono_hard_d256"]


def _opt(g, name, **kw):
    from oracle.step import default_opt
    D, P, P2, K = (int(v) for v in g[name + ".dims"])
    mono = str(g[name + ".crit"]) == "CRDLoss_v2"
    o = dict(nce_p=P, nce_p2=P2, nce_k=K, nce_k2=K, nce_t=0.07, nce_m=0.5, feat_dim=D, s_dim=int(g["s_dim"]),
             t_dim=D if mono else int(g["s_dim"]), select_pos_pairs=True, select_neg_pairs="False",
             neg_reweight=str(g[name + ".neg_reweight"]), sample_KD="False", select_pos_mode=str(g[name + ".mode"]))
    o.update(kw)
    return default_opt(**o), mono


def _criterion(g, name):
    from multimodal_learning_amd.CL_utils import CRD_loss_v2 as M
    from oracle import weights as W
    from oracle.losses import CRDState
    opt, mono = _opt(g, name)
    crd = getattr(M, str(g[name + ".crit"]))(opt, int(g["n_data"]))
    crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(opt.s_dim, opt.feat_dim), 10))
    if not mono:
        crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(opt.s_dim, opt.feat_dim), 11))
    st = CRDState(int(g["n_data"]), feat_dim=opt.feat_dim, seed=int(g["bank_seed"]))
    crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
    crd = crd.cuda()
    crd.contrast.verbose = False
    return crd, mono


@pytest.mark.parametrize("name", CASES)
def test_dscd_criteria_vs_reference_golden(golden_dir, name):
    """Two consecutive calls: Z is set on the first and frozen on the second; the banks are momentum-updated in between."""
    from tests.gpu_util import assert_close
    g = np.load(os.path.join(golden_dir, "dscd_forward.npz"))
    crd, mono = _criterion(g, name)
    sd = ["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in crd.state_dict().items()]
    assert sd == list(g[name + ".state_dict"])
    D, P, P2, K = (int(v) for v in g[name + ".dims"])
    for it in range(2):
        f_s = torch.as_tensor(g["%s.f_s%d" % (name, it)]).cuda().requires_grad_(True)
        f_t = torch.as_tensor(g["%s.f_t%d" % (name, it)]).cuda()
        y = torch.as_tensor(g["%s.index%d" % (name, it)]).cuda()
        ranks = g[name + ".ranks"][it] if str(g[name + ".mode"]) == "mid" else None
        loss = crd(0.1, f_s, f_t, y, torch.as_tensor(g["%s.sidx%d" % (name, it)]).cuda(), ranks=ranks)
        assert loss.dim() == 0
        ps = [crd.embed_s.linear.weight, crd.embed_s.linear.bias] + ([] if mono else [crd.embed_t.linear.weight])
        gs = torch.autograd.grad(loss, [f_s] + ps)
        last = crd.contrast.last
        assert tuple(last["sel"].shape) == (f_s.shape[0], P2 + K)
        assert np.array_equal(last["sel"][:, :P2].cpu().numpy(), g["%s.sel%d" % (name, it)]), "selected columns, call %d" % it
        assert np.array_equal(last["sel"][:, P2:].cpu().numpy(), np.tile(P + np.arange(K, dtype=np.int32), (f_s.shape[0], 1)))
        assert_close(g["%s.loss%d" % (name, it)], loss, 1e-4, 1e-5, "loss")
        assert_close(g["%s.g_fs%d" % (name, it)], gs[0], 1e-6, 1e-3, "d f_s")
        assert_close(g["%s.g_ws%d" % (name, it)], gs[1], 1e-6, 1e-3, "d W_s")
        assert_close(g["%s.g_bs%d" % (name, it)], gs[2], 1e-6, 1e-3, "d b_s")
        if not mono:
            assert_close(g["%s.g_wt%d" % (name, it)], gs[3], 1e-6, 1e-3, "d W_t")
        assert_close(g["%s.params%d" % (name, it)], crd.contrast.params, 1e-2, 1e-4, "params (Z)")
        assert_close(g["%s.bank_v1_rows%d" % (name, it)], crd.contrast.memory_v1[y], 1e-6, 0, "bank v1 rows")
        assert_close(g["%s.bank_v2_rows%d" % (name, it)], crd.contrast.memory_v2[y], 1e-6, 0, "bank v2 rows")
    if mono:
        assert crd.memory_t is crd.contrast.memory_v1 and crd.contrast.params.numel() == 5


@pytest.mark.parametrize("name", ["v4_rw_hard_d64", "mono_hard_d256"])
def test_dscd_bank_forward_returns_the_reference_tensors(golden_dir, name):
    """A direct call of a bank's forward goes through the outputs path: the reference's tuple ((out_v1, out_v2) for v4, (out_v2,
    memory_v1) for mono), and ContrastLoss_v2 on it gives the criterion's loss and, through autograd, its gradient."""
    from multimodal_learning_amd.CL_utils.CRD_loss_v2 import ContrastLoss_v2
    from tests.gpu_util import assert_close
    g = np.load(os.path.join(golden_dir, "dscd_forward.npz"))
    crd, mono = _criterion(g, name)
    D, P, P2, K = (int(v) for v in g[name + ".dims"])
    f_s = torch.as_tensor(g[name + ".f_s0"]).cuda().requires_grad_(True)
    f_t = torch.as_tensor(g[name + ".f_t0"]).cuda()
    y, idx = torch.as_tensor(g[name + ".index0"]).cuda(), torch.as_tensor(g[name + ".sidx0"]).cuda()
    crit = ContrastLoss_v2(int(g["n_data"]), "False")
    if mono:
        out, mem_t = crd.contrast(0.1, crd.l2norm(f_t), crd.embed_s(f_s), y, idx, "hard")
        assert mem_t is crd.contrast.memory_v1 and tuple(out.shape) == (f_s.shape[0], P2 + K, 1)
        loss = crit(out, P2)
    else:
        o1, o2 = crd.contrast(0.1, crd.embed_s(f_s), crd.embed_t(f_t), y, idx, "hard")
        assert tuple(o1.shape) == tuple(o2.shape) == (f_s.shape[0], P2 + K, 1)
        loss = crit(o1, P2) + crit(o2, P2)
    (gf,) = torch.autograd.grad(loss, [f_s])
    assert_close(g[name + ".loss0"], loss, 1e-4, 1e-5, "loss through the outputs path")
    assert_close(g[name + ".g_fs0"], gf, 1e-6, 1e-3, "d f_s through the outputs path")
    assert_close(g[name + ".params0"], crd.contrast.params, 1e-2, 1e-4, "params (Z)")


def test_dscd_construction_and_call_errors(golden_dir):
    from multimodal_learning_amd.CL_utils import CRD_loss_v2 as M
    from multimodal_learning_amd.CL_utils.memory_new import ContrastMemory_v4, ContrastMemory_mono
    g = np.load(os.path.join(golden_dir, "dscd_forward.npz"))
    with pytest.raises(UnboundLocalError, match="out_v2_pos"):
        ContrastMemory_v4(128, 64, 12, 40, select_pos_pairs=False, neg_reweight="True")
    for rw in (True, False, "true", None):
        with pytest.raises(UnboundLocalError, match="out_v2_neg"):
            ContrastMemory_v4(128, 64, 12, 40, neg_reweight=rw)
    ContrastMemory_mono(128, 64, 12, 40, neg_reweight=True)            # stored and unused there
    for crit in ("CRDLoss", "CRDLoss_v2"):
        with pytest.raises(ValueError, match="feat_dim"):
            getattr(M, crit)(_opt(g, "mono_hard", feat_dim=96, t_dim=96)[0], 64)
    with pytest.raises(ValueError, match="t_dim"):
        M.CRDLoss_v2(_opt(g, "mono_hard", t_dim=64)[0], 64)
    # a rank at or above P, and an index tensor of the K + 1 width the v3 criterion takes
    crd, _ = _criterion(g, "v4_rw_hard_d64")
    f_s, f_t = torch.as_tensor(g["v4_rw_hard_d64.f_s0"]).cuda(), torch.as_tensor(g["v4_rw_hard_d64.f_t0"]).cuda()
    y, idx = torch.as_tensor(g["v4_rw_hard_d64.index0"]).cuda(), torch.as_tensor(g["v4_rw_hard_d64.sidx0"]).cuda()
    with pytest.raises(RuntimeError):
        crd(0.1, f_s, f_t, y, idx, ranks=np.array([0, 3, 12, 1]))
    with pytest.raises(RuntimeError, match="nce_p"):
        crd(0.1, f_s, f_t, y, idx[:, :41].contiguous())
    crd.select_pos_mode = "mid"                                         # `mid` draws ranks 30 .. 99: needs nce_p > the largest
    with pytest.raises(RuntimeError):
        crd(0.1, f_s, f_t, y, idx)
    crd.select_pos_mode = "hard"
    loss = crd(0.1, f_s, f_t, y, None)                                  # contrast_idx = None: drawn on the device
    assert loss.dim() == 0 and bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------ DistillStep(variant="mia2022")
def _tuple(bt):
    B = bt["x_path"].shape[0]
    z = torch.zeros(B)
    return ((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"])


def _columns(index, n_data, width, seed):
    """[B, width] bank rows, column 0 = index, no row twice within a sample (distinct columns: no ties between equal rows)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(index.shape[0]):
        perm = torch.randperm(n_data, generator=g)
        rows.append(torch.cat([index[b:b + 1], perm[perm != index[b]][:width - 1]]))
    return torch.stack(rows)


def _dscd_opt(crit="dscd", **kw):
    from oracle.step import default_opt
    o = dict(crd_criterion=crit, nce_p=100, nce_p2=20, nce_k=512, nce_k2=512, neg_reweight="True", select_pos_mode="hard",
             grads_m=0.9, grads_thresh="False", thresh=0.1, niter_decay=10, batch_size=8)
    o.update(kw)
    return default_opt(**o)


def _dscd_step(opt, n_data, sync=None):
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.losses import CRDState
    step = m.DistillStep(opt, n_data, device="cuda", variant="mia2022", sync=sync)
    step.model.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    step.ema_model.load_state_dict(W.make_state_dict(W.student_shapes(), 2))
    step.fix_model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
        crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 10 + 2 * i))
        if hasattr(crd, "embed_t"):
            crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 11 + 2 * i))
        st = CRDState(n_data, seed=20 + i)
        crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
        crd.contrast.verbose = False
    return step


def _dscd_batch(B, H, n_data, opt, seed):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, H, n_data=n_data, P=opt.nce_p, K=opt.nce_k, seed=seed)
    bt["sample_idx"] = _columns(bt["index"], n_data, opt.nce_p + opt.nce_k, 7000 + seed)
    return bt


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3/x1"])
def test_dscd_step_vs_reference_golden(golden_dir, pmode):
    """DistillStep(variant="mia2022", crd_criterion="dscd") = the batch body of "MIA 2022/train_test_path_multi_distill_v2.py"
    :397-507 over CRD_loss_v2.CRDLoss (neg_reweight True, hard, nce_p 100, nce_p2 20, nce_k 512) against vectors produced by
    running the reference's own modules (tests/golden/make_golden_dscd_step.py), by the comparison rule of
    test_mia2022_variant_steps_vs_reference_golden: step 0 at 1e-3; steps 1-2 |HIP - fp64 run| <= 6 x |reference fp32 - fp64
    run| + noise scale + 1e-3.  At step 0 (identical weights on both sides) the selected positives are EQUAL."""
    import multimodal_learning_amd as m
    from tests.gpu_util import Report, maxerr
    g = np.load(os.path.join(golden_dir, "dscd_step_b8_h64.npz"))
    t64 = np.load(os.path.join(golden_dir, "dscd_step_b8_h64_fp64.npz"))
    B, H, n_data = int(g["B"]), int(g["H"]), int(g["n_data"])
    opt = _dscd_opt(nce_p=int(g["P"]), nce_p2=int(g["P2"]), nce_k=int(g["K"]), nce_k2=int(g["K"]), grads_m=float(g["grads_m"]),
                    niter_decay=int(g["niter_decay"]), batch_size=B)
    m.set_precision(pmode)
    try:
        step = _dscd_step(opt, n_data)
        assert step.plan.rank_draws == 2 and step.crd_criterion == "dscd"
        R = Report("3 MIA-2022 DSCD distill steps, parity mode vs REFERENCE golden (B=8, 64x64)")

        def ref_d(key):
            return maxerr(np.asarray(t64[key]), np.asarray(g[key]))[0]

        def floor(key, got, what, extra=0.0, mult=6):
            err, mx = maxerr(np.asarray(t64[key]), got)
            R.rows.append((what + " [vs fp64 truth]", err, mx, mult * ref_d(key) + extra + 1e-3))
        from oracle.step import synthetic_batch
        for it in range(3):
            bt = synthetic_batch(B, H, n_data=n_data, P=opt.nce_p, K=opt.nce_k, seed=300 + it)
            bt["sample_idx"] = torch.as_tensor(g[f"sidx{it}"])
            out = step.step(_tuple(bt), epoch=int(g[f"epoch{it}"]))
            assert float(step._e_dev) == 1.0                       # no epoch weight on the DSCD terms
            sd = step.model.state_dict(); esd = step.ema_model.state_dict()
            idx = bt["index"].cuda()
            names = (("logit_path", "logit_path"), ("path_feat", "path_feat"), ("ema_logit", "ema_logit"),
                     ("loss_cls", "loss_cls"), ("loss_div1_", "loss_div1"), ("loss_div2_", "loss_div2"),
                     ("loss_kd1_", "loss_kd1"), ("loss_kd2_", "loss_kd2"), ("scale", "scale"), ("loss", "loss"))
            R.close(g[f"fuse_logit{it}"], out["fuse_logit"], 1e-3, 0, f"teacher logit step {it}")
            R.close(g[f"params0_{it}"], step.criterion_kd.contrast.params, 1e-2, 1e-5, "ContrastMemory_v4 params / Z")
            if it == 0:
                P2 = opt.nce_p2
                for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
                    assert np.array_equal(crd.contrast.last["sel"][:, :P2].cpu().numpy(), g[f"sel{i}_0"]), "selected positives, criterion %d" % i
                P = dict(step.model.named_parameters())
                R.close(g["g0_fc2_w"], P["fc_new2.weight"].grad, 1e-5, 1e-3, "grad fc2")
                floor("g0_conv1", P["conv1.weight"].grad, "grad conv1", mult=8 if pmode == "fp16x3/x1" else 6)
                R.close(g["g0_embed_s0"], step.criterion_kd.embed_s.linear.weight.grad, 1e-7, 1e-3, "grad embed_s")
                R.close(g["g0_embed_t1"], step.criterion_kd_path.embed_t.linear.weight.grad, 1e-7, 1e-3, "grad embed_t")
                for key, name in names:
                    R.close(g[f"{key}{it}"], out[name], 1e-3, 0, f"{name} step 0")
                R.close(g["p_fc2_0"], sd["fc_new2.weight"], 1e-4, 0, "Adam-updated fc2 step 0")
                R.close(g["ema_fc2_0"], esd["fc_new2.weight"], 1e-4, 0, "EMA fc2 step 0")
                R.close(g["bank0_v1_rows0"], step.criterion_kd.contrast.memory_v1[idx], 1e-4, 0, "bank0 rows step 0")
                R.close(g["bank1_v2_rows0"], step.criterion_kd_path.contrast.memory_v2[idx], 1e-4, 0, "bank1 rows step 0")
            else:
                nz = 6 * max(ref_d(f"logit_path{it}"), ref_d(f"ema_logit{it}"), ref_d(f"path_feat{it}"))
                for key, name in names:
                    floor(f"{key}{it}", out[name], f"{name} step {it}", extra=nz)
                floor(f"bank0_v1_rows{it}", step.criterion_kd.contrast.memory_v1[idx], f"bank0 rows step {it}")
                floor(f"bank1_v2_rows{it}", step.criterion_kd_path.contrast.memory_v2[idx], f"bank1 rows step {it}")
                R.close(g[f"p_fc2_{it}"], sd["fc_new2.weight"], 1.5e-3, 0, f"Adam-updated fc2 step {it}")
                R.close(g[f"ema_fc2_{it}"], esd["fc_new2.weight"], 1.5e-3, 0, f"EMA fc2 step {it}")
        R.finish()
    finally:
        m.set_precision("bf16")


def test_dscd_mono_steps_run_and_compose_the_module_losses():
    """crd_criterion="dscd_mono": no embed_t (the optimiser holds the student and the two embed_s heads), the generic path; three
    finite steps, and the first step's CRD terms are beta x what a CRDLoss_v2 module of the same state (the class pinned against
    the reference above) gives on the step's own student and teacher features."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd.CL_utils.CRD_loss_v2 import CRDLoss_v2
    n_data = 1024
    m.set_precision("bf16x6")
    try:
        opt = _dscd_opt("dscd_mono")
        step = _dscd_step(opt, n_data)
        assert not step._fused_head_ok() and step.plan.rank_draws == 2
        assert not hasattr(step.criterion_kd, "embed_t") and len(step.module_list) == 3
        twins = []
        for crd in (step.criterion_kd, step.criterion_kd_path):
            t = CRDLoss_v2(opt, n_data).cuda()
            t.load_state_dict(crd.state_dict())
            t.contrast.verbose = False
            twins.append(t)
        assert list(step.criterion_kd.state_dict()) == ["embed_s.linear.weight", "embed_s.linear.bias", "contrast.params",
                                                        "contrast.memory_v1", "contrast.memory_v2"]
        for it in range(3):
            bt = _dscd_batch(8, 64, n_data, opt, 40 + it)
            out = step.step(_tuple(bt), epoch=3)
            for k in ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2"):
                assert bool(torch.isfinite(out[k]).all()), (it, k)
            if it == 0:
                idx, sidx = bt["index"].cuda(), bt["sample_idx"].cuda()
                for k, t, tf in (("loss_kd1", twins[0], out["fuse_feat"]), ("loss_kd2", twins[1], out["ema_feat"])):
                    ref = opt.beta * t(0.3, out["path_feat"], tf, idx, sidx).detach()
                    assert abs(float(out[k]) - float(ref)) <= 1e-5 * abs(float(ref)), (k, float(out[k]), float(ref))
                assert torch.equal(twins[0].contrast.memory_v1, step.criterion_kd.contrast.memory_v1)
                assert step.criterion_kd.embed_s.linear.weight.grad is not None
    finally:
        m.set_precision("bf16")


def test_dscd_fused_loss_head_equals_generic_autograd_path():
    """As test_fused_loss_head_equals_generic_autograd_path_mia2022, for crd_criterion="dscd": two consecutive steps."""
    import multimodal_learning_amd as m
    n_data = 1024
    m.set_precision("bf16x6")
    try:
        res = {}
        for fused in (True, False):
            opt = _dscd_opt()
            opt.fused_loss_head = fused
            step = _dscd_step(opt, n_data)
            rec = []
            for it in range(2):
                out = step.step(_tuple(_dscd_batch(8, 64, n_data, opt, 400 + it)), epoch=3 + it)
                if it == 0:
                    assert step._fused_head_ok() == fused
                P = dict(step.module_list.named_parameters())
                rec.append(dict(out={k: out[k].detach().float().clone() for k in ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1",
                                                                               "loss_kd2", "scale", "logit_path")},
                                grads={k: p.grad.detach().clone() for k, p in P.items() if p.grad is not None},
                                mo=step._mo_state.clone(), bank=step.criterion_kd.contrast.memory_v1.clone(),
                                sel=step.criterion_kd_path.contrast.last["sel"].clone()))
            res[fused] = rec
        for it in range(2):
            a, b = res[True][it], res[False][it]
            tol = 1e-5 if it == 0 else 1e-2
            for k in a["out"]:
                d = (a["out"][k] - b["out"][k]).abs().max().item()
                assert d <= tol * max(1.0, b["out"][k].abs().max().item()), (it, k, d)
            assert (a["mo"] - b["mo"]).abs().max().item() <= tol * max(1.0, b["mo"].abs().max().item()), (it, a["mo"], b["mo"])
            if it == 0:
                assert torch.equal(a["bank"], b["bank"]) and torch.equal(a["sel"], b["sel"])
                assert set(a["grads"]) == set(b["grads"])
                for k in b["grads"]:
                    ga, gb = a["grads"][k], b["grads"][k]
                    d = max((ga - gb).abs().max().item() - 1e-6, 0.0) / (gb.abs().max().item() + 1e-12)
                    assert d <= 2e-4, (k, d)
    finally:
        m.set_precision("bf16")


def test_dscd_replayed_steps_equal_eager_steps_and_resume_is_bit_identical():
    """Host-drawn ranks (select_pos_mode "mid") enter the captured graph as inputs: from the same state, three replayed steps
    equal three eager steps bitwise, with the graph path taken; and a checkpoint taken after two steps, loaded into another
    object, continues bit-identically (the numpy RNG behind the rank draws included).  Loading under another criterion raises."""
    import io
    import multimodal_learning_amd as m
    n_data = 1024
    m.set_precision("bf16")
    opt = _dscd_opt(select_pos_mode="mid")
    batches = [{k: v.cuda() for k, v in _dscd_batch(8, 64, n_data, opt, 60 + i % 2).items()} for i in range(5)]
    res = []
    for graph in (False, True):
        np.random.seed(17)
        step = _dscd_step(opt, n_data)
        if graph:
            step.enable_graph()
        losses = []
        for it in range(5):
            out = step.step(_tuple(batches[it]), epoch=1)
            losses.append(torch.stack([out[k].reshape(()) for k in ("loss", "loss_kd1", "loss_kd2")]).clone())
            if it == 1 and not graph:
                buf = io.BytesIO()
                torch.save(step.state_dict(), buf)
        torch.cuda.synchronize()
        if graph:
            assert step._static is not None and step._static["graph"] is not None, "graph path was not taken"
        res.append((torch.stack(losses).cpu(), step.optimizer.flat.flat.clone(), step.criterion_kd.contrast.memory_v1.clone(),
                    step.criterion_kd.contrast.last["call"].ranks.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert res[0][3].min() >= 30 and res[0][3].max() < 100          # the `mid` ranks of ContrastMemory_v4
    # resume
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    assert sd["crd_criterion"] == "dscd"
    np.random.seed(99)
    other = _dscd_step(opt, n_data)
    other.step(_tuple(batches[3]), epoch=1)
    other.load_state_dict(sd)
    for it in range(2, 5):
        out = other.step(_tuple(batches[it]), epoch=1)
        assert torch.equal(torch.stack([out[k].reshape(()) for k in ("loss", "loss_kd1", "loss_kd2")]).cpu(), res[0][0][it]), it
    assert torch.equal(other.optimizer.flat.flat, res[0][1]) and torch.equal(other.criterion_kd.contrast.memory_v1, res[0][2])
    with pytest.raises(ValueError, match="crd_criterion"):
        _dscd_step(_dscd_opt("dscd_mono"), n_data).load_state_dict(sd)


def test_dscd_two_replicas_equal_one_process_on_the_global_batch():
    """The LocalSync harness and the bounds of tests/test_gpu_replicas.py::test_two_replicas_equal_one_process_on_the_global_batch,
    for crd_criterion="dscd": bank-row all-gather and Z all-reduce through the ContrastBank hooks, no new collective."""
    import threading
    import multimodal_learning_amd as m
    from multimodal_learning_amd.dist import shard_batch
    from tests.test_gpu_replicas import LocalGroup, LocalSync, _head_grads
    B, H, n_data = 8, 64, 1024
    m.set_precision("bf16x6")
    try:
        opt = _dscd_opt()
        bt = _dscd_batch(B, H, n_data, opt, 900)
        h = B // 2
        for k in ("x_path", "ema_x_path", "x_omic"):
            bt[k][h:] = bt[k][:h]              # per-shard BatchNorm statistics == whole-batch statistics
        batch = _tuple(bt)
        single = _dscd_step(opt, n_data)
        o1 = single.step(batch, epoch=3)
        torch.cuda.synchronize()
        g1 = _head_grads(single)
        idx = batch[6].cuda()
        crds = lambda s: (s.criterion_kd, s.criterion_kd_path)
        banks1 = [c.contrast.memory_v1[idx].clone() for c in crds(single)] + [c.contrast.memory_v2[idx].clone() for c in crds(single)]
        group = LocalGroup(2)
        reps = [_dscd_step(_dscd_opt(batch_size=B // 2), n_data, sync=LocalSync(group, r)) for r in range(2)]
        outs, errs = [None, None], []

        def run(r):
            try:
                torch.cuda.set_device(0)
                outs[r] = reps[r].step(shard_batch(batch, r, 2), epoch=3)
                torch.cuda.synchronize()
            except BaseException as e:      # noqa: BLE001 - re-raised in the main thread
                errs.append(e)
                group.barrier.abort()
        ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(300)
        if errs:
            raise errs[0]
        f0, f1 = reps[0].optimizer.flat, reps[1].optimizer.flat
        assert torch.equal(f0.grad, f1.grad) and torch.equal(f0.flat, f1.flat)
        for k in ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2"):
            tot, ref = sum(float(o[k]) for o in outs), float(o1[k])
            assert abs(tot - ref) <= 2e-4 * max(abs(ref), 1e-2), (k, tot, ref)
        s1, s2 = o1["scale"].cpu().numpy(), outs[0]["scale"].cpu().numpy()
        assert np.abs(s1 - s2).max() <= 2e-4 * np.abs(s1).max(), (s1, s2)
        g2 = _head_grads(reps[0])
        gmax = max(float(v.abs().max()) for v in g1.values())
        for k, v in g1.items():
            err = float((g2[k] - v).abs().max())
            assert err <= 1e-3 * float(v.abs().max()) + 1e-6 * gmax, (k, err, float(v.abs().max()))
        banks2 = [c.contrast.memory_v1[idx].clone() for c in crds(reps[0])] + [c.contrast.memory_v2[idx].clone() for c in crds(reps[0])]
        for a, b in zip(banks1, banks2):
            assert float((a - b).abs().max()) <= 1e-5
        for c0, c1 in zip(crds(reps[0]), crds(reps[1])):
            assert torch.equal(c0.contrast.memory_v1, c1.contrast.memory_v1) and torch.equal(c0.contrast.params, c1.contrast.params)
    finally:
        m.set_precision("bf16")


def test_dscd_readme_command_shapes_run_one_step():
    """The MIA-2022 README's stage-2 shapes (--nce_p 300 --nce_p2 20 --nce_k 1024, select_pos_mode hard) at B = 4, 64 x 64: the
    [B, nce_p + nce_k] index tensor the v3 criterion refuses; P2 + K >= 1024 takes the split loss kernel."""
    import multimodal_learning_amd as m
    n_data = 2048
    m.set_precision("bf16")
    opt = _dscd_opt(nce_p=300, nce_p2=20, nce_k=1024, nce_k2=1024, neg_reweight="False", batch_size=4)
    step = _dscd_step(opt, n_data)
    bt = _dscd_batch(4, 64, n_data, opt, 5)
    out = step.step(_tuple(bt), epoch=1)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("loss", "loss_kd1", "loss_kd2")) and float(out["loss_kd1"]) > 0
    assert tuple(step.criterion_kd.contrast.last["sel"].shape) == (4, 20 + 1024)
    with pytest.raises(RuntimeError, match="1024"):
        bad = dict(bt, sample_idx=bt["sample_idx"][:, :1025].contiguous())
        step.step(_tuple(bad), epoch=1)
    with pytest.raises(ValueError, match="crd_criterion"):
        m.DistillStep(_dscd_opt("dscd_v9"), 64, device="cuda", variant="mia2022")
    with pytest.raises(ValueError, match="crd_criterion"):
        m.DistillStep(_dscd_opt("dscd"), 64, device="cuda")

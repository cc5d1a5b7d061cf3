"""The drop-in CRD classes at feat_dim 64 and 256 against the reference's own classes run on the CPU
(tests/golden/make_golden_crd_width.py -> tests/golden/crd_width.npz): ContrastMemory_v3 standalone, CRD_loss.CRDLoss, the
stage-1 CRD_criterion.CRDLoss, CRD_criterion_v3.CRDLoss and CRD_criterion_v10.CRDLoss with `neighbors` (the KNN at NG = 2 and 8
through the module).  Two calls each: Z set, then frozen, the second call against the momentum-updated bank.  Tolerances: those of
the 128-wide tests of the same classes (tests/test_gpu_losses.py).  Before the kernels took a width these failed in the first
forward with `RuntimeError: libpathomic_hip: ph_crd_score failed with code -22`."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (64, 256)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "crd_width.npz"))


def bank(n, D, seed):
    gen = torch.Generator().manual_seed(seed)
    stdv = 1.0 / (D / 3) ** 0.5
    return torch.rand(n, D, generator=gen).mul_(2 * stdv).add_(-stdv)


def head(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(*s, generator=gen) * (0.1 if len(s) == 2 else 0.02) for k, s in shapes.items()}


def _load(crd, g, D, seeds, two_layer=False):
    S, n = int(g["s_dim"]), int(g["n_data"])
    shapes = ({"linear.0.weight": (D, S), "linear.0.bias": (D,), "linear.2.weight": (D, D), "linear.2.bias": (D,)} if two_layer
              else {"linear.weight": (D, S), "linear.bias": (D,)})
    crd.embed_s.load_state_dict(head(shapes, seeds[0])); crd.embed_t.load_state_dict(head(shapes, seeds[1]))
    crd.contrast.memory_v1.copy_(bank(n, D, seeds[2])); crd.contrast.memory_v2.copy_(bank(n, D, seeds[3]))
    crd = crd.cuda()
    crd.contrast.verbose = False
    return crd


def _c(g, key):
    return torch.as_tensor(g[key]).cuda()


@pytest.mark.parametrize("D", WIDTHS)
def test_contrast_memory_v3_standalone(g, D):
    from multimodal_learning_amd.CL_utils.memory_new import ContrastMemory_v3
    from tests.gpu_util import Report
    n = int(g["n_data"])
    mem = ContrastMemory_v3(D, n, int(g["P"]), int(g["K"]), 0.07, 0.5, True, int(g["P2"]), "True", int(g["K2"]))
    mem.memory_v1.copy_(bank(n, D, 21)); mem.memory_v2.copy_(bank(n, D, 22))
    mem = mem.cuda(); mem.verbose = False
    R = Report(f"ContrastMemory_v3 standalone, feat_dim {D}")
    for it in range(2):
        t = f"v3mem{D}_{it}"
        v1, v2 = _c(g, f"{t}_v1").requires_grad_(True), _c(g, f"{t}_v2").requires_grad_(True)
        y = _c(g, f"{t}_y")
        o1, o2 = mem(0.1, v1, v2, y, _c(g, f"{t}_idx"), select_pos_mode="hard")
        assert o1.shape == o2.shape == (v1.shape[0], int(g["P2"]) + int(g["K2"]), 1)
        gv1, gv2 = torch.autograd.grad((o1 * _c(g, f"{t}_w1")).sum() + (o2 * _c(g, f"{t}_w2")).sum(), [v1, v2])
        R.close(g[f"{t}_out1"], o1, 1e-9, 1e-4, f"out_v1 call {it}"); R.close(g[f"{t}_out2"], o2, 1e-9, 1e-4, f"out_v2 call {it}")
        R.close(g[f"{t}_gv1"], gv1, 1e-6, 1e-3, f"d v1 call {it}"); R.close(g[f"{t}_gv2"], gv2, 1e-6, 1e-3, f"d v2 call {it}")
        R.close(g[f"{t}_params"], mem.params, 1e-2, 1e-4, f"params (Z) call {it}")
        R.close(g[f"{t}_rows1"], mem.memory_v1[y], 1e-6, 0, f"bank v1 rows call {it}")
        R.close(g[f"{t}_rows2"], mem.memory_v2[y], 1e-6, 0, f"bank v2 rows call {it}")
    R.finish()


def _opt(g, D, **kw):
    S = int(g["s_dim"])
    return SimpleNamespace(s_dim=S, t_dim=S, feat_dim=D, nce_t=0.07, nce_m=0.5, n_data=int(g["n_data"]), **kw)


@pytest.mark.parametrize("D", WIDTHS)
def test_crd_loss(g, D):
    from multimodal_learning_amd.CL_utils.CRD_loss import CRDLoss
    from tests.gpu_util import Report
    opt = _opt(g, D, nce_p=int(g["P"]), nce_k=int(g["K"]), nce_p2=int(g["P2"]), nce_k2=int(g["K2"]), select_pos_pairs=True,
               select_neg_pairs="True", sample_KD="False", select_pos_mode="hard")
    crd = _load(CRDLoss(opt, opt.n_data), g, D, (10, 11, 21, 22))
    R = Report(f"CRD_loss.CRDLoss, feat_dim {D}")
    for it in range(2):
        t = f"crd{D}_{it}"
        f_s, idx = _c(g, f"{t}_f_s").requires_grad_(True), _c(g, f"{t}_index")
        loss = crd(0.1, f_s, _c(g, f"{t}_f_t"), idx, _c(g, f"{t}_sidx"))
        assert loss.dim() == 0
        gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
        R.close(g[f"{t}_loss"], loss, 1e-4, 1e-5, f"loss call {it}"); R.close(g[f"{t}_g_fs"], gs[0], 1e-6, 1e-3, f"d f_s call {it}")
        if it:
            R.close(g[f"{t}_g_ws"], gs[1], 1e-6, 1e-3, "d W_s call 1"); R.close(g[f"{t}_g_wt"], gs[2], 1e-6, 1e-3, "d W_t call 1")
        R.close(g[f"{t}_params"], crd.contrast.params, 1e-2, 1e-4, f"params (Z) call {it}")
        R.close(g[f"{t}_rows1"], crd.contrast.memory_v1[idx], 1e-6, 0, f"bank v1 rows call {it}")
        R.close(g[f"{t}_rows2"], crd.contrast.memory_v2[idx], 1e-6, 0, f"bank v2 rows call {it}")
    R.finish()


@pytest.mark.parametrize("D", WIDTHS)
def test_stage1_crd_criterion(g, D):
    from multimodal_learning_amd.CL_utils.CRD_criterion import CRDLoss
    from tests.gpu_util import Report
    crd = _load(CRDLoss(_opt(g, D, nce_k=int(g["K1"]))), g, D, (70, 71, 81, 82), two_layer=True)
    R = Report(f"stage-1 CRD_criterion.CRDLoss, feat_dim {D}")
    for it in range(2):
        t = f"s1{D}_{it}"
        f_s, idx = _c(g, f"{t}_f_s").requires_grad_(True), _c(g, f"{t}_index")
        loss = crd(f_s, _c(g, f"{t}_f_t"), idx, _c(g, f"{t}_sidx"))
        assert tuple(loss.shape) == (1,)
        gs = torch.autograd.grad(loss.sum(), [f_s, crd.embed_s.linear[0].weight, crd.embed_t.linear[2].bias])
        R.close(g[f"{t}_loss"], loss, 1e-4, 1e-5, f"loss call {it}"); R.close(g[f"{t}_g_fs"], gs[0], 1e-6, 2e-3, f"d f_s call {it}")
        if it:
            R.close(g[f"{t}_g_w0"], gs[1], 1e-6, 2e-3, "d embed_s.linear.0.weight call 1")
        R.close(g[f"{t}_g_tb2"], gs[2], 1e-6, 2e-3, f"d embed_t.linear.2.bias call {it}")
        R.close(g[f"{t}_params"], crd.contrast.params, 1e-2, 1e-5, f"params (Z) call {it}")
        R.close(g[f"{t}_rows1"], crd.contrast.memory_v1[idx], 1e-5, 0, f"bank v1 rows call {it}")
        R.close(g[f"{t}_rows2"], crd.contrast.memory_v2[idx], 1e-5, 0, f"bank v2 rows call {it}")
    R.finish()


@pytest.mark.parametrize("D", WIDTHS)
def test_mia2022_crd_criterion_v3(g, D):
    from multimodal_learning_amd.CL_utils import CRD_criterion_v3 as V3
    from tests.gpu_util import Report
    opt = _opt(g, D, nce_k=int(g["K1"]))
    crd = _load(V3.CRDLoss(opt, opt.n_data), g, D, (30, 31, 41, 42))
    R = Report(f"MIA-2022 CRD_criterion_v3.CRDLoss, feat_dim {D}")
    for it in range(2):
        t = f"v3{D}_{it}"
        f_s, idx = _c(g, f"{t}_f_s").requires_grad_(True), _c(g, f"{t}_index")
        loss = crd(float(g[f"{t}_w"]), f_s, _c(g, f"{t}_f_t"), idx, _c(g, f"{t}_sidx"))
        assert tuple(loss.shape) == (1,)
        gs = torch.autograd.grad(loss.sum(), [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
        R.close(g[f"{t}_loss"], loss, 1e-4, 1e-5, f"loss call {it}"); R.close(g[f"{t}_g_fs"], gs[0], 1e-6, 1e-3, f"d f_s call {it}")
        if it:
            R.close(g[f"{t}_g_ws"], gs[1], 1e-6, 1e-3, "d W_s call 1"); R.close(g[f"{t}_g_wt"], gs[2], 1e-6, 1e-3, "d W_t call 1")
        R.close(g[f"{t}_params"], crd.contrast.params, 1e-2, 1e-4, f"params (Z) call {it}")
        R.close(g[f"{t}_rows1"], crd.contrast.memory_v1[idx], 1e-6, 0, f"bank rows call {it}")
    R.finish()


@pytest.mark.parametrize("D", WIDTHS)
def test_mia2023_crd_criterion_v10_neighbors(g, D):
    from multimodal_learning_amd.CL_utils import CRD_criterion_v10 as V10
    from tests.gpu_util import Report
    labels = torch.as_tensor(g["labels"])
    class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
    opt = _opt(g, D, nce_k=int(g["K1"]), nce_p=int(g["num_pos"]), pos_extra="neighbors")
    crd = _load(V10.CRDLoss(opt, opt.n_data, class_idx), g, D, (50, 51, 61, 62))
    R = Report(f"MIA-2023 CRD_criterion_v10.CRDLoss (neighbors), feat_dim {D}")
    for it in range(2):
        t = f"v10{D}_{it}"
        f_s, idx = _c(g, f"{t}_f_s").requires_grad_(True), _c(g, f"{t}_index")
        loss, sl = crd(_c(g, f"{t}_w"), f_s, _c(g, f"{t}_f_t"), _c(g, f"{t}_grade"), idx, _c(g, f"{t}_sidx"))
        gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
        R.close(g[f"{t}_loss"], loss, 1e-4, 1e-5, f"loss call {it}"); R.close(g[f"{t}_sample_loss"], sl, 1e-3, 1e-5, f"sample_loss call {it}")
        R.close(g[f"{t}_g_fs"], gs[0], 1e-6, 1e-3, f"d f_s call {it}")
        if it:
            R.close(g[f"{t}_g_ws"], gs[1], 1e-6, 1e-3, "d W_s call 1"); R.close(g[f"{t}_g_wt"], gs[2], 1e-6, 1e-3, "d W_t call 1")
        R.close(g[f"{t}_params"], crd.contrast.params, 1e-2, 1e-4, f"params (Z) call {it}")
        R.close(g[f"{t}_rows1"], crd.contrast.memory_v1[idx], 1e-6, 0, f"bank rows call {it}")
    R.finish()


@pytest.mark.parametrize("D", WIDTHS)
def test_bank_of_another_width_round_trips_through_a_checkpoint(g, D):
    """state_dict -> load_state_dict into a fresh module of the same width: same keys, banks and Z bitwise, the next call agrees."""
    from multimodal_learning_amd.CL_utils import CRD_criterion_v3 as V3
    opt = _opt(g, D, nce_k=int(g["K1"]))
    a = _load(V3.CRDLoss(opt, opt.n_data), g, D, (30, 31, 41, 42))
    t = f"v3{D}_0"
    args = lambda: (float(g[f"{t}_w"]), _c(g, f"{t}_f_s"), _c(g, f"{t}_f_t"), _c(g, f"{t}_index"), _c(g, f"{t}_sidx"))
    a(*args())
    sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    assert sd["contrast.memory_v1"].shape == (opt.n_data, D)
    b = V3.CRDLoss(opt, opt.n_data)
    b.load_state_dict(sd)
    b = b.cuda(); b.contrast.verbose = False
    assert b.contrast._z_set
    la, lb = a(*args()), b(*args())
    assert torch.equal(la, lb) and torch.equal(a.contrast.memory_v1, b.contrast.memory_v1)
    wrong = V3.CRDLoss(_opt(g, 128, nce_k=int(g["K1"])), opt.n_data)
    with pytest.raises(RuntimeError, match="size mismatch"):
        wrong.load_state_dict(sd)


@pytest.mark.parametrize("D", WIDTHS)
def test_mia2023_bank_scan_form_equals_gathered_form(g, D, monkeypatch):
    """nce_k at the number of bank rows: the bank-scan form of the negatives (memory_new._crd_core_scan: ph_crd_neg_hist, the two
    width-D GEMMs, ph_crd_scan_neg, ph_crd_loss_grad_pos, the split-K gradient GEMMs) against the gathered kernels on the same
    inputs (PH_CRD_SCAN=0; pinned on the reference golden above), two calls, at the tolerances of
    test_gpu_losses.py::test_mia2023_crd_v10_with_as_many_negatives_as_bank_rows."""
    from multimodal_learning_amd.CL_utils import CRD_criterion_v10 as V10
    from tests.gpu_util import Report
    n, B, K, S = 1024, 5, 1024, int(g["s_dim"])      # (1024 rows: the 32-way split-K of the gradient GEMMs)
    labels = torch.arange(n) % 3
    class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
    res = {}
    for form in ("scan", "gathered"):
        monkeypatch.setenv("PH_CRD_SCAN", "1" if form == "scan" else "0")
        opt = SimpleNamespace(s_dim=S, t_dim=S, feat_dim=D, nce_t=0.07, nce_m=0.5, n_data=n, nce_k=K, nce_p=3, pos_extra="neighbors")
        crd = V10.CRDLoss(opt, n, class_idx)
        shapes = {"linear.weight": (D, S), "linear.bias": (D,)}
        crd.embed_s.load_state_dict(head(shapes, 50)); crd.embed_t.load_state_dict(head(shapes, 51))
        crd.contrast.memory_v1.copy_(bank(n, D, 61)); crd.contrast.memory_v2.copy_(bank(n, D, 62))
        crd = crd.cuda(); crd.contrast.verbose = False
        gen = torch.Generator().manual_seed(90 + D)
        rec = []
        for it in range(2):
            index = torch.randperm(n, generator=gen)[:B]
            sidx = torch.randint(0, n, (B, K + 1), generator=gen); sidx[:, 0] = index
            f_s = torch.randn(B, S, generator=gen).relu_().cuda().requires_grad_(True)
            f_t = torch.randn(B, S, generator=gen).relu_().cuda()
            w = (torch.rand(B, generator=gen) + 0.5).cuda()
            loss, sl = crd(w, f_s, f_t, labels[index].cuda(), index.cuda(), sidx.cuda())
            assert (crd.contrast.last["call"].scan is not None) == (form == "scan")
            gs = torch.autograd.grad(loss, [f_s, crd.embed_t.linear.weight])
            rec.append(dict(loss=loss.detach(), sl=sl.detach(), g_fs=gs[0], g_wt=gs[1], params=crd.contrast.params.clone(),
                            rows=crd.contrast.memory_v1[index.cuda()].clone()))
        res[form] = rec
    R = Report(f"MIA-2023 CRD v10 at feat_dim {D}: bank-scan form vs gathered form")
    for it in range(2):
        a, b = res["scan"][it], res["gathered"][it]
        R.close(b["loss"], a["loss"], 1e-4, 1e-5, f"loss call {it}"); R.close(b["sl"], a["sl"], 1e-3, 1e-5, f"sample_loss call {it}")
        R.close(b["g_fs"], a["g_fs"], 1e-6, 2e-3, f"d f_s call {it}"); R.close(b["g_wt"], a["g_wt"], 1e-6, 2e-3, f"d W_t call {it}")
        R.close(b["params"], a["params"], 1e-2, 1e-4, f"params/Z call {it}"); R.close(b["rows"], a["rows"], 1e-6, 0, f"bank rows call {it}")
    R.finish()

"""More than eight KNN positives (`--pos_extra neighbors`, nce_p up to 64) through the modules and the MIA-2023 step.

  criterion   the drop-in CRDLoss with nce_p 16 and 24 against the reference's own CRDLoss
              (tests/golden/make_golden_mia2023_np.py -> mia2023_crd_v10_np.npz: two calls each, B = 8, a bank of 384 rows in which
              every query has at least nce_p same-class rows of positive similarity), at the tolerances
              tests/test_gpu_losses.py::test_mia2023_crd_v10_golden holds mia2023_crd_v10.npz to: loss, sample losses, three
              gradients, params, updated bank rows.
  step        DistillStep(variant="mia2023") with nce_p = 16 at B = 4, 64 x 64: the fused loss head against the generic autograd
              path (one step), and three steps replayed from captured graphs against three eager steps - both at the tolerances
              of tests/test_gpu_step_width.py: losses and logits within 1e-5 relative, every parameter gradient within 2e-4, the
              updated bank bitwise.
  range       nce_p 0 and 65 raise ValueError at construction, from CRDLoss and from the step; so does nce_p above n_data."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("NP", (16, 24))
def test_crd_v10_with_more_than_eight_neighbours_vs_reference_golden(golden_dir, NP):
    import multimodal_learning_amd as m
    from multimodal_learning_amd.CL_utils import CRD_criterion_v10 as V10
    from oracle import weights as W
    from oracle.variants import CRDv10State
    from tests.gpu_util import Report
    g = np.load(os.path.join(golden_dir, "mia2023_crd_v10_np.npz"))
    assert NP in g["num_pos"]
    p = f"p{NP}_"
    labels = torch.as_tensor(g["labels"])
    class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
    opt = m.stage2_opt(nce_k=int(g["K"]), nce_p=NP)
    crd = V10.CRDLoss(opt, int(g["n_data"]), class_idx)
    crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 50))
    crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 51))
    st = CRDv10State(int(g["n_data"]), labels, K=int(g["K"]), seed=int(g["bank_seed"]))
    crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
    crd = crd.cuda(); crd.contrast.verbose = False
    R = Report(f"MIA-2023 CRD_criterion_v10 (neighbors, nce_p {NP}) vs reference golden")
    for it in range(2):
        f_s = torch.as_tensor(g[f"{p}f_s{it}"]).cuda().requires_grad_(True)
        index = torch.as_tensor(g[f"{p}index{it}"]).cuda()
        loss, sl = crd(torch.as_tensor(g[f"{p}w{it}"]).cuda(), f_s, torch.as_tensor(g[f"{p}f_t{it}"]).cuda(),
                       torch.as_tensor(g[f"{p}grade{it}"]).cuda(), index, torch.as_tensor(g[f"{p}sidx{it}"]).cuda())
        gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
        knn = crd.contrast.last
        assert tuple(knn["nb1"].shape) == (f_s.shape[0], NP) and bool((knn["sim1"] > 0).all()) and bool((knn["sim2"] > 0).all())
        R.close(g[f"{p}loss{it}"], loss, 1e-4, 1e-5, f"loss call {it}")
        R.close(g[f"{p}sample_loss{it}"], sl, 1e-3, 1e-5, f"sample_loss call {it}")
        R.close(g[f"{p}g_fs{it}"], gs[0], 1e-6, 1e-3, f"d f_s call {it}"); R.close(g[f"{p}g_ws{it}"], gs[1], 1e-6, 1e-3, f"d W_s call {it}")
        R.close(g[f"{p}g_wt{it}"], gs[2], 1e-6, 1e-3, f"d W_t call {it}")
        R.close(g[f"{p}params{it}"], crd.contrast.params, 1e-2, 1e-4, f"params/Z call {it}")
        R.close(g[f"{p}bank_v1_rows{it}"], crd.contrast.memory_v1[index], 1e-6, 0, f"bank rows call {it}")
    R.finish()


N_DATA, K, B, NP_STEP = 256, 64, 4, 16
LABELS = torch.arange(N_DATA) % 3


def _class_idx():
    return [np.nonzero((LABELS == c).numpy())[0] for c in range(3)]


def _step(fused, nce_p=NP_STEP):
    import multimodal_learning_amd as m
    from oracle.step import default_opt
    opt = default_opt(nce_k=K, nce_p=nce_p, pos_extra="neighbors", neg_mode="all_others", start_reweight=0, discrep_scale=1,
                      max_discrep=2.0, use_grads_thresh="True", grads_thresh=0.1, loss_weighting="GK_refine", batch_size=B)
    opt.fused_loss_head = fused
    torch.manual_seed(7)
    step = m.DistillStep(opt, N_DATA, device="cuda", variant="mia2023", train_class_idx=_class_idx())
    for crd in (step.criterion_kd, step.criterion_kd_path):
        crd.contrast.verbose = False
    return step


def _batch(seed, on_device=False):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, 64, n_data=N_DATA, P=1, K=K, seed=seed)
    bt["grade"] = LABELS[bt["index"]].long()
    if on_device:
        bt = {k: v.cuda() for k, v in bt.items()}
    return ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], torch.zeros(B), torch.zeros(B), bt["grade"], bt["index"],
            bt["sample_idx"])


def _record(step, out):
    names = [k for k in ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2", "scale", "logit_path") if k in out]
    Pm = dict(step.module_list.named_parameters())
    return dict(out={k: out[k].detach().float().clone() for k in names},
                grads={k: p.grad.detach().clone() for k, p in Pm.items() if p.grad is not None},
                bank=[step.criterion_kd.contrast.memory_v1.clone(), step.criterion_kd_path.contrast.memory_v2.clone()])


def _hold(a, b, what):
    """The tolerances of tests/test_gpu_step_width.py::test_fused_step_equals_eager_composition_at_dims_64."""
    assert {"loss", "loss_kd1", "scale"} <= set(a["out"]) and set(a["out"]) == set(b["out"])
    for k in a["out"]:
        assert torch.isfinite(a["out"][k]).all(), (what, k)
        d = (a["out"][k].reshape(-1) - b["out"][k].reshape(-1)).abs().max().item()
        print(f"   {what} {k}: max |diff| {d:.2e}")
        assert d <= 1e-5 * max(1.0, b["out"][k].abs().max().item()), (what, k, d)
    assert set(a["grads"]) == set(b["grads"])
    worst = 0.0
    for k in b["grads"]:
        ga, gb = a["grads"][k], b["grads"][k]
        d = max((ga - gb).abs().max().item() - 1e-6, 0.0) / (gb.abs().max().item() + 1e-12)
        worst = max(worst, d)
        assert d <= 2e-4, (what, k, d)
    print(f"   {what}: worst relative gradient difference {worst:.2e}")
    for x, y in zip(a["bank"], b["bank"]):
        assert torch.equal(x, y), what


def test_mia2023_step_with_16_neighbours_fused_head_equals_autograd_path():
    import multimodal_learning_amd as m
    m.set_precision("bf16x6")
    try:
        rec = []
        for fused in (True, False):
            step = _step(fused)
            out = step.step(_batch(600), epoch=2)
            assert step._fused_head_ok() == fused
            call = step.criterion_kd.contrast.last["call"]
            assert call.P == NP_STEP and tuple(call.posw_s.shape) == (B, NP_STEP)
            rec.append(_record(step, out))
    finally:
        m.set_precision("bf16")
    _hold(rec[0], rec[1], "fused vs autograd")


def test_mia2023_step_with_16_neighbours_replays_from_captured_graphs():
    """Three steps with enable_graph() against three eager steps: the KNN call of 2 + 2 x 2 launches has no host read and no
    allocation, so the step is captured and replays to the eager numbers."""
    import multimodal_learning_amd as m
    m.set_precision("bf16x6")
    try:
        recs = []
        for graph in (False, True):
            step = _step(True)
            if graph:
                step.enable_graph()
            batches = [_batch(610 + s, on_device=True) for s in range(2)]
            per_step = []
            for it in range(3):
                out = step.step(batches[it % 2], epoch=2)
                per_step.append(_record(step, out))
            torch.cuda.synchronize()
            if graph:
                assert step._want_graph and step._slots and step._slots[0]["graph"] is not None, "the step was not captured"
            recs.append(per_step)
    finally:
        m.set_precision("bf16")
    for it in range(3):
        _hold(recs[1][it], recs[0][it], f"graph vs eager, step {it}")


@pytest.mark.parametrize("nce_p", (0, 65))
def test_neighbour_count_outside_the_range_raises_at_construction(nce_p):
    import multimodal_learning_amd as m
    from multimodal_learning_amd.CL_utils import CRD_criterion_v10 as V10
    with pytest.raises(ValueError, match=r"1 \.\. 64"):
        V10.CRDLoss(m.stage2_opt(nce_k=16, nce_p=nce_p), N_DATA, _class_idx())
    with pytest.raises(ValueError, match=r"1 \.\. 64"):
        _step(True, nce_p=nce_p)
    V10.CRDLoss(m.stage2_opt(nce_k=16, nce_p=64), N_DATA, _class_idx())
    with pytest.raises(ValueError, match="n_data"):      # more neighbours than bank rows: empty KNN slots
        V10.CRDLoss(m.stage2_opt(nce_k=16, nce_p=24), 20, [np.arange(0, 10), np.arange(10, 20)])

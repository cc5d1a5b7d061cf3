"""The survival (Cox) task of the stage-1 teacher (MICCAI-2022/train_test_MT.py with --task surv --act_type Sigmoid
--label_dim 1): the sigmoid-range heads, the fused survival loss kernel, the step against the reference's own modules
(tests/golden/make_golden_stage1_surv.py), graph replay, the concordance counts and the stage-1 evaluation."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _surv_opt(**kw):
    import multimodal_learning_amd as m
    base = dict(task="surv", act_type="Sigmoid", label_dim=1, dropout_rate=0.0, batch_size=8, cut_fuse_grad=False,
                num_teachers=2, reg_type="none")
    base.update(kw)
    opt = m.stage2_opt(**base)
    opt.pred_distill = 1
    return opt


# ------------------------------------------------------------------------------------------------ heads
def test_sigmoid_range_fn_matches_autograd():
    import multimodal_learning_amd.ops as ops
    torch.manual_seed(0)
    for r, s in ((6.0, -3.0), (2.5, 0.75), (-1.5, 4.0)):
        h = torch.randn(37, 1, device="cuda", requires_grad=True)
        rp = torch.tensor([r], device="cuda"); sp = torch.tensor([s], device="cuda")
        y = ops.SigmoidRangeFn.apply(h, rp, sp)
        g = torch.randn_like(y)
        dh, = torch.autograd.grad(y, h, g)
        h2 = h.detach().clone().requires_grad_(True)
        y2 = torch.sigmoid(h2) * rp + sp
        dh2, = torch.autograd.grad(y2, h2, g)
        assert (y - y2).abs().max().item() <= 1e-6
        assert (dh - dh2).abs().max().item() <= 1e-6


@pytest.mark.parametrize("train", [True, False])
def test_surv_networks_tuples_shapes_and_state_dict_keys(train):
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt = _surv_opt()
    t = m.define_net(opt, 1).cuda()
    s = m.define_net(opt, 1, path_only=True).cuda()
    o = m.define_net(opt, 1, omic_only=True).cuda()
    assert list(t.state_dict().keys()) == list(W.teacher_shapes(320, label_dim=1).keys())
    assert list(s.state_dict().keys()) == list(W.student_shapes(label_dim=1).keys())
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    sd["output_range"] = torch.tensor([4.0]); sd["output_shift"] = torch.tensor([-1.0])
    t.load_state_dict(sd)
    for net in (t, s, o):
        net.train(train)
    B = 4
    x_path = torch.rand(B, 3, 64, 64, device="cuda") * 2 - 1
    x_omic = torch.randn(B, 320, device="cuda")
    with torch.set_grad_enabled(train):
        out = t(x_path=x_path, x_omic=x_omic)
    assert len(out) == 11
    feat, path_vec, omic_vec, _, logits, pred, pred_path, pred_omic, _, _, _ = out
    assert pred.shape == pred_path.shape == pred_omic.shape == (B, 1)
    assert [l.shape for l in logits] == [(B, 1)] * 3
    # the fused head reads the MODULE's range / shift (4 / -1 here), the sub-networks their own (6 / -3)
    want = torch.sigmoid(logits[2].float()) * 4.0 - 1.0
    assert (pred - want).abs().max().item() <= 1e-5
    assert (pred_path - (torch.sigmoid(logits[0]) * 6 - 3)).abs().max().item() <= 1e-5
    assert (pred_omic - (torch.sigmoid(logits[1]) * 6 - 3)).abs().max().item() <= 1e-5
    so = s(x_path=x_path)
    assert len(so) == 5 and so[3].shape == (B, 1)
    oo = o(x_omic=x_omic)
    assert len(oo) == 4 and oo[2].shape == (B, 1)


def test_surv_resnet_eval_with_image_gradient():
    """The eval-mode ResNet path with a gradient to the image (MIA-2023 attention) takes the sigmoid head too."""
    import multimodal_learning_amd as m
    s = m.define_net(_surv_opt(), 1, path_only=True).cuda().eval()
    x = (torch.rand(2, 3, 64, 64, device="cuda") * 2 - 1).requires_grad_(True)
    out = s(x_path=x)
    out[3].sum().backward()
    assert out[3].shape == (2, 1) and x.grad is not None and torch.isfinite(x.grad).all()
    assert out[3].min().item() >= -3.0 and out[3].max().item() <= 3.0


# ------------------------------------------------------------------------------------------------ fused loss
def _ref_surv_total(p, q, t, c, nt, lam, kw):
    """The reference formulas in torch autograd: CoxLoss (utils.py:361-376) x 3 + pred_KD_loss MSE terms (:180-201)."""
    R = (t.reshape(1, -1) >= t.reshape(-1, 1)).float()

    def cox(theta):
        theta = theta.reshape(-1)
        return -torch.mean((theta - torch.log(torch.sum(torch.exp(theta) * R, dim=1))) * c)

    mse = torch.nn.functional.mse_loss
    cx = [cox(x) for x in p]
    kd = [torch.zeros(())] * 3
    if nt:
        kd[0] = mse(p[0], q[0])
        if nt == 1:
            kd[1], kd[2] = mse(p[1], q[1]), mse(p[2], q[2])
        elif nt == 2:
            kd[1] = (mse(p[1], q[1]) + mse(p[1], q[0])) / 2.0
            kd[2] = (mse(p[2], q[2]) + mse(p[2], q[0])) / 2.0
        else:
            kd[1] = (mse(p[1], q[1]) + mse(p[1], q[0]) + mse(p[1], q[2])) / 3.0
            kd[2] = (mse(p[2], q[2]) + mse(p[2], q[0]) + mse(p[2], q[1])) / 3.0
    return lam * (cx[1] + cx[2] + cx[0]) + kw * (kd[0] + kd[1] + kd[2]), cx, kd


@pytest.mark.parametrize("B", [8, 64, 300])
def test_fused_surv_loss_cox_terms_vs_reference_golden(golden_dir, B):
    import multimodal_learning_amd.ops as ops
    g = np.load(os.path.join(golden_dir, "cox_loss.npz"))
    theta = torch.from_numpy(g[f"theta{B}"]).cuda()
    t, c = torch.from_numpy(g[f"t{B}"]).cuda(), torch.from_numpy(g[f"c{B}"]).cuda()
    # the golden theta as the fused prediction, shifted for path (same loss), scaled for omic (restated in torch)
    ps = [theta, theta + 0.25, theta * 0.5]
    terms = ops.surv_loss_terms(ps[0], ps[1], ps[2], t, c).cpu().numpy()
    assert abs(terms[0] - float(g[f"loss{B}"])) <= 1e-5
    assert abs(terms[1] - float(g[f"loss{B}"])) <= 1e-5          # the Cox loss is invariant to a constant shift of theta
    want, _, _ = _ref_surv_total([ps[2].cpu()] * 3, None, t.cpu(), c.cpu(), 0, 1.0, 0.0)
    assert abs(terms[2] - want.item() / 3.0) <= 1e-5


@pytest.mark.parametrize("nt", [0, 1, 2, 3])
@pytest.mark.parametrize("B", [8, 64, 300])
def test_fused_surv_loss_grad_vs_autograd(golden_dir, nt, B):
    import multimodal_learning_amd.ops as ops
    g = np.load(os.path.join(golden_dir, "cox_loss.npz"))
    torch.manual_seed(B + nt)
    t, c = torch.from_numpy(g[f"t{B}"]), torch.from_numpy(g[f"c{B}"])
    p = [torch.from_numpy(g[f"theta{B}"]) + 0.3 * k for k in range(3)]
    q = [x + 0.2 * torch.randn_like(x) for x in p]
    lam, kw = 0.7, 1.3
    pr = [x.clone().requires_grad_(True) for x in p]
    want, cx, kd = _ref_surv_total(pr, q, t, c, nt, lam, kw)
    dwant = torch.autograd.grad(want, pr)
    pg = [x.cuda().requires_grad_(True) for x in p]
    total, terms = ops.SurvStage1LossFn.apply(pg[0], pg[1], pg[2], *[x.cuda() for x in q], t.cuda(), c.cuda(), nt, lam, kw)
    (2.0 * total).backward()
    assert abs(total.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    tv = terms.cpu().numpy()
    for k in range(3):
        assert abs(tv[k] - cx[k].item()) <= 1e-5
        assert abs(tv[3 + k] - kd[k].item()) <= 1e-5
        assert (pg[k].grad.cpu() - 2.0 * dwant[k]).abs().max().item() <= 1e-6, k
    assert abs(tv[6] - sum(x.item() for x in cx)) <= 1e-5
    assert abs(tv[7] - kw * sum(x.item() for x in kd)) <= 1e-5


def test_fused_surv_loss_rejects_oversized_batch():
    from multimodal_learning_amd._lib import lib, ptr, stream
    B = 4097
    x = torch.zeros(B, device="cuda")
    out = torch.zeros(9, device="cuda")
    rc = lib().ph_surv_stage1_loss_grad(ptr(x), ptr(x), ptr(x), None, None, None, ptr(x), ptr(x), B, 0, 1.0, 0.0, ptr(out),
                                        None, stream())
    assert rc == -22


# ------------------------------------------------------------------------------------------------ the step
def _load_crd(st, K, n_data):
    from oracle.variants import CRDv3State
    from tests.test_oracle_variants import _embed2_state
    for i, c in enumerate((st.CRD_criterion_path, st.CRD_criterion_omic, st.CRD_criterion_fuse)):
        c.embed_s.load_state_dict(_embed2_state(90 + 2 * i)); c.embed_t.load_state_dict(_embed2_state(91 + 2 * i))
        bank = CRDv3State(n_data, K=K, seed=100 + i)
        c.contrast.memory_v1.copy_(bank.memory_v1); c.contrast.memory_v2.copy_(bank.memory_v2)


def _golden_step(g, tag):
    import multimodal_learning_amd as m
    from oracle import weights as W
    crd_orth = bool(int(g[f"{tag}_crd_orth"]))
    opt = _surv_opt(num_teachers=int(g[f"{tag}_num_teachers"]))
    opt.KD_weight, opt.lambda_cox = float(g[f"{tag}_KD_weight"]), float(g[f"{tag}_lambda_cox"])
    opt.lr, opt.weight_decay, opt.ema_decay = float(g[f"{tag}_lr"]), float(g[f"{tag}_weight_decay"]), float(g[f"{tag}_ema_decay"])
    opt.nce_k, opt.n_data = int(g[f"{tag}_K"]), int(g[f"{tag}_n_data"])
    if crd_orth:
        opt.CRD_distill, opt.CRD_weight, opt.orth_loss, opt.SP_distill = 1, float(g[f"{tag}_CRD_weight"]), "True", 0
    model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    ema.load_state_dict(sd)
    sd = dict(sd)
    sd["output_range"] = torch.tensor([float(g["output_range"])]); sd["output_shift"] = torch.tensor([float(g["output_shift"])])
    model.load_state_dict(sd)
    st = m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()))
    if crd_orth:
        _load_crd(st, opt.nce_k, opt.n_data)
    return opt, st, sd


def _golden_batch(g, opt, it):
    from oracle.step import synthetic_batch
    B, H = int(g["B"]), int(g["H"])
    bt = synthetic_batch(B, H, n_data=opt.n_data, P=1, K=opt.nce_k, seed=70 + it)
    return ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], torch.from_numpy(g["censor"]),
            torch.from_numpy(g["survtime"]), bt["grade"], bt["index"], bt["sample_idx"])


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3/x1"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_stage1_surv_step_vs_reference_golden(golden_dir, pmode, tag):
    """Two stage-1 steps under --task surv against the reference's modules: option set (a) num_teachers 2, (b) num_teachers 3
    + CRD + orthogonality.  Tolerances of test_stage1_teacher_step_vs_reference_golden."""
    import multimodal_learning_amd as m
    g = np.load(os.path.join(golden_dir, "stage1_surv_b8_h64.npz"))
    m.set_precision(pmode)
    try:
        opt, st, sd = _golden_step(g, tag)
        for it in range(2):
            out = st.step(_golden_batch(g, opt, it), epoch=it)
            tol = 1e-3 if it == 0 else 5e-2
            for k, gk in (("loss", "loss"), ("loss_cox", "loss_cox"), ("loss_cox_fuse", "loss_cox_fuse"),
                          ("loss_cox_path", "loss_cox_path"), ("loss_cox_omic", "loss_cox_omic")):
                ref = float(np.asarray(g[f"{tag}_{gk}{it}"]).reshape(()))
                assert abs(out[k].item() - ref) <= tol * abs(ref), (it, k, out[k].item(), ref)
            kd_tol = tol if it == 0 else 0.25
            for k, gk in (("loss_pred_KD", "loss_kd"), ("loss_kd_fuse", "kd_fuse"), ("loss_kd_path", "kd_path"),
                          ("loss_kd_omic", "kd_omic")):
                ref = float(np.asarray(g[f"{tag}_{gk}{it}"]).reshape(()))
                assert abs(out[k].item() - ref) <= kd_tol * max(abs(ref), 1e-2), (it, k, out[k].item(), ref)
            assert out["loss_nll"].item() == 0.0
            for k in ("pred", "pred_path", "pred_omic"):
                assert np.abs(out[k].cpu().numpy() - g[f"{tag}_{k}{it}"]).max() <= tol * 10, (it, k)
            if it == 0:
                msd = st.model.state_dict()
                for key in g.files:
                    if key.startswith(f"{tag}_w0_"):
                        name = key[len(tag) + 4:]
                        upd_ref = g[key] - sd[name].numpy()
                        upd = msd[name].cpu().numpy() - sd[name].numpy()
                        frac_bad = float((np.abs(upd - upd_ref) > 0.2 * float(opt.lr)).mean())
                        assert frac_bad < 0.02, (name, frac_bad)
        esd = st.ema_model.state_dict()
        for key in g.files:
            if key.startswith(f"{tag}_ema_") and key != f"{tag}_ema_decay":
                name = key[len(tag) + 5:]
                assert np.array_equal(esd[name].cpu().numpy(), g[key]), (name, esd[name], g[key])
    finally:
        m.set_precision("bf16")


def _graph_pair_inputs(B, seed):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, 64, seed=seed, P=1, K=16)
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 6, (B,), generator=gen).float()
    c = (torch.rand(B, generator=gen) > 0.4).float()
    return bt, t, c


def test_stage1_surv_graph_replay_equals_eager():
    """enable_graph() under surv: steps 2 to 6 replayed from captured graphs equal the same steps launched eagerly.  Odd steps
    feed device-resident inputs filled in place into the same buffers (survtime / censor included: one ADOPTED input set),
    even steps host tensors (copied into one STAGED set).  Both sets must hold a captured graph and no capture may have
    fallen back to eager launches."""
    import warnings
    import multimodal_learning_amd as m
    from oracle import weights as W
    B = 8
    opt = _surv_opt(num_teachers=3)
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    steps = {}
    for mode in ("eager", "graph"):
        model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
        model.load_state_dict(sd); ema.load_state_dict(sd)
        st = m.TeacherStage1Step(copy.deepcopy(opt), device="cuda", models=(model.cuda(), ema.cuda()))
        if mode == "graph":
            st.enable_graph()
        res, resident = [], None
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for it in range(7):
                bt, t, c = _graph_pair_inputs(B, 40 + min(it, 5))
                host = [bt["x_path"], bt["ema_x_path"], bt["x_omic"], c, t, bt["grade"], bt["index"], bt["sample_idx"]]
                if it % 2 == 1:
                    if resident is None:
                        resident = [x.cuda().contiguous() for x in host]
                    for r, x in zip(resident, host):
                        r.copy_(x)
                    ins = resident
                else:
                    ins = host
                batch = ((ins[0], ins[1]), torch.zeros(B), ins[2], ins[3], ins[4], ins[5], ins[6], ins[7])
                out = st.step(batch)
                res.append({k: v.detach().clone() for k, v in out.items() if k.startswith("loss")})
                res[-1]["w"] = st.model.classifier[0].weight.detach().clone()
                res[-1]["w_omic"] = st.model.omic_net.encoder[0][0].weight.detach().clone()
                res[-1]["ema_range"] = st.ema_model.output_range.detach().clone()
            torch.cuda.synchronize()
        if mode == "graph":
            assert not [w for w in caught if "capture" in str(w.message)], [str(w.message) for w in caught]
            assert st._want_graph, "the survival step fell back to eager launches"
            sets = st._g_sets
            assert len(sets) == 2 and sorted(q["adopted"] for q in sets) == [False, True], \
                "steps 2.. must have been replayed from graphs (one adopted, one staged input set)"
            assert all(len(q["graphs"]) == 1 for q in sets)
            adopted = next(q for q in sets if q["adopted"])
            assert adopted["bufs"]["survtime"].data_ptr() == resident[4].data_ptr()
            assert adopted["bufs"]["censor"].data_ptr() == resident[3].data_ptr()
        steps[mode] = res
    for it in range(2, 7):
        e, g = steps["eager"][it], steps["graph"][it]
        for k in ("loss", "loss_cox", "loss_cox_fuse", "loss_cox_path", "loss_cox_omic", "loss_pred_KD"):
            assert abs(g[k].item() - e[k].item()) <= 2e-3 * max(abs(e[k].item()), 1e-3), (it, k, g[k].item(), e[k].item())
        for k in ("w", "w_omic"):
            assert (g[k] - e[k]).abs().max().item() <= 5e-3 * max(e[k].abs().max().item(), 1e-3), (it, k)
        assert torch.equal(g["ema_range"], e["ema_range"])


def test_surv_inputs_of_other_dtypes_keep_one_device_buffer():
    """A device survtime / censor of another dtype is converted into the same persistent float32 buffer every step (a graph
    can adopt it); float32 passes as it is; host tensors are converted on the host."""
    import multimodal_learning_amd as m
    st = m.TeacherStage1Step(_surv_opt(), device="cuda")
    a = torch.arange(8, device="cuda", dtype=torch.float64)
    b1, b2 = st._as_f32("survtime", a), st._as_f32("survtime", a + 1)
    assert b1.dtype == torch.float32 and b1.data_ptr() == b2.data_ptr() and torch.equal(b2.cpu(), (a + 1).float().cpu())
    f = torch.ones(8, device="cuda")
    assert st._as_f32("censor", f) is f
    assert not st._as_f32("censor", torch.ones(8, dtype=torch.int64)).is_cuda


# ------------------------------------------------------------------------------------------------ concordance
def _np_counts(t, e, h):
    """float64 numpy restatement of the lifelines rule (blocked to bound memory)."""
    t, e, h = (np.asarray(x, dtype=np.float64) for x in (t, e, h))
    comp = conc = tie = 0
    for i0 in range(0, len(t), 512):
        ti, ei, hi = t[i0:i0 + 512, None], e[i0:i0 + 512, None] > 0.5, h[i0:i0 + 512, None]
        cm = ei & ((ti < t[None]) | ((ti == t[None]) & (e[None] <= 0.5)))
        comp += int(cm.sum()); conc += int((cm & (hi > h[None])).sum()); tie += int((cm & (hi == h[None])).sum())
    return comp, conc, tie


def test_cindex_worked_case():
    import multimodal_learning_amd as m
    from multimodal_learning_amd import utils as U
    t = torch.tensor([1.0, 2.0, 2.0, 3.0]); e = torch.tensor([1.0, 1.0, 0.0, 1.0]); h = torch.tensor([0.9, 0.5, 0.5, 0.1])
    counts = m.ops.cindex_counts(t.cuda(), e.cuda(), [h.cuda()]).cpu().numpy()
    assert counts.dtype == np.int64 and counts[0].tolist() == [5, 4, 1]
    assert U.CIndex_lifeline(h.numpy(), e.numpy(), t.numpy()) == 0.9


def test_cindex_without_comparable_pairs_raises():
    from multimodal_learning_amd import utils as U
    with pytest.raises(ZeroDivisionError):
        U.CIndex_lifeline(np.array([0.3, 0.7]), np.array([1.0, 1.0]), np.array([2.0, 2.0]))


def test_cindex_rejects_n_below_two():
    from multimodal_learning_amd._lib import lib, ptr, stream
    x = torch.zeros(1, device="cuda")
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert lib().ph_cindex_counts(ptr(x), ptr(x), ptr(x), None, None, 1, 1, ptr(out), stream()) == -22


def test_cindex_tie_free_vs_reference_cindex(golden_dir):
    from multimodal_learning_amd import utils as U
    g = np.load(os.path.join(golden_dir, "cindex_tiefree.npz"))
    got = U.CIndex_lifeline(g["hazards"], g["labels"], g["survtime"])
    assert abs(got - float(g["cindex"])) <= 1e-12


def test_cindex_counts_with_ties_vs_numpy_n4096():
    import multimodal_learning_amd as m
    rs = np.random.RandomState(3)
    N = 4096
    t = rs.randint(1, 200, N).astype(np.float32)                    # many time ties
    e = (rs.rand(N) > 0.4).astype(np.float32)
    hs = [np.round(rs.randn(N), 1).astype(np.float32) for _ in range(3)]   # many hazard ties
    got = m.ops.cindex_counts(torch.from_numpy(t).cuda(), torch.from_numpy(e).cuda(), [torch.from_numpy(h).cuda() for h in hs])
    got = got.cpu().numpy()
    for v in range(3):
        assert tuple(int(x) for x in got[v]) == _np_counts(t, e, hs[v]), v


def _cindex_tied_case(N, seed, with_nan=False):
    rs = np.random.RandomState(seed)
    t = rs.randint(1, 6, N).astype(np.float32)                      # five distinct times, three hazard levels: heavy ties
    e = (rs.rand(N) > 0.4).astype(np.float32)
    e[0] = 1.0                                                      # (an event in every case, N = 2 included)
    hs = [rs.randint(0, 3, N).astype(np.float32) for _ in range(3)]
    if with_nan:
        t[N // 3] = np.nan
        hs[0][N // 2] = hs[2][N - 1] = np.nan
    return t, e, hs


@pytest.mark.parametrize("N,with_nan", [(2, False), (255, False), (256, False), (257, False), (513, False), (257, True)])
def test_cindex_counts_at_the_tile_edges_vs_numpy(N, with_nan):
    """One row, one short, one more than the 256-row tile, two tiles and a row: the rows past the end are staged as NaN
    times and must count in nothing.  A NaN time or hazard among the rows is comparable / concordant / tied with nothing
    either (every comparison with it is false, in numpy as on the device)."""
    import multimodal_learning_amd as m
    t, e, hs = _cindex_tied_case(N, 11 + N, with_nan)
    got = m.ops.cindex_counts(torch.from_numpy(t).cuda(), torch.from_numpy(e).cuda(), [torch.from_numpy(h).cuda() for h in hs])
    got = got.cpu().numpy()
    want = [_np_counts(t, e, h) for h in hs]
    assert want[0][0] > 0
    for v in range(3):
        assert tuple(int(x) for x in got[v]) == want[v], (v, got[v], want[v])


def test_cindex_counts_independent_of_row_order_n100000():
    import multimodal_learning_amd as m
    rs = np.random.RandomState(5)
    N = 100000
    t = torch.from_numpy(rs.randint(1, 5000, N).astype(np.float32)).cuda()
    e = torch.from_numpy((rs.rand(N) > 0.5).astype(np.float32)).cuda()
    hs = [torch.from_numpy(np.round(rs.randn(N), 2).astype(np.float32)).cuda() for _ in range(2)]
    a = m.ops.cindex_counts(t, e, hs)
    perm = torch.from_numpy(rs.permutation(N)).cuda()
    b = m.ops.cindex_counts(t[perm].contiguous(), e[perm].contiguous(), [h[perm].contiguous() for h in hs])
    assert torch.equal(a.cpu(), b.cpu())
    assert int(a[0, 0]) > 0


# ------------------------------------------------------------------------------------------------ evaluation
class _Loader(list):
    def __init__(self, batches, n):
        super().__init__(batches)
        self.dataset = range(n)


def _golden_eval_loader(sizes, H):
    """The loader of tests/golden/make_golden_eval_stage1.py (same seeds)."""
    from oracle.step import synthetic_batch
    batches = []
    for i, B in enumerate(sizes):
        bt = synthetic_batch(B, H, seed=600 + i)
        g = torch.Generator().manual_seed(610 + i)
        censor = (torch.rand(B, generator=g) > 0.35).float()
        survtime = torch.randint(1, 12, (B,), generator=g).float()
        batches.append((bt["x_path"], torch.zeros(B), bt["x_omic"], censor, survtime, bt["grade"]))
    return _Loader(batches, sum(sizes))


def _golden_eval_model(g, task):
    import multimodal_learning_amd as m
    from oracle import weights as W
    if task == "surv":
        opt = _surv_opt(reg_type="omic")
        sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
        for k in ("classifier.0.weight", "path_net.fc_new2.weight", "omic_net.classifier.0.weight"):
            sd[k] = sd[k] * float(g["head_scale"])
    else:
        opt = m.stage2_opt(dropout_rate=0.0, cut_fuse_grad=False, reg_type="omic")
        sd = W.make_state_dict(W.teacher_shapes(320), 3)
    opt.lambda_reg, opt.lambda_cox, opt.lambda_nll = (float(g[f"{task}_{k}"]) for k in ("lambda_reg", "lambda_cox", "lambda_nll"))
    model = m.define_net(opt, 1).cuda()
    model.load_state_dict(sd)
    return opt, model


def _close(got, ref, rel=1e-3):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and np.abs(got - ref).max() <= rel * max(np.abs(ref).max(), 1.0)


def test_test_teacher_surv_vs_reference_golden(golden_dir):
    """evaluate.test_teacher under surv against the reference's own train_test_MT.test() (make_golden_eval_stage1.py):
    losses and arrays within 1e-3; the C-index / p-value against float64 numpy / scipy restatements on the RETURNED arrays
    (a 1e-4 difference can flip a pair); the median-split accuracy equal to the reference's."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import evaluate as EV
    stats = pytest.importorskip("scipy.stats")
    g = np.load(os.path.join(golden_dir, "eval_stage1_b6_h64.npz"))
    m.set_precision("bf16x6")
    try:
        opt, model = _golden_eval_model(g, "surv")
        res = EV.test_teacher(opt, model, _golden_eval_loader(tuple(g["sizes"]), int(g["H"])), "cuda")
    finally:
        m.set_precision("bf16")
    assert len(res) == 16
    (loss_test, l_fuse, l_path, l_omic, c_fuse, c_path, c_omic, pval, acc, ga, gp, go, gm, pred_test, grads_test,
     feats_test) = res
    assert ga is None and gp is None and go is None and gm is None and grads_test == [None, None, None]
    for got, key in ((loss_test, "loss_test"), (l_fuse, "loss_fuse_test"), (l_path, "loss_path_test"),
                     (l_omic, "loss_omic_test")):
        assert _close(got, g["surv_" + key]), (key, got, float(g["surv_" + key]))
    for i, key in enumerate(("risk_pred_all", "risk_path_all", "risk_omic_all", "survtime_all", "censor_all")):
        assert _close(pred_test[i], g["surv_" + key]), key
    assert pred_test[5] is None and pred_test[6] is None and pred_test[7] is None
    assert np.array_equal(pred_test[8], g["surv_gt_all"])
    for i, key in enumerate(("feat_fuse_all", "feat_path_all", "feat_omic_all")):
        assert _close(feats_test[i], g["surv_" + key]), key
    risk, risk_path, risk_omic, st, ce = pred_test[:5]
    for h, c in ((risk, c_fuse), (risk_path, c_path), (risk_omic, c_omic)):
        comp, conc, tie = _np_counts(st, ce, h)
        assert abs(c - (conc + 0.5 * tie) / comp) <= 1e-12
    grp = risk > np.median(risk)
    x = stats.CensoredData(uncensored=st[~grp & (ce > 0)], right=st[~grp & (ce == 0)])
    y = stats.CensoredData(uncensored=st[grp & (ce > 0)], right=st[grp & (ce == 0)])
    assert abs(pval - stats.logrank(x, y, alternative="two-sided").pvalue) <= 1e-10
    assert acc == float(g["surv_surv_acc_test"])


def test_test_teacher_grad_vs_reference_golden(golden_dir):
    """evaluate.test_teacher under grad against the reference's train_test_MT.test(): losses, log-probabilities and features
    within 1e-3, the three accuracies exactly; the ranking metrics as in test_eval_loop (step functions of nearly tied,
    saturated scores: within 0.02, the micro-F1 exactly)."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import evaluate as EV
    g = np.load(os.path.join(golden_dir, "eval_stage1_b6_h64.npz"))
    m.set_precision("bf16x6")
    try:
        opt, model = _golden_eval_model(g, "grad")
        res = EV.test_teacher(opt, model, _golden_eval_loader(tuple(g["sizes"]), int(g["H"])), "cuda")
    finally:
        m.set_precision("bf16")
    assert len(res) == 16 and all(res[i] is None for i in range(4, 9))
    for got, key in ((res[0], "loss_test"), (res[1], "loss_fuse_test"), (res[2], "loss_path_test"), (res[3], "loss_omic_test")):
        assert _close(got, g["grad_" + key]), (key, got, float(g["grad_" + key]))
    for got, key in ((res[9], "grad_acc_test"), (res[10], "grad_path_test"), (res[11], "grad_omic_test")):
        assert got == float(g["grad_" + key]), key
    pred_test, feats_test = res[13], res[15]
    for i, key in ((5, "probs_all"), (6, "probs_path"), (7, "probs_omic")):
        assert _close(pred_test[i], g["grad_" + key]), key
    assert np.array_equal(pred_test[8], g["grad_gt_all"]) and pred_test[8].dtype == g["grad_gt_all"].dtype
    for i, key in enumerate(("feat_fuse_all", "feat_path_all", "feat_omic_all")):
        assert _close(feats_test[i], g["grad_" + key]), key
    got = np.asarray(res[12], dtype=np.float64)
    assert got.shape == (12,) and np.abs(got - g["grad_metrics"]).max() <= 0.02
    assert np.allclose(got[[2, 6, 10]], g["grad_metrics"][[2, 6, 10]], atol=1e-12)


def _eval_loader(B_list, seed=0):
    gen = torch.Generator().manual_seed(seed)
    batches = []
    for B in B_list:
        x_path = torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1
        x_omic = torch.randn(B, 320, generator=gen)
        censor = (torch.rand(B, generator=gen) > 0.4).float()
        survtime = torch.randint(1, 30, (B,), generator=gen).float()
        grade = torch.randint(0, 3, (B,), generator=gen)
        batches.append((x_path, torch.zeros(B), x_omic, censor, survtime, grade))
    return _Loader(batches, sum(B_list))


@pytest.mark.parametrize("task", ["surv", "grad"])
def test_test_teacher_has_no_per_batch_host_syncs(monkeypatch, task):
    """Per-batch outputs stay on the device: the number of .cpu() / .item() calls does not grow with the number of batches
    (3 against 6 batches) and is exactly the after-the-loop transfers of test_teacher."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import evaluate as EV
    from oracle import weights as W
    if task == "surv":
        opt = _surv_opt()
        sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    else:
        opt = m.stage2_opt(dropout_rate=0.0, reg_type="none")
        sd = W.make_state_dict(W.teacher_shapes(320), 3)
    model = m.define_net(opt, 1).cuda()
    model.load_state_dict(sd)
    calls = {"cpu": 0, "item": 0}
    real = {k: getattr(torch.Tensor, k) for k in calls}

    def counting(name):
        def f(self, *a, **k):
            calls[name] += 1
            return real[name](self, *a, **k)
        return f

    seen = []
    for nb in (3, 6):
        loader = _eval_loader([5] * (nb - 1) + [3], seed=nb)
        for k in calls:
            calls[k] = 0
        for k in calls:
            monkeypatch.setattr(torch.Tensor, k, counting(k))
        try:
            EV.test_teacher(opt, model, loader, "cuda")
        finally:
            for k in calls:
                monkeypatch.setattr(torch.Tensor, k, real[k])
        seen.append(dict(calls))
    # after the loop: losses, 3 feature arrays, labels; surv: the counts, 3 risk vectors, censor, time; grad: 3 probability arrays
    want = {"cpu": 11 if task == "surv" else 8, "item": 0}
    assert seen == [want, want], seen



# ------------------------------------------------------------------------------------------------ still raising
def test_surv_combinations_that_still_raise():
    import multimodal_learning_amd as m
    from multimodal_learning_amd import evaluate as EV
    for bad in (dict(tSVD_loss="True", n_views=2, tSVD_mode="path", mu=1.0), dict(masking=1),
                dict(act_type="LSM", label_dim=3), dict(label_dim=3)):
        opt = _surv_opt()
        for k, v in bad.items():
            setattr(opt, k, v)
        with pytest.raises(NotImplementedError):
            m.TeacherStage1Step(opt, device="cuda")

    class _Sync:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError):
        m.TeacherStage1Step(_surv_opt(), device="cuda", sync=_Sync())
    with pytest.raises(NotImplementedError):
        m.DistillStep(_surv_opt(), 64, device="cuda")
    with pytest.raises(NotImplementedError):
        EV.test(_surv_opt(), None, None, [], "cuda")
    with pytest.raises(NotImplementedError):
        m.TeacherStage1Step(m.stage2_opt(act_type="Sigmoid", label_dim=1), device="cuda")

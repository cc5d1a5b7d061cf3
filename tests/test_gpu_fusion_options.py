"""The fusion heads over their option set on the MI355X: BilinearFusion and PolynomialFusion with skip, linear gate, a gate
off and scaled widths, forward-only and taped, against the golden vectors of the reference's own classes
(tests/golden/fusion_options.npz) and the float64 restatement (tests/fusion_emulation.py); the stage-1 step with unused
fusion parameters and the stage-2 step with a skip / polynomial teacher.

Gradient tolerance, the dense rule of tests/test_gpu_dense.py: |device - float64 restatement| <= 4 x |float32 restatement -
float64 restatement| + FLOOR x scale, per recorded quantity (largest absolute difference).  The float32 restatement sums
the wide Linears in the kernels' split-K order.  `scale` is the largest |float64 value| of the quantity; for the bias of a
Linear in front of a BatchNorm, whose gradient is exactly zero in exact arithmetic (what any float32 evaluation returns
is the rounding residue of a sum of dY over the batch), it is the largest |gradient| of the case.  Against the golden (the
reference in float32) the same bound is widened by the reference's own recorded float32-vs-float64 distance.
FLOOR was measured on the MI355X against the float64 restatement: the largest excess of the device's error over the
float32 restatement's, in units of `scale`, is printed by every test as `excess[class]`; FLOOR is 4 x the largest seen
(the fusion-options section)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fusion_emulation as FE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fusion_options.npz")
# measured excess over the float32 restatement, in units of scale (see the module docstring), x 4.  Measured over the 19
# taped runs below: out 1.57e-6, loss 2.71e-6, dinput 2.80e-6, grad 7.50e-6, norm 4.74e-6, zero_bias 1.12e-6 (two BatchNorms
# over 4 or 7 rows amplify every rounding by the inverse of a small batch deviation: the float32 restatement itself sits
# 1e-6 .. 1e-5 of scale from the float64 one, and the device is another draw of the same rounding)
FLOOR = dict(out=6.3e-6, loss=1.1e-5, dinput=1.2e-5, grad=3.0e-5, norm=1.9e-5, zero_bias=4.5e-6)
EXCESS = {}


def _meta():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta_json"]))


_Z, _M = _meta()
CASES = {c["tag"]: c for c in _M["cases"]}
_REF = {}       # (tag, B) -> (float64 result, float32 split-K result): computed once, shared, never modified


def _inputs(case, B):
    w = case["width"]
    if B == 4:
        return tuple(torch.as_tensor(_Z["in_w%d_%s" % (w, n)]) for n in ("v1", "v2", "r"))
    g = torch.Generator().manual_seed(100 + B + w)
    return tuple(torch.randn(B, w, generator=g) for _ in range(3))


def _state_dict(case):
    from oracle import weights as W
    return W.make_state_dict({k: tuple(s) for k, s in case["shapes"]}, _M["weight_seed"])


def _module(case, dropout_rate=0.0):
    import multimodal_learning_amd as m
    cls = dict(bf=m.BilinearFusion, pf=m.PolynomialFusion)[case["kind"]]
    w = case["width"]
    net = cls(dim1=w, dim2=w, mmhid=w, dropout_rate=dropout_rate, **case["opts"])
    net.load_state_dict(_state_dict(case))
    return net.cuda().train()


def _reference(case, B):
    key = (case["tag"], B)
    if key not in _REF:
        v1, v2, r = _inputs(case, B)
        sd = _state_dict(case)
        q64 = FE.quantities(FE.run_case(case["kind"], case["opts"], sd, v1, v2, r), _M["sample_above"], _M["sample_n"])
        q32 = FE.quantities(FE.run_case(case["kind"], case["opts"], sd, v1, v2, r, dtype=torch.float32, splitk=True),
                            _M["sample_above"], _M["sample_n"])
        _REF[key] = (q64, q32)
    return _REF[key]


def _klass(k):
    if k in ("out", "loss"):
        return k
    if k in ("dv1", "dv2"):
        return "dinput"
    if k.startswith("gn_"):
        return "norm"
    if k.startswith("g_encoder") and k.endswith(".0.bias"):
        return "zero_bias"
    return "grad"


def _taped(case, B):
    net = _module(case)
    v1, v2, r = (t.cuda() for t in _inputs(case, B))
    v1.requires_grad_(True); v2.requires_grad_(True)
    out = net(v1, v2)
    loss = (out * r).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu(), loss=loss.detach().cpu(), dv1=v1.grad.cpu(), dv2=v2.grad.cpu(),
               grads={k: (None if p.grad is None else p.grad.cpu()) for k, p in net.named_parameters()})
    return res


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_only_vs_golden(tag):
    from tests.gpu_util import assert_close
    case = CASES[tag]
    net = _module(case)
    v1, v2, _ = _inputs(case, 4)
    with torch.no_grad():
        out = net(v1.cuda(), v2.cuda())
    assert tuple(out.shape) == (4, case["width"]) and not out.requires_grad
    assert_close(_Z[tag + "|out"], out, 1e-4, 1e-4, tag + " forward-only")


# B = 7 (an odd batch reaches the row tails) on one case per path: scaled widths with the vector tails, linear gate with
# skip, both gates off, bilinear gates without skip at scaled widths, the polynomial head
_B7 = ("bf_1111_2x4_w64", "bf_1011_1x1_w128", "bf_1000_1x1_w128", "bf_0011_2x4_w128", "pf_1111_1x1_w128")


@pytest.mark.parametrize("tag,B", [(t, 4) for t in CASES] + [(t, 7) for t in _B7])
def test_taped_vs_float64_restatement_and_golden(tag, B):
    from tests.gpu_util import Report
    case = CASES[tag]
    q64, q32 = _reference(case, B)
    res = _taped(case, B)
    assert sorted(k for k, g in res["grads"].items() if g is None) == sorted(case["none_grads"])
    q = FE.quantities(res, _M["sample_above"], _M["sample_n"])
    assert set(q) == set(q64)
    gscale = max(float(v.abs().max()) for k, v in q64.items() if k.startswith(("g_", "gs_")))
    R = Report("%s B=%d taped vs float64 restatement%s" % (tag, B, " and golden" if B == 4 else ""))
    for k, ref in q64.items():
        kl = _klass(k)
        sc = gscale if kl == "zero_bias" else float(ref.abs().max())
        e_dev = float((q[k].double() - ref).abs().max())
        e_rest = float((q32[k].double() - ref).abs().max())
        EXCESS[kl] = max(EXCESS.get(kl, 0.0), (e_dev - e_rest) / sc)
        tol = 4.0 * e_rest + FLOOR[kl] * sc
        R.add(k, e_dev, sc, tol)
        if B == 4:
            g = torch.as_tensor(_Z[tag + "|" + k]).double()
            R.add(k + " (golden)", float((q[k].double() - g.reshape(q[k].shape)).abs().max()), sc,
                  tol + case["ref_f32_vs_f64"][k])
    print("   " + "  ".join("excess[%s] = %.3e (floor %.1e)" % (kl, EXCESS[kl], FLOOR[kl]) for kl in sorted(EXCESS)))
    R.finish()


@pytest.mark.parametrize("tag", ["bf_1111_1x1_w128", "pf_1111_1x1_w128", "bf_1000_1x1_w128"])
def test_both_paths_draw_the_same_dropout_masks(tag):
    """dropout 0.25, equal seeds and counters: the forward-only and the taped forward agree bit for bit."""
    case = CASES[tag]
    v1, v2, _ = _inputs(case, 4)
    a, b = _module(case, 0.25), _module(case, 0.25)
    with torch.no_grad():
        ya = a(v1.cuda(), v2.cuda())
    yb = b(v1.cuda().requires_grad_(True), v2.cuda())
    assert yb.requires_grad and not ya.requires_grad
    assert a._rng_offset == b._rng_offset > 0
    assert float((ya == 0).float().mean()) > 0.1      # the last dropout zeroes a quarter of the ReLU's survivors
    assert torch.equal(ya, yb.detach())
    assert int(a.rng_step) == int(b.rng_step) == 1
    # a second call draws other masks, again the same on both paths
    with torch.no_grad():
        ya2 = a(v1.cuda(), v2.cuda())
    yb2 = b(v1.cuda().requires_grad_(True), v2.cuda())
    assert torch.equal(ya2, yb2.detach()) and not torch.equal(ya, ya2)


def test_default_options_are_bitwise_what_the_parent_commit_gives(golden_dir):
    """fusion_default_parent_bits.npz was written on the MI355X by the commit before the option set was built (which ran
    the default options alone): BilinearFusion(skip=0, use_bilinear=1, gate1=1, gate2=1, 128, 128, 128) with the `fusion.`
    tensors of make_state_dict(teacher_shapes(320), 3), train mode, on fus_in1 / fus_in2 of modules_b4_h64.npz -
    the forward-only output at dropout 0 and 0.25, the taped output and both input gradients of sum(out * out)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    g = np.load(os.path.join(golden_dir, "modules_b4_h64.npz"))
    bits = np.load(os.path.join(golden_dir, "fusion_default_parent_bits.npz"))
    sd = {k[len("fusion."):]: v for k, v in W.make_state_dict(W.teacher_shapes(320), 3).items() if k.startswith("fusion.")}
    v1, v2 = torch.as_tensor(g["fus_in1"]).cuda(), torch.as_tensor(g["fus_in2"]).cuda()

    def net(p):
        f = m.BilinearFusion(skip=0, use_bilinear=1, gate1=1, gate2=1, dim1=128, dim2=128, mmhid=128, dropout_rate=p)
        f.load_state_dict(sd)
        return f.cuda().train()

    def same(name, t):
        assert np.array_equal(t.detach().cpu().numpy().view(np.int32), bits[name].view(np.int32)), name

    with torch.no_grad():
        same("fwd_p0", net(0.0)(v1, v2))
        same("fwd_p25", net(0.25)(v1, v2))
    a, b = v1.clone().requires_grad_(True), v2.clone().requires_grad_(True)
    out = net(0.0)(a, b)
    (out * out).sum().backward()
    same("taped_p0", out); same("taped_dv1", a.grad); same("taped_dv2", b.grad)


def test_stage1_step_with_unused_fusion_parameters_vs_reference_golden(golden_dir):
    """TeacherStage1Step with --skip 1 --use_bilinear 0 --omic_gate 0 against two steps of the reference's own modules
    (tests/golden/make_golden_stage1_fusion_options.py), tolerances of test_stage1_teacher_step_vs_reference_golden.  The
    student's unused tensors stay bitwise what they were; their EMA copies follow update_ema_variables."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch
    g = np.load(os.path.join(golden_dir, "stage1_fusion_options_b4_h64.npz"))
    m.set_precision("bf16x6")
    try:
        opt = m.stage2_opt(dropout_rate=0.0, batch_size=4, cut_fuse_grad=False, num_teachers=2, skip=1, use_bilinear=0,
                           omic_gate=0, reg_type=str(g["reg_type"]))
        opt.pred_distill, opt.KD_weight = 1, float(g["KD_weight"])
        opt.lr, opt.weight_decay, opt.ema_decay = float(g["lr"]), float(g["weight_decay"]), float(g["ema_decay"])
        model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd, esd0 = W.make_state_dict(shapes, int(g["weight_seed"])), W.make_state_dict(shapes, int(g["ema_weight_seed"]))
        model.load_state_dict(sd); ema.load_state_dict(esd0)
        st = m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()))
        names = dict(st.model.named_parameters())
        assert sorted(k for k, p in names.items() if id(p) in st._unused_ids) == sorted(g["none_grads"])
        lr = float(g["lr"])
        for it in range(2):
            bt = synthetic_batch(4, 64, seed=20 + it)
            z = torch.zeros(4)
            out = st.step(((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"]))
            tol = 1e-3 if it == 0 else 5e-2
            for k in ("loss", "loss_nll"):
                assert abs(out[k].item() - float(g[f"{k}{it}"])) <= tol * abs(float(g[f"{k}{it}"])), (it, k, out[k].item())
            kd_tol = tol if it == 0 else 0.25
            assert abs(out["loss_pred_KD"].item() - float(g[f"loss_kd{it}"])) <= kd_tol * max(abs(float(g[f"loss_kd{it}"])), 1e-2)
            for k in ("pred", "pred_path", "pred_omic"):
                assert np.abs(out[k].cpu().numpy() - g[f"{k}{it}"]).max() <= tol * 10, (it, k)
            msd, esd = st.model.state_dict(), st.ema_model.state_dict()
            for name in g["unused"]:
                # no gradient, no Adam step, no weight decay: the student tensor is bitwise the loaded one
                assert torch.equal(msd[name].cpu(), sd[name]), (it, name)
                assert np.array_equal(g[f"w{it}_{name}"], sd[name].numpy()), name
                # the EMA copy: alpha * ema + (1 - alpha) * student, alpha = min(1 - 1 / (step + 1), ema_decay)
                assert np.abs(esd[name].cpu().numpy() - g[f"e{it}_{name}"]).max() <= 1e-6, (it, name)
            if it == 0:
                for name in g["used"]:
                    # Adam's first step moves every weight by ~lr * sign(g): compare the update, not the weight
                    upd_ref = g[f"w0_{name}"] - sd[name].numpy()
                    upd = msd[name].cpu().numpy() - sd[name].numpy()
                    assert float((np.abs(upd - upd_ref) > 0.2 * lr).mean()) < 0.02, name
                    assert float((np.abs(esd[name].cpu().numpy() - g[f"e0_{name}"]) > 0.2 * lr).mean()) < 0.02, name
        # replayed from captured graphs the unused tensors are treated the same: the EMA update of their segments is part of
        # the captured step and reads its rate from device memory
        st.enable_graph()
        for it in range(2, 4):
            before = {n: st.ema_model.state_dict()[n].clone() for n in g["unused"]}
            bt = synthetic_batch(4, 64, seed=20 + it)
            z = torch.zeros(4)
            st.step(((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"]))
            torch.cuda.synchronize()
            a = min(1 - 1 / (it + 1), opt.ema_decay)
            msd, esd = st.model.state_dict(), st.ema_model.state_dict()
            for name in g["unused"]:
                assert torch.equal(msd[name].cpu(), sd[name]), (it, name)
                want = a * before[name].double() + (1 - a) * msd[name].double()
                assert (esd[name].double() - want).abs().max().item() <= 1e-6, (it, name)
        assert st._want_graph and len(st._g_sets) == 1 and st._g_sets[0]["graph"] is not None, "no captured graph"
    finally:
        m.set_precision("bf16")


@pytest.mark.parametrize("extra", [dict(skip=1), dict(fusion_type="polynomial_fusion")], ids=["skip", "polynomial"])
def test_distill_step_with_an_option_teacher_eager_and_replayed(extra):
    """DistillStep (miccai2022, B = 4, 64 x 64) with a frozen teacher built with skip = 1 / the polynomial head: five eager
    steps and two eager + three replayed steps give bitwise equal losses and student weights, a graph exists, and the
    teacher's fuse_feat is bitwise the standalone module's forward on the same feature rows."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.losses import CRDState
    from oracle.step import synthetic_batch
    from tests.test_gpu_step import _tuple
    n_data = 256
    m.set_precision("bf16")
    runs = []
    for graph in (False, True):
        torch.manual_seed(0); np.random.seed(2019)
        opt = m.stage2_opt(dropout_rate=0.0, batch_size=4, nce_p=120, nce_k=200, nce_p2=20, nce_k2=128, **extra)
        step = m.DistillStep(opt, n_data, device="cuda")
        step.model.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
        step.ema_model.load_state_dict(W.make_state_dict(W.student_shapes(), 2))
        shapes = {k: tuple(v.shape) for k, v in step.fix_model.state_dict().items()}
        step.fix_model.load_state_dict(W.make_state_dict(shapes, 3))
        for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
            crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 10 + 2 * i))
            crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 11 + 2 * i))
            st = CRDState(n_data, opt.feat_dim, opt.nce_p, opt.nce_k, seed=20 + i)
            crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
            crd.contrast.verbose = False
        fus = step.fix_model.fusion
        assert type(fus) is (m.PolynomialFusion if "fusion_type" in extra else m.BilinearFusion) and fus.skip == opt.skip
        rng = np.random.RandomState(5)
        ranks = [[rng.choice(np.arange(30, 100), opt.nce_p2, replace=False) for _ in range(2)] for _ in range(5)]
        bts = [synthetic_batch(4, 64, n_data=n_data, P=opt.nce_p, K=opt.nce_k, seed=s) for s in range(2)]
        seen = {}
        hook = fus.register_forward_hook(lambda mod, inp, out: seen.update(v1=inp[0].clone(), v2=inp[1].clone()))
        losses = []
        for it in range(5):
            if it == 1:
                hook.remove()
            if graph and it == 2:
                step.enable_graph()
            out = step.step(_tuple(bts[it % 2]), epoch=1, ranks=ranks[it])
            losses.append(out["loss"].clone())
            if it == 0:
                twin = type(fus)(skip=opt.skip, use_bilinear=opt.use_bilinear, gate1=opt.path_gate, gate2=opt.omic_gate,
                                 dim1=opt.path_dim, dim2=opt.omic_dim, scale_dim1=opt.path_scale, scale_dim2=opt.omic_scale,
                                 mmhid=opt.mmhid, dropout_rate=opt.dropout_rate)
                twin.load_state_dict(fus.state_dict())
                with torch.no_grad():
                    alone = twin.cuda().train()(seen["v1"], seen["v2"])
                assert torch.equal(alone, out["fuse_feat"])
        torch.cuda.synchronize()
        if graph:
            assert step._static is not None and step._static["graph"] is not None, "graph path was not taken"
        runs.append((torch.stack(losses).cpu(), step.optimizer.flat.flat.detach().cpu().clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])

"""The general-depth BasicBlock trunk on the GPU, at ResNet-34 depth [3, 4, 6, 3]: parity against golden vectors produced by RUNNING
the reference's ResNet(BasicBlock, [3, 4, 6, 3]) (tests/golden/make_golden_resnet34.py), the two-part and one-stream backward, the
forward-only fused form, perf mode against parity mode, the distillation step with a ResNet-34 in it, and a state_dict round trip.

Tolerances of the golden comparison: the bounds tests/test_gpu_resnet.py holds ResNet-18 to - 1e-3 absolute on forwards,
(1e-4, 1e-2) on gradients, (1e-5, 1e-4) on running statistics - plus 4 x the golden's OWN error for that quantity, max |float32 run -
float64 run| of the reference module, which the golden files carry (the rule of the operator sweeps; DESIGN.md has the figures)."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R34 = [3, 4, 6, 3]
GOLDEN = {"b4_h64": "resnet34_b4_h64.npz", "b3_96x160": "resnet34_b3_96x160.npz"}
_cache = {}


def _golden(golden_dir, case):
    if case not in _cache:
        _cache[case] = dict(np.load(os.path.join(golden_dir, GOLDEN[case])))
    return _cache[case]


def _shapes(g):
    return {str(k): tuple(int(d) for d in str(s).split(",") if d) for k, s in zip(g["keys"], g["shapes"])}


def _resnet34(golden_dir, seed=None):
    """A ResNet-34 student with the golden's weight recipe (oracle.weights.make_state_dict over the reference module's own shapes)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    g = _golden(golden_dir, "b4_h64")
    net = m.ResNet34(pretrained=False, path_dim=128, act=m.define_act_layer(act_type="LSM"), num_classes=3)
    net.load_state_dict(W.make_state_dict(_shapes(g), int(g["weight_seed"]) if seed is None else seed))
    return net.cuda().train()


def _resnet18():
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    net = m.define_net(default_opt(), 1, path_only=True)
    net.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    return net.cuda().train()


def _crop_batch(B, H, W, seed):
    """The golden script's input recipe: the top-left H x W window of a square synthetic batch."""
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, max(H, W), seed=seed)
    return bt["x_path"][:, :, :H, :W].contiguous(), bt["grade"]


def _row(R, g, key, got, atol, rtol, what):
    """One comparison with the float32 golden at atol + rtol * max|ref| + 4 x (the golden's own float32 - float64 error)."""
    from tests.gpu_util import maxerr
    ref = g[key]
    if key + "__f64err" in g:
        e64 = float(g[key + "__f64err"])
    else:
        e64 = float(np.abs(ref.astype(np.float64) - g[key + "__f64"]).max())
    err, mx = maxerr(ref, got)
    R.add("%s [golden f32-f64 %.1e]" % (what, e64), err, mx, atol + rtol * mx + 4.0 * e64)


# state_dict key of a stored gradient -> golden key (make_golden_resnet34.py GRADS)
_GRADS = (("fc_new2.weight", "g_fc2_w"), ("fc_new1.0.weight", "g_fc1_w"), ("layer4.2.bn2.weight", "g_l4_2_bn2_w"),
          ("layer3.1.conv2.weight", "g_l3_1_conv2"), ("layer2.0.downsample.0.weight", "g_l2_0_ds"),
          ("layer1.0.conv1.weight", "g_l1_0_conv1"), ("bn1.weight", "g_bn1_w"), ("conv1.weight", "g_conv1"),
          ("layer1.2.conv1.weight", "g_l1_2_conv1"), ("layer2.3.bn2.weight", "g_l2_3_bn2_w"),
          ("layer3.4.conv1.weight", "g_l3_4_conv1"), ("layer3.5.bn2.weight", "g_l3_5_bn2_w"),
          ("layer3.5.bn2.bias", "g_l3_5_bn2_b"), ("layer4.2.conv2.weight", "g_l4_2_conv2"))


@pytest.mark.parametrize("case", ["b4_h64", "b3_96x160"])
@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3"])
def test_resnet34_parity_mode_vs_reference_golden(golden_dir, pmode, case):
    """Train forward, gradients, running statistics, eval forward and the eval-mode image gradient (the half-pair mode takes that one
    in the split-plane arithmetic, as for ResNet-18) against the reference's ResNet(BasicBlock, [3, 4, 6, 3])."""
    import multimodal_learning_amd as m
    from tests.gpu_util import Report
    g = _golden(golden_dir, case)
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    x, grade = _crop_batch(B, H, W, int(g["batch_seed"]))
    m.set_precision(pmode)
    R = Report(f"ResNet-34 fwd/bwd, {pmode} vs reference golden (B={B}, {H}x{W})")
    try:
        net = _resnet34(golden_dir)
        assert len(net._units()) == 36
        out = net(x_path=x.cuda())
        assert len(out) == 5 and out[4] is None
        f3, feat, hazard, pred, _ = out
        for key, t in (("f3", f3), ("feat", feat), ("hazard", hazard), ("pred", pred)):
            _row(R, g, key, t, 1e-3, 0, key)
        loss = (feat * torch.linspace(0.5, 1.5, 128).cuda()).sum() + (hazard * torch.tensor([1.0, -2.0, 0.5]).cuda()).sum() \
            + 0.1 * f3.sum()
        loss.backward()
        P = dict(net.named_parameters())
        for key, name in _GRADS:
            gr = P[key].grad
            if name in g:
                _row(R, g, name, gr, 1e-4, 1e-2, "g " + key)
            else:      # (large weight gradients are stored as sums; the abs-sum at the ResNet-18 test's bound for one)
                _row(R, g, name + "_abs", gr.abs().sum(), 1e-3, 1e-2, "g |" + key + "|")
        sd = net.state_dict()
        for key, name in (("bn1.running_mean", "rm_bn1"), ("bn1.running_var", "rv_bn1"), ("layer4.2.bn2.running_mean", "rm_l4"),
                          ("layer4.2.bn2.running_var", "rv_l4")):
            _row(R, g, name, sd[key], 1e-5, 1e-4, key)
        assert int(sd["bn1.num_batches_tracked"]) == 1 and int(sd["layer3.5.bn2.num_batches_tracked"]) == 1
        # eval mode after that step: running statistics, no autograd graph
        net.eval()
        rm = net.layer3[4].bn1.running_mean.clone()
        e = net(x_path=x.cuda())
        assert not e[2].requires_grad and torch.equal(rm, net.layer3[4].bn1.running_mean)
        for key, t in (("eval_f3", e[0]), ("eval_feat", e[1]), ("eval_hazard", e[2]), ("eval_pred", e[3])):
            _row(R, g, key, t, 1e-3, 0, key)
        # the image gradient of the eval-mode NLL
        xg = x.clone().cuda().requires_grad_(True)
        nll = m.ops.NLLFn.apply(net(x_path=xg)[3], grade.cuda(), float(B))
        nll.backward()
        _row(R, g, "eval_nll", nll.detach(), 1e-3, 0, "eval NLL")
        _row(R, g, "eval_dx", xg.grad, 1e-4, 1e-2, "eval d NLL / d image")
        R.finish()
    finally:
        m.set_precision("bf16")


def _unit_in_part0(net):
    """Per C-ABI unit: True where it belongs to layer 3 or 4 (what ph_resnet_backward_part's part 0 finishes)."""
    flags = [False]
    for li, layer in enumerate((net.layer1, net.layer2, net.layer3, net.layer4)):
        for blk in layer:
            flags += [li >= 2] * (3 if blk.downsample is not None else 2)
    return flags


@pytest.mark.parametrize("B,H,W", [(4, 64, 64), (3, 96, 160)])
def test_resnet34_two_part_and_one_stream_backward(golden_dir, B, H, W):
    """Layers 3 + 4 of a ResNet-34 are 9 blocks (odd: part 1 finds the block gradient in the other ping-pong buffer than in a
    ResNet-18).  On one forward's workspace, perf mode: part 0 then part 1 leave bitwise the gradients of the whole backward; after part 0
    alone the gradients of layers 3 and 4 are final and nothing else has been written; the one-stream backward gives the BatchNorm
    gradients bit for bit and the weight gradients up to the fp32 summation order (the rule of test_two_stream_backward_equals_one_stream)."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import ops
    from multimodal_learning_amd._lib import lib, check, ptr, stream
    m.set_precision("bf16")
    net = _resnet34(golden_dir)
    x, _ = _crop_batch(B, H, W, 11)
    f3, feat, hazard, pred, _ = net(x_path=x.cuda())
    plan, ws = net._get_plan(B, H, W), f3.grad_fn.ws
    assert ws is not None and ws.numel() == plan.ws_bytes and plan.layers == (3, 4, 6, 3)
    packed, table = net._get_packed(plan), net._param_table()
    gen = torch.Generator(device="cuda").manual_seed(5)
    g3 = torch.randn(B, 256, device="cuda", generator=gen)
    g4 = torch.randn(B, 512, device="cuda", generator=gen)
    params = net._trunk_params()
    in0 = [f for f in _unit_in_part0(net) for _ in range(3)]
    assert len(in0) == len(params) == 108

    def buffers():
        bufs = [torch.full_like(p, float("nan")) for p in params]
        return bufs, ops.void_array([b.data_ptr() for b in bufs])

    def part(gptrs, which):
        check(lib().ph_resnet_backward_part(plan.h, table, ptr(packed), ptr(ws), ptr(g3), ptr(g4), gptrs, which, stream()), "backward_part")
        torch.cuda.synchronize()

    whole, gp = buffers()
    part(gp, -1)
    assert all(torch.isfinite(t).all() for t in whole)
    again, gp = buffers()
    part(gp, -1)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "the backward is not re-runnable on one forward's workspace"
    split, gp = buffers()
    part(gp, 0)
    for i, (a, b) in enumerate(zip(whole, split)):
        if in0[i]:
            assert torch.equal(a, b), ("after part 0", i)
        else:
            assert torch.isnan(b).all(), ("part 0 wrote a gradient of layers 1-2 / the stem", i)
    part(gp, 1)
    for i, (a, b) in enumerate(zip(whole, split)):
        assert torch.equal(a, b), ("after part 1", i)
    try:
        check(lib().ph_resnet_plan_set_backward_overlap(plan.h, 0), "set_backward_overlap")
        one, gp = buffers()
        part(gp, -1)
    finally:
        check(lib().ph_resnet_plan_set_backward_overlap(plan.h, 1), "set_backward_overlap")
    nbit = 0
    for a, b in zip(one, whole):
        if a.dim() == 4:
            assert (a - b).abs().max() <= 2e-5 * a.abs().max() + 1e-12, ((a - b).abs().max() / a.abs().max()).item()
        else:
            assert torch.equal(a, b)
            nbit += 1
    assert nbit == 72
    del f3, feat, hazard, pred


def test_captured_backward_of_a_depth_no_eager_call_has_run_stays_on_one_stream():
    """The side stream's event blocks grow to a plan's need outside stream captures only.  A backward captured for a depth that no eager
    two-stream call has run yet in this process ([3, 4, 7, 3]: 38 units, used by no other test) finds the captures' block too small and
    runs on the caller's stream: replayed, it gives the one-stream backward's gradients bit for bit, weight gradients included (which
    the two-stream form may sum from other chunks).  After one eager two-stream call of that depth a capture may take the side stream
    again and is held to the two-stream rule."""
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    depths = [3, 4, 7, 3]
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda()

    def build():
        net = m.ResNet(m.BasicBlock, depths, path_dim=128, act=m.define_act_layer(act_type="LSM"), num_classes=3)
        return _load_recipe(net, 9).cuda().train()

    def run(net):
        for p in net.parameters():
            p.grad = None
        f3, feat, hazard, pred, _ = net(x_path=x)
        (feat.square().mean() + hazard.sum() + f3.sum()).backward()

    def captured(net):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            run(net)
        for p in net.parameters():
            if p.grad is not None:
                p.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters() if p.grad is not None]

    _resnet18_fwd_bwd_once()      # (the side stream and its blocks exist: created by the first eager two-stream backward of the process)
    one = build()
    one._no_bwd_overlap = True
    run(one)
    torch.cuda.synchronize()
    ref = [p.grad.clone() for p in one.parameters() if p.grad is not None]
    assert len(ref) == 3 * 38 + 6 and all(torch.isfinite(t).all() for t in ref)
    got = captured(build())
    assert len(got) == len(ref)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    # an eager two-stream call of this depth grows the blocks; a capture after it replays finite gradients within the two-stream rule
    two = build()
    run(two)
    torch.cuda.synchronize()
    again = captured(two)
    for a, b in zip(ref, again):
        if a.dim() == 4:
            assert (a - b).abs().max() <= 2e-5 * a.abs().max() + 1e-12
        else:
            assert torch.equal(a, b)


def _resnet18_fwd_bwd_once():
    net = _resnet18()
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    out = net(x_path=x)
    (out[1].square().mean() + out[2].sum()).backward()
    torch.cuda.synchronize()


def test_resnet34_fused_forward_only_equals_separate_passes(golden_dir):
    """Forward-only ResNet-34 (flag bit 2: conv2 of the 64- and 128-channel blocks applies bn1 + ReLU while it stages its input, the stem
    pools its raw output) against the separate passes (bit 3), train and eval mode: bitwise, the rule of
    test_fused_input_batchnorm_equals_separate_pass."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    x = synthetic_batch(3, 96, seed=31)["x_path"].cuda()
    for training in (True, False):
        outs = {}
        for no_fuse in (True, False, False):
            net = _resnet34(golden_dir)
            net.train(training)
            net._no_fuse = no_fuse
            with torch.no_grad():
                f3, feat, hazard, pred, _ = net(x_path=x)
            key = "separate" if no_fuse else ("fused" if "fused" not in outs else "fused again")
            outs[key] = (f3.clone(), feat.clone(), hazard.clone(), {k: v.clone() for k, v in net.state_dict().items() if "running" in k})
        assert len(outs["separate"][3]) == 2 * 36 + 2
        for other in ("fused", "fused again"):
            for a, b in zip(outs["separate"][:3], outs[other][:3]):
                assert torch.equal(a, b), (training, other, (a - b).abs().max().item())
            for k, v in outs["separate"][3].items():
                assert torch.equal(v, outs[other][3][k]), (training, k)
        assert torch.isfinite(outs["fused"][2]).all()


def test_resnet34_perf_mode_error_grows_at_most_linearly_in_depth(golden_dir):
    """Relative L2 error of the perf-mode (bf16) features against the parity mode (bf16x6), ResNet-34 against ResNet-18 on the same
    batch: a chain of bf16 layers accumulates rounding at most linearly in its depth - sixteen blocks against eight is a factor of 2 -
    so ResNet-34's error is held to 3 x ResNet-18's."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    x = synthetic_batch(16, 128, seed=3)["x_path"].cuda()
    rel = {}
    try:
        for name, build in (("resnet18", _resnet18), ("resnet34", lambda: _resnet34(golden_dir))):
            feats = {}
            for mode in ("bf16x6", "bf16"):
                m.set_precision(mode)
                with torch.no_grad():
                    feats[mode] = build()(x_path=x)[1].double()
            rel[name] = ((feats["bf16"] - feats["bf16x6"]).norm() / feats["bf16x6"].norm()).item()
    finally:
        m.set_precision("bf16")
    print("\nperf mode vs parity mode, relative L2 error of the features: ResNet-18 %.4e, ResNet-34 %.4e, ratio %.2f"
          % (rel["resnet18"], rel["resnet34"], rel["resnet34"] / rel["resnet18"]))
    assert np.isfinite(rel["resnet34"]) and rel["resnet18"] > 0
    assert rel["resnet34"] <= 3.0 * rel["resnet18"], rel


def _load_recipe(net, seed):
    from oracle import weights as W
    net.load_state_dict(W.make_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed))
    return net


@pytest.mark.parametrize("variant", ["path_arch", "mixed"])
def test_distill_step_with_a_resnet34_replays_like_eager(variant):
    """DistillStep at B = 8, 64 x 64, perf mode: with opt.path_arch = "resnet34" (three 36-unit trunks) and with a ResNet-34 teacher
    encoder beside a ResNet-18 student and EMA (models=...).  Five steps on two batches, replayed from captured graphs against the same
    steps launched eagerly: the losses and the updated student bit for bit, as the ResNet-18 steps of tests/test_gpu_step_graph.py and
    test_option_branch_replays_from_a_captured_graph.  The default opt still builds three 20-unit trunks."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.losses import CRDState
    from oracle.step import default_opt, synthetic_batch
    from tests.test_gpu_step import _tuple
    m.set_precision("bf16")
    n_data = 1024
    d = m.DistillStep(default_opt(batch_size=8), n_data, device="cuda")
    assert [len(n._units()) for n in (d.fix_model.path_net, d.model, d.ema_model)] == [20, 20, 20]
    del d
    o34, o18 = default_opt(batch_size=8, path_arch="resnet34"), default_opt(batch_size=8)
    rng = np.random.RandomState(5)
    ranks = [[rng.choice(np.arange(30, 100), 20, replace=False) for _ in range(2)] for _ in range(5)]
    bts = [_tuple(synthetic_batch(8, 64, seed=60 + i)) for i in range(2)]

    def run(graph):
        if variant == "path_arch":
            step = m.DistillStep(o34, n_data, device="cuda")
            want = [36, 36, 36]
        else:
            nets = (m.define_net(o34, 1), m.define_net(o18, 1, path_only=True), m.define_net(o18, 1, path_only=True))
            step = m.DistillStep(o18, n_data, device="cuda", models=tuple(n.cuda() for n in nets))
            want = [36, 20, 20]
        assert [len(n._units()) for n in (step.fix_model.path_net, step.model, step.ema_model)] == want
        for net, seed in ((step.model, 1), (step.ema_model, 2), (step.fix_model, 3)):
            _load_recipe(net, seed)
        for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
            crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 10 + 2 * i))
            crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 11 + 2 * i))
            st = CRDState(n_data, o18.feat_dim, o18.nce_p, o18.nce_k, seed=20 + i)
            crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
            crd.contrast.verbose = False
        if graph:
            step.enable_graph()
        losses = []
        for it in range(5):
            losses.append(step.step(bts[it % 2], epoch=1, ranks=ranks[it])["loss"].clone())
        torch.cuda.synchronize()
        if graph:
            assert step._want_graph and step._slots and step._slots[0]["graph"] is not None, "the step was not captured"
        return torch.stack(losses).cpu(), {k: v.clone() for k, v in step.model.state_dict().items()}, \
            {k: v.clone() for k, v in step.ema_model.state_dict().items()}

    le, se, ee = run(False)
    lg, sg, eg = run(True)
    assert torch.isfinite(le).all()
    assert torch.equal(le, lg), (le, lg)
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    for k in ee:
        assert torch.equal(ee[k], eg[k]), k


def test_resnet34_state_dict_round_trip(golden_dir):
    """Saved and loaded into a fresh ResNet34, the state_dict (torchvision's keys: layer3.5.bn2.weight, ...) gives the identical forward."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    x = synthetic_batch(2, 64, seed=2)["x_path"].cuda()
    a = _resnet34(golden_dir)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    b = m.ResNet34(pretrained=False, path_dim=128, act=m.define_act_layer(act_type="LSM"), num_classes=3).cuda()
    missing = b.load_state_dict(torch.load(buf), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert "layer3.5.bn2.weight" in b.state_dict() and "layer4.2.conv2.weight" in b.state_dict()
    for training in (False, True):
        a.train(training); b.train(training)
        with torch.no_grad():
            oa, ob = a(x_path=x), b(x_path=x)
        for u, v in zip(oa[:4], ob[:4]):
            assert torch.equal(u, v), training

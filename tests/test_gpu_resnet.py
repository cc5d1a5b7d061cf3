"""Parity of the drop-in ResNet (student) and PathomicNet (teacher) modules on the GPU:
  * parity mode vs the golden vectors produced by RUNNING the reference (tests/golden/modules_b4_h64.npz):
    logits/features within 1e-3 (the north-star tolerance), gradients within 2e-3 relative
  * perf mode (bf16) vs the oracle run with the same operand/activation rounding: logits within 1e-3."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _student(seed=1):
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    net = m.define_net(default_opt(), 1, path_only=True)
    net.load_state_dict(W.make_state_dict(W.student_shapes(), seed))
    return net.cuda().train()


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3"])
def test_student_forward_backward_parity_mode(golden_dir, pmode):
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    from tests.gpu_util import assert_close, Report
    g = np.load(os.path.join(golden_dir, "modules_b4_h64.npz"))
    m.set_precision(pmode)
    R = Report("student fwd/bwd, parity mode vs reference golden (B=4, 64x64)")
    assert_close = R.close
    try:
        net = _student()
        bt = synthetic_batch(int(g["B"]), int(g["H"]), seed=int(g["batch_seed"]))
        out = net(x_path=bt["x_path"].cuda())
        assert len(out) == 5 and out[4] is None
        f3, feat, hazard, pred, _ = out
        assert_close(g["f3"], f3, 1e-3, 0, "f3"); assert_close(g["feat"], feat, 1e-3, 0, "features")
        assert_close(g["hazard"], hazard, 1e-3, 0, "hazard"); assert_close(g["pred"], pred, 1e-3, 0, "pred")
        loss = (feat * torch.linspace(0.5, 1.5, 128).cuda()).sum() + (hazard * torch.tensor([1.0, -2.0, 0.5]).cuda()).sum() \
            + 0.1 * f3.sum()
        loss.backward()
        P = dict(net.named_parameters())
        assert_close(g["g_fc2_w"], P["fc_new2.weight"].grad, 1e-4, 1e-2, "g fc2")
        assert_close(g["g_fc1_w"], P["fc_new1.0.weight"].grad, 1e-4, 1e-2, "g fc1")
        assert_close(g["g_l4_1_bn2_w"], P["layer4.1.bn2.weight"].grad, 1e-4, 1e-2, "g l4.1.bn2")
        assert_close(g["g_l3_1_conv2_abs"], P["layer3.1.conv2.weight"].grad.abs().sum(), 1e-3, 1e-2, "g l3.1.conv2")
        assert_close(g["g_l2_0_ds"], P["layer2.0.downsample.0.weight"].grad, 1e-4, 1e-2, "g l2.0.ds")
        assert_close(g["g_l1_0_conv1"], P["layer1.0.conv1.weight"].grad, 1e-4, 1e-2, "g l1.0.conv1")
        assert_close(g["g_bn1_w"], P["bn1.weight"].grad, 1e-4, 1e-2, "g bn1")
        assert_close(g["g_conv1"], P["conv1.weight"].grad, 1e-4, 1e-2, "g conv1")
        sd = net.state_dict()
        assert_close(g["rm_bn1"], sd["bn1.running_mean"], 1e-5, 1e-4, "bn1 running_mean")
        assert_close(g["rv_bn1"], sd["bn1.running_var"], 1e-5, 1e-4, "bn1 running_var")
        assert_close(g["rm_l4"], sd["layer4.1.bn2.running_mean"], 1e-5, 1e-4, "l4 running_mean")
        assert_close(g["rv_l4"], sd["layer4.1.bn2.running_var"], 1e-5, 1e-4, "l4 running_var")
        assert int(sd["bn1.num_batches_tracked"]) == 1
        R.finish()
    finally:
        m.set_precision("bf16")


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3"])
def test_student_non_square_maps_two_shapes(pmode):
    """Non-square maps through the whole network: a student forward and backward at B = 3, 72 x 120 and then 120 x 72 ON THE SAME
    NET (no weight update in between: the second plan reuses the packed weights of the first) against oracle.resnet_forward in
    float64, at the tolerances of test_student_forward_backward_parity_mode.  In half-pair mode the packed weights carry
    fragment-major layouts for some units: a plan that read them with another layout would be off by O(1)."""
    import multimodal_learning_amd as m
    import oracle
    from oracle import weights as W
    from tests.gpu_util import Report
    m.set_precision(pmode)
    R = Report(f"student fwd/bwd, {pmode}, non-square maps vs float64 oracle (B=3)")
    try:
        net = _student()
        for H, Wd in ((72, 120), (120, 72)):
            g = torch.Generator().manual_seed(H)
            x = torch.rand(3, 3, H, Wd, generator=g) * 2 - 1
            for p in net.parameters():
                p.grad = None
            f3, feat, hazard, pred, _ = net(x_path=x.cuda())
            wf, wh = torch.linspace(0.5, 1.5, 128), torch.tensor([1.0, -2.0, 0.5])
            ((feat * wf.cuda()).sum() + (hazard * wh.cuda()).sum() + 0.1 * f3.sum()).backward()
            sd = {k: v.double() for k, v in W.make_state_dict(W.student_shapes(), 1).items()}
            names = ["fc_new2.weight", "fc_new1.0.weight", "layer4.1.bn2.weight", "layer3.1.conv2.weight",
                     "layer2.0.downsample.0.weight", "layer1.0.conv1.weight", "layer1.1.conv2.weight", "bn1.weight", "conv1.weight"]
            for k in names:
                sd[k].requires_grad_(True)
            rf3, rfeat, rhaz, rpred, _ = oracle.resnet_forward(x.double(), sd)
            ((rfeat * wf.double()).sum() + (rhaz * wh.double()).sum() + 0.1 * rf3.sum()).backward()
            tag = f"{H}x{Wd}"
            R.close(rf3.detach(), f3, 1e-3, 0, f"f3 {tag}"); R.close(rfeat.detach(), feat, 1e-3, 0, f"features {tag}")
            R.close(rhaz.detach(), hazard, 1e-3, 0, f"hazard {tag}"); R.close(rpred.detach(), pred, 1e-3, 0, f"pred {tag}")
            P = dict(net.named_parameters())
            for k in names:
                R.close(sd[k].grad, P[k].grad, 1e-4, 1e-2, f"g {k} {tag}")
        R.finish()
    finally:
        m.set_precision("bf16")


def test_student_forward_perf_mode_noise_floor():
    """Perf mode (single-pass bf16) cannot meet 1e-3 on an untrained BN network - nor can ANY bf16 arithmetic:
    one bf16 ulp flipped by a different fp32 summation order is amplified by the 17 train-mode BN layers.
    What is asserted: the HIP path's deviation from the fp32 oracle is no larger than the deviation of the
    oracle's own bf16 emulation (same operand + activation rounding points) - i.e. the kernels add no error
    beyond bf16 arithmetic itself.  Per-kernel like-for-like parity is in test_gpu_conv.py."""
    import multimodal_learning_amd as m
    import oracle
    from oracle import weights as W
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    net = _student()
    bt = synthetic_batch(16, 128, seed=3)
    f3, feat, hazard, pred, _ = net(x_path=bt["x_path"].cuda())
    with torch.no_grad():
        _, f32feat, h32, _, _ = oracle.resnet_forward(bt["x_path"], W.make_state_dict(W.student_shapes(), 1))
        with oracle.Rounding.use("bf16"):
            _, efeat, hemu, _, _ = oracle.resnet_forward(bt["x_path"], W.make_state_dict(W.student_shapes(), 1))
    e_gpu = (hazard.cpu() - h32).abs()
    e_emu = (hemu - h32).abs()
    print(f"\nperf mode |dlogit| vs fp32 oracle: HIP max {e_gpu.max():.4f} mean {e_gpu.mean():.4f} | "
          f"bf16-emulated oracle max {e_emu.max():.4f} mean {e_emu.mean():.4f} | |logit| max {h32.abs().max():.3f}")
    assert e_gpu.mean() <= 2.0 * e_emu.mean() + 1e-3
    assert e_gpu.max() <= 3.0 * e_emu.max() + 1e-3


@pytest.mark.parametrize("pmode", ["bf16x6", "fp16x3"])
def test_teacher_forward_parity_mode(golden_dir, pmode):
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch, default_opt
    from tests.gpu_util import assert_close, Report
    g = np.load(os.path.join(golden_dir, "modules_b4_h64.npz"))
    m.set_precision(pmode)
    try:
        t = m.define_net(default_opt(), 1)
        t.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
        t = t.cuda().train()
        R = Report("teacher PathomicNet fwd, parity mode vs reference golden (B=4, 64x64)")
        assert_close = R.close
        bt = synthetic_batch(int(g["B"]), int(g["H"]), seed=int(g["batch_seed"]))
        with torch.no_grad():
            out = t(x_path=bt["x_path"].cuda(), x_omic=bt["x_omic"].cuda())
            assert len(out) == 11 and out[8] is None and out[9] is None and out[10] is None
            assert_close(g["t_fuse"], out[0], 1e-3, 0, "fuse feat"); assert_close(g["t_path_vec"], out[1], 1e-3, 0, "path vec")
            assert_close(g["t_omic_vec"], out[2], 1e-4, 0, "omic vec"); assert_close(g["t_f3"], out[3], 1e-3, 0, "f3")
            assert_close(g["t_h_path"], out[4][0], 1e-3, 0, "h path"); assert_close(g["t_h_omic"], out[4][1], 1e-4, 0, "h omic")
            assert_close(g["t_h_fuse"], out[4][2], 1e-3, 0, "h fuse"); assert_close(g["t_pred"], out[5], 1e-3, 0, "pred")
            assert_close(g["t_pred_path"], out[6], 1e-3, 0, "pred path"); assert_close(g["t_pred_omic"], out[7], 1e-4, 0, "pred omic")
            om = t.omic_net(x_omic=bt["x_omic"].cuda())
            assert len(om) == 4 and om[3] is None
            assert_close(g["omic_feat"], om[0], 1e-4, 0, "omic feat")
            fo = t.fusion(torch.as_tensor(g["fus_in1"]).cuda(), torch.as_tensor(g["fus_in2"]).cuda())
            assert_close(g["fus_out"], fo, 1e-4, 1e-4, "fusion out")
        R.finish()
    finally:
        m.set_precision("bf16")


def test_eval_mode_forward_vs_reference(golden_dir):
    """model.eval() / fix_model.eval() (reference test()): running-statistics BN, dropout off, no autograd graph."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch, default_opt
    from tests.gpu_util import Report
    g = np.load(os.path.join(golden_dir, "modules_eval_b4_h96.npz"))
    m.set_precision("bf16x6")
    try:
        R = Report("eval-mode student + teacher forward vs reference golden (B=4, 96x96)")
        bt = synthetic_batch(int(g["B"]), int(g["H"]), seed=int(g["batch_seed"]))
        net = _student().eval()
        rm_before = net.bn1.running_mean.clone()
        out = net(x_path=bt["x_path"].cuda())
        assert len(out) == 5 and out[4] is None and not out[2].requires_grad
        assert torch.equal(rm_before, net.bn1.running_mean), "eval mode must not touch the running statistics"
        R.close(g["f3"], out[0], 1e-3, 0, "f3"); R.close(g["feat"], out[1], 1e-3, 0, "features")
        R.close(g["hazard"], out[2], 1e-3, 0, "hazard"); R.close(g["pred"], out[3], 1e-3, 0, "pred")
        t = m.define_net(default_opt(dropout_rate=0.25), 1)      # dropout must be inactive in eval mode
        t.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
        t = t.cuda().eval()
        with torch.no_grad():
            o = t(x_path=bt["x_path"].cuda(), x_omic=bt["x_omic"].cuda())
        R.close(g["t_fuse"], o[0], 1e-3, 0, "teacher fuse feat"); R.close(g["t_path_vec"], o[1], 1e-3, 0, "teacher path vec")
        R.close(g["t_omic_vec"], o[2], 1e-4, 0, "teacher omic vec"); R.close(g["t_h_fuse"], o[4][2], 1e-3, 0, "teacher fuse logits")
        R.close(g["t_pred"], o[5], 1e-3, 0, "teacher pred"); R.close(g["t_pred_omic"], o[7], 1e-4, 0, "teacher pred omic")
        R.finish()
    finally:
        m.set_precision("bf16")


def test_teacher_backward_vs_reference_golden(golden_dir):
    """Row f-1 (kernels): gradients of the three-branch NLL (train_test_MT.py:208-212) through the SNN, the bilinear
    fusion and the path trunk of PathomicNet, parity mode, with and without cut_fuse_grad, against the fixture produced
    by running the reference's PathomicNet (tests/golden/make_golden_teacher_bwd.py)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch, default_opt
    from tests.test_oracle_golden import _teacher_bwd_check
    g = np.load(os.path.join(golden_dir, "teacher_bwd_b4_h64.npz"))
    bt = synthetic_batch(4, 64, seed=7)
    m.set_precision("bf16x6")
    try:
        for tag, cut in (("cut", True), ("nocut", False)):
            opt = default_opt()
            opt.cut_fuse_grad = cut
            t = m.define_net(opt, 1)
            t.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
            t = t.cuda().train()
            x_omic = bt["x_omic"].cuda().requires_grad_(True)
            out = t(x_path=bt["x_path"].cuda(), x_omic=x_omic)
            pred, pred_path, pred_omic = out[5], out[6], out[7]
            grade = bt["grade"].cuda()
            nll = lambda p: m.ops.NLLFn.apply(p, grade, float(p.shape[0]))
            loss = nll(pred_path) + nll(pred_omic) + nll(pred)
            loss.backward()
            named = {k: (p.grad.detach().float().cpu().numpy() if p.grad is not None
                         else np.zeros(tuple(p.shape), np.float32)) for k, p in t.named_parameters()}
            _teacher_bwd_check(named, x_omic.grad.cpu().numpy(), loss.item(), g, tag, 2e-3)
    finally:
        m.set_precision("bf16")


def test_dropout_backward_uses_the_forward_mask():
    """DropoutFn: the mask re-created in backward from the saved step-counter value is the forward mask (plain and
    alpha dropout), also after the module's counter has moved on."""
    import multimodal_learning_amd as m
    gen = torch.Generator(device="cuda").manual_seed(1234)      # (unseeded, an input that happens to equal 0 or the alpha-dropout
    for alpha in (False, True):                                  #  saturation value makes the mask unreadable from y: ~1e-3 per run)
        x = torch.randn(64, 96, device="cuda", generator=gen).requires_grad_(True)
        ctr = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        y = m.ops.DropoutFn.apply(x, 0.25, 0x5EED, 128, ctr, alpha)
        ctr += 3                                     # the forward pass of a later step
        y.backward(torch.ones_like(y))
        if not alpha:
            keep = (y != 0)
            assert torch.allclose(x.grad, keep.float() / 0.75, atol=1e-6)
            assert 0.6 < keep.float().mean().item() < 0.9
        else:
            ap = -1.7580993408473766
            a = ((1 - 0.25) * (1 + 0.25 * ap * ap)) ** -0.5
            b = -a * ap * 0.25
            dropped = torch.isclose(y, torch.full_like(y, a * ap + b), atol=1e-6)
            assert torch.allclose(x.grad, (~dropped).float() * a, atol=1e-6)


def test_student_backward_perf_mode_matches_parity_mode_on_ragged_tiles():
    """The perf-mode (bf16) backward runs different kernels from the parity mode that is pinned to the reference: the
    second-generation tap-convs with the residual add / ReLU mask fused into their dgrad epilogues (conv_tap2.hip,
    including the two-group layer-1 kernel), on partial tiles here (160 -> 40 / 20 / 10 / 5 pixel maps: none is a
    multiple of the 16 x 16 tile).  On this untrained train-mode-BN network bf16 arithmetic alone decorrelates the
    gradients to cosine ~0.82-0.89 against fp32 (the CPU oracle's own bf16 emulation shows 0.84-0.89 against its fp32
    run for the same loss), uniformly over the depth.  Asserted: every conv / linear weight gradient keeps cosine >= 0.70
    with the parity-mode gradient and none falls more than 0.12 below the median (BN scale / shift vectors: >= 0.50) - a wrong residual term in the layer-1 dgrad
    epilogue (found with this test) put layer1.0 at 0.15 and conv1 at 0.05 while the later layers stayed at 0.83.
    Like-for-like kernel parity of that epilogue: test_gpu_conv.py::test_tapconv2_dgrad_with_fused_residual."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    bt = synthetic_batch(8, 160, seed=9)
    wf = torch.linspace(0.5, 1.5, 128).cuda()
    grads = {}
    try:
        for mode in ("bf16x6", "bf16"):
            m.set_precision(mode)
            net = _student()
            net.train()
            f3, feat, hazard, pred, _ = net(x_path=bt["x_path"].cuda())
            loss = (feat * wf).sum() + (hazard * torch.tensor([1.0, -2.0, 0.5]).cuda()).sum() + 0.1 * f3.sum()
            loss.backward()
            grads[mode] = {k: p.grad.detach().float().clone() for k, p in net.named_parameters() if p.grad is not None}
    finally:
        m.set_precision("bf16")
    cosines = {}
    for k, gp in grads["bf16x6"].items():
        gq = grads["bf16"][k]
        denom = gp.norm().item()
        # (a bias in front of a train-mode BN has a mathematically zero gradient: whatever is there is rounding noise)
        if k == "fc_new1.0.bias" or denom < 1e-6 or gp.numel() < 64:
            continue
        cosines[k] = torch.dot(gp.flatten(), gq.flatten()).item() / (denom * gq.norm().item() + 1e-30)
    big = {k: v for k, v in cosines.items() if grads["bf16"][k].numel() >= 4096}      # conv / linear weights
    small = {k: v for k, v in cosines.items() if k not in big}                        # BN scale / shift (64-512 values)
    vals = sorted(big.values())
    med = vals[len(vals) // 2]
    worst, worst_s = min(big, key=big.get), min(small, key=small.get)
    print(f"\nperf-mode vs parity-mode gradients: {len(big)} weight tensors median cosine {med:.4f}, worst {big[worst]:.4f} at {worst}; "
          f"{len(small)} BN tensors worst {small[worst_s]:.4f} at {worst_s}")
    assert big[worst] >= 0.70 and big[worst] >= med - 0.12, (worst, big[worst], med)
    assert small[worst_s] >= 0.50, (worst_s, small[worst_s])


def test_perf_mode_forward_stage_by_stage():
    """Perf mode like for like, one stage at a time: every stage's reference is computed in fp32 torch from the GPU's OWN
    input to that stage (read out of the plan workspace through ph_resnet_tensor_info), so no error is carried from stage
    to stage and each kernel family is held to bf16 rounding: stem conv (the register-prefetch / packed-store path of
    conv_stem.hip), fused BN + ReLU + max-pool, the layer-1 tap-conv (two-group kernel) with its in-kernel BatchNorm
    statistics, BN apply, and the residual BN apply.  160 x 160 input: partial tiles everywhere.
    (The BatchNorm / pooling kernels one by one, bitwise and at odd sizes: tests/test_gpu_bn_act.py.)"""
    import ctypes as C
    import torch.nn.functional as F
    import multimodal_learning_amd as m
    from multimodal_learning_amd._lib import lib, check
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    net = _student()
    net.train()
    B, H = 6, 160
    x = synthetic_batch(B, H, seed=4)["x_path"].cuda()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    f3, feat, hazard, pred, _ = net(x_path=x)            # requires grad -> the workspace persists until backward
    plan = net._get_plan(B, H, H)
    ws = f3.grad_fn.ws                                   # the trunk's autograd node keeps the workspace of this forward
    assert ws is not None and ws.numel() == plan.ws_bytes

    def tensor(what, idx):
        off = C.c_size_t(0)
        dims = (C.c_int * 4)()
        check(lib().ph_resnet_tensor_info(plan.h, what, idx, C.byref(off), dims), "tensor_info")
        n = dims[0] * dims[1] * dims[2] * dims[3]
        t = ws[off.value: off.value + 2 * n].view(torch.bfloat16).view(dims[0], dims[1], dims[2], dims[3])
        return t.float().permute(0, 3, 1, 2).contiguous()            # NCHW fp32 copy

    def rel(ref, got):
        return ((ref - got).abs().max() / ref.abs().max()).item()

    def bn(z, wkey, bkey):   # train-mode BatchNorm with the batch statistics of z
        mu = z.mean(dim=(0, 2, 3), keepdim=True)
        var = z.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        return (z - mu) / torch.sqrt(var + 1e-5) * sd[wkey].view(1, -1, 1, 1) + sd[bkey].view(1, -1, 1, 1)

    rb = lambda t: t.bfloat16().float()
    # stem conv: bf16 operands, fp32 accumulate, bf16 store
    y0 = tensor(0, 0)
    y0_ref = F.conv2d(rb(x), rb(sd["conv1.weight"]), None, 2, 3)
    assert rel(y0_ref, y0) <= 1.0 / 128, ("stem conv", rel(y0_ref, y0))
    # BN + ReLU + maxpool from the stored y0
    p0 = tensor(3, 0)
    p0_ref = F.max_pool2d(F.relu(bn(y0, "bn1.weight", "bn1.bias")), 3, 2, 1)
    assert rel(p0_ref, p0) <= 1.0 / 64, ("stem bn+relu+maxpool", rel(p0_ref, p0))
    # layer1.0: conv1 (unit 1) from the pooled map, BN + ReLU -> a1, conv2 (unit 2), BN + residual + ReLU -> block output
    y1 = tensor(0, 1)
    y1_ref = F.conv2d(p0, rb(sd["layer1.0.conv1.weight"]), None, 1, 1)
    assert rel(y1_ref, y1) <= 1.0 / 128, ("layer1.0.conv1", rel(y1_ref, y1))
    a1 = tensor(2, 0)
    a1_ref = F.relu(bn(y1, "layer1.0.bn1.weight", "layer1.0.bn1.bias"))
    assert rel(a1_ref, a1) <= 1.0 / 64, ("layer1.0 bn1+relu", rel(a1_ref, a1))
    y2 = tensor(0, 2)
    y2_ref = F.conv2d(a1, rb(sd["layer1.0.conv2.weight"]), None, 1, 1)
    assert rel(y2_ref, y2) <= 1.0 / 128, ("layer1.0.conv2", rel(y2_ref, y2))
    o0 = tensor(1, 0)
    o0_ref = F.relu(bn(y2, "layer1.0.bn2.weight", "layer1.0.bn2.bias") + p0)
    assert rel(o0_ref, o0) <= 1.0 / 64, ("layer1.0 bn2+residual+relu", rel(o0_ref, o0))
    # a stride-2 block with a downsample path: layer2.0 (block 2)
    units = {"layer2.0.conv1": None}
    o1 = tensor(1, 1)                                    # layer1.1 output = layer2.0 input
    nunits = lib().ph_resnet_num_units(plan.h)
    # unit order: stem, then per block conv1, conv2, (downsample); layer1 has 2 blocks x 2 convs -> layer2.0.conv1 is unit 5
    y5 = tensor(0, 5)
    y5_ref = F.conv2d(o1, rb(sd["layer2.0.conv1.weight"]), None, 2, 1)
    assert y5.shape == y5_ref.shape and nunits == 20
    assert rel(y5_ref, y5) <= 1.0 / 128, ("layer2.0.conv1 (stride 2)", rel(y5_ref, y5))
    print("\nperf-mode stages: stem conv %.4f, stem pool %.4f, l1 conv %.4f, bn+relu %.4f, conv2 %.4f, bn+res %.4f, s2 conv %.4f"
          % (rel(y0_ref, y0), rel(p0_ref, p0), rel(y1_ref, y1), rel(a1_ref, a1), rel(y2_ref, y2), rel(o0_ref, o0), rel(y5_ref, y5)))


def test_evaluation_loop_vs_reference_test_function(golden_dir):
    """Row f-3: evaluate.test() (eval-mode forwards of the student and the frozen teacher, NLL, accuracy, ROC-AUC / AP /
    F1 through sklearn) against the reference's own test() run over the same three synthetic batches
    (tests/golden/make_golden_eval_loop.py)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt, synthetic_batch
    g = np.load(os.path.join(golden_dir, "eval_loop_b6_h64.npz"))
    nb, B, H = int(g["nb"]), int(g["B"]), int(g["H"])

    class Loader(list):
        dataset = range(nb * B)
    loader = Loader()
    for i in range(nb):
        bt = synthetic_batch(B, H, seed=500 + i)
        z = torch.zeros(B)
        loader.append((bt["x_path"], z, bt["x_omic"], z, z, bt["grade"]))
    m.set_precision("bf16x6")
    try:
        opt = default_opt(dropout_rate=0.25)
        student = m.define_net(opt, 1, path_only=True); teacher = m.define_net(opt, 1)
        student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
        teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
        out = m.evaluate.test(opt, teacher.cuda(), student.cuda(), loader, "cuda")
        loss_test, cidx, pval, sacc, acc, metrics, pred_test, grads_test, feats_test = out
        assert cidx is None and pval is None and sacc is None
        assert abs(loss_test - float(g["loss_test"])) <= 1e-3 * max(abs(float(g["loss_test"])), 1.0)
        assert abs(acc - float(g["grad_path_test"])) < 1e-12
        assert np.array_equal(pred_test[8], g["gt_all"]) and pred_test[8].dtype == g["gt_all"].dtype
        for got, key in ((pred_test[5], "probs_all"), (pred_test[6], "probs_path"), (feats_test[1], "feat_path_all")):
            ref = g[key]
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-3 * max(np.abs(ref).max(), 1.0), key
        # The ranking metrics are step functions of the scores (this fixture's random-weight networks saturate: many
        # log-probabilities tie to within rounding, and one swapped pair moves the micro AUC by 1/(18*36)).  So: the
        # metric function on the REFERENCE's scores reproduces the reference's metrics exactly; end to end the metrics
        # agree to a few pair swaps; accuracy / micro-F1 (argmax only) exactly.
        from sklearn.preprocessing import LabelBinarizer
        onehot = LabelBinarizer().fit(g["gt_all"]).transform(g["gt_all"])
        on_ref_scores = m.evaluate.grading_metrics(onehot, g["probs_path"])
        assert np.allclose(np.asarray(on_ref_scores, dtype=np.float64), g["metrics"], atol=1e-12)
        got = np.asarray(metrics, dtype=np.float64)
        assert np.abs(got - g["metrics"]).max() <= 0.02 and abs(got[2] - g["metrics"][2]) < 1e-12, (got, g["metrics"])
        # test_model(): the student alone - the same student-side results, no teacher probabilities
        out2 = m.evaluate.test_model(opt, student, loader, "cuda")
        assert out2[0] == loss_test and out2[4] == acc and out2[6][5] is None
        assert np.array_equal(out2[6][6], pred_test[6]) and np.allclose(out2[5], metrics)
    finally:
        m.set_precision("bf16")


def test_eval_mode_image_gradient_vs_oracle_autograd():
    """ph_resnet_backward_input + ph_stem_dgrad: the gradient of an eval-mode student's loss with respect to the IMAGE
    (train_test_MT_SP_Masking.py:62-75 takes it for the superpixel attention masks) against torch autograd through the
    oracle's eval-mode forward on the CPU.  Parity mode; a ragged size exercises the tile edges of the stem dgrad."""
    import multimodal_learning_amd as m
    import torch.nn.functional as F
    from oracle import weights as W
    from oracle.step import default_opt

    def eval_forward(sd, x):      # plain PyTorch fp32 restatement of the eval-mode student (resnets.py:217-253)
        def bn(t, p):
            return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.1, 1e-5)
        t = F.max_pool2d(F.relu(bn(F.conv2d(x, sd["conv1.weight"], None, 2, 3), "bn1")), 3, 2, 1)
        for li in range(1, 5):
            for bi in range(2):
                p = f"layer{li}.{bi}"
                stride = 2 if (li > 1 and bi == 0) else 1
                idt = t
                o = F.relu(bn(F.conv2d(t, sd[p + ".conv1.weight"], None, stride, 1), p + ".bn1"))
                o = bn(F.conv2d(o, sd[p + ".conv2.weight"], None, 1, 1), p + ".bn2")
                if p + ".downsample.0.weight" in sd:
                    idt = bn(F.conv2d(t, sd[p + ".downsample.0.weight"], None, stride, 0), p + ".downsample.1")
                t = F.relu(o + idt)
        f4 = t.mean((2, 3))
        h = F.linear(f4, sd["fc_new1.0.weight"], sd["fc_new1.0.bias"])
        feat = F.relu(F.batch_norm(h, sd["fc_new1.1.running_mean"], sd["fc_new1.1.running_var"], sd["fc_new1.1.weight"],
                                   sd["fc_new1.1.bias"], False, 0.1, 1e-5))
        return F.log_softmax(F.linear(feat, sd["fc_new2.weight"], sd["fc_new2.bias"]), dim=1)
    m.set_precision("bf16x6")
    try:
        sd = W.make_state_dict(W.student_shapes(), 1)
        net = m.define_net(default_opt(), 1, path_only=True)
        net.load_state_dict(sd)
        net = net.cuda().eval()
        for B, H in ((2, 64), (3, 72)):
            g = torch.Generator().manual_seed(B)
            x = torch.rand(B, 3, H, H, generator=g) * 2 - 1
            grade = torch.randint(0, 3, (B,), generator=g)
            xg = x.clone().cuda().requires_grad_(True)
            out = net(x_path=xg)
            loss = m.ops.NLLFn.apply(out[3], grade.cuda(), float(B))
            loss.backward()
            xr = x.clone().requires_grad_(True)
            ref_loss = F.nll_loss(eval_forward(sd, xr), grade)
            ref_loss.backward()
            assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(abs(float(ref_loss)), 1.0)
            err = float((xg.grad.cpu() - xr.grad).abs().max()); mx = float(xr.grad.abs().max())
            assert err <= 2e-4 * mx, (B, H, err, mx)
            assert all(p.grad is None for n_, p in net.named_parameters() if n_.startswith(("layer", "conv1", "bn1")))
    finally:
        m.set_precision("bf16")


def test_image_gradient_perf_mode_tracks_parity_mode():
    """The same eval-mode image gradient in perf mode (bf16 activations, bf16 dy into the stem dgrad) stays aligned with
    the parity-mode gradient (cosine > 0.9; measured 0.96 - a saliency map through 17 bf16 layers and their ReLU masks;
    a layout or type slip in the bf16 instantiation would give ~0)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    sd = W.make_state_dict(W.student_shapes(), 1)
    x = torch.rand(4, 3, 96, 96, generator=torch.Generator().manual_seed(9)) * 2 - 1
    grade = torch.tensor([0, 1, 2, 1])
    grads = {}
    try:
        for mode in ("bf16x6", "bf16"):
            m.set_precision(mode)
            net = m.define_net(default_opt(), 1, path_only=True)
            net.load_state_dict(sd)
            net = net.cuda().eval()
            xg = x.clone().cuda().requires_grad_(True)
            loss = m.ops.NLLFn.apply(net(x_path=xg)[3], grade.cuda(), 4.0)
            grads[mode], = torch.autograd.grad(loss, xg)
    finally:
        m.set_precision("bf16")
    a, b = grads["bf16x6"].flatten().double(), grads["bf16"].flatten().double()
    cos = float((a @ b) / (a.norm() * b.norm()))
    assert cos > 0.9, cos
    assert 0.8 < float(b.norm() / a.norm()) < 1.25


@pytest.mark.parametrize("B,H", [(6, 160), (3, 96), (20, 224), (64, 512), (32, 512), (64, 256), (16, 512)])
def test_fused_input_batchnorm_equals_separate_pass(B, H):
    """Forward-only networks (the EMA student and the teacher) run conv2 of every block on the RAW conv1 output and apply
    bn1 + ReLU to each halo tile in LDS (conv_tap2.hip, PhTapConv::in_scale; padding enters as NaN and leaves the ReLU
    as 0).  The separate bn_apply pass rounds the same values to bf16 before conv2 reads them, so both paths feed the
    MFMAs identical operands in identical order: outputs must be BITWISE equal - train and eval mode, ragged tile
    edges (160 -> 40 / 20 / 10 / 5 pixel maps), repeated launches."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    x = synthetic_batch(B, H, seed=31)["x_path"].cuda()
    for training in (True, False):
        outs = {}
        for no_fuse in (True, False, False):
            net = _student()
            net.train(training)
            net._no_fuse = no_fuse
            with torch.no_grad():
                f3, feat, hazard, pred, _ = net(x_path=x)
            key = "separate" if no_fuse else ("fused" if "fused" not in outs else "fused again")
            outs[key] = (f3.clone(), feat.clone(), hazard.clone(), {k: v.clone() for k, v in net.state_dict().items() if "running" in k})
        for other in ("fused", "fused again"):
            for a, b in zip(outs["separate"][:3], outs[other][:3]):
                assert torch.equal(a, b), (training, other, (a - b).abs().max().item())
            for k, v in outs["separate"][3].items():
                assert torch.equal(v, outs[other][3][k]), (training, k)
        assert torch.isfinite(outs["fused"][2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H", [(4, 64), (3, 160), (2, 224), (5, 72), (2, 70), (3, 102), (8, 512), (64, 512)])
def test_stem_conv_with_pooled_epilogue_equals_separate_passes(B, H):
    """Forward-only networks in perf mode never write the stem's conv output: stem_fwd_pool_kernel pools the bf16-rounded
    RAW output inside the conv kernel (maximum where gamma >= 0, minimum where gamma < 0) and BatchNorm + ReLU is applied to
    the pooled tensor - relu(scale * y + shift) is monotone in y, so this equals pooling the activated tensor
    (resnets.py:219-222: conv1 - bn1 - relu - maxpool).  Checked against the separate passes (`_no_stem_pool`):
      * eval mode (fixed running statistics, some gamma negative, one zero): the pooled activation and every output BITWISE;
      * train mode: the BatchNorm sums are taken over other workgroup tiles (strips of 14 columns with a recomputed halo
        column that must be counted once) - batch statistics to 1e-6, pooled activation within one bf16 step, and the
        running statistics to 1e-6;
      * ragged maps (72 -> 36 x 36 conv pixels: strips of 14 + 8, 160 -> 80: a cut strip at the larger batch), odd sizes."""
    import ctypes as C
    import multimodal_learning_amd as m
    from multimodal_learning_amd._lib import lib, check
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    x = synthetic_batch(B, H, seed=37)["x_path"].cuda()
    for training in (False, True):
        outs = {}
        for no_pool in (True, False, False):
            net = _student()
            with torch.no_grad():
                g = net.bn1.weight
                g[::5] = -g[::5].abs() - 0.1          # negative gamma: the pooled raw value must be the window's MINIMUM
                g[7] = 0.0
                net.bn1.running_mean.normal_(0, 0.3, generator=torch.Generator(device="cuda").manual_seed(1))
                net.bn1.running_var.uniform_(0.5, 2.0, generator=torch.Generator(device="cuda").manual_seed(2))
            net.train(training)
            net._no_stem_pool = no_pool
            with torch.no_grad():
                f3, feat, hazard, pred, _ = net(x_path=x)
            plan = net._get_plan(B, H, H)
            ws = net._get_workspace(plan, False)
            off = C.c_size_t(0); dims = (C.c_int * 4)()
            check(lib().ph_resnet_tensor_info(plan.h, 3, 0, C.byref(off), dims), "tensor_info")
            n = dims[0] * dims[1] * dims[2] * dims[3]
            pooled = ws[off.value: off.value + 2 * n].view(torch.bfloat16).clone()
            check(lib().ph_resnet_tensor_info(plan.h, 8, 0, C.byref(off), dims), "tensor_info")
            stats = ws[off.value: off.value + 16 * 64].view(torch.float32).clone()
            if not no_pool:
                # the fused path leaves the pooled tensor RAW: BatchNorm + ReLU is applied by its two consumers (layer1.0.conv1
                # while it stages its input, layer1.0's output pass on its shortcut).  Activate it here for the comparison;
                # torch may round the multiply-add differently from the kernels' fused multiply-add: one bf16 step allowed
                sc, sh = stats[128:192], stats[192:256]
                raw_pooled = pooled
                pooled = torch.relu(pooled.float().view(-1, 64) * sc + sh).bfloat16().view(-1)
            key = "separate" if no_pool else ("pooled" if "pooled" not in outs else "pooled again")
            outs[key] = (pooled, stats, f3.clone(), feat.clone(), hazard.clone(), net.bn1.running_mean.clone(), net.bn1.running_var.clone())
        sep = outs["separate"]
        assert torch.equal(outs["pooled"][0], outs["pooled again"][0]) and torch.equal(outs["pooled"][4], outs["pooled again"][4])
        got = outs["pooled"]
        if not training:
            for a, b in zip(sep[1:], got[1:]):
                assert torch.equal(a, b), (training, (a.float() - b.float()).abs().max().item())
            a, b = sep[0].float(), got[0].float()      # (+ 1e-5: a pre-activation within rounding of zero)
            assert ((a - b).abs() <= torch.maximum(a.abs(), b.abs()) * 2.0 ** -7 + 1e-5).all() and (a != b).float().mean().item() <= 1e-3
        else:
            assert ((sep[1] - got[1]).abs() <= 1e-6 * sep[1].abs() + 1e-6).all(), "batch statistics"
            for a, b in zip(sep[5:], got[5:]):
                assert ((a - b).abs() <= 1e-6 * a.abs() + 1e-7).all(), "running statistics"
            a, b = sep[0].float(), got[0].float()
            assert ((a - b).abs() <= torch.maximum(a.abs(), b.abs()) * 2.0 ** -7 + 1e-5).all(), (a - b).abs().max().item()      # one bf16 step
            assert (a != b).float().mean().item() <= 1e-3
            # (one-step differences of the activation propagate through 17 bf16 layers; the head sits behind a BatchNorm1d
            # over B <= 8 samples, which amplifies them - the eval-mode pass above is the bitwise check of the whole network)
            for (a, b), tol in zip(zip(sep[2:5], got[2:5]), (2e-2, 1e-1, 1e-1)):
                assert (a - b).norm() <= tol * a.norm(), ((a - b).norm() / a.norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H", [(4, 128), (6, 160)])
def test_masked_stride2_grid_vs_first_generation_kernel(B, H):
    """The 3x3 stride-2 convolutions (conv1 of layers 2-4) run in perf mode as a MASKED stride-1 grid over the four
    pixel-parity planes of their input (conv_tap2.hip, ph_tapconv2_setup_s2_fwd).  Same products, another summation
    order than the first-generation stride-2 kernel: the features of a train-mode forward agree to bf16 rounding of the
    activations (ragged maps at 160; like-for-like kernel parity vs F.conv2d: test_gpu_conv.py through ph_conv2d_fwd)."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    m.set_precision("bf16")
    x = synthetic_batch(B, H, seed=33)["x_path"].cuda()
    from tests.gpu_util import dispatch_lib, dispatched
    L = dispatch_lib()
    res, fams = {}, {}
    for no_masked in (True, False):
        net = _student()
        net.train()
        net._no_masked = no_masked
        torch.cuda.synchronize()
        L.ph_debug_dispatch_reset()
        f3, feat, hazard, pred, _ = net(x_path=x)
        torch.cuda.synchronize()
        fams[no_masked] = dispatched(L)
        (feat.square().mean() + hazard.sum()).backward()
        res[no_masked] = (f3.detach(), feat.detach(), torch.cat([p.grad.flatten() for p in net.parameters() if p.grad is not None]))
    # the two forwards ran different kernels for the stride-2 convolutions (no_masked: the first-generation kernel)
    assert "tap6b" in fams[False], fams
    assert "tap6b" not in fams[True] and "tap2_masked" not in fams[True], fams
    for (a, b), tol in zip(zip(res[True][:2], res[False][:2]), (2e-2, 6e-2)):   # trunk; head behind a small-batch BatchNorm1d
        assert torch.isfinite(b).all()
        assert (a - b).norm() <= tol * a.norm(), ((a - b).norm() / a.norm()).item()
    # (gradients of this untrained train-mode-BN network decorrelate under bf16 rounding alone, see
    # test_student_backward_perf_mode_matches_parity_mode_on_ragged_tiles: same bound here)
    ga, gb = res[True][2], res[False][2]
    assert torch.isfinite(gb).all()
    assert torch.dot(ga, gb) >= 0.70 * ga.norm() * gb.norm()


@pytest.mark.gpu
def test_workspace_cache_is_bounded_and_pins_what_a_capture_uses():
    """one trunk workspace per (B, H, W, arithmetic) used to stay alive for good (2.7 GB each at the benchmark
    size).  Un-pinned workspaces now live in a 2-entry LRU per network; a workspace requested while a stream capture is
    running is pinned (the graph holds its raw pointer) and survives any number of other shapes."""
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    net = _student()
    for p in net.parameters():
        p.requires_grad_(False)
    xs = {h: torch.rand(2, 3, h, h, device="cuda") * 2 - 1 for h in (64, 96, 128, 160)}
    with torch.no_grad():
        for h in (64, 96, 128):
            net(x_path=xs[h])
    assert len(net._ws_cache) == 2 and [k[1] for k in net._ws_cache] == [96, 128]      # least recently used first
    with torch.no_grad():
        net(x_path=xs[96])
        net(x_path=xs[160])
    assert [k[1] for k in net._ws_cache] == [96, 160]
    # a capture pins its workspace
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.no_grad():
        with torch.cuda.graph(g):
            out = net(x_path=xs[64])
    ptr64 = net._ws_cache[(2, 64, 64, m.get_precision())].data_ptr()
    with torch.no_grad():
        for h in (96, 128, 160, 96, 128):
            net(x_path=xs[h])
    assert (2, 64, 64, m.get_precision()) in net._ws_cache and net._ws_cache[(2, 64, 64, m.get_precision())].data_ptr() == ptr64
    assert len([k for k in net._ws_cache if k[1] != 64]) == 2
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = net(x_path=xs[64])
    assert torch.equal(out[2], ref[2])
    net.release_workspaces()
    assert not net._ws_cache and not net._ws_pinned


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,mode", [(4, 128, "bf16"), (6, 160, "bf16"), (2, 96, "bf16x6"), (64, 512, "bf16")])
def test_two_stream_backward_equals_one_stream(B, H, mode):
    """The trunk's backward runs its weight gradients on a second stream beside the BatchNorm-backward / dgrad chain
    (csrc/resnet_plan.hip: backward_impl; dz buffers alternate, events order every producer and reader).  The chain's
    kernels are unchanged: BatchNorm gradients are BITWISE the one-stream sequence's.  The weight gradients are split into
    half as many partial sums per launch (one workgroup per CU beside the chain instead of two): equal up to the fp32
    summation order.  Eager and captured-and-replayed (the side stream becomes a parallel branch) agree bitwise."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    m.set_precision(mode)
    try:
        x = synthetic_batch(B, H, seed=35)["x_path"].cuda()
        res = {}
        for one_stream in (True, False):
            net = _student()
            net.train()
            net._no_bwd_overlap = one_stream
            # (torch's capture recipe: eager passes on a side stream, no autograd graph of theirs alive at capture time)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for rep in range(2):         # the second pass re-uses buffers the side stream may still be reading
                    for p in net.parameters():
                        p.grad = None
                    f3, feat, hazard, pred, _ = net(x_path=x)
                    (feat.square().mean() + hazard.sum()).backward()
                    del f3, feat, hazard, pred
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            res[one_stream] = [p.grad.clone() for p in net.parameters() if p.grad is not None]
            if not one_stream:
                # the same forward + backward captured and replayed
                static_x = x.clone()
                for p in net.parameters():
                    p.grad = None
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    f3, feat, hazard, pred, _ = net(x_path=static_x)
                    (feat.square().mean() + hazard.sum()).backward()
                del f3, feat, hazard, pred
                for p in net.parameters():
                    if p.grad is not None:
                        p.grad.zero_()
                g.replay()
                torch.cuda.synchronize()
                res["graph"] = [p.grad.clone() for p in net.parameters() if p.grad is not None]
        assert len(res[True]) == len(res[False]) == len(res["graph"]) > 60
        nbit = 0
        for a, b, c in zip(res[True], res[False], res["graph"]):
            assert torch.isfinite(a).all()
            assert torch.equal(b, c)
            if a.dim() == 4:      # a convolution weight
                assert (a - b).abs().max() <= 2e-5 * a.abs().max() + 1e-12, ((a - b).abs().max() / a.abs().max()).item()
            else:
                assert torch.equal(a, b)
                nbit += 1
        assert nbit >= 40
    finally:
        m.set_precision("bf16")

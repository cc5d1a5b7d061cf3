"""The stem's fused backward (csrc/conv_stem.hip: stem_wgrad_kernel<bf16, FUSE>; csrc/resnet_plan.hip: backward_impl): in the bf16
mode the stem's weight-gradient kernel forms its dz tile itself - from the conv output y0, the pooled gradient and the arg codes,
through the helpers of csrc/stem_dz.h that the separate pass (stem_bwd_kernel<APPLY>) calls too - instead of reading a dz tensor
that pass wrote.  `ph_resnet_plan_set_stem_fused` selects the path.

Every dz element is bitwise the separate pass's and the tiles, chunks and MFMA order are unchanged, so EVERY parameter gradient is
bitwise the same on both paths.  Shapes: B = 3 (chunks cross image boundaries) with the 8 x 16 tile of stem-output pixels and
OH = H / 2: 96 x 96 (both tile counts exact), 80 x 80 (OW = 40: partial column tile), 104 x 104 (OH = OW = 52: partial row and
column tiles), 96 x 80 (non-square).  The plan accepts all four."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(96, 96), (80, 80), (104, 104), (96, 80)]


def _student():
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    net = m.define_net(default_opt(), 1, path_only=True)
    net.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    net = net.cuda()
    net.train()
    return net


def _images(H, W):
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
    base = torch.rand(B, 3, H // 8, W // 8, device="cuda", generator=g) * 2 - 1
    x = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    return (x + 0.2 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp_(-1, 1).contiguous()


def _loss(net, x):
    f3, feat, hazard, pred, _ = net(x_path=x)
    return f3.grad_fn, feat.square().mean() + hazard.sum() + 0.1 * f3.square().mean()


def _info(plan, what, idx):
    from multimodal_learning_amd._lib import lib, check
    off = C.c_size_t(0)
    dims = (C.c_int * 4)()
    check(lib().ph_resnet_tensor_info(plan.h, what, idx, C.byref(off), dims), "tensor_info")
    return off.value, tuple(dims)


def _dz_view(plan, ws, H, W):
    """The stem's dz tensor [B][H/2][W/2][64] bf16 in the workspace (the first dz buffer)."""
    off, _ = _info(plan, 6, 0)
    n = B * (H // 2) * (W // 2) * 64
    return ws[off: off + 2 * n].view(torch.bfloat16)


def _backward(net, x, fused, overlap=True, nan_dz=False):
    """One fresh forward + backward; returns the gradients by parameter name, the workspace and the plan."""
    from multimodal_learning_amd._lib import lib, check
    net._no_bwd_overlap = not overlap
    for p in net.parameters():
        p.grad = None
    ctx, loss = _loss(net, x)
    plan, ws = ctx.plan, ctx.ws
    check(lib().ph_resnet_plan_set_stem_fused(plan.h, 1 if fused else 0), "set_stem_fused")
    if nan_dz:
        _dz_view(plan, ws, x.shape[2], x.shape[3]).fill_(float("nan"))
    loss.backward()
    torch.cuda.synchronize()
    check(lib().ph_resnet_plan_set_stem_fused(plan.h, 1), "set_stem_fused")
    return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, ws, plan


_CACHE = {}


def _case(H, W):
    """Net, images and the SEPARATE path's gradients of a shape: computed once, shared by the tests below, never modified."""
    import multimodal_learning_amd as m
    if (H, W) not in _CACHE:
        m.set_precision("bf16")
        net, x = _student(), _images(H, W)
        sep, _, _ = _backward(net, x, fused=False)
        assert len(sep) > 60 and all(torch.isfinite(g).all() for g in sep.values())
        _CACHE[(H, W)] = (net, x, sep)
    return _CACHE[(H, W)]


def _assert_bitwise(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert torch.equal(a[n], b[n]), (n, (a[n] - b[n]).abs().max().item())


@pytest.mark.parametrize("H,W", SHAPES)
def test_fused_gradients_bitwise_equal_separate_path(H, W):
    """Forward + backward twice on the same seeded weights and images, switch off and on: every parameter gradient bitwise equal -
    the stem weight gradient through the fused kernel, everything else because it is untouched."""
    net, x, sep = _case(H, W)
    fused, _, _ = _backward(net, x, fused=True)
    _assert_bitwise(sep, fused)
    assert sep["conv1.weight"].abs().max() > 0


def test_fused_bitwise_on_one_stream():
    """The same with the whole backward on the caller's stream (ph_resnet_plan_set_backward_overlap 0).  (The weight gradients of
    the other layers are summed from twice as many slabs there: compared with the separate path on one stream.)"""
    net, x, _ = _case(104, 104)
    sep, _, _ = _backward(net, x, fused=False, overlap=False)
    fused, _, _ = _backward(net, x, fused=True, overlap=False)
    _assert_bitwise(sep, fused)


def test_fused_bitwise_captured_and_replayed():
    """The fused backward captured in a graph (two eager passes first, as bench.py's trunk_fwd_bwd) and replayed."""
    from multimodal_learning_amd._lib import lib, check
    net, x, sep = _case(80, 80)
    net._no_bwd_overlap = False
    plan = net._get_plan(B, 80, 80)
    check(lib().ph_resnet_plan_set_stem_fused(plan.h, 1), "set_stem_fused")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in net.parameters():
                p.grad = None
            _loss(net, x)[1].backward()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for p in net.parameters():
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = _loss(net, x)[1]
        loss.backward()
    del loss
    for p in net.parameters():
        if p.grad is not None:
            p.grad.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    _assert_bitwise(sep, got)
    del g
    for p in net.parameters():
        p.grad = None


def test_fused_path_does_not_read_dz():
    """The dz buffer filled with NaN before the backward: the fused path's stem weight gradient is finite and bitwise the separate
    path's, and the part of the buffer only the stem's dz reaches (past the quarter-size dz of layer 1) is still NaN; after a
    backward with the switch off the whole buffer is finite - the switch really selects the path."""
    H = W = 104
    net, x, sep = _case(H, W)
    fused, ws, plan = _backward(net, x, fused=True, nan_dz=True)
    assert torch.isfinite(fused["conv1.weight"]).all()
    _assert_bitwise(sep, fused)
    dz = _dz_view(plan, ws, H, W)
    quarter = B * ((H // 2 + 1) // 2) * ((W // 2 + 1) // 2) * 64
    assert torch.isnan(dz[quarter:]).all()
    _, ws, plan = _backward(net, x, fused=False, nan_dz=True)
    assert torch.isfinite(_dz_view(plan, ws, H, W)).all()


def test_fused_against_float64():
    """Reference distance, so that a change to both kernels at once cannot hide behind the A/B.  104 x 104 (partial row and column
    tiles).  Reference: dz in float64 by tests/bn_emulation.py's stem_bwd_apply from the device's own inputs of the stem backward
    (pooled gradient, arg codes, y0, statistics; c1 / c2 from the device's dbeta / dgamma), rounded to bf16; then the float64
    correlation with the bf16-rounded image.  Tolerance: what the SEPARATE path achieves on the same inputs in this test - the fused
    result is bitwise that path, so its excess is exactly 0.  The separate path itself is held to 2e-3 of max |ref|, the bound of
    tests/test_gpu_fullsize.py for fp32 parameter gradients of bf16 operands (8112 products per output, fp32 accumulation;
    measured 3.8e-5 for both paths)."""
    from tests import bn_emulation as E
    H = W = 104
    OH, OW = H // 2, W // 2
    net, x, sep = _case(H, W)
    fused, ws, plan = _backward(net, x, fused=True)

    def t(what, idx, dims, dtype, es):
        off, d = _info(plan, what, idx)
        d = dims or d
        n = d[0] * d[1] * d[2] * d[3]
        return ws[off: off + es * n].view(dtype).view(*d)
    PH, PW = (OH + 1) // 2, (OW + 1) // 2
    st = t(8, 0, None, torch.float32, 4).view(4, 64).cpu().numpy()
    npix = float(B * OH * OW)
    inp = {"B": B, "H": OH, "W": OW, "prec": E.BF16, "dzs": None,
           "dpool": t(4, 0, (B, PH, PW, 64), torch.bfloat16, 2).float().cpu().numpy(),
           "idx": t(9, 0, None, torch.uint8, 1).cpu().numpy().astype(np.int64),
           "y": t(0, 0, None, torch.bfloat16, 2).float().cpu().numpy(),
           "mean": st[0], "invstd": st[1], "scale": st[2], "shift": st[3],
           "gamma": net.bn1.weight.detach().cpu().numpy(),
           "c1": (sep["bn1.bias"].double() / npix).cpu().numpy(), "c2": (sep["bn1.weight"].double() / npix).cpu().numpy()}
    dz = E.stem_bwd_apply(inp, E.F64)["dy"]
    dz = E.bf16r(dz.astype(np.float32)).astype(np.float64)
    xr = x.bfloat16().double().cpu()
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, None, 2, 3).backward(torch.from_numpy(dz).permute(0, 3, 1, 2).contiguous())
    ref = w.grad
    scale = ref.abs().max().item()
    e_sep = (sep["conv1.weight"].double().cpu() - ref).abs().max().item() / scale
    e_fused = (fused["conv1.weight"].double().cpu() - ref).abs().max().item() / scale
    print(f"stem wgrad vs float64: separate {e_sep:.3e}  fused {e_fused:.3e}  (max |ref| {scale:.3e})")
    assert e_sep <= 2e-3, e_sep
    assert e_fused - e_sep == 0.0, (e_fused, e_sep)


def test_debug_backward_still_writes_dz():
    """ph_resnet_backward_debug cut after the stem's apply stage (61 of 62 with g_f3) writes dz with the switch on as with it off,
    bitwise, at 80 x 80; cut after the last stage its stem weight gradient is the whole backward's."""
    from multimodal_learning_amd import ops
    from multimodal_learning_amd._lib import lib, check, ptr, stream
    H = W = 80
    net, x, sep = _case(H, W)
    L = lib()
    for p in net.parameters():
        p.grad = None
    ctx, _ = _loss(net, x)
    plan, ws, packed, table = ctx.plan, ctx.ws, ctx.packed, ctx.table
    gen = torch.Generator(device="cuda").manual_seed(3)
    g4 = torch.randn(B, 512, device="cuda", generator=gen)
    g3 = 0.5 * torch.randn(B, 256, device="cuda", generator=gen)
    grads = [torch.full_like(p, float("nan")) for p in net._trunk_params()]
    ga = ops.void_array([g.data_ptr() for g in grads])
    dz = _dz_view(plan, ws, H, W)
    got = {}
    for on in (0, 1):
        check(L.ph_resnet_plan_set_stem_fused(plan.h, on), "set_stem_fused")
        dz.fill_(float("nan"))
        check(L.ph_resnet_backward_debug(plan.h, table, ptr(packed), ptr(ws), ptr(g3), ptr(g4), ga, 61, stream()), "backward_debug")
        torch.cuda.synchronize()
        got[on] = dz.clone()
        assert torch.isfinite(got[on]).all()
        grads[0].fill_(float("nan"))
        check(L.ph_resnet_backward_debug(plan.h, table, ptr(packed), ptr(ws), ptr(g3), ptr(g4), ga, 62, stream()), "backward_debug")
        torch.cuda.synchronize()
        got[on, "dw"] = grads[0].clone()
        assert torch.isfinite(got[on, "dw"]).all()
    assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16))
    assert torch.equal(got[0, "dw"], got[1, "dw"])
    # the whole (fused) backward on the same forward and the same incoming gradients
    check(L.ph_resnet_plan_set_stem_fused(plan.h, 1), "set_stem_fused")
    full = [torch.full_like(p, float("nan")) for p in net._trunk_params()]
    check(L.ph_resnet_backward(plan.h, table, ptr(packed), ptr(ws), ptr(g3), ptr(g4), ops.void_array([g.data_ptr() for g in full]),
                               stream()), "backward")
    torch.cuda.synchronize()
    assert torch.equal(full[0], got[1, "dw"])

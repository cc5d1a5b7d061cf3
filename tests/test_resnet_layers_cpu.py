"""Host side of the general-depth BasicBlock trunk (ph_resnet_plan_create_layers, resnets.ResNet with any four depths, ResNet34,
opt.path_arch): plan construction is pure host code, so everything here runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

R18, R34 = (2, 2, 2, 2), (3, 4, 6, 3)


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def _layers(d):
    return (C.c_int * 4)(*d)


def _info(L, p, what, idx):
    off, dims = C.c_size_t(0), (C.c_int * 4)()
    assert L.ph_resnet_tensor_info(p, what, idx, C.byref(off), dims) == 0, (what, idx)
    return off.value, tuple(dims)


def test_create_is_create_layers_with_resnet18_depths():
    """ph_resnet_plan_create(B, H, W, prec) and ph_resnet_plan_create_layers(.., {2,2,2,2}) build the same plan: workspace and packed
    sizes, weight-layout signature and the tensor offsets test_plan_layout_is_pinned pins, at that test's five shapes."""
    from tests.test_cabi_cpu import _PLAN_LAYOUT, _PLAN_TENSORS
    L = _lib()
    for (B, H, W, prec) in _PLAN_LAYOUT:
        a, b = L.ph_resnet_plan_create(B, H, W, prec), L.ph_resnet_plan_create_layers(B, H, W, prec, _layers(R18))
        assert a and b
        try:
            assert L.ph_resnet_num_units(a) == L.ph_resnet_num_units(b)
            assert L.ph_resnet_workspace_bytes(a) == L.ph_resnet_workspace_bytes(b)
            assert L.ph_resnet_packed_bytes(a) == L.ph_resnet_packed_bytes(b)
            assert L.ph_resnet_plan_layout_sig(a) == L.ph_resnet_plan_layout_sig(b)
            for what, idx in _PLAN_TENSORS:
                assert _info(L, a, what, idx) == _info(L, b, what, idx), (B, H, W, prec, what, idx)
        finally:
            L.ph_resnet_plan_destroy(a); L.ph_resnet_plan_destroy(b)


@pytest.mark.parametrize("prec", [0, 1, 3])
def test_unit_count_and_shapes_follow_the_depths(prec):
    """{3,4,6,3} has 36 units whose shapes are the conv weights of the drop-in ResNet's `_units()`, in that order; {1,1,1,1} has 12;
    an uneven deep trunk follows the same formula."""
    import multimodal_learning_amd as m
    L = _lib()
    for depths, n in ((R34, 36), ((1, 1, 1, 1), 12), ((1, 5, 2, 7), 1 + 2 * 15 + 3)):
        p = L.ph_resnet_plan_create_layers(3, 96, 160, prec, _layers(depths))
        assert p
        try:
            assert L.ph_resnet_num_units(p) == n
            net = m.ResNet(m.BasicBlock, list(depths), path_dim=128, num_classes=3)
            units = net._units()
            assert len(units) == n
            out4 = (C.c_int * 4)()
            for u, (conv, bn) in enumerate(units):
                assert L.ph_resnet_unit_shape(p, u, out4) == 0
                assert (out4[0], out4[1], out4[2], out4[2]) == tuple(conv.weight.shape), (depths, u)
                assert out4[3] == conv.stride[0] and bn.weight.shape[0] == out4[0]
            assert L.ph_resnet_unit_shape(p, n, out4) != 0 and L.ph_resnet_unit_shape(p, -1, out4) != 0
        finally:
            L.ph_resnet_plan_destroy(p)


@pytest.mark.parametrize("B,H,W,prec", [(4, 64, 64, 0), (3, 96, 160, 1), (4, 64, 64, 3), (64, 512, 512, 0)])
def test_resnet34_workspace_offsets_are_distinct_aligned_and_inside(B, H, W, prec):
    """Every tensor ph_resnet_tensor_info knows of a {3,4,6,3} plan: 256-byte aligned as in the ResNet-18 plan, no two at one offset, and
    its extent inside the workspace; block ids end at 16, unit ids at 36."""
    L = _lib()
    p = L.ph_resnet_plan_create_layers(B, H, W, prec, _layers(R34))
    assert p
    try:
        ws, es = L.ph_resnet_workspace_bytes(p), (2 if prec == 0 else 4)
        nblk, nun = sum(R34), L.ph_resnet_num_units(p)
        seen = {}
        ids = [(0, u) for u in range(nun)] + [(1, b) for b in range(nblk)] + [(2, b) for b in range(nblk)] + [(3, 0)] + \
              [(w, 0) for w in (4, 5, 6, 7, 9)] + [(8, u) for u in range(nun)]
        for what, idx in ids:
            off, dims = _info(L, p, what, idx)
            assert off % 256 == 0 and off < ws, (what, idx, off)
            n = dims[0] * dims[1] * dims[2] * dims[3]
            nbytes = n * (4 if what == 8 else 1 if what == 9 else es)
            assert off + nbytes <= ws, (what, idx)
            # (half-pair mode keeps the block output twice, `what` 1 is the operand image; 1 / 2 of a block never share an offset)
            assert off not in seen, ((what, idx), seen.get(off))
            seen[off] = (what, idx)
        off, dims = C.c_size_t(0), (C.c_int * 4)()
        assert L.ph_resnet_tensor_info(p, 1, nblk, C.byref(off), dims) != 0
        assert L.ph_resnet_tensor_info(p, 0, nun, C.byref(off), dims) != 0
        # the deeper trunk saves more activations and packs more weights than ResNet-18 at the same shape
        q = L.ph_resnet_plan_create(B, H, W, prec)
        assert ws > L.ph_resnet_workspace_bytes(q) and L.ph_resnet_packed_bytes(p) > L.ph_resnet_packed_bytes(q)
        L.ph_resnet_plan_destroy(q)
    finally:
        L.ph_resnet_plan_destroy(p)


def test_create_layers_refusals():
    """NULL depths, a zero, a negative entry and one above the documented cap return NULL; so do the B / H / W / prec rules of
    ph_resnet_plan_create.  The cap itself builds."""
    import re
    L = _lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pathomic_hip.h")).read()
    cap = int(re.search(r"#define\s+PH_RESNET_MAX_BLOCKS\s+(\d+)", hdr).group(1))
    assert not L.ph_resnet_plan_create_layers(4, 64, 64, 0, None)
    for bad in ((0, 2, 2, 2), (2, 2, 2, 0), (2, -1, 2, 2), (3, 4, cap + 1, 3), (cap + 1, 1, 1, 1), (2, 2, 2, 1 << 30)):
        assert not L.ph_resnet_plan_create_layers(4, 64, 64, 0, _layers(bad)), bad
    for (B, H, W, prec) in ((0, 64, 64, 0), (1, 8, 8, 0), (1, 64, 64, 5), (-3, 64, 64, 1), (2, 66, 64, 3)):
        assert not L.ph_resnet_plan_create_layers(B, H, W, prec, _layers(R34)), (B, H, W, prec)
    p = L.ph_resnet_plan_create_layers(1, 32, 32, 0, _layers((1, 1, cap, 1)))
    assert p and L.ph_resnet_num_units(p) == 1 + 2 * (cap + 3) + 3
    L.ph_resnet_plan_destroy(p)


def test_resnet34_python_surface(golden_dir):
    import multimodal_learning_amd as m
    from multimodal_learning_amd import resnets
    assert "ResNet34" in m.__all__ and "ResNet34" in resnets.__all__ and m.ResNet34 is resnets.ResNet34
    g = np.load(os.path.join(golden_dir, "resnet34_b4_h64.npz"))
    net = m.ResNet34(path_dim=128, act=torch.nn.LogSoftmax(dim=1), num_classes=3)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for k, shp in zip(g["keys"], g["shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(d) for d in str(shp).split(",") if d), k
    assert len(net._units()) == 36 and net._layers == R34
    # the plan cache key and the plan carry the depths
    plan = net._get_plan(2, 64, 64, 0)
    assert plan.layers == R34 and R34 == tuple(list(net._plans)[0][-4:])
    assert m.lib().ph_resnet_num_units(plan.h) == 36
    # a lookup by the workspace key (B, H, W, precision) finds the same plan and adds no entry
    assert plan.key == (2, 64, 64, 0) and net._plans[plan.key] is plan and len(net._plans) == 1
    with pytest.raises(KeyError):
        net._plans[(2, 64, 96, 0)]
    assert len(m.ResNet18(path_dim=128, num_classes=3)._units()) == 20


def test_other_blocks_and_depth_lists_still_raise():
    import multimodal_learning_amd as m

    class Bottleneck(torch.nn.Module):
        expansion = 4

        def __init__(self, inplanes, planes, stride=1, downsample=None):
            super().__init__()
    with pytest.raises(NotImplementedError, match="BasicBlock"):
        m.ResNet(Bottleneck, [3, 4, 6, 3])
    for bad in ([2, 2, 2], [2, 2, 0, 2], [2, 2, 2, 1000]):
        with pytest.raises(ValueError):
            m.ResNet(m.BasicBlock, bad)


def test_path_arch_option():
    """opt.path_arch: absent and "resnet18" build today's 20-unit trunk, "resnet34" the 36-unit one - student, path-only mode and the
    teacher's path encoder; anything else raises from define_net and from the trainers' option check, naming the two."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd.train_step import _validate_opt
    from oracle.step import default_opt
    assert not hasattr(default_opt(), "path_arch")
    assert len(m.define_net(default_opt(), 1, path_only=True)._units()) == 20
    assert len(m.define_net(default_opt(path_arch="resnet18"), 1, path_only=True)._units()) == 20
    assert len(m.define_net(default_opt(path_arch="resnet18"), 1).path_net._units()) == 20
    o34 = default_opt(path_arch="resnet34")
    assert len(m.define_net(o34, 1, path_only=True)._units()) == 36
    assert len(m.define_net(o34, 1).path_net._units()) == 36
    assert len(m.define_net(default_opt(path_arch="resnet34", mode="path"), 1)._units()) == 36
    assert len(m.get_resnet(path_dim=128, label_dim=3)._units()) == 20
    _validate_opt(o34, "test")
    for bad in ("resnet50", "ResNet34", ""):
        o = default_opt(path_arch=bad)
        for build in (lambda: m.define_net(o, 1, path_only=True), lambda: m.define_net(o, 1), lambda: _validate_opt(o, "test")):
            with pytest.raises(NotImplementedError, match="resnet18.*resnet34"):
                build()

"""The weight packers (csrc/pack_weights.hip) against their numpy restatement (tests/pack_emulation.py), byte for byte: the packed
buffer of small ResNet plans (one table and more than one, every arithmetic, the half-pair switches on and off) and the head of the
workspace after single-convolution calls.  Every buffer is pre-filled with a sentinel: what the restatement does not mark as written
must still hold it.  B = 1, 32 x 32 images (8 x 8 maps for the single convolutions), |w| < 32.  tests/test_pack_emulation_cpu.py
shows that the restatement's named defects change the bytes compared here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pack_emulation as P
from tests.gpu_util import DISPATCH_FAMILIES, SENTINEL, hp_pack

pytestmark = pytest.mark.gpu

SENT16 = SENTINEL * 0x0101
WFRAG = {0: "row", 1: "tap5", 2: "tap6"}


def _lib():
    from multimodal_learning_amd._lib import lib
    L = lib()
    L.ph_conv2d_workspace_bytes.restype = ctypes.c_size_t
    return L


@functools.lru_cache(maxsize=None)
def _net_weights(layers):
    units = P.resnet_units(layers)
    return units, P.random_weights([(64, 3, 7, 7)] + [(O, I, KS, KS) for (O, I, KS, S) in units], 100 + sum(layers))


@functools.lru_cache(maxsize=None)
def _net_reference(layers, arith, tap5=True, tap6=True):
    units, ws = _net_weights(layers)
    return P.pack_network(ws[0], units, ws[1:], arith, P.plan_layouts(units, arith, tap5, tap6))


def _pack_plan(L, layers, arith):
    """(packed words of a fresh sentinel-filled buffer, layout signature) of the plan of `layers` at B = 1, 32 x 32."""
    from multimodal_learning_amd._lib import check, ptr, stream
    units, ws = _net_weights(layers)
    plan = L.ph_resnet_plan_create_layers(1, 32, 32, P.ARITHS[arith], (ctypes.c_int * 4)(*layers))
    assert plan
    try:
        n = L.ph_resnet_num_units(plan)
        shape = (ctypes.c_int * 4)()
        got_units = []
        for u in range(n):
            assert L.ph_resnet_unit_shape(plan, u, shape) == 0
            got_units.append(tuple(shape))
        assert got_units == [(64, 3, 7, 2)] + units
        dev = [torch.from_numpy(w).cuda() for w in ws]
        table = (ctypes.c_void_p * (6 * n))()
        for u, w in enumerate(dev):
            table[6 * u] = ptr(w)
        nbytes = L.ph_resnet_packed_bytes(plan)
        buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        check(L.ph_resnet_pack_weights(plan, table, ptr(buf), stream()), "ph_resnet_pack_weights")
        torch.cuda.synchronize()
        return buf.cpu().numpy().view(np.uint16), L.ph_resnet_plan_layout_sig(plan)
    finally:
        L.ph_resnet_plan_destroy(plan)


def _compare(got, words, written, what):
    assert got.size == words.size, (what, got.size, words.size)
    bad = np.flatnonzero(written & (got != words))
    stray = np.flatnonzero(~written & (got != SENT16))
    print(f"{what}: {int(written.sum())} of {words.size} words written, {bad.size} differ, {stray.size} stray")
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:4].tolist()}"
    assert stray.size == 0, f"{what}: {stray.size} words written outside the mask, first at {stray[:4].tolist()}"


@pytest.mark.parametrize("layers,arith", P.NETWORKS, ids=[f"{'_'.join(map(str, l))}-{a}" for l, a in P.NETWORKS])
def test_network_buffer(layers, arith):
    """(1, 1, 1, 1): one table; (8, 1, 1, 1): 25 convolution units behind the stem, more than one table of 20, so two launches."""
    got, _ = _pack_plan(_lib(), layers, arith)
    _compare(got, *_net_reference(layers, arith), f"{layers} {arith}")


def test_network_buffer_half_pair_switches_off():
    L = _lib()
    layers = (1, 1, 1, 1)
    _, sig_on = _pack_plan(L, layers, "fp16x3")
    L.ph_debug_set_tap5(0)
    L.ph_debug_set_tap6(0)
    try:
        got, sig_off = _pack_plan(L, layers, "fp16x3")
    finally:
        L.ph_debug_set_tap5(1)
        L.ph_debug_set_tap6(1)
    assert sig_off != sig_on
    _compare(got, *_net_reference(layers, "fp16x3", False, False), "fp16x3, PH_TAP5 = PH_TAP6 = 0")


def _selected_layout(L, op, geom, arith):
    """The layout the launch of `op` reads, from the selector: half-pair w_frag, or perf mode's copy when conv_tap7 / conv_tap6b run."""
    frag = ctypes.c_int(-1)
    m = L.ph_debug_conv2d_select(op, *geom, P.ARITHS[arith], None, ctypes.byref(frag))
    assert m >= 0, (op, geom, arith, m)
    fams = {f for i, f in enumerate(DISPATCH_FAMILIES) if m >> i & 1}
    if arith == "fp16x3":
        return WFRAG[frag.value]
    return "copy" if arith == "bf16" and fams & {"tap7", "tap6b"} else "row"


@pytest.mark.parametrize("case", P.CONVS, ids=[c[0] for c in P.CONVS])
def test_one_convolution(case):
    """After ph_conv2d_fwd / ph_conv2d_dgrad the head of the workspace holds the restatement's words wherever that launch's kernel reads,
    and the sentinel everywhere else in the weight region."""
    from multimodal_learning_amd._lib import check, ptr, stream
    L = _lib()
    name, Cin, Cout, KS, S, pad, ariths = case
    B, IH, IW = 1, 8, 8
    OH, OW = (IH + 2 * pad - KS) // S + 1, (IW + 2 * pad - KS) // S + 1
    geom = (B, Cin, IH, IW, Cout, KS, S, pad)
    w = P.random_weights([(Cout, Cin, KS, KS)], 5)[0]
    wd = torch.from_numpy(w).cuda()
    n = w.size
    nws = L.ph_conv2d_workspace_bytes(*geom)
    g = torch.Generator().manual_seed(3)
    for arith in ariths:
        prec = P.ARITHS[arith]
        odt = torch.bfloat16 if arith == "bf16" else torch.float32

        def act(shape):
            t = torch.randn(shape, generator=g).cuda()
            return t.bfloat16() if arith == "bf16" else (hp_pack(t) if arith == "fp16x3" else t)
        for op, dgrad in ((0, False), (1, True)):
            layout = _selected_layout(L, op, geom, arith)
            # (the selector's answer is the documented rule: a switch or predicate change must not quietly thin this test out)
            assert layout == P.plan_layouts([(Cout, Cin, KS, S)], arith)[0][dgrad], (name, arith, op, layout)
            ws = torch.full((nws,), SENTINEL, dtype=torch.uint8, device="cuda")
            if op == 0:
                x, y = act((B, IH, IW, Cin)), torch.empty((B, OH, OW, Cout), dtype=odt, device="cuda")
                rc = L.ph_conv2d_fwd(ptr(x), ptr(wd), ptr(y), None, None, B, Cin, IH, IW, Cout, KS, S, pad, prec, ptr(ws), stream())
            else:
                dy, dx = act((B, OH, OW, Cout)), torch.empty((B, IH, IW, Cin), dtype=odt, device="cuda")
                rc = L.ph_conv2d_dgrad(ptr(dy), ptr(wd), ptr(dx), B, Cin, IH, IW, Cout, KS, S, pad, prec, ptr(ws), stream())
            check(rc, f"{name} {arith} op {op}")
            torch.cuda.synchronize()
            got = ws[:2 * P.NPLANES * n].cpu().numpy().view(np.uint16)
            _compare(got, *P.pack_conv(w, arith, dgrad, layout), f"{name} {arith} {'dgrad' if dgrad else 'fwd'} ({layout})")

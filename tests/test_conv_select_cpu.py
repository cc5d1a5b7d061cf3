"""The convolution kernel selector (csrc/conv_select.hip: ph_tapconv_select) without a GPU, through the host-only debug entry
ph_debug_conv2d_select, which builds the descriptors of ph_conv2d_fwd / ph_conv2d_dgrad with the shared builders and makes no HIP
call.  The family table is the one tests/test_gpu_conv_sweep.py asserts against the real dispatch record, so the two cannot drift
apart.  With no device ph_num_cus() is 256."""
import ctypes

import pytest

from tests.conv_emulation import BF16, BF16X6, BF16X3, FP16X3, FP16X1, NAMES
from tests.conv_sweep_cases import CASES, REJECTED, expected_family
from tests.gpu_util import DISPATCH_FAMILIES

EINVAL = -22
PRECS = (BF16, BF16X6, BF16X3, FP16X3, FP16X1)
OPS = {"fwd": 0, "dgrad": 1}
WFRAG_ROW, WFRAG_TAP5, WFRAG_TAP6 = 0, 1, 2


def _lib():
    import multimodal_learning_amd as m
    L = m.lib()
    L.ph_conv2d_workspace_bytes.restype = ctypes.c_size_t
    return L


def _select(L, case, op, prec):
    """(families, stat_parts, w_frag) of the launches `op` of `case` would make; families None = PH_EINVAL."""
    Cin, Cout, IH, IW, KS, S, pad, B = CASES[case]
    parts, frag = ctypes.c_int(-1), ctypes.c_int(-1)
    m = L.ph_debug_conv2d_select(OPS[op], B, Cin, IH, IW, Cout, KS, S, pad, prec, ctypes.byref(parts), ctypes.byref(frag))
    if m < 0:
        assert m == EINVAL, m
        return None, None, None
    return {f for i, f in enumerate(DISPATCH_FAMILIES) if m >> i & 1}, parts.value, frag.value


@pytest.mark.parametrize("prec", PRECS, ids=[NAMES[p] for p in PRECS])
def test_family_of_every_sweep_case(prec):
    L = _lib()
    for case in CASES:
        for op in OPS:
            want = expected_family(case, op, prec)
            got, _, _ = _select(L, case, op, prec)
            assert got == (None if want is None else {want}), (case, op, NAMES[prec], got, want)


def test_row_count_within_bound_and_workspace():
    """What the max() calls of the workspace sizing stood in for: the rows a forward launch writes fit the bound of its arithmetic
    (at the convolution's stride, or stride 1 where a stride-2 convolution is routed to a stride-1 launch) and the workspace."""
    L = _lib()
    up = lambda n: (n + 255) // 256 * 256
    n = 0
    for case, (Cin, Cout, IH, IW, KS, S, pad, B) in CASES.items():
        OH, OW = (IH + 2 * pad - KS) // S + 1, (IW + 2 * pad - KS) // S + 1
        for prec in PRECS:
            fam, parts, _ = _select(L, case, "fwd", prec)
            if fam is None:
                continue
            bound = max(L.ph_tapconv_stat_parts_bound(B, OH, OW, Cout, s, prec) for s in range(1, S + 1))
            assert 1 <= parts <= bound, (case, NAMES[prec], fam, parts, bound)
            ws = L.ph_conv2d_workspace_bytes(B, Cin, IH, IW, Cout, KS, S, pad)
            assert up(3 * KS * KS * Cin * Cout * 2) + parts * 2 * Cout * 4 <= ws, (case, NAMES[prec], parts, ws)
            n += 1
    assert n == 4 * (len(CASES) - 3)      # two rejected geometries, l1_s2 forward; fp16x1 is a backward arithmetic


# switch off -> (case, arithmetic, ops, family reached)
FALLBACKS = [
    ("tap4", "l1", BF16, ("fwd", "dgrad"), "tap2_l1"),
    ("tap7", "c128_128", BF16, ("fwd", "dgrad"), "tap3"),
    ("tap3", "c128_256", BF16, ("fwd", "dgrad"), "tap2"),
    ("tap3", "c128_256", FP16X3, ("fwd", "dgrad"), "gen1_hp16"),
    ("tap5", "l1", FP16X3, ("fwd", "dgrad"), "gen1_hp16"),
    ("tap6", "s2_128_256", FP16X3, ("fwd",), "gen1_hp16"),
    ("tap6b", "s2_128_256_big", BF16, ("fwd",), "tap2_masked"),      # even map: the masked grid
    ("tap6b", "s2_128_256", BF16, ("fwd",), "gen1_bf16"),            # odd map: the first generation
]


@pytest.mark.parametrize("switch,case,prec,ops,want", FALLBACKS, ids=[f"{f[0]}-{f[1]}-{NAMES[f[2]]}" for f in FALLBACKS])
def test_fallback_with_a_switch_off(switch, case, prec, ops, want):
    L = _lib()
    setter = getattr(L, "ph_debug_set_" + switch)
    for op in ops:
        assert _select(L, case, op, prec)[0] == {expected_family(case, op, prec)}
    setter(0)
    try:
        for op in ops:
            assert _select(L, case, op, prec)[0] == {want}, (switch, case, op)
    finally:
        setter(1)


def test_weight_layout_of_every_sweep_case():
    L = _lib()
    by_family = {"tap5": WFRAG_TAP5, "tap6": WFRAG_TAP6}
    for case in CASES:
        for op in OPS:
            for prec in PRECS:
                fam, _, frag = _select(L, case, op, prec)
                if fam is not None:
                    assert frag == by_family.get(expected_family(case, op, prec), WFRAG_ROW), (case, op, NAMES[prec], frag)
    for prec in (FP16X3, FP16X1):
        assert _select(L, "l1", "dgrad", prec)[2] == WFRAG_TAP5
    assert _select(L, "l1", "fwd", FP16X3)[2] == WFRAG_TAP5
    for case in ("s2_128_256", "s2_192_384", "s2_128_256_big"):
        assert _select(L, case, "fwd", FP16X3)[2] == WFRAG_TAP6
        assert _select(L, case, "fwd", BF16)[2] == WFRAG_ROW


def test_workspace_covers_the_weight_gradient_slab():
    """ph_conv2d_wgrad writes a 256-byte zero page and one fp32 [KS * KS][Cout][Cin] slab plane per chunk it launches with
    (ph_debug_conv2d_wgrad_chunks: the same plan_wgrad call, no HIP call); ph_conv2d_workspace_bytes must cover that.  A 1x1 /
    stride-2 convolution is launched through the stride-1 view (tile height 8, not 4) and the chunk count is not monotone in the
    tile count: the sizing once took 170 chunks for the first named shape where the launch used 180 (5 619 968 B reported, 5 898 496
    written), and 130 against 140 for the second."""
    L = _lib()
    shapes = [(B, Cin, IH, IW, Cout, KS, S, pad) for name, (Cin, Cout, IH, IW, KS, S, pad, B) in CASES.items() if name not in REJECTED]
    named = [(4, 64, 130, 130, 128, 1, 2, 0), (5, 64, 98, 98, 128, 1, 2, 0)]
    sweep = [(B, Cin, 2 * OH, 2 * OH, Cout, 1, 2, 0) for (Cin, Cout) in ((64, 128), (128, 256), (256, 512))
             for B in range(1, 9) for OH in range(1, 70)]
    for a in shapes + named + sweep:
        B, Cin, IH, IW, Cout, KS, S, pad = a
        chunks = L.ph_debug_conv2d_wgrad_chunks(*a)
        assert chunks >= 1, a
        assert L.ph_conv2d_workspace_bytes(*a) >= 256 + chunks * KS * KS * Cin * Cout * 4, (a, chunks)
    for a in named:      # (what the two named shapes launch with)
        assert L.ph_debug_conv2d_wgrad_chunks(*a) == {130: 180, 98: 140}[a[2]]
    for name in REJECTED:
        Cin, Cout, IH, IW, KS, S, pad, B = CASES[name]
        assert L.ph_debug_conv2d_wgrad_chunks(B, Cin, IH, IW, Cout, KS, S, pad) == EINVAL

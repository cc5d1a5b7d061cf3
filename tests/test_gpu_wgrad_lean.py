"""The lean tile loop of the perf-mode weight gradient (conv_wgrad.hip, wgrad_kernel<.., LEAN = true>: x fragments read once per
halo row, LDS-DMA sources from per-lane offsets and per-tile validity words, pieces issued inside the MFMA stream) against the
loop it replaces (PH_WG_LEAN off, ph_debug_set_wg_lean(0)), through ph_conv2d_wgrad.  For every case

  * dw of the lean arm is BITWISE dw of the old arm (same operands, same MFMAs, same order per accumulator);
  * dw of the lean arm meets the emulated-arithmetic reference (tests/conv_emulation.py) at the tolerance the dispatch sweep
    (tests/test_gpu_conv_sweep.py) applies to that arithmetic, conv_emulation.TAU, with the sweep's sparse dy operand;
  * the output's guard bands and the workspace's sentinel tail are untouched, no output element is left unwritten.

The shapes are the smallest at which the new code can go wrong: one tile (prologue only, the dz window never full), 2 x 2 tiles
with one valid row and column (validity words on every border, zero page), one tile per chunk (every workgroup starts on another
tile and image), Cin != Cout with partial last tile row and column, two Cin blocks with one tile column, 64 blocks with three
tiles per chunk, and (added here) four tiles per chunk with a shorter last chunk, so that chunks cross images and either LDS
buffer is the last one.  The half-pair arithmetics run the same loop three times / once per chunk.  One 3x3 / stride-2 and one
1x1 / stride-2 case cover the precomputed offsets in front of the plain loop and the strided 1x1 view."""
import pytest
import torch

from tests import conv_emulation as E
from tests.conv_sweep_cases import WGRAD
from tests.gpu_util import GUARD, SENTINEL, Guarded, dispatch_lib, dispatched, hp_pack, nhwc

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W), 3x3 / stride 1 / pad 1
S1_CASES = [
    (1, 64, 64, 8, 16),
    (1, 64, 64, 9, 17),
    (5, 64, 64, 16, 32),
    (3, 64, 128, 20, 40),
    (2, 128, 128, 24, 16),
    (2, 512, 512, 24, 48),
    (3, 512, 512, 24, 48),      # 27 tiles in chunks of 4, the last one of 3
]
S1_RUNS = [(c, E.BF16) for c in S1_CASES] + [(c, prec) for c in (S1_CASES[1], S1_CASES[3]) for prec in (E.FP16X3, E.FP16X1)]
# (B, Cin, Cout, H, W, KS, pad), stride 2
S2_RUNS = [((2, 64, 128, 18, 34, 3, 1), E.BF16), ((2, 64, 128, 18, 34, 1, 0), E.BF16)]


def _act(t, prec):
    return nhwc(t, torch.bfloat16) if prec == E.BF16 else hp_pack(nhwc(t, torch.float32))


def _check(B, Cin, Cout, H, W, KS, S, pad, prec):
    from multimodal_learning_amd._lib import ptr, stream
    L = dispatch_lib()
    x, _, dy, dy_w, geom = E.operands(B, Cin, H, W, Cout, KS, S, pad, seed=B + Cin + Cout + H + W + KS)
    xd, dyd = _act(x, prec), _act(dy_w, prec)
    nws = L.ph_conv2d_workspace_bytes(B, Cin, H, W, Cout, KS, S, pad)

    def run(dyd=dyd):
        ws = torch.full((nws + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = Guarded((Cout, Cin, KS, KS), torch.float32)
        L.ph_debug_dispatch_reset()
        rc = L.ph_conv2d_wgrad(ptr(xd), ptr(dyd), ptr(out.t), B, Cin, H, W, Cout, KS, S, pad, prec, ptr(ws), stream())
        torch.cuda.synchronize()
        assert rc == 0, f"rc {rc}"
        assert dispatched(L) == {WGRAD[prec]}
        assert out.guards_intact(), "output guard band overwritten"
        assert bool((ws[nws:] == SENTINEL).all()), "workspace written past ph_conv2d_workspace_bytes"
        return out.t.clone()

    # (the bitwise comparison also with the DENSE dy: every pixel of every tile then contributes to every gradient word)
    dyd_dense = _act(dy, prec)
    lean, lean_dense = run(), run(dyd_dense)
    assert L.ph_debug_set_wg_lean(0) == 0
    try:
        old, old_dense = run(), run(dyd_dense)
    finally:
        assert L.ph_debug_set_wg_lean(1) == 1
    assert not torch.isnan(lean).any() and not torch.isnan(lean_dense).any(), "output elements never written"
    ndiff = int((lean.view(torch.int32) != old.view(torch.int32)).sum())
    ndiff += int((lean_dense.view(torch.int32) != old_dense.view(torch.int32)).sum())
    ref = E.emulate("wgrad", prec, x, dy_w, geom)
    e = E.excess(ref, lean.cpu(), False)
    print(f"\n   wgrad lean {E.NAMES[prec]} {(B, Cin, Cout, H, W, KS, S)}: {ndiff} words differ from the old loop, "
          f"excess {e:.2e} tau {E.TAU[prec]:.1e}")
    assert ndiff == 0, f"{ndiff} of {lean.numel()} gradient words differ from the old loop"
    assert e <= E.TAU[prec], f"excess {e:.2e} > tau {E.TAU[prec]:.1e}"


@pytest.mark.parametrize("case,prec", S1_RUNS, ids=lambda v: E.NAMES[v] if isinstance(v, int) else "x".join(map(str, v)))
def test_wgrad_lean_3x3_stride1(case, prec):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, Cin, Cout, H, W = case
    _check(B, Cin, Cout, H, W, 3, 1, 1, prec)


@pytest.mark.parametrize("case,prec", S2_RUNS, ids=lambda v: E.NAMES[v] if isinstance(v, int) else "x".join(map(str, v)))
def test_wgrad_lean_stride2(case, prec):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, Cin, Cout, H, W, KS, pad = case
    _check(B, Cin, Cout, H, W, KS, 2, pad, prec)

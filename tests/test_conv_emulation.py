"""CPU self-test of the convolution sweep's tolerances (tests/conv_emulation.py TAU): at every shape class of the sweep and
in every arithmetic, the emulation with float32 accumulation (a stand-in for a kernel's fp32 accumulation noise) passes with a
margin of at least 4, and the emulation with any ONE product left out fails with a margin of at least 4.  For bf16x6 the latter
includes bf16x3 (its three low products each missing)."""
import pytest
import torch

from tests import conv_emulation as E
from tests.conv_sweep_cases import CASES, REJECTED

MARGIN = 4.0
OPS = ("fwd", "dgrad", "wgrad")


def _precs(op):
    return (E.BF16, E.BF16X6, E.BF16X3, E.FP16X3) + ((E.FP16X1,) if op != "fwd" else ())


@pytest.mark.parametrize("case", [c for c in CASES if c not in REJECTED and not c.endswith("_big")])
def test_tolerance_accepts_fp32_noise_and_rejects_a_missing_product(case):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    Cin, Cout, IH, IW, KS, S, pad, B = CASES[case]
    x, w, dy, dy_w, geom = E.operands(B, Cin, IH, IW, Cout, KS, S, pad, seed=Cin + Cout + IH)
    ab = {"fwd": (x, w), "dgrad": (dy, w), "wgrad": (x, dy_w)}
    rows, bad = [], []
    for op in OPS:
        a, b = ab[op]
        for prec in _precs(op):
            tau = E.TAU[prec]
            perf = prec == E.BF16 and op != "wgrad"
            ref = E.emulate(op, prec, a, b, geom)
            noisy = E.emulate(op, prec, a, b, geom, acc=torch.float32, round_out=perf)
            acc = E.excess(ref, noisy, perf)
            rows.append((op, E.NAMES[prec], "fp32", acc, tau))
            if acc * MARGIN > tau:
                bad.append((op, E.NAMES[prec], "accepts", acc))
            if len(E.PRODUCTS[prec]) > 1:
                for k in range(len(E.PRODUCTS[prec])):
                    wrong = E.emulate(op, prec, a, b, geom, acc=torch.float32, drop=k)
                    rej = E.excess(ref, wrong, perf)
                    rows.append((op, E.NAMES[prec], f"-{E.PRODUCTS[prec][k][:2]}", rej, tau))
                    if rej < MARGIN * tau:
                        bad.append((op, E.NAMES[prec], f"rejects {E.PRODUCTS[prec][k][:2]}", rej))
    for r in rows:
        print("  %-6s %-7s %-10s excess %.3e  tau %.1e" % r)
    assert not bad, bad

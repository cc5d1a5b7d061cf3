"""Dispatch sweep of the convolution entry points (ph_conv2d_fwd / _dgrad / _dgrad_res / _wgrad): every case of
tests/conv_sweep_cases.py in every arithmetic, against the emulated-arithmetic reference (tests/conv_emulation.py) with the
tolerances its CPU self-test (tests/test_conv_emulation.py) shows to accept fp32 accumulation noise and to reject any one
missing product.  Each call also asserts
  * the kernel family it reached (ph_debug_dispatch_mask), so that a predicate change cannot quietly stop covering a kernel;
  * no stray writes: outputs are NaN-filled inside guard bands of a sentinel pattern (256-B aligned), the workspace has a sentinel
    tail past ph_conv2d_workspace_bytes, both are bitwise unchanged afterwards and no NaN is left in the output;
  * rejected calls (geometry, or fp16x1 forward) return PH_EINVAL and leave the guarded output bitwise untouched.

Measured on the MI355X: the largest excess per arithmetic was bf16 7.5e-8, bf16x6 5.4e-7 (c128_128 dgrad), bf16x3 4.1e-7, fp16x3
5.0e-7, fp16x1 2.4e-7 of max |ref|.  For bf16x6 that is 4.5 x the CPU float32 stand-in's 1.2e-7 (the MFMAs accumulate the six
products of a k-step into one fp32 register set) and 0.9 of tau: a margin of only 1.1.  The kernels and operands are
deterministic, so this is not a flaky margin, but a change of the kernels' accumulation order can use it up; re-measure then.  The
smallest single missing product, 2.4e-6 = 4.05 tau, is the CPU emulation's figure (a kernel cannot be made to drop a product on
the GPU); nothing measured on the GPU bounds it."""
import ctypes

import pytest
import torch

from tests import conv_emulation as E
from tests.conv_sweep_cases import CASES, expected_family
from tests.gpu_util import GUARD, SENTINEL, Guarded, dispatch_lib, dispatched

pytestmark = pytest.mark.gpu

EINVAL = -22


def _workspace(L, B, Cin, IH, IW, Cout, KS, S, pad):
    n = L.ph_conv2d_workspace_bytes(B, Cin, IH, IW, Cout, KS, S, pad)
    ws = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return ws, n


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _to_act(x, prec):
    """NCHW fp32 cpu -> the NHWC activation the entry points read in arithmetic `prec`."""
    from tests.gpu_util import hp_pack
    t = _nhwc(x)
    if prec == E.BF16:
        return t.bfloat16()
    if prec in (E.FP16X3, E.FP16X1):
        return hp_pack(t)
    return t


def _nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def _run_case(name, precs, ops):
    from multimodal_learning_amd._lib import ptr, stream
    L = dispatch_lib()
    Cin, Cout, IH, IW, KS, S, pad, B = CASES[name]
    OH = (IH + 2 * pad - KS) // S + 1
    OW = (IW + 2 * pad - KS) // S + 1
    x, w, dy, dy_w, geom = E.operands(B, Cin, IH, IW, Cout, KS, S, pad, seed=Cin + Cout + IH)
    wd = w.cuda()
    rows, bad = [], []
    for prec in precs:
        perf = prec == E.BF16
        adt = torch.bfloat16 if perf else torch.float32
        xd, dyd, dywd = _to_act(x, prec), _to_act(dy, prec), _to_act(dy_w, prec)
        for op in ops:
            fam = expected_family(name, "dgrad" if op.startswith("dgrad") else op, prec)
            if S == 2 and KS == 1 and op in ("dgrad_res", "dgrad_res_masked"):
                fam = None      # (1x1 / stride 2: the classes no tap reaches take the residual in place only)
            what = f"{name} {op} {E.NAMES[prec]}"
            ws, nws = _workspace(L, B, Cin, IH, IW, Cout, KS, S, pad)
            L.ph_debug_dispatch_reset()
            extra = {}
            if op == "fwd":
                out = Guarded((B, OH, OW, Cout), adt)
                s1, s2 = Guarded((Cout,), torch.float32), Guarded((Cout,), torch.float32)
                extra = {"s1": s1, "s2": s2}
                before = out.snapshot()
                rc = L.ph_conv2d_fwd(ptr(xd), ptr(wd), ptr(out.t), ptr(s1.t), ptr(s2.t), B, Cin, IH, IW, Cout, KS, S, pad, prec,
                                     ptr(ws), stream())
            elif op == "wgrad":
                out = Guarded((Cout, Cin, KS, KS), torch.float32)
                before = out.snapshot()
                rc = L.ph_conv2d_wgrad(ptr(xd), ptr(dywd), ptr(out.t), B, Cin, IH, IW, Cout, KS, S, pad, prec, ptr(ws), stream())
            else:
                out = Guarded((B, IH, IW, Cin), adt)
                res_g = res_a = None
                if op == "dgrad":
                    before = out.snapshot()
                    rc = L.ph_conv2d_dgrad(ptr(dyd), ptr(wd), ptr(out.t), B, Cin, IH, IW, Cout, KS, S, pad, prec, ptr(ws),
                                           stream())
                else:
                    g = torch.Generator().manual_seed(7)
                    rg = torch.randn(B, Cin, IH, IW, generator=g)
                    ra = torch.randn(B, Cin, IH, IW, generator=g) if op == "dgrad_res_masked" else None
                    if perf:
                        rg = rg.bfloat16().float()
                    rgd = _nhwc(rg).to(adt)
                    if op == "dgrad_res_inplace":
                        out.t.copy_(rgd)
                        rgd = out.t
                    rad = None if ra is None else _nhwc(ra).to(adt)
                    res_g, res_a = rg, ra
                    before = out.snapshot()
                    rc = L.ph_conv2d_dgrad_res(ptr(dyd), ptr(wd), ptr(out.t), ptr(rgd), ptr(rad), B, Cin, IH, IW, Cout, KS, S,
                                               pad, prec, ptr(ws), stream())
            torch.cuda.synchronize()
            got_fams = dispatched(L)
            if fam is None:
                ok = rc == EINVAL and torch.equal(out.buf, before)
                rows.append((what, f"rc {rc} (rejected)", ok))
                if not ok:
                    bad.append(f"{what}: expected PH_EINVAL and an untouched output, got rc {rc}")
                continue
            if rc != 0:
                bad.append(f"{what}: rc {rc}")
                continue
            if got_fams != {fam}:
                bad.append(f"{what}: dispatched {sorted(got_fams)}, expected {fam}")
            if not out.guards_intact() or not all(t.guards_intact() for t in extra.values()):
                bad.append(f"{what}: output guard band overwritten")
            if not bool((ws[nws:] == SENTINEL).all()):
                bad.append(f"{what}: workspace written past ph_conv2d_workspace_bytes")
            got = out.t.float().cpu()
            if torch.isnan(got).any():
                bad.append(f"{what}: {int(torch.isnan(got).sum())} output elements never written")
                continue
            if op == "fwd":
                ref = E.emulate("fwd", prec, x, w, geom)
                gotn = _nchw(out.t)
                e = E.excess(ref, gotn, perf)
                # channel sums: the float64 sums of the unrounded emulated outputs
                es1 = E.excess(ref.sum(dim=(0, 2, 3)), s1.t.cpu(), False)
                es2 = E.excess((ref ** 2).sum(dim=(0, 2, 3)), s2.t.cpu(), False)
                stol = 4 * E.TAU[prec] if not perf else 2e-3      # perf mode: the sums are of the fp32 tile values
                rows.append((what + " sum", f"{es1:.2e} / {es2:.2e} tol {stol:.1e}", es1 <= stol and es2 <= stol))
                if not (es1 <= stol and es2 <= stol):
                    bad.append(f"{what}: channel sums {es1:.2e} / {es2:.2e} > {stol:.1e}")
            elif op == "wgrad":
                ref = E.emulate("wgrad", prec, x, dy_w, geom)
                e = E.excess(ref, out.t.cpu(), False)
            else:
                d = E.emulate("dgrad", prec, dy, w, geom)
                allow = None
                if res_g is not None:
                    r = res_g.double() if res_a is None else res_g.double() * (res_a.to(adt).float() > 0)
                    # perf mode: dx = bf16(bf16(dgrad) + res): the inner rounding of the kernel's fp32 sum may fall either way
                    allow = E.bf16_half_ulp(d) if perf else None
                    d = d + r
                e = E.excess(d, _nchw(out.t), perf, allow)
            tau = E.TAU[prec]
            rows.append((what, f"excess {e:.2e} tau {tau:.1e} [{fam}]", e <= tau))
            if e > tau:
                bad.append(f"{what}: excess {e:.2e} > tau {tau:.1e}")
    print(f"\n== sweep {name}")
    for what, msg, ok in rows:
        print(f"   {what:<36s} {msg}{'' if ok else '   <-- FAIL'}")
    assert not bad, "\n".join(bad)


ALL = (E.BF16, E.BF16X6, E.BF16X3, E.FP16X3, E.FP16X1)


@pytest.mark.parametrize("name", list(CASES))
def test_conv_sweep(name):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    Cin, Cout, IH, IW, KS, S, pad, B = CASES[name]
    ops = ["fwd", "dgrad", "wgrad", "dgrad_res", "dgrad_res_masked"] + (["dgrad_res_inplace"] if S == 2 else [])
    # (dgrad_res: res_g / res_a in the output's type - bf16 in perf mode, fp32 in the split and half-pair arithmetics, where the
    # epilogue reads them as the fp32 copies the plan's elementwise passes keep)
    _run_case(name, ALL, ops)

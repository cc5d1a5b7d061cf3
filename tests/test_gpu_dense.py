"""Sweep of the dense fp32 entry points (csrc/dense.hip) through the C ABI, against tests/dense_emulation.py.

  exact class   both GEMMs (every stride form, bias, accumulate, ldc > N, ReLU, the K remainders of each kernel, both sides of the
                size rule, split-K with nsplit above K / 32), ph_outer / ph_outer_bwd, ph_sum and the ops of ph_eltwise without a
                transcendental, on integer operands: bitwise equal to the int64 numpy result.
  real class    everything else against the float64 reference, within 4 x the float32 restatement's error on the same inputs plus
                the operator's floor (dense_emulation.FLOOR).
  dropout       the keep mask equals the numpy restatement of u01 exactly.
  ph_logit_losses   bitwise equal to the five kernels it replaces.

Every output lives in a NaN-filled buffer between sentinel guard bands: after each call the guards are intact, no NaN is left in
the written region and, where ldc > N, the padding columns are bitwise untouched.  Each GEMM row asserts the kernel it reached
(ph_debug_dispatch_mask).

Measured on the MI355X, the largest excess of the device's error over the float32 restatement's, in units of max |ref|, per
operator: sgemm_act 9.1e-8, bn1d_eval 4.2e-8, bn1d_eval_bwd 2.1e-8, log_softmax 4.1e-10, kl_bwd 6.5e-8, kl_rows_fwd 1.06e-6,
kl_rows_bwd 5.5e-8, conf_discrepancy 4.2e-7; dense_emulation.FLOOR is 4 x each.  splitk_act, log_softmax_bwd, kl_fwd,
eltwise_real, gate_bwd and the alpha dropout never exceeded the restatement (no floor), nor did bn1d_fwd, nll_fwd, nll_bwd,
l2norm_fwd and row_scale; l2norm_bwd 9.1e-9 and row_invnorm_scale 2.0e-9 have no transcendental and stay inside 4 x the
restatement.  bn1d_bwd's 6.9e-4 is of a dx column whose reference is 4e-6 (B = 2, the mean-1000 column), inside its tolerance.
ph_bn1d_fwd equals the restatement only with its two multiply-adds contracted to fmas, as hipcc compiles them: the uncontracted
form differs by up to 8.8e-5 in the mean-1000 column (B16 C130) - the same u |m| |sc| error, another draw of it.
Every test prints `excess[operator]` next to the floor; re-measure after a change of the kernels or of the toolchain.
The smallest injected-defect ratio of the CPU self-test (tests/test_dense_emulation_cpu.py) is 2.2e4 x the tolerance (one dropped
K element under the split-K sigmoid epilogue); biased running variance 2.3e4, dropped batch row 8.4e4, softmax without max
subtraction 2.3e5, missing 1/T 8.6e5, ReLU mask from x 5.2e6, dropout scale 1/p 1.9e7."""
import numpy as np
import pytest
import torch

from tests import dense_emulation as E
from tests.gpu_util import GUARD, Guarded, Report, dispatch_lib, dispatched

pytestmark = pytest.mark.gpu

EINVAL = -22
F32 = np.float32
EXCESS = {}         # operator -> largest (device error - restatement error) / max |ref| seen in this process


def _api():
    from multimodal_learning_amd._lib import ptr, stream
    return dispatch_lib(), ptr, stream()


_LIVE = []          # the operands of the running test: `ptr(dev(a))` inside an argument list must not free `a` before the launch


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _LIVE.clear()


def dev(a, dtype=None):
    """numpy array (or None) -> device tensor, kept alive until the test ends."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    _LIVE.append(torch.from_numpy(a.astype(dtype) if dtype is not None else a).cuda())
    return _LIVE[-1]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _collect(what, outs, bad):
    """Synchronise; guards intact and nothing left unwritten in every Guarded of `outs`; their contents as numpy arrays."""
    torch.cuda.synchronize()
    res = {}
    for k, G in outs.items():
        if not G.guards_intact():
            bad.append(f"{what} {k}: guard band overwritten")
        a = G.t.cpu().numpy()
        if a.dtype.kind == "f" and np.isnan(a).any():
            bad.append(f"{what} {k}: {int(np.isnan(a).sum())} elements never written (or NaN)")
        res[k] = a
    return res


def _bitwise(what, got, expect, bad):
    """`got` (float32) equals the integer array `expect` bit for bit."""
    exp = np.asarray(expect).astype(F32)
    same = got.reshape(exp.shape).view(np.int32) == exp.view(np.int32)
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        bad.append(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {i}: got {got.reshape(exp.shape)[i]!r} "
                   f"expected {exp[i]!r} (max |ref| {np.abs(exp).max():g})")
    return bool(same.all())


def _compare(R, e, got, bad):
    """The real class: every output array of suite entry `e` present in `got` against its tolerance."""
    op = e["op"]
    for k, a in got.items():
        ref, rest = e["ref"][k], e["rest"][k]
        tol, er, sc = E.entry_tolerance(e, k), E.err(ref, np.asarray(a).reshape(np.shape(ref))), E.scale(ref)
        if sc > 0:
            EXCESS[op] = max(EXCESS.get(op, 0.0), (er - E.err(ref, rest)) / sc)
        R.add(f"{e['name']} {k}", er, sc, tol)


def _finish(R, bad, ops=()):
    for op in ops:
        print(f"   excess[{op}] = {EXCESS.get(op, 0.0):.3e} of max |ref| (floor {E.FLOOR.get(op, 0.0):.1e})")
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad)


def _out(shape, dtype=torch.float32):
    return Guarded(tuple(shape), dtype)


# ------------------------------------------------------------------------------------------------ GEMM
def _sgemm_call(L, ptr, st, a, b, bias, G, M, N, K, strides, ldc, act, acc):
    sam, sak, sbk, sbn = strides
    return L.ph_sgemm(ptr(a), ptr(b), ptr(bias), ptr(G.t), M, N, K, sam, sak, sbk, sbn, ldc, act, acc, st)


def test_sgemm_exact():
    L, ptr, st = _api()
    bad, rows = [], []
    for n, c in enumerate(E.GEMM_CASES):
        M, N, K, form = c["M"], c["N"], c["K"], c["form"]
        what = "sgemm %dx%dx%d %s bias%d acc%d pad%d act%d" % (M, N, K, form, c["bias"], c["acc"], c["pad"], c["act"])
        A, B, a_s, b_s, strides = E.gemm_operands(M, N, K, form, 1)
        rng = np.random.default_rng([2, n])
        bias = rng.integers(-4, 5, size=N) if c["bias"] else None
        prior = rng.integers(-4, 5, size=(M, N)) if c["acc"] else None
        ldc = N + c["pad"]
        G = _out((M, ldc))
        if prior is not None:
            G.t[:, :N] = dev(prior, F32)
        before = G.snapshot()
        L.ph_debug_dispatch_reset()
        rc = _sgemm_call(L, ptr, st, dev(a_s), dev(b_s), dev(bias, F32), G, M, N, K, strides, ldc, c["act"], c["acc"])
        torch.cuda.synchronize()
        fam = dispatched(L)
        if rc != 0:
            bad.append(f"{what}: rc {rc}")
            continue
        if fam != {E.gemm_kernel(M, N)}:
            bad.append(f"{what}: dispatched {sorted(fam)}, expected {E.gemm_kernel(M, N)}")
        if not G.guards_intact():
            bad.append(f"{what}: guard band overwritten")
        if c["pad"]:
            was = before[GUARD:GUARD + G.nbytes].view(torch.float32).view(M, ldc)
            if not torch.equal(_bits(G.t[:, N:]), _bits(was[:, N:])):
                bad.append(f"{what}: padding columns written")
        got = G.t[:, :N].contiguous().cpu().numpy()
        if np.isnan(got).any():
            bad.append(f"{what}: {int(np.isnan(got).sum())} outputs never written")
            continue
        ok = _bitwise(what, got, E.gemm_exact(A, B, bias, prior, c["act"]), bad)
        rows.append(f"   {what:<52s} [{','.join(sorted(fam))}] {'bitwise' if ok else '<-- FAIL'}")
    print("\n== ph_sgemm, exact class\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)


def test_sgemm_activations():
    L, ptr, st = _api()
    R, bad = Report("ph_sgemm ELU / sigmoid epilogue"), []
    for e in E.suite("sgemm_act"):
        i = e["inp"]
        M, N, K = i["M"], i["N"], i["K"]
        G = _out((M, N))
        L.ph_debug_dispatch_reset()
        rc = _sgemm_call(L, ptr, st, dev(i["a"]), dev(i["b"]), dev(i["bias"]), G, M, N, K, i["strides"], N, i["act"], 0)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], {"c": G}, bad)
        if dispatched(L) != {E.gemm_kernel(M, N)}:
            bad.append(f"{e['name']}: dispatched {sorted(dispatched(L))}")
        _compare(R, e, got, bad)
    _finish(R, bad, ["sgemm_act"])


def _splitk_call(L, ptr, st, a, b, bias, G, P, nsplit, M, N, K, strides, ldc, act):
    sam, sak, sbk, sbn = strides
    return L.ph_sgemm_splitk(ptr(a), ptr(b), ptr(bias), ptr(G.t), ptr(P.t), nsplit, M, N, K, sam, sak, sbk, sbn, ldc, act, st)


def test_sgemm_splitk_exact():
    L, ptr, st = _api()
    bad, rows = [], []
    for n, c in enumerate(E.SPLITK_CASES):
        M, N, K, form, ns = c["M"], c["N"], c["K"], c["form"], c["nsplit"]
        what = "splitk %dx%dx%d nsplit %d %s bias%d act%d pad%d" % (M, N, K, ns, form, c["bias"], c["act"], c["pad"])
        A, B, a_s, b_s, strides = E.gemm_operands(M, N, K, form, 1)
        bias = np.random.default_rng([3, n]).integers(-4, 5, size=N) if c["bias"] else None
        ad, bd, biasd, ldc = dev(a_s), dev(b_s), dev(bias, F32), N + c["pad"]
        expect = E.gemm_exact(A, B, bias, None, c["act"])
        slabs = E.splitk_slabs(K, ns)
        first = None
        for rep in range(2):
            G, P = _out((M, ldc)), _out((ns * M * N,))      # `part` sized for the requested nsplit
            L.ph_debug_dispatch_reset()
            rc = _splitk_call(L, ptr, st, ad, bd, biasd, G, P, ns, M, N, K, strides, ldc, c["act"])
            torch.cuda.synchronize()
            if rc != 0:
                bad.append(f"{what}: rc {rc}")
                break
            if dispatched(L) != {"sgemm_splitk"}:
                bad.append(f"{what}: dispatched {sorted(dispatched(L))}")
            if not (G.guards_intact() and P.guards_intact()):
                bad.append(f"{what}: guard band of the output or of `part` overwritten")
            if not bool(torch.isnan(P.t[slabs * M * N:]).all()) or bool(torch.isnan(P.t[:slabs * M * N]).any()):
                bad.append(f"{what}: `part` is not exactly {slabs} written slabs")
            if c["pad"] and not bool(torch.isnan(G.t[:, N:]).all()):
                bad.append(f"{what}: padding columns written")
            got = G.t[:, :N].contiguous().cpu().numpy()
            if np.isnan(got).any():
                bad.append(f"{what}: {int(np.isnan(got).sum())} outputs never written")
                break
            ok = _bitwise(what, got, expect, bad)
            if first is None:
                first = got
            elif not np.array_equal(first.view(np.int32), got.view(np.int32)):
                bad.append(f"{what}: a repeated call differs")
        rows.append(f"   {what:<52s} {slabs:3d} slabs")
    print("\n== ph_sgemm_splitk, exact class\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)


def test_sgemm_splitk_activations():
    L, ptr, st = _api()
    R, bad = Report("ph_sgemm_splitk ELU / sigmoid epilogue"), []
    for e in E.suite("splitk_act"):
        i = e["inp"]
        M, N, K, ns = i["M"], i["N"], i["K"], i["nsplit"]
        G, P = _out((M, N)), _out((ns * M * N,))
        rc = _splitk_call(L, ptr, st, dev(i["a"]), dev(i["b"]), dev(i["bias"]), G, P, ns, M, N, K, i["strides"], N, i["act"])
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], {"c": G}, bad)
        if not P.guards_intact():
            bad.append(f"{e['name']}: guard band of `part` overwritten")
        _compare(R, e, got, bad)
    _finish(R, bad, ["splitk_act"])


def test_sgemm_splitk_rejects_nsplit_below_one():
    L, ptr, st = _api()
    G, P = _out((4, 4)), _out((16,))
    a = torch.ones(4, 40, device="cuda")
    for ns in (0, -1):
        assert _splitk_call(L, ptr, st, a, a, None, G, P, ns, 4, 4, 40, (40, 1, 1, 40), 4, 0) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(G.t).all()) and bool(torch.isnan(P.t).all())


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def test_bn1d():
    L, ptr, st = _api()
    R, bad = Report("BatchNorm1d"), []
    eps, mom = E.BN_EPS, E.BN_MOM
    for ef, ee, eb, eeb in zip(E.suite("bn1d_fwd"), E.suite("bn1d_eval"), E.suite("bn1d_bwd"), E.suite("bn1d_eval_bwd")):
        i = ef["inp"]
        B, C, relu = i["B"], i["C"], i["relu"]
        x, gamma, beta = dev(i["x"]), dev(i["gamma"]), dev(i["beta"])
        # training forward
        outs = {"y": _out((B, C)), "mean": _out((C,)), "invstd": _out((C,))}
        rm = rv = nbt = None
        if i["running"]:
            rm, rv, nbt = _out((C,)), _out((C,)), Guarded((1,), torch.int64, fill=int(i["nbt"]))
            rm.t.copy_(dev(i["rm"]))
            rv.t.copy_(dev(i["rv"]))
            outs.update(running_mean=rm, running_var=rv, nbt=nbt)
        rc = L.ph_bn1d_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(outs["y"].t), ptr(outs["mean"].t), ptr(outs["invstd"].t),
                           ptr(rm.t) if rm else None, ptr(rv.t) if rv else None, ptr(nbt.t) if nbt else None, B, C, eps, mom,
                           relu, st)
        assert rc == 0, (ef["name"], rc)
        got = _collect("fwd " + ef["name"], outs, bad)
        if i["running"] and int(got.pop("nbt")[0]) != int(i["nbt"]) + 1:
            bad.append(f"fwd {ef['name']}: num_batches_tracked not incremented by one")
        _compare(R, dict(ef, name="fwd " + ef["name"]), E.bn_split(got), bad)
        # eval forward
        G = _out((B, C))
        rc = L.ph_bn1d_eval(ptr(x), ptr(gamma), ptr(beta), ptr(dev(i["rm"])), ptr(dev(i["rv"])), ptr(G.t), B, C, eps, relu, st)
        assert rc == 0, (ee["name"], rc)
        _compare(R, dict(ee, name="eval " + ee["name"]), E.bn_split(_collect("eval " + ee["name"], {"y": G}, bad)), bad)
        # training backward, from the float32 mean / invstd / y of the reference forward
        ib = eb["inp"]
        outs = {"dx": _out((B, C))}
        if ib["dparams"]:
            outs.update(dgamma=_out((C,)), dbeta=_out((C,)))
        rc = L.ph_bn1d_bwd(ptr(dev(ib["g"])), ptr(dev(ib["y"])), ptr(x), ptr(dev(ib["mean"])), ptr(dev(ib["invstd"])), ptr(gamma),
                           ptr(outs["dx"].t), ptr(outs["dgamma"].t) if ib["dparams"] else None,
                           ptr(outs["dbeta"].t) if ib["dparams"] else None, B, C, relu, st)
        assert rc == 0, (eb["name"], rc)
        _compare(R, dict(eb, name="bwd " + eb["name"]), E.bn_split(_collect("bwd " + eb["name"], outs, bad)), bad)
        # eval backward
        ie = eeb["inp"]
        G = _out((B, C))
        rc = L.ph_bn1d_eval_bwd(ptr(dev(ie["g"])), ptr(dev(ie["y"])), ptr(gamma), ptr(dev(ie["rv"])), ptr(G.t), B, C, eps, relu, st)
        assert rc == 0, (eeb["name"], rc)
        _compare(R, dict(eeb, name="evbwd " + eeb["name"]), E.bn_split(_collect("evbwd " + eeb["name"], {"dx": G}, bad)), bad)
    _finish(R, bad, ["bn1d_fwd", "bn1d_eval", "bn1d_bwd", "bn1d_eval_bwd"])


# ------------------------------------------------------------------------------------------------ row operators
def _row_call(L, ptr, st, op, i):
    """Runs row operator `op` on the inputs of a suite entry; returns {name: Guarded}."""
    B, C, T, inv = i["B"], i["C"], i["T"], i["inv_bnorm"]
    ys, yt, grade = dev(i["ys"]), dev(i["yt"]), dev(i["grade"])
    if op == "log_softmax":
        o = {"y": _out((B, C))}
        rc = L.ph_log_softmax(ptr(ys), ptr(o["y"].t), B, C, st)
    elif op == "log_softmax_bwd":
        o = {"dx": _out((B, C))}
        rc = L.ph_log_softmax_bwd(ptr(dev(i["g"])), ptr(dev(i["pred"])), ptr(o["dx"].t), B, C, st)
    elif op == "nll_fwd":
        o = {"loss": _out((1,))}
        rc = L.ph_nll_fwd(ptr(dev(i["pred"])), ptr(grade), ptr(o["loss"].t), B, C, inv, st)
    elif op == "nll_bwd":
        o = {"dpred": _out((B, C))}
        rc = L.ph_nll_bwd(ptr(dev(i["gs"])), ptr(grade), ptr(o["dpred"].t), B, C, inv, st)
    elif op == "kl_fwd":
        o = {"loss": _out((1,))}
        rc = L.ph_kl_fwd(ptr(ys), ptr(yt), ptr(o["loss"].t), B, C, T, inv, st)
    elif op == "kl_bwd":
        o = {"dys": _out((B, C))}
        rc = L.ph_kl_bwd(ptr(dev(i["gs"])), ptr(ys), ptr(yt), ptr(o["dys"].t), B, C, T, inv, st)
    elif op == "kl_rows_fwd":
        o = {"sample_loss": _out((B,))}
        rc = L.ph_kl_rows_fwd(ptr(ys), ptr(yt), ptr(o["sample_loss"].t), B, C, T, st)
    elif op == "kl_rows_bwd":
        o = {"dys": _out((B, C))}
        rc = L.ph_kl_rows_bwd(ptr(dev(i["grow"])), ptr(ys), ptr(yt), ptr(o["dys"].t), B, C, T, st)
    else:
        o = {"out": _out((B,))}
        rc = L.ph_conf_discrepancy(ptr(ys), ptr(yt), ptr(grade), ptr(o["out"].t), B, C, i["cap"], st)
    assert rc == 0, (op, rc)
    return o


ROW_OPS = ("log_softmax", "log_softmax_bwd", "nll_fwd", "nll_bwd", "kl_fwd", "kl_bwd", "kl_rows_fwd", "kl_rows_bwd",
           "conf_discrepancy")


@pytest.mark.parametrize("op", ROW_OPS)
def test_row_operator(op):
    L, ptr, st = _api()
    R, bad = Report("ph_" + op), []
    for e in E.suite(op):
        _compare(R, e, E.row_split(_collect(e["name"], _row_call(L, ptr, st, op, e["inp"]), bad), e["inp"]), bad)
    if op == "conf_discrepancy":        # the cases reach both sides of the cap (in the rows that are not wide, too)
        caps = [(np.asarray(e["ref"]["out"]) >= 1.0).mean() for e in E.suite(op) if e["inp"]["cap"] == 1.0 and e["inp"]["B"] > 1]
        assert all(0.0 < c < 1.0 for c in caps), caps
    _finish(R, bad, [op])


@pytest.mark.parametrize("C", [3, 64])
def test_logit_losses_equal_the_separate_kernels_bitwise(C):
    L, ptr, st = _api()
    bad, T = [], 4.0
    # (with and without the wide rows: their terms of 1e4 absorb the roundings of every other row's in the one-block sums)
    for B, wide in [(B, w) for B in (1, 255, 256, 257, 600) for w in (True, False)]:
        i = E.row_inputs(dict(B=B, C=C, T=T), wide)
        inv = 1.0 / B
        ys, t1, t2, grade = dev(i["ys"]), dev(i["yt"]), dev(i["yt2"]), dev(i["grade"])
        fused = {"pred": _out((B, C)), "losses": _out((3,)), "dl": _out((3, B, C))}
        rc = L.ph_logit_losses(ptr(ys), ptr(t1), ptr(t2), ptr(grade), ptr(fused["pred"].t), ptr(fused["losses"].t),
                               ptr(fused["dl"].t), B, C, T, inv, st)
        assert rc == 0, rc
        sep = {k: _out((B, C)) for k in ("pred", "dkl1", "dkl2", "dpred", "dnll")}
        sep.update({k: _out((1,)) for k in ("kl1", "kl2", "nll")})
        one = torch.ones(1, device="cuda")
        rcs = [L.ph_log_softmax(ptr(ys), ptr(sep["pred"].t), B, C, st),
               L.ph_kl_fwd(ptr(ys), ptr(t1), ptr(sep["kl1"].t), B, C, T, inv, st),
               L.ph_kl_fwd(ptr(ys), ptr(t2), ptr(sep["kl2"].t), B, C, T, inv, st),
               L.ph_nll_fwd(ptr(sep["pred"].t), ptr(grade), ptr(sep["nll"].t), B, C, inv, st),
               L.ph_kl_bwd(ptr(one), ptr(ys), ptr(t1), ptr(sep["dkl1"].t), B, C, T, inv, st),
               L.ph_kl_bwd(ptr(one), ptr(ys), ptr(t2), ptr(sep["dkl2"].t), B, C, T, inv, st),
               L.ph_nll_bwd(ptr(one), ptr(grade), ptr(sep["dpred"].t), B, C, inv, st),
               L.ph_log_softmax_bwd(ptr(sep["dpred"].t), ptr(sep["pred"].t), ptr(sep["dnll"].t), B, C, st)]
        assert not any(rcs), rcs
        f, s = _collect(f"fused B{B}", fused, bad), _collect(f"separate B{B}", sep, bad)
        pairs = [("pred", f["pred"], s["pred"]), ("loss KL(t1)", f["losses"][0:1], s["kl1"]), ("loss KL(t2)", f["losses"][1:2], s["kl2"]),
                 ("loss NLL", f["losses"][2:3], s["nll"]), ("d KL(t1)", f["dl"][0], s["dkl1"]), ("d KL(t2)", f["dl"][1], s["dkl2"]),
                 ("d NLL", f["dl"][2], s["dnll"])]
        for name, a, b in pairs:
            same = a.view(np.int32) == b.view(np.int32)
            d = float(np.abs(a.astype(np.float64) - b).max())
            print(f"   B{B} C{C} wide{int(wide)} {name:<12s} {'bitwise' if same.all() else '<-- FAIL'}  max |diff| {d:.3e}  max |ref| {np.abs(b).max():.3e}")
            if not same.all():
                bad.append(f"B{B} C{C} wide{int(wide)} {name}: {int((~same).sum())} elements differ, max |diff| {d:.3e} of {np.abs(b).max():.3e}")
    assert not bad, "\n".join(bad)


def test_logit_losses_rejects_more_than_64_classes():
    L, ptr, st = _api()
    B, C = 4, 65
    x, grade = torch.zeros(B, C, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    outs = {"pred": _out((B, C)), "losses": _out((3,)), "dl": _out((3, B, C))}
    before = {k: G.snapshot() for k, G in outs.items()}
    rc = L.ph_logit_losses(ptr(x), ptr(x), ptr(x), ptr(grade), ptr(outs["pred"].t), ptr(outs["losses"].t), ptr(outs["dl"].t), B, C,
                           4.0, 0.25, st)
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert all(torch.equal(G.buf, before[k]) for k, G in outs.items())


# ------------------------------------------------------------------------------------------------ L2 normalise rows
@pytest.mark.parametrize("op", ["l2norm_fwd", "l2norm_bwd", "row_invnorm_scale", "row_scale"])
def test_l2_row_operator(op):
    L, ptr, st = _api()
    R, bad = Report("ph_" + op), []
    for e in E.suite(op):
        i = e["inp"]
        B, D, x = i["B"], i["D"], dev(i["x"])
        if op == "l2norm_fwd":
            o = {"y": _out((B, D)), "nrm": _out((B,))}
            rc = L.ph_l2norm_fwd(ptr(x), ptr(o["y"].t), ptr(o["nrm"].t), B, D, st)
        elif op == "l2norm_bwd":
            o = {"dx": _out((B, D))}
            rc = L.ph_l2norm_bwd(ptr(dev(i["g"])), ptr(dev(i["y"])), ptr(dev(i["nrm"])), ptr(o["dx"].t), B, D, st)
        elif op == "row_invnorm_scale":
            o = {"y": _out((B, D)), "inv": _out((B,))}
            rc = L.ph_row_invnorm_scale(ptr(x), ptr(o["y"].t), ptr(o["inv"].t), B, D, i["eps"], st)
        else:
            o = {"y": _out((B, D))}
            rc = L.ph_row_scale(ptr(x), ptr(dev(i["r"])), ptr(o["y"].t), B, D, st)
        assert rc == 0, (e["name"], rc)
        _compare(R, e, _collect(e["name"], o, bad), bad)
    _finish(R, bad, [op])


# ------------------------------------------------------------------------------------------------ elementwise, outer, sum
def test_eltwise_exact():
    L, ptr, st = _api()
    bad = []
    for n in E.ELTWISE_N:
        rng = np.random.default_rng([61, n])
        a, b = rng.integers(-4, 5, size=n), rng.integers(-4, 5, size=n)
        ad, bd = dev(a, F32), dev(b, F32)
        for code in E.EW_EXACT:
            G = _out((n,))
            assert L.ph_eltwise(ptr(ad), ptr(bd), ptr(G.t), n, code, st) == 0
            got = _collect(f"eltwise op{code} n{n}", {"o": G}, bad)["o"]
            # (float32 numpy on the integer operands: exact, and it keeps the sign of a zero product, which int64 has not)
            exp = E.eltwise(a, b, code, F32)
            assert np.array_equal(exp.astype(np.int64), E.eltwise(a, b, code, np.int64))
            _bitwise(f"eltwise op{code} n{n}", got, exp, bad)
    assert not bad, "\n".join(bad)


def test_eltwise_gate_and_elu_bwd():
    L, ptr, st = _api()
    R, bad = Report("ph_eltwise GATE / ELU_BWD"), []
    for e in E.suite("eltwise_real"):
        i = e["inp"]
        G = _out((i["n"],))
        assert L.ph_eltwise(ptr(dev(i["a"])), ptr(dev(i["b"])), ptr(G.t), i["n"], i["code"], st) == 0
        _compare(R, e, _collect(e["name"], {"o": G}, bad), bad)
    _finish(R, bad, ["eltwise_real"])


def test_gate_bwd():
    L, ptr, st = _api()
    R, bad = Report("ph_gate_bwd"), []
    for e in E.suite("gate_bwd"):
        i = e["inp"]
        o = {"dz": _out((i["n"],)), "dh": _out((i["n"],))}
        assert L.ph_gate_bwd(ptr(dev(i["g"])), ptr(dev(i["a"])), ptr(dev(i["b"])), ptr(o["dz"].t), ptr(o["dh"].t), i["n"], st) == 0
        _compare(R, e, _collect(e["name"], o, bad), bad)
    _finish(R, bad, ["gate_bwd"])


def test_outer_and_outer_bwd_exact():
    L, ptr, st = _api()
    bad = []
    for (B, D1, D2, ap) in E.OUTER_CASES:
        rng = np.random.default_rng([71, B, D1, D2, ap])
        o1, o2 = E._ints(rng, (B, D1), True), E._ints(rng, (B, D2), True)
        g = E._ints(rng, (B, (D1 + ap) * (D2 + ap)), True)
        what = f"outer B{B} {D1}x{D2} append_one {ap}"
        G = _out((B, (D1 + ap) * (D2 + ap)))
        assert L.ph_outer(ptr(dev(o1, F32)), ptr(dev(o2, F32)), ptr(G.t), B, D1, D2, ap, st) == 0
        _bitwise(what, _collect(what, {"o12": G}, bad)["o12"], E.outer_exact(o1, o2, ap), bad)
        o = {"do1": _out((B, D1)), "do2": _out((B, D2))}
        assert L.ph_outer_bwd(ptr(dev(g, F32)), ptr(dev(o1, F32)), ptr(dev(o2, F32)), ptr(o["do1"].t), ptr(o["do2"].t), B, D1, D2,
                              ap, st) == 0
        got = _collect(what + " bwd", o, bad)
        do1, do2 = E.outer_bwd_exact(g, o1, o2, ap)
        _bitwise(what + " do1", got["do1"], do1, bad)
        _bitwise(what + " do2", got["do2"], do2, bad)
    assert not bad, "\n".join(bad)


def test_sum_exact():
    L, ptr, st = _api()
    bad = []
    for n in E.SUM_N:
        x = E._ints(np.random.default_rng([81, n]), (n,), True)
        for sc in (1.0, 0.5):
            G = _out((1,))
            assert L.ph_sum(ptr(dev(x, F32)), ptr(G.t), n, sc, st) == 0
            got = _collect(f"sum n{n}", {"s": G}, bad)["s"]
            if got.view(np.int32)[0] != np.array([x.sum() * sc], dtype=F32).view(np.int32)[0]:
                bad.append(f"sum n{n} scale {sc}: got {got[0]!r}, expected {x.sum() * sc!r}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ dropout
def _ctr(step):
    return torch.full((1,), step, dtype=torch.int64, device="cuda")      # (the counter is a uint64; same bits)


def test_dropout_mask_values_and_forms():
    L, ptr, st = _api()
    R, bad = Report("dropout (alpha form and backward against float64)"), []
    for e in E.suite("dropout"):
        i = e["inp"]
        n, p, seed, off, step, alpha, what = i["n"], i["p"], i["seed"], i["offset"], i["step"], i["alpha"], e["name"]
        x, ctr = dev(i["x"]), _ctr(step)
        G = _out((n,))
        G.t.copy_(x)
        assert L.ph_dropout_dev(ptr(G.t), n, p, seed, off, ptr(ctr), alpha, st) == 0
        y = _collect(what, {"y": G}, bad)["y"]
        if not alpha:
            # (no x is 0: the zeros of y are the dropped elements)
            if not np.array_equal(y != 0, i["keep"]):
                bad.append(f"{what}: keep mask differs from the u01 restatement in {int(((y != 0) != i['keep']).sum())} places")
            if not np.array_equal(y.view(np.int32), e["rest"]["y"].view(np.int32)):
                bad.append(f"{what}: kept values are not x / (1 - p) in float32, or a dropped value is not +0")
        # out of place == in place; the host-counter entry == the device-counter entry at counter 0
        G2 = _out((n,))
        assert L.ph_dropout_dev_to(ptr(x), ptr(G2.t), n, p, seed, off, ptr(ctr), alpha, st) == 0
        if not np.array_equal(_collect(what + " _to", {"y": G2}, bad)["y"].view(np.int32), y.view(np.int32)):
            bad.append(f"{what}: ph_dropout_dev_to differs from ph_dropout_dev")
        if step == 0:
            G3 = _out((n,))
            G3.t.copy_(x)
            assert L.ph_dropout(ptr(G3.t), n, p, seed, off, alpha, st) == 0
            if not np.array_equal(_collect(what + " host", {"y": G3}, bad)["y"].view(np.int32), y.view(np.int32)):
                bad.append(f"{what}: ph_dropout differs from ph_dropout_dev at counter 0")
        # two calls over adjacent halves with shifted offsets == one call over the whole
        G4, h = _out((n,)), n // 2
        G4.t.copy_(x)
        assert L.ph_dropout_dev(ptr(G4.t[:h]), h, p, seed, off, ptr(ctr), alpha, st) == 0
        assert L.ph_dropout_dev(ptr(G4.t[h:]), n - h, p, seed, off + h, ptr(ctr), alpha, st) == 0
        if not np.array_equal(_collect(what + " halves", {"y": G4}, bad)["y"].view(np.int32), y.view(np.int32)):
            bad.append(f"{what}: two half calls differ from the whole")
        # backward: the forward's mask
        G5, G6 = _out((n,)), _out((n,))
        G5.t.copy_(x)
        assert L.ph_dropout_bwd_dev(ptr(G5.t), n, p, seed, off, ptr(ctr), alpha, st) == 0
        assert L.ph_dropout_bwd_dev_to(ptr(x), ptr(G6.t), n, p, seed, off, ptr(ctr), alpha, st) == 0
        dg = _collect(what + " bwd", {"dg": G5, "dg_to": G6}, bad)
        if not np.array_equal(dg["dg"] != 0, i["keep"]):
            bad.append(f"{what}: the backward's mask differs from the forward's")
        if not np.array_equal(dg["dg"].view(np.int32), dg["dg_to"].view(np.int32)):
            bad.append(f"{what}: ph_dropout_bwd_dev_to differs from ph_dropout_bwd_dev")
        _compare(R, e, {"y": y, "dg": dg["dg"]}, bad)
    _finish(R, bad, ["dropout"])


def test_dropout_p_zero_counter_and_kept_fraction():
    L, ptr, st = _api()
    n = 1000
    x = torch.randn(n, device="cuda")
    ctr = _ctr(5)
    for p in (0.0, -1.0):
        G = _out((n,))
        G.t.copy_(x)
        assert L.ph_dropout(ptr(G.t), n, p, 1, 0, 0, st) == 0 and L.ph_dropout_dev(ptr(G.t), n, p, 1, 0, ptr(ctr), 0, st) == 0
        assert L.ph_dropout_bwd_dev(ptr(G.t), n, p, 1, 0, ptr(ctr), 1, st) == 0
        G2, G3 = _out((n,)), _out((n,))
        assert L.ph_dropout_dev_to(ptr(x), ptr(G2.t), n, p, 1, 0, ptr(ctr), 0, st) == 0
        assert L.ph_dropout_bwd_dev_to(ptr(x), ptr(G3.t), n, p, 1, 0, ptr(ctr), 1, st) == 0
        torch.cuda.synchronize()
        for g in (G, G2, G3):
            assert g.guards_intact() and torch.equal(_bits(g.t), _bits(x))
    C = Guarded((1,), torch.int64, fill=5)
    assert L.ph_counter_inc(ptr(C.t), st) == 0
    torch.cuda.synchronize()
    assert C.guards_intact() and int(C.t[0]) == 6
    n = 1 << 20
    for p in (0.25, 0.5):
        G = _out((n,))
        G.t.fill_(1.0)
        assert L.ph_dropout(ptr(G.t), n, p, 99, 0, 0, st) == 0
        torch.cuda.synchronize()
        f = float((G.t != 0).double().mean())
        assert G.guards_intact() and abs(f - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (p, f)

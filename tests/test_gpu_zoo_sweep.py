"""Sweep of the relational and survival loss kernels through the C ABI - ph_rkd_loss_grad_part (csrc/zoo_rkd.hip), ph_rkd_loss_grad,
ph_pkt_loss_grad, ph_cox_loss_grad (csrc/zoo.hip) and the Cox terms of ph_surv_stage1_loss_grad (csrc/surv.hip) - at their tile,
stride and dispatch edges against the float64 references of tests/zoo_emulation.py (torch on the CPU, none of the project's kernels),
under that module's rule: the device's error is at most 4 x the float32 restatement's error on the same inputs plus the operator's
floor, in units of max |ref|, for the loss and for the gradient separately.

`loss`, `dx` and the workspace of every call live between sentinel guard bands (gpu_util.Guarded; the workspace is exactly
ph_*_workspace_bytes long) and are pre-filled with NaN: after each call the return code is PH_OK, the guards are intact and no NaN is
left in `loss` / `dx`; a second identical call gives the same bits.  A refused shape returns PH_EINVAL and leaves the prefill alone.

Measured on the MI355X, the largest excess of the device's error over the float32 restatement's, in units of max |ref| (loss / dx):
rkd_part 6.57e-8 (Bg = 3) / 3.34e-7 (Bg = 1024, one anchor); rkd 3.42e-7 / 5.87e-7 (both at 66 x 512); pkt 1.52e-6 (65 x 65: the KL
is a sum of B^2 terms of either sign, 1e-3 of their size) / 3.79e-7 (1030 x 24); cox 5.82e-8 (1025) / 1.18e-6 (4096).  The losses are
scalars one to four ulp32 off; the gradients' excess grows with the rows - 2.6e-7 at 64, 5.0e-7 at 1024, 1.2e-6 at 4096 for Cox -
as a serial float32 chain of that many terms does against torch's blocked sums, fma contraction and the device's sqrtf / logf / expf
on top.  zoo_emulation.FLOOR is 4 x each figure.  Every test prints `excess[operator output]` next to the floor; re-measure after a
change of the kernels or of the toolchain.
The smallest failing error / tolerance of the CPU self-test's injected defects (tests/test_zoo_emulation_cpu.py, with these floors):
tiled RKD - last partial row tile j or k dropped 6.0e3, dE columns past the last whole 64-chunk dropped 1.5e5, the 65th anchor skipped
2.0e4, the anchor's own -sum_j dv_ij missing 1.5e5, corr for 2 corr 248, the part's mean distance 2.8e3; one-workgroup RKD - rows >= 16
not revisited 3.0e4, columns >= 64 dropped from g[q] 1.1e5; PKT - row sums stopping at the last multiple of 64 1.6e4, pkt_finish at 16
rows 5.2e4, the projection term missing 4.2e4; Cox - `>` for `>=` infinite (an empty risk set), rows >= 1024 left out 1.5e3.
The sweep found two things wrong.  (1) test_rkdloss_where_the_one_workgroup_form_does_not_fit, 128 x 256 and 67 x 512:
RKDLoss raised (ph_rkd_loss_grad returns PH_EINVAL above 150 KiB of LDS, and every B <= 128 was sent there); it now asks
ph_rkd_one_workgroup_fits and runs the tiled kernels where the answer is no.  (2) test_fused_stage1_cox_terms_are_ph_cox_loss_grad_bitwise,
B = 1023 and 1025: 4 .. 7 gradient rows of the fused kernel one ulp from ph_cox_loss_grad's dtheta (`* (1 / B)` against `/ B`; at 4096
the two agree); cox_kernel now multiplies by 1 / B.  No kernel was found wrong beyond a last-place rounding.
With a scratch build in which the tiled angle kernel skipped the last partial k tile, the gather kernel lost the anchor's own term,
pkt_finish and the one-workgroup dv loop stopped after 16 rows and Cox compared with `>`, 44 of the 53 tests failed - every tiled case,
the one-workgroup RKD and PKT above 16 rows (93 reports of elements never written), every Cox case - each naming case, output and the
worst element; the 9 that passed run none of the changed lines.
"""
import numpy as np
import pytest
import torch

from tests import zoo_emulation as E
from tests.gpu_util import Guarded, Report

pytestmark = pytest.mark.gpu

OK, EINVAL = E.OK, E.EINVAL
F32 = torch.float32
EXCESS = {}         # (operator, output) -> largest (device error - restatement error) / max |ref| seen in this process


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(what, launch, outs, ws_bytes, bad, expect=OK):
    """launch(ptr of every output in `outs` order.., ptr of the workspace) -> rc, twice.  outs: {name: shape}.  Returns the first call's
    outputs as numpy arrays (None for a call that must be refused)."""
    _, ptr, _ = _api()
    assert ws_bytes % 4 == 0
    G = {k: Guarded(tuple(s), F32) for k, s in outs.items()}
    ws = Guarded((ws_bytes // 4,), F32) if ws_bytes else None
    before = {k: g.snapshot() for k, g in G.items()}
    args = [ptr(g.t) for g in G.values()] + ([ptr(ws.t)] if ws else [])
    rc = launch(*args)
    torch.cuda.synchronize()
    if expect != OK:
        if rc != expect:
            bad.append(f"{what}: returned {rc}, expected {expect}")
        for k, g in G.items():
            if not torch.equal(g.buf, before[k]):
                bad.append(f"{what} {k}: a refused call wrote the buffer")
        return None
    if rc != OK:
        bad.append(f"{what}: returned {rc}")
        return None
    first = {}
    for k, g in list(G.items()) + ([("workspace", ws)] if ws else []):
        if not g.guards_intact():
            bad.append(f"{what} {k}: guard band overwritten")
        if k != "workspace":
            n = int(torch.isnan(g.t).sum())
            if n:
                bad.append(f"{what} {k}: {n} of {g.t.numel()} elements never written (or NaN), first at "
                           f"{tuple(int(v[0]) for v in torch.nonzero(torch.isnan(g.t), as_tuple=True))}")
            first[k] = g.t.clone()
            g.t.fill_(float("nan"))
    if ws:
        ws.t.fill_(float("nan"))
    rc = launch(*args)
    torch.cuda.synchronize()
    if rc != OK:
        bad.append(f"{what}: the second call returned {rc}")
    for k, g in G.items():
        if not _bits_equal(first[k], g.t):
            bad.append(f"{what} {k}: a second identical call gives other bits")
        if not g.guards_intact():
            bad.append(f"{what} {k}: guard band overwritten by the second call")
    return {k: v.cpu().numpy().astype(np.float64) for k, v in first.items()}


def _compare(R, kind, e, got, bad, what, outs=None, ref=None, rest=None, factor=1.0):
    """Each output of `got` against the case's float64 reference under the rule (factor: the reference, and so the tolerance, scaled)."""
    op = E.base_op(kind)
    for o in outs or tuple(e["abs"]):
        r = np.asarray((ref or e["ref"])[o], np.float64) * factor
        rs = np.asarray((rest or e["rest"])[o], np.float64) * factor
        g = np.asarray(got[o], np.float64).reshape(r.shape)
        tol = E.tolerance(op, o, r, rs, e["abs"][o] * factor)
        er, sc = E.err(r, g), E.scale(r)
        if sc > 0 and np.isfinite(er) and not e["abs"][o]:          # (a case with an absolute allowance has no max |ref| to speak of)
            key = (op, "dx" if o == "dx_live" else o)
            EXCESS[key] = max(EXCESS.get(key, 0.0), (er - E.err(r, rs)) / sc)
        print(f"   {what} {o}: err {er:.3e} restatement {E.err(r, rs):.3e} tol {tol:.3e} max|ref| {sc:.3e}")
        if not er <= tol:
            with np.errstate(invalid="ignore"):
                d = np.abs(g - r)
            i = np.unravel_index(int(np.argmax(np.where(np.isnan(d), np.inf, d))), d.shape)
            bad.append(f"{op} {what} {o}: max |err| {er:.3e} > tol {tol:.3e}, worst at {tuple(int(v) for v in i)}: got {g[i]!r} expected {r[i]!r}")
        R.add(f"{what} {o}", er, sc, tol)


def _finish(R, bad, op):
    for o in ("loss", "dx"):
        print(f"   excess[{op} {o}] = {EXCESS.get((op, o), 0.0):.3e} of max |ref| (floor {E.FLOOR.get((op, o), 0.0):.1e})")
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad[:30])


def _dev(*ts):
    return tuple(t.contiguous().cuda() for t in ts)


# ------------------------------------------------------------------------------------------------ the tiled, anchor-partitioned RKD
def _rkd_part(what, f_s, f_t, lo, na, bad, expect=OK):
    L, ptr, st = _api()
    Bg, D = f_s.shape
    x, t = _dev(f_s, f_t)
    return _call(what, lambda loss, dx, ws: L.ph_rkd_loss_grad_part(ptr(x), ptr(t), Bg, D, lo, na, E.W_D, E.W_A, loss, dx, ws, st),
                 {"loss": (1,), "dx": (Bg, D)}, L.ph_rkd_part_workspace_bytes(Bg, D, na), bad, expect)


@pytest.mark.parametrize("case", E.RKD_PART_CASES, ids=lambda c: "Bg%d-D%d-lo%d-na%d" % c)
def test_rkd_part(case):
    """Each part against the float64 statement of what a part is (zoo_emulation.rkd_part_torch)."""
    R, bad, what = Report("rkd_part"), [], "Bg=%d D=%d lo=%d na=%d" % case
    e = E.case("rkd_part", case)
    got = _rkd_part(what, e["inp"]["f_s"], e["inp"]["f_t"], case[2], case[3], bad)
    if got:
        _compare(R, "rkd_part", e, got, bad, what)
    _finish(R, bad, "rkd_part")


@pytest.mark.parametrize("shape,ranges", E.RKD_PARTITIONS, ids=["%dx%d" % s for s, _ in E.RKD_PARTITIONS])
def test_rkd_parts_of_an_uneven_partition_meet_the_float64_whole(shape, ranges):
    """The parts, summed in rank order in float32 as the all-reduce does, against the float64 full-range result."""
    Bg, D = shape
    R, bad = Report("rkd_part, partition"), []
    e = E.case("rkd_part", (Bg, D, 0, Bg))
    loss, dx = np.zeros(1, np.float32), np.zeros((Bg, D), np.float32)
    for lo, na in ranges:
        got = _rkd_part(f"Bg={Bg} D={D} lo={lo} na={na}", e["inp"]["f_s"], e["inp"]["f_t"], lo, na, bad)
        assert got, bad
        loss, dx = loss + got["loss"].astype(np.float32), dx + got["dx"].astype(np.float32)
    _compare(R, "rkd_part", e, {"loss": loss, "dx": dx}, bad, f"Bg={Bg} D={D} sum of {len(ranges)} parts")
    _finish(R, bad, "rkd_part")


@pytest.mark.parametrize("rng", [(0, 70), (60, 10)], ids=["full", "lo60-na10"])
def test_rkd_part_with_coinciding_rows_and_a_zero_row(rng):
    """Student rows 3 and 64 equal (on both sides of the first tile boundary; the range [60, 70) holds one of the two as an anchor) while
    the teacher's differ, and student row 10 all zero: finite, and the reference's convention under the rule."""
    R, bad, what = Report("rkd_part, degenerate"), [], "70 x 48 lo=%d na=%d" % rng
    e = E.case("rkd_part_deg", rng)
    got = _rkd_part(what, e["inp"]["f_s"], e["inp"]["f_t"], rng[0], rng[1], bad)
    assert got, bad
    assert np.isfinite(got["loss"]).all() and np.isfinite(got["dx"]).all()
    _compare(R, "rkd_part_deg", e, got, bad, what)
    _finish(R, bad, "rkd_part")


# ------------------------------------------------------------------------------------------------ the one-workgroup RKD
def _rkd_one(what, f_s, f_t, bad, expect=OK):
    L, ptr, st = _api()
    B, D = f_s.shape
    x, t = _dev(f_s, f_t)
    return _call(what, lambda loss, dx, ws: L.ph_rkd_loss_grad(ptr(x), ptr(t), loss, dx, B, D, E.W_D, E.W_A, ws, st),
                 {"loss": (1,), "dx": (B, D)}, L.ph_rkd_workspace_bytes(B, D), bad, expect)


@pytest.mark.parametrize("case", E.RKD_ONE_CASES, ids=lambda c: "B%d-D%d" % c[:2])
def test_rkd_one_workgroup(case):
    """Up to the LDS limit (all eight g[q] at D = 512, the 16-wave row loops revisited at B > 16); one row more is PH_EINVAL with the
    prefill untouched.  At the three largest shapes the tiled kernels run the full range on the same rows: they meet the float64
    reference under their own rule, and the two kernels lie within the sum of their tolerances of each other."""
    B, D, rc, with_dx = case
    R, bad, what = Report("rkd"), [], "B=%d D=%d" % (B, D)
    L = _api()[0]
    assert L.ph_rkd_one_workgroup_fits(B, D) == int(rc == OK)
    if rc != OK:
        f_s, f_t = E.rows(E.seed_of(B, D), B, D)
        assert _rkd_one(what, f_s, f_t, bad, expect=rc) is None
        assert not bad, bad
        return
    e = E.case("rkd", (B, D))
    outs = ("loss", "dx") if with_dx else ("loss",)
    got = _rkd_one(what, e["inp"]["f_s"], e["inp"]["f_t"], bad)
    if got:
        _compare(R, "rkd", e, got, bad, what, outs)
    if got and (B, D) in E.RKD_ONE_VS_TILED:
        et = E.case("rkd_part", (B, D, 0, B))
        tiled = _rkd_part(what + " tiled", e["inp"]["f_s"], e["inp"]["f_t"], 0, B, bad)
        assert tiled, bad
        _compare(R, "rkd_part", et, tiled, bad, what + " tiled")
        for o in outs:
            tol = E.case_tolerance("rkd", e, o) + E.case_tolerance("rkd_part", et, o)
            R.add(f"{what} one-workgroup vs tiled {o}", E.err(tiled[o], got[o].reshape(tiled[o].shape)), E.scale(e["ref"][o]), tol)
    _finish(R, bad, "rkd")


# ------------------------------------------------------------------------------------------------ PKT
def _pkt(what, f_s, f_t, bad):
    L, ptr, st = _api()
    B, D = f_s.shape
    x, t = _dev(f_s, f_t)
    return _call(what, lambda loss, dx, ws: L.ph_pkt_loss_grad(ptr(x), ptr(t), loss, dx, B, D, ws, st),
                 {"loss": (1,), "dx": (B, D)}, L.ph_pkt_workspace_bytes(B, D), bad)


@pytest.mark.parametrize("case", E.PKT_CASES + ("zero_row",), ids=lambda c: c if isinstance(c, str) else "B%d-D%d" % c)
def test_pkt(case):
    """Rows per block of 4, the lane strides over B and over D, the 16-wave row loop of pkt_finish, the 1024-strided sum of loss_rows;
    and one all-zero student row (k = 0: its gradient is ds / eps, the other rows are judged on their own as well)."""
    kind, key = ("pkt_zero_row", ()) if case == "zero_row" else ("pkt", case)
    e = E.case(kind, key)
    R, bad, what = Report("pkt"), [], "B=%d D=%d%s" % (*e["inp"]["f_s"].shape, " zero row" if case == "zero_row" else "")
    got = _pkt(what, e["inp"]["f_s"], e["inp"]["f_t"], bad)
    if got:
        if kind == "pkt_zero_row":
            got["dx_live"] = E.live_rows(got["dx"])
        _compare(R, kind, e, got, bad, what)
    _finish(R, bad, "pkt")


# ------------------------------------------------------------------------------------------------ Cox
def _cox(what, theta, t, c, bad, with_grad=True, expect=OK, B=None):
    L, ptr, st = _api()
    B = B or theta.shape[0]
    th, tt, cc = _dev(theta, t, c)
    if with_grad:
        return _call(what, lambda loss, dx: L.ph_cox_loss_grad(ptr(th), ptr(tt), ptr(cc), loss, dx, B, st), {"loss": (1,), "dx": (B,)}, 0, bad, expect)
    return _call(what, lambda loss: L.ph_cox_loss_grad(ptr(th), ptr(tt), ptr(cc), loss, None, B, st), {"loss": (1,)}, 0, bad, expect)


@pytest.mark.parametrize("case", E.COX_CASES + ("censored",), ids=str)
def test_cox(case):
    """The 1024-strided loops once, exactly once, twice and four times; ties everywhere (>=); every row censored: loss 0, gradient 0."""
    kind, key = ("cox_censored", ()) if case == "censored" else ("cox", case)
    e = E.case(kind, key)
    i = e["inp"]
    R, bad, what = Report("cox"), [], "B=%d%s" % (i["theta"].shape[0], " censored" if case == "censored" else "")
    got = _cox(what, i["theta"], i["t"], i["c"], bad)
    if got:
        _compare(R, kind, e, got, bad, what)
        if case == "censored":
            assert not got["loss"].any() and not got["dx"].any(), "every row censored: loss 0, gradient 0"
    _finish(R, bad, "cox")


def test_cox_without_gradient_and_above_4096_rows():
    """dtheta = NULL: the same loss, bit for bit.  B = 4097: PH_EINVAL, nothing written."""
    bad = []
    i = E.case("cox", 1025)["inp"]
    both = _cox("B=1025", i["theta"], i["t"], i["c"], bad)
    only = _cox("B=1025 dtheta=NULL", i["theta"], i["t"], i["c"], bad, with_grad=False)
    assert both and only, bad
    assert np.array_equal(both["loss"], only["loss"])
    z = torch.zeros(4097)
    assert _cox("B=4097", z, z, z, bad, expect=EINVAL) is None
    assert not bad, bad


@pytest.mark.parametrize("B", E.COX_FUSED)
def test_fused_stage1_cox_terms_are_ph_cox_loss_grad_bitwise(B):
    """ph_surv_stage1_loss_grad with nt = 0: terms[0..2] are the three ph_cox_loss_grad losses on the same vectors, bit for bit (what the
    comment at surv_stage1_body says), and the gradient rows are lambda_cox x its dtheta - bit for bit at lambda_cox = 1 and as the
    float32 product at 0.375."""
    L, ptr, st = _api()
    bad = []
    i = E.case("cox", B)["inp"]
    thetas = [i["theta"]] + [E.cox_inputs(B + 7 * k, B)[0] for k in (1, 2)]
    sep = [_cox(f"B={B} theta{k}", th, i["t"], i["c"], bad) for k, th in enumerate(thetas)]
    assert all(sep), bad
    p = _dev(*thetas)
    t, c = _dev(i["t"], i["c"])
    for lam in (1.0, 0.375):
        what = f"stage1 B={B} lambda_cox={lam}"
        got = _call(what, lambda terms, dgrad: L.ph_surv_stage1_loss_grad(ptr(p[0]), ptr(p[1]), ptr(p[2]), None, None, None, ptr(t), ptr(c), B, 0,
                                                                          lam, 0.0, terms, dgrad, st), {"terms": (9,), "dgrad": (3, B)}, 0, bad)
        assert got, bad
        for k in range(3):
            if np.float32(got["terms"][k]).tobytes() != np.float32(sep[k]["loss"][0]).tobytes():
                bad.append(f"{what}: terms[{k}] = {got['terms'][k]!r}, ph_cox_loss_grad gives {sep[k]['loss'][0]!r}")
            want = (np.float32(lam) * sep[k]["dx"].astype(np.float32)).view(np.int32)
            same = got["dgrad"][k].astype(np.float32).view(np.int32) == want
            if not same.all():
                j = int(np.nonzero(~same)[0][0])
                bad.append(f"{what}: gradient row {k} differs from lambda_cox x dtheta in {int((~same).sum())} of {B} elements, first at {j}: "
                           f"{got['dgrad'][k][j]!r} vs {float(np.float32(lam)) * sep[k]['dx'][j]!r}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ RKDLoss past the LDS limit
@pytest.mark.parametrize("shape", [(128, 256), (67, 512)], ids=lambda s: "%dx%d" % s)
def test_rkdloss_where_the_one_workgroup_form_does_not_fit(shape):
    """RKDLoss()(f_s, f_t) at a batch of at most 128 rows whose E and A do not fit the one-workgroup kernel's LDS (it raised there): the
    tiled kernels over the full range; value and the gradient of 3.0 * loss against float64 under the rule."""
    from multimodal_learning_amd.distiller_zoo import RKDLoss
    B, D = shape
    assert not _api()[0].ph_rkd_one_workgroup_fits(B, D)
    R, bad = Report("RKDLoss"), []
    e = E.case("rkd_part", (B, D, 0, B))
    f_s, f_t = _dev(e["inp"]["f_s"], e["inp"]["f_t"])
    f_s.requires_grad_(True)
    loss = RKDLoss()(f_s, f_t)
    g, = torch.autograd.grad(3.0 * loss, f_s)
    _compare(R, "rkd_part", e, {"loss": loss.detach().cpu().numpy().reshape(1)}, bad, "RKDLoss %d x %d" % shape, ("loss",))
    _compare(R, "rkd_part", e, {"dx": g.cpu().numpy()}, bad, "RKDLoss %d x %d, 3.0 * loss" % shape, ("dx",), factor=3.0)
    _finish(R, bad, "rkd_part")

"""Sweep of the CRD memory-bank entry points (csrc/crd.hip) through the C ABI, against tests/crd_emulation.py.

  exact class   ph_crd_select (columns and gathered scores: numpy's stable argsort, lower column first among equal values, -0 == +0;
                tie cases drawn from six values, tie-free cases at both parities of P % 4, the four (select_pos, select_neg) pairs,
                host ranks with rank P - 1, the unranked copy at K = 70000 and one ranked list above 64 KiB of LDS),
                ph_crd_neg_hist (np.bincount; centre rows ignored, every element written), the gathered rows of ph_crd_outputs,
                ph_crd_zsum on integers, ph_crd_setz on powers of two, ph_crd_class_centers on an integer bank, the zero rows of
                ph_crd_outputs_bwd under a NULL gradient: bit for bit.
  real class    ph_crd_score, ph_crd_loss_grad (1 to 8 splits, the clamp, workspace NULL, posw and idx_bank2 at ragged lengths),
                ph_crd_loss_grad_pos, ph_crd_scan_neg (both forms), ph_crd_update, out1 / out2 of ph_crd_outputs,
                ph_crd_outputs_bwd, ph_contrast_loss_v2: against the float64 reference, within 4 x the float32 restatement's error
                on the same inputs plus the operator's floor (crd_emulation.FLOOR).
  cross form    the negatives of one index list through ph_crd_neg_hist + ph_crd_scan_neg and through ph_crd_loss_grad minus
                ph_crd_loss_grad_pos, both against one float64 reference.

Every output lives in a buffer between sentinel guard bands, NaN-filled (floats) or filled with -7 (integers): after each call the
guards are intact and nothing in the written region is left unwritten; bank rows other than y[b] (ph_crd_update), the n_data bank
rows under ph_crd_class_centers, params[0, 1, 4, 5] under ph_crd_setz and S1 / S2 under zsum_only are bitwise unchanged.  The
workspaces of ph_crd_loss_grad and ph_crd_scan_neg are guarded too, sized exactly by their *_workspace_bytes, and hold exactly the
documented number of partials afterwards.  y holds distinct rows: the reference's index_copy_ is undefined on duplicates as well.

The largest excess of the device's error over the float32 restatement's, in units of max |ref|, per operator, is what
crd_emulation.FLOOR holds 4 x of.  NOT YET MEASURED: no MI355X run of this file exists, FLOOR is empty, and an operator whose
expf / logf differs from numpy's by a few ulp will miss its tolerance until its `excess[operator]` (printed by every test next
to the floor) has been entered there and here.  A floor above 1e-5 of max |ref| would be a finding, not a floor.  Whether the
list above 64 KiB of LDS launches without the kernel's dynamic-LDS limit raised is unmeasured as well; the last test asserts it.
The smallest injected-defect factor of the CPU self-test (tests/test_crd_emulation_cpu.py) is 167 x the tolerance (Z1 and Z2
swapped under ph_crd_loss_grad_pos at P = 8, m_neg = 4096, T = 1, where c = 15.9 dwarfs x); the next are scan chunk tail 1.2e4
(zsum_only at n_data = 4097), swapped Z's under ph_crd_loss_grad 1.5e4, a split left out of the reduce 1.9e4, outputs' swapped Z's
1.3e5, scan_neg 2.1e5, dropped last column 2.9e5, uniform posw 3.0e5, ignored idx_bank2 3.8e5, update without renormalisation
1.0e6, mPn from K2 2.9e6; in the exact class a reversed tie-break changes at least 3 elements of every tie case, the shifted
sixteen-byte path at least 9 of every ranked case with P % 4 != 0 and K >= 4, the histogram boundary at least 1, a mean over
max_class_rows at least 608."""
import numpy as np
import pytest
import torch

from tests import crd_emulation as E
from tests.gpu_util import Guarded, Report

pytestmark = pytest.mark.gpu

F32, D = np.float32, E.D
UNWRITTEN = -7          # fill of the integer outputs: no column, row count or multiplicity is negative
EXCESS = {}             # operator -> largest (device error - restatement error) / max |ref| seen in this process
_LIVE = []              # the operands of the running test, kept alive across the launches


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _LIVE.clear()


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def dev(a, dtype=None):
    """numpy array (or None) -> device tensor, kept alive until the test ends."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    _LIVE.append(torch.from_numpy(a.astype(dtype) if dtype is not None else a).cuda())
    return _LIVE[-1]


def _out(shape, dtype=torch.float32):
    return Guarded(tuple(shape), dtype, fill=float("nan") if dtype.is_floating_point else UNWRITTEN)


def _filled(a):
    """A Guarded holding a copy of numpy array `a` (an in / out operand)."""
    G = Guarded(tuple(a.shape), torch.from_numpy(a[:0].copy()).dtype, fill=0)
    G.t.copy_(dev(a))
    return G


def _workspace(nbytes):
    return Guarded((max(nbytes // 4, 1),), torch.float32)


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
        if a.dtype.kind == "i" and (a == UNWRITTEN).any():
            bad.append(f"{what} {k}: {int((a == UNWRITTEN).sum())} elements never written")
        res[k] = a
    return res


def _same_bits(what, got, exp, bad):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    same = got.view(np.int32 if got.dtype.itemsize == 4 else np.int64) == exp.view(np.int32 if exp.dtype.itemsize == 4 else np.int64)
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        bad.append(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {i}: got {got[i]!r} expected {exp[i]!r}")
    return bool(same.all())


def _compare(R, e, got, bad, op=None):
    """The real class: every output array of suite entry `e` present in `got` against its tolerance."""
    op = op or e["op"]
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


# ------------------------------------------------------------------------------------------------ ph_crd_score
def test_score():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_score"), []
    for e in E.suite("score"):
        i = e["inp"]
        B, PK = i["B"], i["PK"]
        o = {k: _out((B, PK)) for k in ("out1", "out2", "diff")}
        rc = L.ph_crd_score(ptr(dev(i["v1"])), ptr(dev(i["v2"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])), ptr(dev(i["mem1"])),
                            ptr(dev(i["mem2"])), ptr(o["out1"].t), ptr(o["out2"].t), ptr(o["diff"].t), B, PK, D, i["T"], st)
        assert rc == 0, (e["name"], rc)
        _compare(R, e, _collect(e["name"], o, bad), bad)
    _finish(R, bad, ["score"])


# ------------------------------------------------------------------------------------------------ ph_crd_select
def _select_case(L, ptr, st, c, n, bad):
    B, P, K, P2, K2 = c["B"], c["P"], c["K"], c["P2"], c["K2"]
    what = "select B%d P%d K%d P2 %d K2 %d pos%d neg%d ranks%d ties%d" % (B, P, K, P2, K2, c["sp"], c["sn"], c["ranks"], c["ties"])
    i = E.select_inputs(c, n)
    exp = E.select_ref(i["diff"], i["out1"], i["out2"], i["ranks"], P, K, P2, K2, c["sn"], c["sp"])
    o = {"sel": _out((B, P2 + K2), torch.int32), "xs": _out((B, P2 + K2)), "xt": _out((B, P2 + K2))}
    rc = L.ph_crd_select(ptr(dev(i["diff"])), ptr(dev(i["out1"])), ptr(dev(i["out2"])), ptr(dev(i["ranks"])), ptr(o["sel"].t),
                         ptr(o["xs"].t), ptr(o["xt"].t), B, P, K, P2, K2, c["sn"], c["sp"], st)
    if rc != 0:
        torch.cuda.synchronize()
        bad.append(f"{what}: rc {rc}")
        return what, rc
    got = _collect(what, o, bad)
    for k in ("sel", "xs", "xt"):
        _same_bits(f"{what} {k}", got[k], exp[k], bad)
    return what, rc


def test_select_exact():
    L, ptr, st = _api()
    bad = []
    for n, c in enumerate(E.SELECT_CASES + [E.SELECT_COPY_CASE]):
        _select_case(L, ptr, st, c, n, bad)
    print(f"\n== ph_crd_select, exact class: {len(E.SELECT_CASES) + 1} cases, {len(bad)} failures")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_crd_zsum / ph_crd_setz
def test_zsum_and_setz_exact():
    L, ptr, st = _api()
    bad = []
    for n in E.ZSUM_N:
        xs, xt = E.zsum_inputs(n)
        G = _out((2,))
        assert L.ph_crd_zsum(ptr(dev(xs)), ptr(dev(xt)), ptr(G.t), n, st) == 0
        got = _collect(f"zsum n{n}", {"sums": G}, bad)["sums"]
        _same_bits(f"zsum n{n}", got, np.array([xs.astype(np.int64).sum(), xt.astype(np.int64).sum()], dtype=F32), bad)
    sums, count, n_data = np.array([64.0, 512.0], dtype=F32), 16.0, 256.0
    for (Z1, Z2) in E.SETZ_CASES:
        par = E.make_params(16.0, 0.0625, Z1, Z2, 2.0)
        G = _filled(par)
        before = G.snapshot()
        assert L.ph_crd_setz(ptr(G.t), ptr(dev(sums)), count, n_data, st) == 0
        got = _collect(f"setz Z {Z1} {Z2}", {"params": G}, bad)["params"]
        exp = E.setz_exact(par, sums, count, n_data)
        assert exp[2] == (1024.0 if Z1 < 0 else Z1) and exp[3] == (8192.0 if Z2 < 0 else Z2)
        _same_bits(f"setz Z {Z1} {Z2}", got, exp, bad)       # (params[0, 1, 4, 5] and a positive Z bitwise unchanged)
        assert torch.equal(before[:4096], G.buf[:4096])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_crd_loss_grad / _pos
def _lg_call(L, ptr, st, i, W, pos_only):
    B = i["B"]
    o = {"lossp": _out((B,)), "dv1": _out((B, D)), "dv2": _out((B, D))}
    a = [ptr(dev(i["xs"])), ptr(dev(i["xt"])), ptr(dev(i["sel"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])), ptr(dev(i["posw_s"])),
         ptr(dev(i["posw_t"])), ptr(dev(i["mem1"])), ptr(dev(i["mem2"])), ptr(dev(i["params"])), ptr(o["lossp"].t), ptr(o["dv1"].t),
         ptr(o["dv2"].t)]
    if pos_only:
        rc = L.ph_crd_loss_grad_pos(*a, B, i["P2"], i["m_neg"], D, i["n_data"], i["inv_bnorm"], st)
    else:
        rc = L.ph_crd_loss_grad(*a, B, i["PK"], i["P2"], i["K2"], D, i["n_data"], i["inv_bnorm"], ptr(W.t) if W is not None else None, st)
    return rc, o


def test_loss_grad():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_loss_grad"), []
    for e in E.suite("loss_grad"):
        i = e["inp"]
        B, ns = i["B"], i["ns"]
        W = _workspace(L.ph_crd_loss_grad_workspace_bytes(B)) if i["ws"] else None
        rc, o = _lg_call(L, ptr, st, i, W, False)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], o, bad)
        if W is not None:
            # [B][ns][2][128] gradient partials then [B][ns] loss partials, nothing behind them; no partials with one split
            written = int((~torch.isnan(W.t)).sum())
            expect = B * ns * (2 * D + 1) if ns > 1 else 0
            if not W.guards_intact() or written != expect or (expect and bool(torch.isnan(W.t[:expect]).any())):
                bad.append(f"{e['name']}: workspace holds {written} partials, expected the first {expect} (guards intact: {W.guards_intact()})")
        _compare(R, e, got, bad)
    assert {e["inp"]["ns"] for e in E.suite("loss_grad")} >= {1, 2, 3, 5, 7, 8}
    _finish(R, bad, ["loss_grad"])


def test_loss_grad_pos():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_loss_grad_pos"), []
    for e in E.suite("loss_grad_pos"):
        rc, o = _lg_call(L, ptr, st, e["inp"], None, True)
        assert rc == 0, (e["name"], rc)
        _compare(R, e, _collect(e["name"], o, bad), bad)
    _finish(R, bad, ["loss_grad_pos"])


# ------------------------------------------------------------------------------------------------ ph_crd_neg_hist
def test_neg_hist_exact():
    L, ptr, st = _api()
    bad = []
    for c in E.HIST_CASES:
        n, K, col0, B = c["n_data"], c["K"], c["col0"], c["B"]
        what = "neg_hist n_data %d K%d col0 %d B%d" % (n, K, col0, B)
        idx, stride = E.hist_inputs(c)
        G = _out((B, n), torch.int32)
        rc = L.ph_crd_neg_hist(ptr(dev(idx)), stride, col0, K, B, n, ptr(G.t), st)
        assert rc == 0, (what, rc)
        _same_bits(what, _collect(what, {"mult": G}, bad)["mult"], E.neg_hist(idx, col0, K, n), bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_crd_scan_neg
def _scan_call(L, ptr, st, i):
    B, n = i["B"], i["n_data"]
    S1, S2, W = _filled(i["S1"]), _filled(i["S2"]), _workspace(L.ph_crd_scan_neg_workspace_bytes(B, n))
    loss, zs = _out((B,)), _filled(i["zsums0"])
    rc = L.ph_crd_scan_neg(ptr(S1.t), ptr(S2.t), ptr(dev(i["mult"])), ptr(dev(i["params"])), ptr(W.t), ptr(loss.t), ptr(zs.t), B, n,
                           i["m_neg"], i["inv_bnorm"], i["zsum_only"], st)
    return rc, S1, S2, W, loss, zs


def test_scan_neg():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_scan_neg (loss / coefficients, and zsum_only)"), []
    for e, ez in zip(E.suite("scan_neg"), E.suite("scan_zsum")):
        i = e["inp"]
        B, n = i["B"], i["n_data"]
        nparts = B * -(-n // E.SCAN_CHUNK) * 4
        rc, S1, S2, W, loss, zs = _scan_call(L, ptr, st, i)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], {"loss_neg": loss, "S1": S1, "S2": S2, "workspace": W}, bad)
        assert got.pop("workspace").size == nparts
        if not (zs.guards_intact() and np.array_equal(zs.t.cpu().numpy(), i["zsums0"])):
            bad.append(f"{e['name']}: zsums touched by the loss form")
        for k in ("S1", "S2"):
            if np.any(got[k][i["mult"] == 0] != 0):
                bad.append(f"{e['name']} {k}: a row of multiplicity 0 has a non-zero coefficient")
        _compare(R, e, got, bad)
        # zsum_only: adds onto zsums, leaves S1 / S2 and loss_neg alone
        iz = ez["inp"]
        rc, S1, S2, W, loss, zs = _scan_call(L, ptr, st, iz)
        assert rc == 0, (ez["name"], rc)
        got = _collect("zsum " + ez["name"], {"zsums": zs, "S1": S1, "S2": S2, "workspace": W}, bad)
        _same_bits(f"zsum {ez['name']} S1 untouched", got.pop("S1"), iz["S1"], bad)
        _same_bits(f"zsum {ez['name']} S2 untouched", got.pop("S2"), iz["S2"], bad)
        got.pop("workspace")
        if not (loss.guards_intact() and bool(torch.isnan(loss.t).all())):
            bad.append(f"zsum {ez['name']}: loss_neg written by zsum_only")
        _compare(R, dict(ez, name="zsum " + ez["name"]), got, bad)
    _finish(R, bad, ["scan_neg", "scan_zsum"])


def test_scan_form_equals_gathered_form_on_one_list():
    """The negatives of one index list, B = 3, P = 6, K = 600 over 257 rows (multiplicities up to ~9): ph_crd_neg_hist +
    ph_crd_scan_neg + the coefficient-weighted bank sum (taken in float64 on the host) against ph_crd_loss_grad minus
    ph_crd_loss_grad_pos, both against the float64 loss and gradients of the negative columns.  Each form's tolerance is 4 x the
    error of its own float32 restatement (which reads the same float32-rounded scores) against that one reference + its floor."""
    L, ptr, st = _api()
    R, bad = Report("negatives: bank-scan form and gathered form against one float64 reference"), []
    B, P, K, T, n = 3, 6, 600, 0.07, E.N_DATA
    PK = P + K
    rng = np.random.default_rng([111])
    mem1, mem2 = E.banks()
    v1, v2 = E.unit_rows(B, [112]), E.unit_rows(B, [113])
    idx = E.row_lists(rng, (B, PK), n)
    sel = np.concatenate([np.tile(np.arange(P), (B, 1)), P + np.stack([rng.permutation(K) for _ in range(B)])], 1).astype(np.int32)
    sc = E.score(v1, v2, idx, None, mem1, mem2, T, np.float64)
    gat = lambda a: np.take_along_axis(a, sel.astype(np.int64), 1).astype(F32)
    xs, xt = gat(sc["out1"]), gat(sc["out2"])
    par = E.make_params(K, T, xs.astype(np.float64).mean() * n, xt.astype(np.float64).mean() * n * 1.25, P)
    full = dict(xs=xs, xt=xt, sel=sel, idx=idx, idx2=None, posw_s=None, posw_t=None, mem1=mem1, mem2=mem2, params=par, B=B, PK=PK,
                P2=P, K2=K, m_neg=K, n_data=float(n), inv_bnorm=1.0 / B, ns=E.lg_splits(PK), ws=True)
    pos = dict(full, xs=xs[:, :P].copy(), xt=xt[:, :P].copy(), sel=sel[:, :P].copy(), idx=idx[:, :P].copy(), PK=P, K2=0, ns=1, ws=False)
    # the one reference: the float64 loss and gradient of the negative columns alone
    neg = {k: E.loss_grad(full, np.float64)[k] - E.loss_grad(pos, np.float64)[k] for k in ("lossp", "dv1", "dv2")}
    # gathered form
    W = _workspace(L.ph_crd_loss_grad_workspace_bytes(B))
    rc1, of = _lg_call(L, ptr, st, full, W, False)
    rc2, op_ = _lg_call(L, ptr, st, pos, None, True)
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    gf, gp = _collect("gathered full", of, bad), _collect("gathered positives", op_, bad)
    rf, rp = E.loss_grad(full, F32), E.loss_grad(pos, F32)
    reff, refp = E.loss_grad(full, np.float64), E.loss_grad(pos, np.float64)
    for k in ("lossp", "dv1", "dv2"):
        rest = rf[k].astype(np.float64) - rp[k]
        tol = E.MARGIN * E.err(neg[k], rest) + E.FLOOR.get("loss_grad", 0.0) * E.scale(reff[k]) + E.FLOOR.get("loss_grad_pos", 0.0) * E.scale(refp[k])
        R.add(f"gathered {k}", E.err(neg[k], gf[k].astype(np.float64) - gp[k]), E.scale(neg[k]), tol)
    # bank-scan form
    G = _out((B, n), torch.int32)
    assert L.ph_crd_neg_hist(ptr(dev(idx)), PK, P, K, B, n, ptr(G.t), st) == 0
    mult = _collect("neg_hist", {"mult": G}, bad)["mult"]
    _same_bits("neg_hist of the list", mult, E.neg_hist(idx, P, K, n), bad)
    assert mult.max() > 1 and mult.min() == 0
    S1, S2 = (v1.astype(np.float64) @ mem2.astype(np.float64).T).astype(F32), (v2.astype(np.float64) @ mem1.astype(np.float64).T).astype(F32)
    si = dict(S1=S1, S2=S2, mult=mult, params=par, m_neg=K, inv_bnorm=1.0 / B, zsum_only=0, zsums0=np.zeros(2, dtype=F32), B=B, n_data=n)
    rc, GS1, GS2, W2, loss, zs = _scan_call(L, ptr, st, si)
    assert rc == 0, rc
    got = _collect("scan", {"loss_neg": loss, "S1": GS1, "S2": GS2, "workspace": W2}, bad)
    rest = E.scan_neg(si, F32)
    form = lambda o: {"lossp": o["loss_neg"].astype(np.float64), "dv1": o["S1"].astype(np.float64) @ mem2.astype(np.float64),
                      "dv2": o["S2"].astype(np.float64) @ mem1.astype(np.float64)}
    fg, fr = form(got), form(rest)
    for k in ("lossp", "dv1", "dv2"):
        tol = E.MARGIN * E.err(neg[k], fr[k]) + E.FLOOR.get("scan_neg", 0.0) * E.scale(neg[k])
        R.add(f"bank scan {k}", E.err(neg[k], fg[k]), E.scale(neg[k]), tol)
    _finish(R, bad)


# ------------------------------------------------------------------------------------------------ ph_crd_update
def test_update():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_update"), []
    for e in E.suite("update"):
        i = e["inp"]
        B, y = len(i["y"]), i["y"]
        M1, M2 = _filled(i["mem1"]), _filled(i["mem2"])
        rc = L.ph_crd_update(ptr(M1.t), ptr(M2.t), ptr(dev(i["v1"])), ptr(dev(i["v2"])), ptr(dev(y)), ptr(dev(i["params"])), B, D, st)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], {"mem1": M1, "mem2": M2}, bad)
        others = np.setdiff1d(np.arange(E.N_DATA), y)
        _same_bits(f"{e['name']} other rows of bank 1", got["mem1"][others], i["mem1"][others], bad)
        _same_bits(f"{e['name']} other rows of bank 2", got["mem2"][others], i["mem2"][others], bad)
        _compare(R, e, {"rows1": got["mem1"][y], "rows2": got["mem2"][y]}, bad)
    _finish(R, bad, ["update"])


# ------------------------------------------------------------------------------------------------ ph_crd_class_centers
@pytest.mark.parametrize("max_rows", E.CLASS_MAX_ROWS)
def test_class_centers_exact(max_rows):
    L, ptr, st = _api()
    bad = []
    bank, members, offsets = E.class_inputs()
    n, C = bank.shape[0], len(E.CLASS_SIZES)
    assert max(E.CLASS_SIZES) == E.CLASS_MAX_ROWS[0]
    M = _out((n + C, D))
    M.t[:n].copy_(dev(bank))
    W = _workspace(L.ph_crd_class_centers_workspace_bytes(C, max_rows))
    rc = L.ph_crd_class_centers(ptr(M.t), ptr(dev(members)), ptr(dev(offsets)), C, max_rows, n, D, ptr(W.t), st)
    assert rc == 0, rc
    got = _collect("class_centers", {"mem_ext": M}, bad)["mem_ext"]
    assert W.guards_intact()
    _same_bits("the n_data bank rows", got[:n], bank, bad)
    exp = E.class_centers(bank, members, offsets)
    assert not exp[E.CLASS_SIZES.index(0)].any()
    _same_bits("the class centres", got[n:], exp, bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_crd_outputs / _bwd
def test_outputs():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_outputs"), []
    for e in E.suite("outputs"):
        i = e["inp"]
        B, S2 = i["xs"].shape
        o = {"out1": _out((B, S2)), "out2": _out((B, S2)), "rows1": _out((B, S2, D)), "rows2": _out((B, S2, D))}
        rc = L.ph_crd_outputs(ptr(dev(i["xs"])), ptr(dev(i["xt"])), ptr(dev(i["sel"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])),
                              ptr(dev(i["mem1"])), ptr(dev(i["mem2"])), ptr(dev(i["params"])), ptr(o["out1"].t), ptr(o["out2"].t),
                              ptr(o["rows1"].t), ptr(o["rows2"].t), B, i["PK"], S2, D, st)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], o, bad)
        r1, r2 = E.outputs_rows(i)
        _same_bits(f"{e['name']} rows1", got.pop("rows1"), r1, bad)
        _same_bits(f"{e['name']} rows2", got.pop("rows2"), r2, bad)
        _compare(R, e, got, bad)
    _finish(R, bad, ["outputs"])


def test_outputs_bwd():
    L, ptr, st = _api()
    R, bad = Report("ph_crd_outputs_bwd"), []
    for e in E.suite("outputs_bwd"):
        i = e["inp"]
        B, S2 = i["B"], i["S2"]
        o = {"dv1": _out((B, D)), "dv2": _out((B, D))}
        rc = L.ph_crd_outputs_bwd(ptr(dev(i["g1"])), ptr(dev(i["g2"])), ptr(dev(i["out1"])), ptr(dev(i["out2"])), ptr(dev(i["rows1"])),
                                  ptr(dev(i["rows2"])), i["T"], ptr(o["dv1"].t), ptr(o["dv2"].t), B, S2, D, st)
        assert rc == 0, (e["name"], rc)
        got = _collect(e["name"], o, bad)
        for k, g in (("dv1", i["g1"]), ("dv2", i["g2"])):
            if g is None and np.any(got[k] != 0):
                bad.append(f"{e['name']} {k}: not exactly 0 under a NULL gradient")
        _compare(R, e, got, bad)
    _finish(R, bad, ["outputs_bwd"])


# ------------------------------------------------------------------------------------------------ ph_contrast_loss_v2
def test_contrast_loss_v2():
    L, ptr, st = _api()
    R, bad = Report("ph_contrast_loss_v2"), []
    for e in E.suite("contrast_loss_v2"):
        i = e["inp"]
        B, S = i["x"].shape
        o = {"rows": _out((B,)), "dx": _out((B, S))}
        rc = L.ph_contrast_loss_v2(ptr(dev(i["x"])), ptr(o["rows"].t), ptr(o["dx"].t), B, S, i["P"], i["n_data"], st)
        assert rc == 0, (e["name"], rc)
        _compare(R, e, _collect(e["name"], o, bad), bad)
    _finish(R, bad, ["contrast_loss_v2"])


# ------------------------------------------------------------------------------------------------ the list above 64 KiB of LDS (last)
def test_select_ranked_list_above_64_kib_of_lds():
    """B = 1, P = 4, K = 20000: 80 032 bytes of dynamic LDS, above the 64 KiB a kernel may use without its limit raised."""
    L, ptr, st = _api()
    bad = []
    c = E.SELECT_BIG_LDS_CASE
    assert (c["P"] + c["K"]) * 4 + c["P"] * 4 > 64 * 1024
    what, rc = _select_case(L, ptr, st, c, 1000, bad)
    assert rc == 0, f"{what}: the launch was refused (rc {rc})"
    assert not bad, "\n".join(bad)

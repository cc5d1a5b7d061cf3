"""Every csrc/crd.hip entry that takes a row width, and ph_gk_rows, at widths 64 and 256 through the C ABI, against
tests/crd_width_emulation.py (tests/test_gpu_crd.py is the same sweep at 128).

  real class    ph_crd_score (B in {1, 5}; 1, 63, 65 and 130 columns: the 64-column block edge), ph_crd_loss_grad (S2 = 1023 and 1025
                with and without workspace: one split / two splits; the workspace sized by ph_crd_loss_grad_workspace_bytes_w and
                guarded), ph_crd_update (B = 3: a partly filled block), ph_crd_outputs_bwd, ph_gk_rows (ng 3 and 5, both forms):
                against float64 within 4 x the float32 restatement's error plus the operator's floor.
  exact class   the gathered rows of ph_crd_outputs, ph_crd_class_centers on an integer bank (workspace sized by
                ph_crd_class_centers_workspace_bytes_w), the untouched bank rows of ph_crd_update: bit for bit.
  KNN           ph_crd_bank_topk against a stable descending sort of the class-masked float64 cosine: rows equal, similarities
                within 1e-5; seeds chosen on the CPU so that the similarities around rank num_pos of every query are more than
                crd_width_emulation.KNN_GAP apart.  At width 256, 33 to 64 queries take the four-wave kernel, up to 32 the eight-wave
                one; 65 and 100 queries are two passes.
  refused       widths 0, 32, 96, 192 and 512: PH_EINVAL from every entry with every output buffer bitwise untouched.

Outputs live between guard bands (tests/gpu_util.Guarded), NaN-filled or filled with -7.

The excess of the device's error over the restatement's, per operator (printed by every test), is what
crd_width_emulation.FLOOR holds 4 x of; a floor above 1e-5 of max |ref| would be a finding."""
import numpy as np
import pytest
import torch

from tests import crd_emulation as E
from tests import crd_width_emulation as W
from tests.gpu_util import Guarded, Report

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PH_EINVAL = -22
UNWRITTEN = -7
REFUSED = (0, 32, 96, 192, 512)
EXCESS = {}
_LIVE = []


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _LIVE.clear()


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    _LIVE.append(torch.from_numpy(a.astype(dtype) if dtype is not None else a).cuda())
    return _LIVE[-1]


def _out(shape, dtype=torch.float32):
    return Guarded(tuple(shape), dtype, fill=float("nan") if dtype.is_floating_point else UNWRITTEN)


def _filled(a):
    G = Guarded(tuple(a.shape), torch.from_numpy(a[:0].copy()).dtype, fill=0)
    G.t.copy_(dev(a))
    return G


def _workspace(nbytes):
    return Guarded((max(nbytes // 4, 1),), torch.float32)


def _collect(what, outs, bad):
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
    if got.tobytes() != exp.tobytes():
        bad.append(f"{what}: {int((got != exp).sum())} of {got.size} elements differ")


def _compare(R, op, name, ref, rest, got, bad):
    for k, a in got.items():
        tol = W.tolerance(op, ref[k], rest[k])
        er, sc = W.err(ref[k], np.asarray(a).reshape(np.shape(ref[k]))), W.scale(ref[k])
        if sc > 0:
            EXCESS[op] = max(EXCESS.get(op, 0.0), (er - W.err(ref[k], rest[k])) / sc)
        R.add(f"{name} {k}", er, sc, tol)


def _finish(R, bad, ops=()):
    for op in ops:
        print(f"   excess[{op}] = {EXCESS.get(op, 0.0):.3e} of max |ref| (floor {W.FLOOR.get(op, 0.0):.1e})")
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_crd_score
@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_score(D):
    L, ptr, st = _api()
    R, bad = Report(f"ph_crd_score, width {D}"), []
    for n, PK in enumerate((1, 63, 65, 130)):
        for k, B in enumerate((1, 5)):
            i = W.score_inputs(PK, B, (n + k) % 2 == 1, (0.07, 1.0)[(n // 2 + k) % 2], D)
            o = {key: _out((B, PK)) for key in ("out1", "out2", "diff")}
            rc = L.ph_crd_score(ptr(dev(i["v1"])), ptr(dev(i["v2"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])), ptr(dev(i["mem1"])),
                                ptr(dev(i["mem2"])), ptr(o["out1"].t), ptr(o["out2"].t), ptr(o["diff"].t), B, PK, D, i["T"], st)
            name = f"PK{PK} B{B}"
            assert rc == 0, (name, rc)
            _compare(R, "score", name, W.score(i, F64, D), W.score(i, F32, D), _collect(name, o, bad), bad)
    _finish(R, bad, ["score"])


# ------------------------------------------------------------------------------------------------ ph_crd_loss_grad
def _lg_call(L, ptr, st, i, Wk, D):
    B = i["B"]
    o = {"lossp": _out((B,)), "dv1": _out((B, D)), "dv2": _out((B, D))}
    rc = L.ph_crd_loss_grad(ptr(dev(i["xs"])), ptr(dev(i["xt"])), ptr(dev(i["sel"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])),
                            ptr(dev(i["posw_s"])), ptr(dev(i["posw_t"])), ptr(dev(i["mem1"])), ptr(dev(i["mem2"])),
                            ptr(dev(i["params"])), ptr(o["lossp"].t), ptr(o["dv1"].t), ptr(o["dv2"].t), B, i["PK"], i["P2"], i["K2"], D,
                            i["n_data"], i["inv_bnorm"], ptr(Wk.t) if Wk is not None else None, st)
    return rc, o


@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_loss_grad_at_the_split_edge(D):
    L, ptr, st = _api()
    R, bad = Report(f"ph_crd_loss_grad, width {D}"), []
    splits = set()
    for n, (S2, ws) in enumerate(((1023, True), (1023, False), (1025, True), (1025, False), (70, True))):
        B = (5, 1)[n % 2]
        i = W.lg_inputs(dict(S2=S2, P2=(6, 20)[n % 2], B=B, posw=n % 2 == 0, idx2=n < 2 or n == 4, ws=ws, T=(0.07, 1.0)[n // 2 % 2]), D)
        ns = i["ns"]
        splits.add(ns)
        nbytes = L.ph_crd_loss_grad_workspace_bytes_w(B, D)
        assert nbytes == B * E.LG_SPLIT_MAX * (2 * D + 1) * 4
        Wk = _workspace(nbytes) if ws else None
        rc, o = _lg_call(L, ptr, st, i, Wk, D)
        name = f"S2 {S2} B{B} ws{int(ws)}"
        assert rc == 0, (name, rc)
        got = _collect(name, o, bad)
        if Wk is not None:
            written, expect = int((~torch.isnan(Wk.t)).sum()), (B * ns * (2 * D + 1) if ns > 1 else 0)
            if not Wk.guards_intact() or written != expect:
                bad.append(f"{name}: workspace holds {written} partials, expected {expect} (guards intact: {Wk.guards_intact()})")
        _compare(R, "loss_grad", name, W.loss_grad(i, F64, D), W.loss_grad(i, F32, D), got, bad)
    assert splits == {1, 2}
    assert L.ph_crd_loss_grad_workspace_bytes(3) == L.ph_crd_loss_grad_workspace_bytes_w(3, 128)
    _finish(R, bad, ["loss_grad"])


# ------------------------------------------------------------------------------------------------ ph_crd_update
@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_update_partly_filled_block(D):
    L, ptr, st = _api()
    R, bad = Report(f"ph_crd_update, width {D}"), []
    for B, mom in ((3, 0.5), (1, 0.0), (5, 0.5)):
        i = W.update_inputs(B, mom, D)
        y = i["y"]
        M1, M2 = _filled(i["mem1"]), _filled(i["mem2"])
        rc = L.ph_crd_update(ptr(M1.t), ptr(M2.t), ptr(dev(i["v1"])), ptr(dev(i["v2"])), ptr(dev(y)), ptr(dev(i["params"])), B, D, st)
        name = f"B{B} momentum {mom}"
        assert rc == 0, (name, rc)
        got = _collect(name, {"mem1": M1, "mem2": M2}, bad)
        others = np.setdiff1d(np.arange(W.N_DATA), y)
        _same_bits(f"{name} other rows of bank 1", got["mem1"][others], i["mem1"][others], bad)
        _same_bits(f"{name} other rows of bank 2", got["mem2"][others], i["mem2"][others], bad)
        _compare(R, "update", name, W.update(i, F64, D), W.update(i, F32, D), {"rows1": got["mem1"][y], "rows2": got["mem2"][y]}, bad)
    _finish(R, bad, ["update"])


# ------------------------------------------------------------------------------------------------ ph_crd_outputs / _bwd
@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_outputs_rows_bit_for_bit_and_backward(D):
    L, ptr, st = _api()
    R, bad = Report(f"ph_crd_outputs / ph_crd_outputs_bwd, width {D}"), []
    groups = 1024 // D
    for n, S2 in enumerate((1, groups - 1, groups, groups + 1, 65)):
        B = (5, 1)[n % 2]
        i = W.lg_inputs(dict(S2=S2, P2=1, B=B, posw=False, idx2=S2 % 2 == 1, ws=False, T=0.07), D)
        o = {"out1": _out((B, S2)), "out2": _out((B, S2)), "rows1": _out((B, S2, D)), "rows2": _out((B, S2, D))}
        rc = L.ph_crd_outputs(ptr(dev(i["xs"])), ptr(dev(i["xt"])), ptr(dev(i["sel"])), ptr(dev(i["idx"])), ptr(dev(i["idx2"])),
                              ptr(dev(i["mem1"])), ptr(dev(i["mem2"])), ptr(dev(i["params"])), ptr(o["out1"].t), ptr(o["out2"].t),
                              ptr(o["rows1"].t), ptr(o["rows2"].t), B, i["PK"], S2, D, st)
        name = f"outputs S2 {S2} B{B}"
        assert rc == 0, (name, rc)
        got = _collect(name, o, bad)
        r1, r2 = E.outputs_rows(i)
        _same_bits(f"{name} rows1", got.pop("rows1"), r1, bad)
        _same_bits(f"{name} rows2", got.pop("rows2"), r2, bad)
        _compare(R, "outputs", name, E.outputs(i, F64), E.outputs(i, F32), got, bad)
        ib = W.outputs_bwd_inputs(S2, B, D)
        ob = {"dv1": _out((B, D)), "dv2": _out((B, D))}
        rc = L.ph_crd_outputs_bwd(ptr(dev(ib["g1"])), ptr(dev(ib["g2"])), ptr(dev(ib["out1"])), ptr(dev(ib["out2"])),
                                  ptr(dev(ib["rows1"])), ptr(dev(ib["rows2"])), ib["T"], ptr(ob["dv1"].t), ptr(ob["dv2"].t), B, S2, D, st)
        name = f"outputs_bwd S2 {S2} B{B}"
        assert rc == 0, (name, rc)
        _compare(R, "outputs_bwd", name, W.outputs_bwd(ib, F64, D), W.outputs_bwd(ib, F32, D), _collect(name, ob, bad), bad)
    _finish(R, bad, ["outputs", "outputs_bwd"])


# ------------------------------------------------------------------------------------------------ ph_crd_class_centers
@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_class_centers_bit_for_bit(D):
    L, ptr, st = _api()
    bad = []
    bank, members, offsets = W.class_inputs(D)
    n, C = bank.shape[0], len(E.CLASS_SIZES)
    for max_rows in E.CLASS_MAX_ROWS:
        M = _out((n + C, D))
        M.t[:n].copy_(dev(bank))
        nbytes = L.ph_crd_class_centers_workspace_bytes_w(C, max_rows, D)
        assert nbytes == C * -(-max_rows // E.CC_ROWS) * D * 4
        Wk = _workspace(nbytes)
        rc = L.ph_crd_class_centers(ptr(M.t), ptr(dev(members)), ptr(dev(offsets)), C, max_rows, n, D, ptr(Wk.t), st)
        assert rc == 0, rc
        got = _collect("class_centers", {"mem_ext": M}, bad)["mem_ext"]
        assert Wk.guards_intact()
        _same_bits("the n_data bank rows", got[:n], bank, bad)
        _same_bits("the class centres", got[n:], W.class_centers(bank, members, offsets), bad)
    assert L.ph_crd_class_centers_workspace_bytes(C, 513) == L.ph_crd_class_centers_workspace_bytes_w(C, 513, 128)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ ph_gk_rows
@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_gk_rows(D):
    L, ptr, st = _api()
    R, bad = Report(f"ph_gk_rows, width {D}"), []
    for ng in (3, 5):
        for B in (1, 5):      # (four samples per block: a partly filled block and a second one)
            G = np.random.default_rng([131, ng, D, B]).standard_normal((ng, B, D)).astype(F32)
            if B > 2:
                G[1, 2] = 0      # a zero-norm gradient: cosine 0
            for th in (0, 1):
                o = _out((B, ng))
                rc = L.ph_gk_rows(ptr(dev(G)), ng, B, D, th, 0.05, ptr(o.t), st)
                name = f"ng{ng} B{B} thresh{th}"
                assert rc == 0, (name, rc)
                got = _collect(name, {"all_scale": o}, bad)
                ref, rest = W.gk_rows(G, F64, th, 0.05), W.gk_rows(G, F32, th, 0.05)
                if th:      # (a count: a cosine within rounding of the threshold would flip a whole unit - there is none)
                    c = np.abs(_cosines(G) - 0.05)
                    assert c.min() > 1e-4
                _compare(R, "gk_rows", name, {"all_scale": ref}, {"all_scale": rest}, got, bad)
    _finish(R, bad, ["gk_rows"])


def _cosines(G):
    g = G.astype(F64)
    n = np.linalg.norm(g, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.nan_to_num(np.einsum("ibd,jbd->bij", g, g) / (n.T[:, :, None] * n.T[:, None, :]))


# ------------------------------------------------------------------------------------------------ ph_crd_bank_topk
def _knn_case(L, ptr, st, n, B, NP, D, bad):
    i, ref, gap = W.knn_seed(n, B, NP, D)
    what = f"knn width {D} n {n} B {B} NP {NP}"
    nb = [_out((B, NP), torch.int64), _out((B, NP), torch.int64)]
    sm = [_out((B, NP)), _out((B, NP))]
    ws = Guarded((L.ph_crd_bank_topk_workspace_bytes(B, n),), torch.uint8, fill=0)
    rc = L.ph_crd_bank_topk(ptr(dev(i["mem1"])), ptr(dev(i["mem2"])), ptr(dev(i["labels"])), ptr(dev(i["idx"])), 5,
                            ptr(dev(i["batch_label"])), B, n, NP, D, ptr(nb[0].t), ptr(nb[1].t), ptr(sm[0].t), ptr(sm[1].t),
                            ptr(ws.t), st)
    assert rc == 0, (what, rc)
    got = _collect(what, {"nb1": nb[0], "nb2": nb[1], "sim1": sm[0], "sim2": sm[1]}, bad)
    if not ws.guards_intact():
        bad.append(f"{what}: workspace guard band overwritten")
    worst = 0.0
    for k, (rows, sims) in enumerate(ref):
        if not np.array_equal(got["nb%d" % (k + 1)], rows):
            d = got["nb%d" % (k + 1)] != rows
            bad.append(f"{what} bank {k + 1}: {int(d.sum())} of {d.size} rows differ, first at {tuple(int(v[0]) for v in np.nonzero(d))}")
        worst = max(worst, float(np.abs(got["sim%d" % (k + 1)].astype(F64) - sims).max()))
    print(f"   {what}: gap {gap:.2e}, max |similarity error| {worst:.2e}")
    if worst > 1e-5:
        bad.append(f"{what}: similarity error {worst:.2e}")


@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_knn_small_banks(D):
    L, ptr, st = _api()
    bad = []
    for (n, B, NP) in W.KNN_CASES:
        _knn_case(L, ptr, st, n, B, NP, D, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_knn_65536_rows_64_queries(D):
    """The only case in which a wave walks more than one tile: the label parity, the ring wrap and the issue-ahead into the next
    tile in steady state (two tiles per wave with eight waves; width 256: four waves, four tiles per wave)."""
    L, ptr, st = _api()
    bad = []
    n, B, NP = W.KNN_BIG_CASE
    _knn_case(L, ptr, st, n, B, NP, D, bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ refused widths
@pytest.mark.parametrize("D", REFUSED)
def test_refused_widths_touch_nothing(D):
    L, ptr, st = _api()
    Dn = max(D, 4)
    z = lambda *s: dev(np.zeros(s, dtype=F32))
    zi = lambda *s: dev(np.zeros(s, dtype=np.int64))
    B, PK, S2, n = 2, 3, 3, 8
    mem1, mem2, v1, v2 = _filled(np.ones((n, Dn), F32)), _filled(np.ones((n, Dn), F32)), z(B, Dn), z(B, Dn)
    idx, sel, par = zi(B, PK), dev(np.zeros((B, S2), dtype=np.int32)), dev(E.make_params(2, 0.07, 1.0, 1.0, 1))
    outs = {k: _out(s) for k, s in (("a", (B, PK)), ("b", (B, PK)), ("c", (B, PK)), ("l", (B,)), ("d1", (B, Dn)), ("d2", (B, Dn)),
                                    ("r1", (B, S2, Dn)), ("r2", (B, S2, Dn)), ("gk", (B, 3)))}
    nb = {k: _out((B, 1), torch.int64) for k in ("nb1", "nb2")}
    ws = _workspace(1 << 16)
    before = {k: G.snapshot() for k, G in {**outs, **nb, "m1": mem1, "m2": mem2, "ws": ws}.items()}
    o = {k: ptr(G.t) for k, G in outs.items()}
    lab, bl = dev(np.zeros(n, dtype=np.int32)), zi(B)
    rcs = {
        "score": L.ph_crd_score(ptr(v1), ptr(v2), ptr(idx), None, ptr(mem1.t), ptr(mem2.t), o["a"], o["b"], o["c"], B, PK, D, 0.07, st),
        "loss_grad": L.ph_crd_loss_grad(o["a"], o["b"], ptr(sel), ptr(idx), None, None, None, ptr(mem1.t), ptr(mem2.t), ptr(par), o["l"],
                                        o["d1"], o["d2"], B, PK, 1, 2, D, float(n), 0.5, ptr(ws.t), st),
        "loss_grad_pos": L.ph_crd_loss_grad_pos(o["a"], o["b"], ptr(sel), ptr(idx), None, None, None, ptr(mem1.t), ptr(mem2.t), ptr(par),
                                                o["l"], o["d1"], o["d2"], B, PK, 4, D, float(n), 0.5, st),
        "update": L.ph_crd_update(ptr(mem1.t), ptr(mem2.t), ptr(v1), ptr(v2), ptr(bl), ptr(par), B, D, st),
        "outputs": L.ph_crd_outputs(o["a"], o["b"], ptr(sel), ptr(idx), None, ptr(mem1.t), ptr(mem2.t), ptr(par), o["b"], o["c"], o["r1"],
                                    o["r2"], B, PK, S2, D, st),
        "outputs_bwd": L.ph_crd_outputs_bwd(None, None, o["a"], o["b"], o["r1"], o["r2"], 0.07, o["d1"], o["d2"], B, S2, D, st),
        "class_centers": L.ph_crd_class_centers(ptr(mem1.t), ptr(sel), ptr(sel), 1, 1, n - 1, D, ptr(ws.t), st),
        "bank_topk": L.ph_crd_bank_topk(ptr(mem1.t), ptr(mem2.t), ptr(lab), ptr(idx), PK, ptr(bl), B, n, 1, D, ptr(nb["nb1"].t),
                                        ptr(nb["nb2"].t), o["a"], o["b"], ptr(ws.t), st),
        "gk_rows": L.ph_gk_rows(ptr(mem1.t), 3, B, D, 0, 0.0, o["gk"], st),
    }
    torch.cuda.synchronize()
    assert all(rc == PH_EINVAL for rc in rcs.values()), rcs
    for k, G in {**outs, **nb, "m1": mem1, "m2": mem2, "ws": ws}.items():
        assert torch.equal(before[k], G.buf), f"width {D}: {k} was written"

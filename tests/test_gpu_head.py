"""Sweep of the GK-Refine loss weights (csrc/optim.hip), the masks of the MIA-2023 masking teacher (csrc/superpixel.hip) and the
flat-buffer updates and reductions (csrc/optim.hip, csrc/surv.hip, csrc/tsvd.hip) through the C ABI, against tests/head_emulation.py.

  exact class   ph_gram and ph_l1_sum on small integers, ph_l1_sign_axpy and ph_apply_mask on binary fractions, every 0/1 mask of
                ph_superpixel_mask and ph_topk_threshold_mask, the thresholded counts of ph_gk_scale_momentum / ph_gk_finish_momentum
                on cosines that are exact ties with the threshold or far from it, the CE weight of ph_gk_finish_momentum (= lam),
                the sigmoid backward at saturation (= 0): bitwise equal to the numpy result.  ph_adam_ema_step equals
                ph_adam_ema_step_dev bitwise (both ways of passing the betas).
  real class    everything else against the float64 reference, within 4 x the float32 restatement's error on the same inputs plus
                the operator's floor (head_emulation.FLOOR).

Every output and every buffer updated in place lives between sentinel guard bands (the payload starts 256-byte aligned): after each
call the return code is PH_OK, the guards are intact and no NaN is left in the written region.

Measured on the MI355X, the largest excess of the device's error over the float32 restatement's, in units of max |ref|, per
operator: adam 3.57e-8 and adagrad 1.096e-8 (the kernels' `b1 * m + omb1 * g` and `g + wd * p` are contracted to fmas where hipcc
chooses; the restatement rounds every product); head_emulation.FLOOR is 4 x each.  No other operator exceeded its restatement
(no floor): gram, gk_scale, gk_finish, gk_scale_momentum, gk_finish_momentum, the superpixel means, ema_update, ema_update_dev,
scaled_diff, l1_sum, sqdiff_sum, maxnorm_mix, sigmoid_range_fwd, sigmoid_range_bwd.  The loss totals of the GK kernels equal the
restatement only with `t += w * loss` as one fma: with the product rounded first ph_gk_finish_momentum's total exceeded it by
1.08e-7 (half an ulp of a sum of five terms whose restatement happened to land on the reference).
Every test prints `excess[operator]` next to the floor; re-measure after a change of the kernels or of the toolchain.
The smallest injected-defect ratios of the CPU self-test (tests/test_head_emulation_cpu.py): Adagrad's eps inside the square root
73.6 x the tolerance, a dropped tail element 80.4 (ph_sqdiff_sum) and 87.4 (ph_gram), the EMA from the old p 115, weight decay after
the moments 228, Adam's bc2 without the root 3.1e3; every other defect above 1e5 or rejected by an exact array.
The sweep found no kernel wrong."""
import numpy as np
import pytest
import torch

from tests import head_emulation as E
from tests.gpu_util import Guarded, Report, dispatch_lib

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -22
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


def dev(a):
    """numpy array (or None) -> device tensor, kept alive until the test ends."""
    if a is None:
        return None
    _LIVE.append(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return _LIVE[-1]


def _out(*shape, dtype=torch.float32):
    return Guarded(tuple(shape), dtype, float("nan") if dtype.is_floating_point else 0)


def _inout(a):
    """A guarded buffer that starts with the contents of numpy array a (updated in place by the call)."""
    a = np.ascontiguousarray(a)
    G = _out(*a.shape, dtype=torch.from_numpy(a).dtype)
    G.t.copy_(torch.from_numpy(a))
    return G


def _collect(what, rc, outs, bad, scratch=()):
    """The return code is PH_OK; synchronise; guards intact and nothing left unwritten in every Guarded of `outs` (`scratch`: guards
    only); their contents as numpy arrays."""
    if rc != OK:
        bad.append(f"{what}: returned {rc}")
    torch.cuda.synchronize()
    res = {}
    for k, G in list(outs.items()) + [("scratch%d" % i, G) for i, G in enumerate(scratch)]:
        if not G.guards_intact():
            bad.append(f"{what} {k}: guard band overwritten")
        if k in outs:
            a = G.t.cpu().numpy()
            if a.dtype.kind == "f" and np.isnan(a).any():
                bad.append(f"{what} {k}: {int(np.isnan(a).sum())} elements never written (or NaN)")
            res[k] = a
    return res


def _bitwise(what, got, expect, bad):
    got, exp = np.asarray(got), np.asarray(expect)
    if exp.dtype.kind == "f":
        exp = exp.astype(F32)
        same = got.reshape(exp.shape).view(np.int32) == exp.view(np.int32)
    else:
        same = got.reshape(exp.shape) == exp
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        bad.append(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {i}: got {got.reshape(exp.shape)[i]!r} "
                   f"expected {exp[i]!r}")


def _compare(R, e, got, bad, tag=""):
    """Every output array of suite entry e: bitwise in the exact class, against its tolerance otherwise."""
    op = e["op"]
    for k, ref in e["ref"].items():
        what = f"{e['name']}{tag} {k}"
        if k not in got:
            bad.append(f"{what}: not produced")
        elif k in e["exact"]:
            _bitwise(f"{op} {what}", got[k], ref, bad)
        else:
            tol, er, sc = E.entry_tolerance(e, k), E.err(ref, np.asarray(got[k]).reshape(np.shape(ref))), E.scale(ref)
            if sc > 0 and np.isfinite(er):
                EXCESS[op] = max(EXCESS.get(op, 0.0), (er - E.err(ref, e["rest"][k])) / sc)
            R.add(what, er, sc, tol)


def _finish(R, bad, ops=()):
    for op in ops:
        print(f"   excess[{op}] = {EXCESS.get(op, 0.0):.3e} of max |ref| (floor {E.FLOOR.get(op, 0.0):.1e})")
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad)


def _sweep(op, launch):
    """launch(L, ptr, st, inp, what, bad) -> {output name: numpy array} for every case of operator op."""
    L, ptr, st = _api()
    R, bad = Report(op), []
    for e in E.suite(op):
        _compare(R, e, launch(L, ptr, st, e["inp"], f"{op} {e['name']}", bad), bad)
        _LIVE.clear()
    _finish(R, bad, (op,))


def _untouched(what, G, before, bad):
    torch.cuda.synchronize()
    if not torch.equal(G.buf, before):
        bad.append(f"{what}: the buffer was written")


# ------------------------------------------------------------------------------------------------ GK-Refine
def _gram(L, ptr, st, i, what, bad):
    out = _out(i["ng"], i["ng"])
    rc = L.ph_gram(ptr(dev(i["G"])), ptr(out.t), i["ng"], i["n"], st)
    return _collect(what, rc, {"gram": out}, bad)


def test_gram_exact():
    _sweep("gram_exact", _gram)


def test_gram():
    _sweep("gram", _gram)
    L, ptr, st = _api()
    bad, out, g = [], _out(6, 6), dev(np.ones((6, 8), F32))
    before = out.snapshot()
    for ng in (1, 6):
        assert L.ph_gram(ptr(g), ptr(out.t), ng, 8, st) == EINVAL
    assert L.ph_gram(ptr(g), ptr(out.t), 3, 0, st) == EINVAL
    _untouched("ph_gram ng 1 / 6, n 0", out, before, bad)
    assert not bad, bad


def test_gk_scale():
    def launch(L, ptr, st, i, what, bad):
        outs = {"scale": _out(i["ng"])}
        lp = None
        if i["losses"] is not None:
            lv = dev(i["losses"])
            lp = dev(np.array([lv.data_ptr() + 4 * k for k in range(i["nl"])], dtype=np.int64))
            outs["total"] = _out(1)
        rc = L.ph_gk_scale(ptr(dev(i["gram"])), ptr(lp), i["ng"], i["nl"], i["mult"], ptr(outs["scale"].t),
                           ptr(outs["total"].t) if "total" in outs else None, st)
        return _collect(what, rc, outs, bad)
    _sweep("gk_scale", launch)


def test_gk_finish():
    def launch(L, ptr, st, i, what, bad):
        outs = {k: _out(n) for k, n in (("scale_int", 5), ("w", 5), ("total", 1), ("scaled", 5), ("scale_ext", 5))}
        rc = L.ph_gk_finish(ptr(dev(i["gram"])), ptr(dev(i["losses"])), ptr(dev(i["coef"])), ptr(dev(i["add"])), ptr(dev(i["logc"])),
                            i["mult"], ptr(outs["scale_int"].t), ptr(outs["w"].t), ptr(outs["total"].t), ptr(outs["scaled"].t),
                            ptr(outs["scale_ext"].t), st)
        return _collect(what, rc, outs, bad)
    _sweep("gk_finish", launch)


def test_gk_scale_momentum():
    def launch(L, ptr, st, i, what, bad):
        mo = _out(i["ng"])                                         # NaN before the first call: a first call must not read it
        init = None if i["mo_init"] is None else _out(1, dtype=torch.int32)
        res = {}
        for c, g in enumerate(i["grams"]):
            rc = L.ph_gk_scale_momentum(ptr(dev(g)), i["ng"], i["use_thresh"], i["thresh"], i["momentum"], ptr(mo.t),
                                        None if init is None else ptr(init.t), st)
            got = _collect(f"{what} call {c}", rc, {"mo": mo} if init is None else {"mo": mo, "init": init}, bad)
            res["mo%d" % c] = got["mo"]
            if init is not None:
                res["init"] = got["init"]
        return res
    _sweep("gk_scale_momentum", launch)


def test_gk_finish_momentum():
    def launch(L, ptr, st, i, what, bad):
        mo = _out(5)
        init = None if i["mo_init"] is None else _out(1, dtype=torch.int32)
        e_dev = None if i["e_dev"] is None else dev(np.array([i["e_dev"]], F32))
        res = {}
        for c, (g, lo) in enumerate(zip(i["grams"], i["losses"])):
            outs = {"mo": mo, "w": _out(5), "total": _out(1), "scaled": _out(5), "scale_ext": _out(5)}
            if init is not None:
                outs["init"] = init
            rc = L.ph_gk_finish_momentum(ptr(dev(g)), ptr(dev(lo)), i["alpha"], i["beta"], ptr(e_dev), i["lam"], i["mult"],
                                         i["use_thresh"], i["thresh"], i["momentum"], ptr(mo.t), None if init is None else ptr(init.t),
                                         ptr(outs["w"].t), ptr(outs["total"].t), ptr(outs["scaled"].t), ptr(outs["scale_ext"].t), st)
            got = _collect(f"{what} call {c}", rc, outs, bad)
            for k in ("mo", "w", "total", "scaled", "scale_ext"):
                res["%s%d" % (k, c)] = got[k]
            res["wce%d" % c] = got["w"][2:3]
            if init is not None:
                res["init"] = got["init"]
        return res
    _sweep("gk_finish_momentum", launch)


# ------------------------------------------------------------------------------------------------ masks
def test_superpixel_mask():
    def launch(L, ptr, st, i, what, bad):
        outs = {"mask": _out(i["B"], i["H"] * i["W"])}
        if i["want_mean"]:
            outs["mean"] = _out(i["B"], i["N"])
        rc = L.ph_superpixel_mask(ptr(dev(i["grad"])), ptr(dev(i["lab"])), ptr(outs["mask"].t),
                                  ptr(outs["mean"].t) if i["want_mean"] else None, i["B"], i["C"], i["H"], i["W"], i["N"], i["K"], st)
        return _collect(what, rc, outs, bad)
    _sweep("superpixel", launch)
    L, ptr, st = _api()
    bad, out = [], _out(1, 16)
    before = out.snapshot()
    assert L.ph_superpixel_mask(ptr(dev(np.ones((1, 1, 16), F32))), ptr(dev(np.zeros((1, 16), np.int64))), ptr(out.t), None,
                                1, 1, 4, 4, 2049, 1, st) == EINVAL
    _untouched("ph_superpixel_mask N 2049", out, before, bad)
    assert not bad, bad


def test_topk_threshold_mask():
    def launch(L, ptr, st, i, what, bad):
        out = _out(i["B"], i["D"])
        rc = L.ph_topk_threshold_mask(ptr(dev(i["x"])), ptr(out.t), i["B"], i["D"], i["K"], st)
        return _collect(what, rc, {"mask": out}, bad)
    _sweep("topk_mask", launch)
    L, ptr, st = _api()
    bad, out = [], _out(1, 16385)
    before = out.snapshot()
    assert L.ph_topk_threshold_mask(ptr(dev(np.ones((1, 16385), F32))), ptr(out.t), 1, 16385, 2, st) == EINVAL
    _untouched("ph_topk_threshold_mask D 16385", out, before, bad)
    assert not bad, bad


def test_apply_mask():
    def launch(L, ptr, st, i, what, bad):
        out = _out(i["B"], i["C"], i["P"])
        rc = L.ph_apply_mask(ptr(dev(i["x"])), ptr(dev(i["mask"])), ptr(out.t), i["B"], i["C"], i["P"], st)
        return _collect(what, rc, {"out": out}, bad)
    _sweep("apply_mask", launch)


# ------------------------------------------------------------------------------------------------ Adam, Adagrad, EMA
def _state(i, keys):
    bufs = {k: _inout(i[k]) for k in keys}
    if i["use_ema"]:
        bufs["ema"] = _inout(i["ema"])
    return bufs


def test_adam_host_and_device_forms():
    """Each case three times from the same start: ph_adam_ema_step, ph_adam_ema_step_dev with the betas as arguments and with
    beta1 < 0 (the betas read from hyper[8..11]).  All three within the tolerance, and bitwise equal to one another."""
    L, ptr, st = _api()
    R, bad = Report("adam"), []
    for e in E.suite("adam"):
        i, got = e["inp"], {}
        hy = dev(i["hyper"])
        for form in ("host", "dev", "dev_betas"):
            b = _state(i, "pmv")
            pe = ptr(b["ema"].t) if i["use_ema"] else None
            args = (ptr(b["p"].t), ptr(dev(i["g"])), ptr(b["m"].t), ptr(b["v"].t), pe, i["n"])
            if form == "host":
                rc = L.ph_adam_ema_step(*args, E.LR, E.BETA1, E.BETA2, i["eps"], i["wd"], i["step"], E.EMA_ALPHA, st)
            else:
                rc = L.ph_adam_ema_step_dev(*args, E.BETA1 if form == "dev" else -1.0, E.BETA2, i["eps"], i["wd"], ptr(hy), st)
            got[form] = _collect(f"adam {e['name']} {form}", rc, b, bad)
            _compare(R, e, got[form], bad, " " + form)
        for form in ("dev", "dev_betas"):
            for k in got["host"]:
                _bitwise(f"adam {e['name']} {k}: {form} against host", got[form][k], got["host"][k], bad)
        _LIVE.clear()
    _finish(R, bad, ("adam",))


def test_adagrad():
    def launch(L, ptr, st, i, what, bad):
        b = _state(i, "pv")
        rc = L.ph_adagrad_ema_step_dev(ptr(b["p"].t), ptr(dev(i["g"])), ptr(b["v"].t), ptr(b["ema"].t) if i["use_ema"] else None,
                                       i["n"], i["eps"], i["wd"], ptr(dev(i["hyper"])), st)
        return _collect(what, rc, b, bad)
    _sweep("adagrad", launch)


def test_ema_update_and_ema_update_dev():
    def launch(L, ptr, st, i, what, bad):
        ema = _inout(i["ema"])
        if i["dev"]:
            rc = L.ph_ema_update_dev(ptr(ema.t), ptr(dev(i["p"])), i["n"], ptr(dev(i["hyper"])), st)
        else:
            rc = L.ph_ema_update(ptr(ema.t), ptr(dev(i["p"])), i["n"], i["alpha"], st)
        return _collect(what, rc, {"ema": ema}, bad)
    _sweep("ema_update", launch)
    _sweep("ema_update_dev", launch)


def test_n_zero_updates_touch_nothing():
    L, ptr, st = _api()
    bad = []
    b = {k: _inout(np.arange(8, dtype=F32)) for k in ("p", "m", "v", "ema", "out")}
    before = {k: G.snapshot() for k, G in b.items()}
    g, hy = dev(np.ones(8, F32)), dev(E.hyper_record(1))
    p, m, v, ema, out = (ptr(b[k].t) for k in ("p", "m", "v", "ema", "out"))
    assert L.ph_adam_ema_step(p, ptr(g), m, v, ema, 0, E.LR, E.BETA1, E.BETA2, 1e-8, 0.0, 1, E.EMA_ALPHA, st) == OK
    assert L.ph_adam_ema_step_dev(p, ptr(g), m, v, ema, 0, E.BETA1, E.BETA2, 1e-8, 0.0, ptr(hy), st) == OK
    assert L.ph_adagrad_ema_step_dev(p, ptr(g), v, ema, 0, 1e-10, 0.0, ptr(hy), st) == OK
    assert L.ph_ema_update(ema, ptr(g), 0, 0.9, st) == OK and L.ph_ema_update_dev(ema, ptr(g), 0, ptr(hy), st) == OK
    assert L.ph_scaled_diff(ptr(g), ptr(g), ptr(hy), 0.5, out, 0, st) == OK
    assert L.ph_l1_sign_axpy(ptr(g), out, 0, None, 1.0, st) == OK
    for k, G in b.items():
        _untouched("n == 0: " + k, G, before[k], bad)
    # ph_sqdiff_sum of nothing writes 0 * scale
    o = _out(1)
    rc = L.ph_sqdiff_sum(ptr(g), ptr(g), ptr(o.t), 0, 3.0, st)
    got = _collect("ph_sqdiff_sum n 0", rc, {"out": o}, bad)
    _bitwise("ph_sqdiff_sum n 0", got["out"], np.zeros(1, F32), bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ tsvd / L1 / sigmoid-range
def test_scaled_diff():
    def launch(L, ptr, st, i, what, bad):
        out = _out(i["n"])
        rc = L.ph_scaled_diff(ptr(dev(i["a"])), ptr(dev(i["b"])), ptr(dev(i["gs"])), i["alpha"], ptr(out.t), i["n"], st)
        return _collect(what, rc, {"out": out}, bad)
    _sweep("scaled_diff", launch)


def test_l1_sign_axpy():
    def launch(L, ptr, st, i, what, bad):
        g = _inout(i["g"])
        cd = None if i["coef_dev"] is None else dev(np.array([i["coef_dev"]], F32))
        rc = L.ph_l1_sign_axpy(ptr(dev(i["w"])), ptr(g.t), i["n"], ptr(cd), i["coef"], st)
        return _collect(what, rc, {"g": g}, bad)
    _sweep("l1_sign_axpy", launch)


def _l1_sum(L, ptr, st, i, what, bad):
    parts = _out(1024)
    out = _inout(np.array([i["prior"]], F32)) if i["accumulate"] else _out(1)
    rc = L.ph_l1_sum(ptr(dev(i["w"])), i["n"], ptr(parts.t), ptr(out.t), i["accumulate"], st)
    return _collect(what, rc, {"out": out}, bad, scratch=(parts,))


def test_l1_sum_exact():
    _sweep("l1_sum_exact", _l1_sum)


def test_l1_sum():
    _sweep("l1_sum", _l1_sum)


def test_sqdiff_sum():
    def launch(L, ptr, st, i, what, bad):
        out = _out(1)
        rc = L.ph_sqdiff_sum(ptr(dev(i["a"])), ptr(dev(i["b"])), ptr(out.t), i["n"], i["scale"], st)
        return _collect(what, rc, {"out": out}, bad)
    _sweep("sqdiff_sum", launch)


def test_maxnorm_mix():
    def launch(L, ptr, st, i, what, bad):
        out = _out(i["n"])
        rc = L.ph_maxnorm_mix(ptr(dev(i["a"])), ptr(dev(i["b"])), ptr(out.t), i["n"], i["wa"], i["wb"], st)
        return _collect(what, rc, {"out": out}, bad)
    _sweep("maxnorm_mix", launch)


def test_sigmoid_range_fwd_and_bwd():
    def fwd(L, ptr, st, i, what, bad):
        outs = {"pred": _out(i["n"]), "sigma": _out(i["n"])}
        rc = L.ph_sigmoid_range_fwd(ptr(dev(i["h"])), ptr(dev(i["range"])), ptr(dev(i["shift"])), ptr(outs["pred"].t),
                                    ptr(outs["sigma"].t), i["n"], st)
        got = _collect(what, rc, outs, bad)
        if not (np.isfinite(got["pred"]).all() and np.isfinite(got["sigma"]).all()):
            bad.append(f"{what}: the forward is not finite")
        return got

    def bwd(L, ptr, st, i, what, bad):
        out = _out(i["n"])
        rc = L.ph_sigmoid_range_bwd(ptr(dev(i["dpred"])), ptr(dev(i["sigma"])), ptr(dev(i["range"])), ptr(out.t), i["n"], st)
        got = _collect(what, rc, {"dh": out}, bad)
        got["dh_sat"] = got["dh"][(i["sigma"] == 0) | (i["sigma"] == 1)]
        return got
    _sweep("sigmoid_range_fwd", fwd)
    _sweep("sigmoid_range_bwd", bwd)

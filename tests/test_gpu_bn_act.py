"""Sweep of the BatchNorm, ReLU, pooling and stem-backward kernels of the ResNet trunk (csrc/bn_act.hip) through their test entry
points (ph_debug_bn_*, at the end of that file), against tests/bn_emulation.py, in PH_PREC_BF16, PH_PREC_BF16X6 (fp32 tensors) and
PH_PREC_FP16X3 (half-pair images, decoded with gpu_util.hp_unpack; the [2][npix][4] planes of pack_input in numpy).

  exact class   inputs from dyadic grids on which every product and sum of the kernel is exact in float32: every ReLU mask, every
                max-pool output, idx code and raw value (windows of zeros and ties between positive taps included), the stem scatter
                dz, the outputs of bn_apply (the three grid-stride shapes too), avgpool_bwd (HW a power of two), bn_bwd_reduce and
                bn_bwd_apply, pack_input, the per-block amax rows, dzs, num_batches_tracked: bitwise equal to the numpy result.  The
                `raw` and `pooled` stem-reduce rows are bitwise equal to each other on every input.
  real class    normal random data against the float64 reference, within 4 x the float32 restatement's error on the same inputs plus
                the operator's floor (bn_emulation.FLOOR).

Every output and every buffer updated in place lives between sentinel guard bands (the payload starts 256-byte aligned): after each
call the return code is PH_OK, the guards are intact and no NaN (no arg-max code above 8) is left in the written region - every
partial row is written, the rows of blocks that own no pixel too.

The three grid-stride shapes of the issue are stated in eight-channel vectors (n8); a tensor has whole pixels, so each runs at
ceil(n8 / (C / 8)) pixels - at most C / 8 - 1 vectors more, the same grid and the same last block (tests/test_bn_emulation_cpu.py
checks that).

Measured on the MI355X, the largest excess of the device's error over the float32 restatement's, in units of max |ref|, per
operator: bn_finalize 5.37e-8 (the running statistics' `(1 - m) * old + m * new` and `beta - mean * scale`, contracted to fmas where
hipcc chooses), avgpool_bwd 9.573e-10 (`g * inv + old`), bn_eval_params 7.882e-10 (the device's rsqrtf); bn_emulation.FLOOR is 4 x
each.  No other operator exceeded its restatement (no floor): pack_input, bn_apply, bn_relu_maxpool, avgpool, avgpool_t,
bn_bwd_reduce, bn_bwd_finalize, bn_bwd_apply, stem_bwd_reduce, stem_bwd_apply.  Every test prints `excess[operator]` next to the
floor; re-measure after a change of the kernels or of the toolchain.
The smallest injected-defect ratios of the CPU self-test (tests/test_bn_emulation_cpu.py): the biased variance in the running
statistics 44.1 x the tolerance, `accumulate` ignored in the average-pool backward 69.6, the neighbouring channel group's constants
in bn_apply 78.9, the variance not clamped 7.8e3, the lane-rounded pixel count 3.9e4; every other defect above 1e5 or rejected by
an exact array.
With a scratch copy of bn_act.hip in which the arg-max took the last maximum, the reduce lanes strode npl + 1 pixels, bn_apply
dropped its tail iteration and the stem amax lost its factor 4, test_bn_relu_maxpool_exact, test_bn_bwd_reduce*,
test_bn_apply_grid_stride, test_stem_bwd_reduce* and test_stem_bwd_apply failed, each naming operator, case and first element.
The sweep found no kernel wrong."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bn_emulation as E
from tests.gpu_util import Guarded, Report, dispatch_lib, hp_pack, hp_unpack

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -22
F32 = np.float32
BF16, HP = E.BF16, E.FP16X3
EXCESS = {}         # operator -> largest (device error - restatement error) / max |ref| seen in this process


def _api():
    from multimodal_learning_amd._lib import ptr, stream
    return E.bind(dispatch_lib()), ptr, stream()


_LIVE = []          # the operands of the running test: `ptr(dev(a))` inside an argument list must not free `a` before the launch


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _LIVE.clear()


def dev(a, kind="f32", prec=E.BF16X6):
    """numpy array (or None) -> device tensor of the storage type of `kind` ("T": an activation as the convolutions read it, "TY": a
    convolution output or gradient, else as it is), kept alive until the case ends."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if kind in ("T", "TY") and prec == BF16:
        assert bool((t.bfloat16().float() == t).all()), "the input is no bf16"
        t = t.bfloat16()
    elif kind == "T" and prec == HP:
        p = hp_pack(t)
        assert bool((hp_unpack(p) == t).all()), "the input is no half pair"
        t = p
    _LIVE.append(t)
    return t


def _out(shape, kind="f32", prec=E.BF16X6):
    """A guarded output of the storage type of `kind` (half-pair images: the float32 container of the same shape)."""
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
    if kind == "u8":
        return Guarded(shape, torch.uint8, 255)
    if kind == "i64":
        return Guarded(shape, torch.int64, 0)
    if kind == "f16":
        return Guarded(shape, torch.float16)
    return Guarded(shape, torch.bfloat16 if kind in ("T", "TY") and prec == BF16 else torch.float32)


def _inout(a, kind="f32", prec=E.BF16X6):
    a = np.ascontiguousarray(a)
    G = _out(a.shape, "i64" if a.dtype == np.int64 else kind, prec)
    G.t.copy_(torch.from_numpy(a).to(G.t.dtype))
    return G


def _collect(what, rc, outs, bad, hp=()):
    """The return code is PH_OK; synchronise; guards intact and nothing left unwritten in every Guarded of `outs`; their contents as numpy
    arrays (bf16 widened, the half-pair images named in `hp` decoded)."""
    if rc != OK:
        bad.append(f"{what}: returned {rc}")
    torch.cuda.synchronize()
    res = {}
    for k, G in outs.items():
        if not G.guards_intact():
            bad.append(f"{what} {k}: guard band overwritten")
        t = hp_unpack(G.t) if k in hp else G.t
        a = (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()
        if a.dtype.kind == "f" and np.isnan(a).any():
            bad.append(f"{what} {k}: {int(np.isnan(a).sum())} elements never written (or NaN), first at {tuple(int(v[0]) for v in np.nonzero(np.isnan(a)))}")
        if a.dtype == np.uint8 and (a > 8).any():
            bad.append(f"{what} {k}: {int((a > 8).sum())} codes never written (or above 8)")
        res[k] = a
    return res


def _bitwise(what, got, expect, bad):
    got, exp = np.asarray(got), np.asarray(expect)
    got = got.reshape(exp.shape)
    if exp.dtype == np.float16:
        same = got.astype(np.float16).view(np.uint16) == exp.view(np.uint16)
    elif exp.dtype.kind == "f":
        exp = exp.astype(F32)
        same = got.astype(F32).view(np.int32) == exp.view(np.int32)
    else:
        same = got == exp
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        bad.append(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {i}: got {got[i]!r} expected {exp[i]!r}")


def _compare(R, e, got, bad, tag=""):
    """Every output array of suite entry e: bitwise in the exact class, against its tolerance otherwise."""
    op = E.base_op(e["op"])
    for k, ref in e["ref"].items():
        what = f"{e['name']}{tag} {k}"
        if k not in got:
            bad.append(f"{op} {what}: not produced")
        elif k in e["exact"]:
            _bitwise(f"{op} {what}", got[k], e["rest"][k], bad)
        else:
            g = np.asarray(got[k]).reshape(np.shape(ref))
            tol, er, sc = E.entry_tolerance(e, k), E.err(ref, g), E.scale(ref)
            if sc > 0 and np.isfinite(er):
                EXCESS[op] = max(EXCESS.get(op, 0.0), (er - E.err(ref, e["rest"][k])) / sc)
            if not er <= tol:
                with np.errstate(invalid="ignore"):
                    d = np.abs(g.astype(np.float64) - ref)
                i = np.unravel_index(int(np.argmax(np.where(np.isnan(d), np.inf, d))), d.shape)
                bad.append(f"{op} {what}: max |err| {er:.3e} > tol {tol:.3e}, first at {tuple(int(v) for v in i)}: got {g[i]!r} expected {ref[i]!r}")
            R.add(what, er, sc, tol)


def _finish(R, bad, ops=()):
    for op in ops:
        print(f"   excess[{op}] = {EXCESS.get(op, 0.0):.3e} of max |ref| (floor {E.FLOOR.get(op, 0.0):.1e})")
    if len(R.rows) > 60:                      # (the table of a long sweep: its worst rows)
        R.rows = sorted(R.rows, key=lambda r: -(r[1] / r[3] if r[3] > 0 else (np.inf if r[1] > 0 else 0)))[:30]
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad[:30])


def _sweep(suite, launch):
    """launch(L, ptr, st, e, what, bad) -> {output name: numpy array} for every case of `suite`."""
    L, ptr, st = _api()
    R, bad = Report(suite), []
    for e in E.suite(suite):
        _compare(R, e, launch(L, ptr, st, e["inp"], f"{E.base_op(suite)} {e['name']}", bad), bad)
        _LIVE.clear()
    _finish(R, bad, (E.base_op(suite),))


def _untouched(what, G, before, bad):
    torch.cuda.synchronize()
    if not torch.equal(G.buf, before):
        bad.append(f"{what}: the buffer was written")


# ------------------------------------------------------------------------------------------------ pack_input, bn_apply
def test_pack_input():
    def launch(L, ptr, st, i, what, bad):
        npix = i["B"] * i["H"] * i["W"]
        if i["prec"] == HP:
            G = _out((2, npix, 4), "f16")
        else:
            G = _out((npix, 4), "T", i["prec"])
        rc = L.ph_debug_bn_pack_input(ptr(dev(i["x"])), ptr(G.t), i["B"], i["H"], i["W"], i["prec"], st)
        got = _collect(what, rc, {"x4": G}, bad)
        if i["prec"] == HP:
            pl = got["x4"]
            got = {"hi": pl[0], "lo": pl[1], "x4": E.hp_join(pl[0], pl[1])}
        return got
    _sweep("pack_input", launch)


def _bn_apply(L, ptr, st, i, what, bad):
    p, shape = i["prec"], (i["npix"], i["C"])
    outs = {"out": _out(shape, "T", p)}
    if i["out32"]:
        outs["out32"] = _out(shape)
    rc = L.ph_debug_bn_apply(ptr(dev(i["y"], "TY", p)), ptr(dev(i["scale"])), ptr(dev(i["shift"])),
                             ptr(dev(i["res"], "T" if i["res_as_t"] else "TY", p)), ptr(dev(i["y_r"], "TY", p)), ptr(dev(i["scale_r"])),
                             ptr(dev(i["shift_r"])), ptr(outs["out"].t), ptr(outs["out32"].t) if i["out32"] else None, i["npix"], i["C"],
                             i["relu"], p, i["res_as_t"], st)
    return _collect(what, rc, outs, bad, hp=("out",) if p == HP else ())


def test_bn_apply_exact():
    _sweep("bn_apply_exact", _bn_apply)


def test_bn_apply():
    _sweep("bn_apply", _bn_apply)


def test_bn_apply_grid_stride():
    """More than 2048 blocks of 256 vectors: the grid-stride loop with its prefetch, the partial second iteration, the ragged last
    iteration and a grid above 2048 blocks; bitwise."""
    _sweep("bn_apply_stride", _bn_apply)


# ------------------------------------------------------------------------------------------------ pooling
def _maxpool(L, ptr, st, i, what, bad):
    p, B, H, W = i["prec"], i["B"], i["H"], i["W"]
    shape = (B, (H + 1) // 2, (W + 1) // 2, 64)
    outs = {"out": _out(shape, "T", p)}
    if p == HP:
        outs["out32"] = _out(shape)
    if i["idx"]:
        outs["idx"] = _out(shape, "u8")
        if i["raw"]:
            outs["raw"] = _out(shape, "TY", p)
    rc = L.ph_debug_bn_relu_maxpool(ptr(dev(i["y"], "TY", p)), ptr(dev(i["scale"])), ptr(dev(i["shift"])), ptr(outs["out"].t),
                                    ptr(outs["idx"].t) if i["idx"] else None, ptr(outs["raw"].t) if i["raw"] else None,
                                    ptr(outs["out32"].t) if p == HP else None, B, H, W, 64, p, st)
    return _collect(what, rc, outs, bad, hp=("out",) if p == HP else ())


def test_bn_relu_maxpool_exact():
    """Outputs, arg-max codes (first maximum wins, kh * 3 + kw) and raw values, with windows of zeros and ties; odd and even sizes."""
    _sweep("bn_relu_maxpool_exact", _maxpool)


def test_bn_relu_maxpool():
    _sweep("bn_relu_maxpool", _maxpool)


def test_avgpool_and_avgpool_t():
    def launch(kind, entry):
        def f(L, ptr, st, i, what, bad):
            out = _out((i["B"], i["C"]))
            rc = getattr(L, entry)(ptr(dev(i["x"], kind, i["prec"])), ptr(out.t), i["B"], i["HW"], i["C"], i["prec"], st)
            return _collect(what, rc, {"out": out}, bad)
        return f
    _sweep("avgpool", launch("TY", "ph_debug_bn_avgpool"))
    _sweep("avgpool_t", launch("T", "ph_debug_bn_avgpool_t"))


def test_avgpool_bwd():
    def launch(L, ptr, st, i, what, bad):
        p, shape = i["prec"], (i["B"], i["HW"], i["C"])
        dx = _inout(i["dx"], "TY", p) if i["accumulate"] else _out(shape, "TY", p)
        rc = L.ph_debug_bn_avgpool_bwd(ptr(dev(i["g"])), ptr(dx.t), i["B"], i["HW"], i["C"], i["accumulate"], p, st)
        return _collect(what, rc, {"dx": dx}, bad)
    _sweep("avgpool_bwd", launch)


# ------------------------------------------------------------------------------------------------ forward statistics
def test_bn_finalize():
    def launch(L, ptr, st, i, what, bad):
        C = i["C"]
        outs = {k: _out(C) for k in ("mean", "invstd", "scale", "shift")}
        rm = rv = nbt = None
        if i["running"] is not None:
            outs["running_mean"], outs["running_var"] = rm, rv = _inout(i["running"][0]), _inout(i["running"][1])
            outs["nbt"] = nbt = _inout(np.array([i["nbt"]], np.int64))
        rc = L.ph_debug_bn_finalize(ptr(dev(i["parts"])), i["nparts"], C, i["count"], i["eps"], i["momentum"], ptr(dev(i["gamma"])),
                                    ptr(dev(i["beta"])), *(ptr(outs[k].t) for k in ("mean", "invstd", "scale", "shift")),
                                    ptr(rm.t) if rm else None, ptr(rv.t) if rv else None, ptr(nbt.t) if nbt else None, st)
        return _collect(what, rc, outs, bad)
    _sweep("bn_finalize", launch)


def test_bn_eval_params():
    def launch(L, ptr, st, i, what, bad):
        n, keys = i["n"], ("mean", "invstd", "scale", "shift")
        outs = {(k, u): _out(i["units"][u]["C"]) for k in keys for u in range(n)}
        tabs = [(ctypes.c_void_p * n)(*(ptr(dev(u[k])) for u in i["units"])) for k in ("gamma", "beta", "running_mean", "running_var")]
        tabs += [(ctypes.c_void_p * n)(*(ptr(outs[(k, u)].t) for u in range(n))) for k in keys]
        widths = (ctypes.c_int * n)(*(u["C"] for u in i["units"]))
        rc = L.ph_debug_bn_eval_params(*(ctypes.addressof(t) for t in tabs), ctypes.addressof(widths), n, i["eps"], st)
        got = _collect(what, rc, {"%s%d" % ku: G for ku, G in outs.items()}, bad)
        return {k: np.concatenate([got["%s%d" % (k, u)] for u in range(n)]) for k in keys}
    _sweep("bn_eval_params", launch)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def _bwd_operands(ptr, i):
    p = i["prec"]
    return (ptr(dev(i["g"], "TY", p)), ptr(dev(i["a"], "TY", p)), ptr(dev(i["y"], "TY", p)), ptr(dev(i["mean"])), ptr(dev(i["invstd"])))


def _bwd_reduce(L, ptr, st, i, what, bad):
    nb = L.ph_debug_bn_bwd_parts(i["npix"], i["C"])
    if nb != E.bn_bwd_parts(i["npix"], i["C"]):
        bad.append(f"{what}: ph_debug_bn_bwd_parts = {nb}")
        return {}
    outs = {"parts": _out((nb, 2, i["C"]))}
    if i["amax"]:
        outs["amax"] = _out(nb)
    rc = L.ph_debug_bn_bwd_reduce(*_bwd_operands(ptr, i), ptr(outs["parts"].t), i["npix"], i["C"], i["prec"], ptr(dev(i["mscale"])),
                                  ptr(dev(i["mshift"])), ptr(outs["amax"].t) if i["amax"] else None, st)
    return _collect(what, rc, outs, bad)


def test_bn_bwd_reduce_exact():
    _sweep("bn_bwd_reduce_exact", _bwd_reduce)


def test_bn_bwd_reduce():
    """Fewer pixels per block than lanes, ragged last blocks, masks from a / from mscale, mshift / none, amax in half-pair mode."""
    _sweep("bn_bwd_reduce", _bwd_reduce)


def test_bn_bwd_reduce_at_the_row_clamp():
    _sweep("bn_bwd_reduce_clamp", _bwd_reduce)


def _bwd_finalize(L, ptr, st, i, what, bad):
    C = i["C"]
    outs = {"c1": _out(C), "c2": _out(C)}
    if i["dgb"]:
        outs["dgamma"], outs["dbeta"] = _out(C), _out(C)
    dg, db = (ptr(outs[k].t) if i["dgb"] else None for k in ("dgamma", "dbeta"))
    if i["fused"]:
        rc = L.ph_debug_bn_bwd_finalize_fused(ptr(dev(i["parts"])), i["nparts"], C, i["count"], dg, db, ptr(outs["c1"].t), ptr(outs["c2"].t),
                                              ptr(dev(i["invstd"])), i["row2"], st)
    else:
        outs["dzs"] = _out(2)
        rc = L.ph_debug_bn_bwd_finalize(ptr(dev(i["parts"])), i["nparts"], C, i["count"], dg, db, ptr(outs["c1"].t), ptr(outs["c2"].t),
                                        ptr(dev(i["amax"])), len(i["amax"]), ptr(dev(i["gamma"])), ptr(dev(i["invstd"])), ptr(outs["dzs"].t), st)
    return _collect(what, rc, outs, bad)


def test_bn_bwd_finalize():
    _sweep("bn_bwd_finalize", _bwd_finalize)
    L, ptr, st = _api()
    bad, out = [], _out(64)
    before = out.snapshot()
    z = dev(np.zeros((4, 3, 64), F32))
    for row2 in (0, 3, -1):
        assert L.ph_debug_bn_bwd_finalize_fused(ptr(z), 4, 64, 4.0, None, None, ptr(out.t), ptr(out.t), ptr(z), row2, st) == EINVAL
    _untouched("ph_debug_bn_bwd_finalize_fused row2 0 / 3 / -1", out, before, bad)
    assert not bad, bad


def test_dzs_across_the_binades():
    """bound dzs[0] in [2^9, 2^10), dzs[0] dzs[1] = 1, both powers of two; the exponent clamp; a bound of 0 or infinity gives 1."""
    L, ptr, st = _api()
    R, bad = Report("dzs"), []
    for e in E.suite("dzs"):
        got = _bwd_finalize(L, ptr, st, e["inp"], f"bn_bwd_finalize {e['name']}", bad)
        _compare(R, e, got, bad)
        d, j = got["dzs"].astype(np.float64), e["inp"]["j"]
        if not (d[0] * d[1] == 1 and np.frexp(d[0])[0] == 0.5):
            bad.append(f"{e['name']}: dzs {d} is no reciprocal pair of powers of two")
        if j in ("zero", "inf"):
            if d[0] != 1:
                bad.append(f"{e['name']}: dzs[0] = {d[0]}, expected 1")
        elif -91 <= j <= 109 and not 2.0 ** 9 <= np.ldexp(1.5, j) * d[0] < 2.0 ** 10:
            bad.append(f"{e['name']}: bound dzs[0] = {np.ldexp(1.5, j) * d[0]} outside [2^9, 2^10)")
        _LIVE.clear()
    _finish(R, bad, ("bn_bwd_finalize",))


def _device_dzs(L, ptr, st, i, what, bad, amax, nb):
    """The dz scale the finalize pass derives from the amax rows of the reduce pass that just ran; equal to the emulation's, bitwise."""
    C = i["C"] if "C" in i else 64
    dzs, c = _out(2), _out((2, C))
    z = dev(np.zeros((nb, 2, C), F32))
    rc = L.ph_debug_bn_bwd_finalize(ptr(z), nb, C, 1.0, None, None, ptr(c.t[0]), ptr(c.t[1]), ptr(amax.t), nb, ptr(dev(i["gamma"])),
                                    ptr(dev(i["invstd"])), ptr(dzs.t), st)
    got = _collect(what + " (dzs)", rc, {"dzs": dzs, "amax": amax}, bad)
    _bitwise(what + " amax rows", got["amax"], i["amax_rows"], bad)
    _bitwise(what + " dzs", got["dzs"], i["dzs"], bad)
    return dzs


def _bwd_apply(L, ptr, st, i, what, bad):
    p, shape = i["prec"], (i["npix"], i["C"])
    dzs = None
    if i["dzs"] is not None:
        nb = E.bn_bwd_parts(i["npix"], i["C"])
        parts, amax = _out((nb, 2, i["C"])), _out(nb)
        rc = L.ph_debug_bn_bwd_reduce(*_bwd_operands(ptr, i), ptr(parts.t), i["npix"], i["C"], p, ptr(dev(i["mscale"])), ptr(dev(i["mshift"])),
                                      ptr(amax.t), st)
        _collect(what + " (reduce)", rc, {"parts": parts}, bad)
        dzs = _device_dzs(L, ptr, st, i, what, bad, amax, nb)
    dy = _out(shape, "T", p)
    rc = L.ph_debug_bn_bwd_apply(*_bwd_operands(ptr, i), ptr(dev(i["gamma"])), ptr(dev(i["c1"])), ptr(dev(i["c2"])), ptr(dy.t), i["npix"], i["C"],
                                 p, ptr(dev(i["mscale"])), ptr(dev(i["mshift"])), ptr(dzs.t) if dzs else None, st)
    got = _collect(what, rc, {"dy": dy}, bad, hp=("dy",) if p == HP else ())
    if dzs:
        got["dy"] = got["dy"] * i["dzs"][1]
    return got


def test_bn_bwd_apply_exact():
    _sweep("bn_bwd_apply_exact", _bwd_apply)


def test_bn_bwd_apply():
    """Half-pair mode: amax from the reduce pass, dzs from the finalize pass, the decoded output times dzs[1] is compared."""
    _sweep("bn_bwd_apply", _bwd_apply)


def test_bn_bwd_apply_grid_stride():
    _sweep("bn_bwd_apply_stride", _bwd_apply)


# ------------------------------------------------------------------------------------------------ stem backward
def _stem_operands(ptr, i):
    p = i["prec"]
    return ptr(dev(i["dpool"], "TY", p)), ptr(dev(i["idx"])), ptr(dev(i["y"], "TY", p))


def _stem_reduce(L, ptr, st, i, what, bad, form=None, amax=None):
    form, p = form or i["form"], i["prec"]
    nb = L.ph_debug_bn_stem_bwd_parts(i["B"], i["H"])
    assert nb == E.stem_blocks(i["B"], i["H"])
    outs = {"parts": _out((nb, 2, 64))}
    if i["amax"] if amax is None else amax:
        outs["amax"] = _out(nb)
    rc = L.ph_debug_bn_stem_bwd_reduce(*_stem_operands(ptr, i), ptr(dev(i["raw"], "TY", p)) if form == "raw" else None, ptr(dev(i["mean"])),
                                       ptr(dev(i["invstd"])), ptr(dev(i["scale"])), ptr(dev(i["shift"])), ptr(outs["parts"].t), i["B"], i["H"],
                                       i["W"], 64, p, ptr(outs["amax"].t) if "amax" in outs else None,
                                       1 if form == "pixel" and i["H"] % 2 == 0 else 0, st)
    got = _collect(what, rc, outs, bad)
    got["sums"] = got["parts"].astype(np.float64).sum(0).astype(F32)
    got["_amax_buf"] = outs.get("amax")
    return got


def _stem_reduce_sweep(suite):
    L, ptr, st = _api()
    R, bad, rows = Report(suite), [], {}
    for e in E.suite(suite):
        i = e["inp"]
        got = _stem_reduce(L, ptr, st, i, f"stem_bwd_reduce {e['name']}", bad)
        _compare(R, e, got, bad)
        rows[(i["B"], i["H"], i["W"], i["prec"], i["form"])] = got["parts"]
        _LIVE.clear()
    pairs = 0
    for (B, H, W, p, form), parts in rows.items():            # raw against pooled: the same rows, bit for bit
        if form == "raw":
            _bitwise(f"stem_bwd_reduce B{B} H{H} W{W} {E.PNAME[p]}: raw rows against pooled rows", parts, rows[(B, H, W, p, "pooled")], bad)
            pairs += 1
    assert pairs == 6
    _finish(R, bad, ("stem_bwd_reduce",))


def test_stem_bwd_reduce_exact():
    _stem_reduce_sweep("stem_bwd_reduce_exact")


def test_stem_bwd_reduce():
    """raw, pooled and per-pixel forms (the per-pixel form at an even H through the entry's `form` argument); amax = 4 x the block's
    largest masked window gradient, bitwise; amax with an odd H is refused."""
    _stem_reduce_sweep("stem_bwd_reduce")
    L, ptr, st = _api()
    bad = []
    i = next(e["inp"] for e in E.suite("stem_bwd_reduce") if e["inp"]["H"] % 2)
    parts, amax = _out((E.stem_blocks(i["B"], i["H"]), 2, 64)), _out(8)
    before = parts.snapshot(), amax.snapshot()
    rc = L.ph_debug_bn_stem_bwd_reduce(*_stem_operands(ptr, i), None, ptr(dev(i["mean"])), ptr(dev(i["invstd"])), ptr(dev(i["scale"])),
                                       ptr(dev(i["shift"])), ptr(parts.t), i["B"], i["H"], i["W"], 64, i["prec"], ptr(amax.t), 0, st)
    assert rc == EINVAL
    _untouched("stem reduce, amax with an odd H: parts", parts, before[0], bad)
    _untouched("stem reduce, amax with an odd H: amax", amax, before[1], bad)
    assert not bad, bad


def _stem_apply(L, ptr, st, i, what, bad):
    p = i["prec"]
    dzs = None
    if i["dzs"] is not None:
        red = _stem_reduce(L, ptr, st, i, what + " (reduce)", bad, form="raw", amax=True)
        dzs = _device_dzs(L, ptr, st, i, what, bad, red["_amax_buf"], E.stem_blocks(i["B"], i["H"]))
    dy = _out((i["B"], i["H"], i["W"], 64), "T", p)
    rc = L.ph_debug_bn_stem_bwd_apply(*_stem_operands(ptr, i), ptr(dev(i["mean"])), ptr(dev(i["invstd"])), ptr(dev(i["scale"])),
                                      ptr(dev(i["shift"])), ptr(dev(i["gamma"])), ptr(dev(i["c1"])), ptr(dev(i["c2"])), ptr(dy.t), i["B"], i["H"],
                                      i["W"], 64, p, ptr(dzs.t) if dzs else None, st)
    got = _collect(what, rc, {"dy": dy}, bad, hp=("dy",) if p == HP else ())
    if dzs:
        got["dy"] = got["dy"] * i["dzs"][1]
    return got


def test_stem_bwd_apply_exact():
    """gamma invstd = 1, c1 = c2 = 0: dy0 is the scattered, masked gradient itself - the stem scatter dz, bitwise."""
    _sweep("stem_bwd_apply_exact", _stem_apply)


def test_stem_bwd_apply():
    _sweep("stem_bwd_apply", _stem_apply)


def test_widths_the_kernels_cannot_take_are_refused_before_a_launch():
    L, ptr, st = _api()
    bad, out = [], _out((33, 24), "TY", BF16)
    before = out.snapshot()
    x, c = dev(np.zeros((33, 24), F32), "TY", BF16), dev(np.zeros(24, F32))
    assert L.ph_debug_bn_bwd_parts(33, 24) == EINVAL
    assert L.ph_debug_bn_apply(ptr(x), ptr(c), ptr(c), None, None, None, None, ptr(out.t), None, 33, 24, 1, BF16, 0, st) == EINVAL
    assert L.ph_debug_bn_bwd_reduce(ptr(x), None, ptr(x), ptr(c), ptr(c), ptr(out.t), 33, 24, BF16, None, None, None, st) == EINVAL
    assert L.ph_debug_bn_bwd_apply(ptr(x), None, ptr(x), ptr(c), ptr(c), ptr(c), ptr(c), ptr(c), ptr(out.t), 33, 24, BF16, None, None, None, st) == EINVAL
    _untouched("C = 24", out, before, bad)
    assert not bad, bad

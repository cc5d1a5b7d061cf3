"""CPU self-test of tests/zoo_emulation.py, the references and the tolerance rule of the RKD / PKT / Cox sweep
(tests/test_gpu_zoo_sweep.py): the float64 references reproduce the committed goldens of the reference's own classes, so they are
not their own oracle; the rule accepts the float32 restatement of every operator on every case and each injected defect
(zoo_emulation.DEFECTS) fails it on at least one listed case; the case tables reach what they are meant to reach; the host rule of
ph_rkd_one_workgroup_fits at its fit / no-fit pairs."""
import os

import numpy as np
import pytest
import torch

from tests import zoo_emulation as E

# The goldens were recorded by the reference's float32 code; a float32 statement of these formulas lies within 1e-7 .. 4e-6 of float64
# in units of max |ref| (sums of up to B^2 D products at 6e-8 each), so the float64 reference meets them within 1e-5.
GOLDEN_RTOL = 1e-5


def _rel(ref, golden):
    ref = np.asarray(ref, np.float64)
    return E.err(ref, np.asarray(golden, np.float64).reshape(ref.shape)) / E.scale(ref)


def test_rkd_and_pkt_references_reproduce_the_small_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "zoo_sp_featskl.npz"))
    for B in (8, 64, 128):
        f_s, f_t = g[f"r_f_s{B}"], g[f"r_f_t{B}"]
        for name, r in (("rkd", E.rkd_ref(f_s, f_t)), ("pkt", E.pkt_ref(f_s, f_t))):
            assert _rel(r["loss"], g[f"{name}{B}"]) <= GOLDEN_RTOL, (name, B)
            assert _rel(r["dx"], g[f"{name}_g{B}"]) <= GOLDEN_RTOL, (name, B)


@pytest.mark.parametrize("shape", [(192, 128), (256, 64), (512, 128)])
def test_rkd_part_and_pkt_references_reproduce_the_global_goldens(golden_dir, shape):
    """The float64 parts of a partition into ranges of 128 anchors, summed, are RKD.py's loss and gradient."""
    Bg, D = shape
    g = np.load(os.path.join(golden_dir, "zoo_global_b%d_d%d.npz" % shape))
    f_s, f_t = g["f_s"].astype(np.float32), g["f_t"].astype(np.float32)
    loss, dx = 0.0, 0.0
    for lo in range(0, Bg, 128):
        r = E.rkd_part_ref(f_s, f_t, lo, min(128, Bg - lo))
        loss, dx = loss + r["loss"], dx + r["dx"]
    assert _rel(loss, g["rkd"]) <= GOLDEN_RTOL and _rel(dx, g["rkd_g"]) <= GOLDEN_RTOL
    p = E.pkt_ref(f_s, f_t)
    assert _rel(p["loss"], g["pkt"]) <= GOLDEN_RTOL and _rel(p["dx"], g["pkt_g"]) <= GOLDEN_RTOL


def test_cox_reference_reproduces_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "cox_loss.npz"))
    for B in (8, 64, 300):
        r = E.cox_ref(g[f"theta{B}"], g[f"t{B}"], g[f"c{B}"])
        assert _rel(r["loss"], g[f"loss{B}"]) <= GOLDEN_RTOL and _rel(r["dx"], g[f"g{B}"]) <= GOLDEN_RTOL, B


# ------------------------------------------------------------------------------------------------ the rule
def _cases(op):
    if op == "rkd_part":
        return [("rkd_part", c) for c in E.RKD_PART_CASES] + [("rkd_part_deg", (0, 70)), ("rkd_part_deg", (60, 10))]
    if op == "rkd":
        return [("rkd", (B, D)) for B, D, rc, _ in E.RKD_ONE_CASES if rc == E.OK]
    if op == "pkt":
        return [("pkt", c) for c in E.PKT_CASES] + [("pkt_zero_row", ())]
    return [("cox", B) for B in E.COX_CASES] + [("cox_censored", ())]


def _outputs(kind, key, e):
    """The outputs of a case the sweep compares."""
    if kind == "rkd" and not next(c[3] for c in E.RKD_ONE_CASES if c[:2] == key):
        return ("loss",)
    return tuple(e["abs"])


def _defective(kind, e, defect):
    i = e["inp"]
    if kind.startswith("rkd_part"):
        return E.rkd_part_f32(i["f_s"], i["f_t"], i["lo"], i["na"], defect=defect)
    if kind == "rkd":
        return E.rkd_f32(i["f_s"], i["f_t"], defect=defect)
    if kind.startswith("pkt"):
        out = E.pkt_f32(i["f_s"], i["f_t"], defect=defect)
        if kind == "pkt_zero_row":
            out["dx_live"] = E.live_rows(out["dx"])
        return out
    return E.cox_f32(i["theta"], i["t"], i["c"], defect=defect)


def _ratio(kind, key, e, outs):
    r = 0.0
    for o in _outputs(kind, key, e):
        tol, er = E.case_tolerance(kind, e, o), E.err(e["ref"][o], outs[o])
        r = max(r, er / tol if tol > 0 else (np.inf if er > 0 else 0.0))
    return r


@pytest.mark.parametrize("op", sorted(E.DEFECTS))
def test_restatement_inside_and_every_defect_outside_the_rule(op):
    """Every defect fails the rule on at least one listed case; printed per defect: the cases it changes, how many of them fail, and the
    smallest and the largest error / tolerance among them (the figures in the docstring of tests/test_gpu_zoo_sweep.py)."""
    bad, seen = [], {d: [] for d in E.DEFECTS[op]}
    for kind, key in _cases(op):
        e = E.case(kind, key)
        for o in _outputs(kind, key, e):
            if not E.err(e["ref"][o], e["rest"][o]) <= E.case_tolerance(kind, e, o):
                bad.append(f"{kind} {key} {o}: the restatement misses its own tolerance")
        for d in E.DEFECTS[op]:
            outs = _defective(kind, e, d)
            if all(np.array_equal(outs[o], e["rest"][o], equal_nan=True) for o in ("loss", "dx")):
                continue                                        # the defect does not touch this case
            seen[d].append(_ratio(kind, key, e, outs))
    for d, rs in seen.items():
        fails = [r for r in rs if r > 1.0]
        print(f"\n{op:<9s} {d:<17s} changes {len(rs):2d} cases, fails {len(fails):2d}; error / tolerance: smallest {min(rs, default=0):.3g}, "
              f"smallest failing {min(fails, default=0):.3g}, largest {max(rs, default=0):.3g}")
        if not fails:
            bad.append(f"{op}: defect {d} ({E.DEFECTS[op][d]}) fails no case")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the tables
def test_inputs_have_no_zero_row_and_a_reference_to_measure_against():
    for kind, key in [c for op in sorted(E.DEFECTS) for c in _cases(op)]:
        e, i = E.case(kind, key), E.case(kind, key)["inp"]
        zero_ref = any(v > 0 for v in e["abs"].values()) or kind == "cox_censored"
        if "f_s" in i and kind not in ("pkt_zero_row", "rkd_part_deg"):
            assert bool((i["f_s"].abs().sum(1) > 0).all()) and bool((i["f_t"].abs().sum(1) > 0).all()), (kind, key)
        for o in _outputs(kind, key, e):
            assert np.isfinite(e["ref"][o]).all() and np.isfinite(e["rest"][o]).all(), (kind, key, o)
            assert zero_ref or E.scale(e["ref"][o]) > 0, (kind, key, o)
    f_s, f_t = E.rkd_degenerate_rows()
    assert torch.equal(f_s[3], f_s[64]) and not torch.equal(f_t[3], f_t[64]) and float(f_s[10].abs().sum()) == 0
    assert float(E.case("pkt_zero_row", ())["inp"]["f_s"][E.PKT_ZERO_ROW[2]].abs().sum()) == 0
    for B in E.COX_CASES[2:]:
        _, t, c = E.cox_inputs(B, B)
        assert len(set(t.tolist())) <= B // 3 and 0.5 < float(c.mean()) < 0.7, B


def test_tables_reach_the_kernel_variants_and_edges():
    part = E.RKD_PART_CASES
    variant = lambda D: 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8
    assert {variant(c[1]) for c in part} == {1, 2, 4, 8}
    assert {129, 256, 257, 512} <= {c[1] for c in part}                                  # <4> and <8> at both of their edges
    assert any(Bg > 64 and Bg % 64 for Bg, *_ in part) and any(Bg > 128 and Bg % 64 for Bg, *_ in part)
    assert any(D > 64 and D % 32 for _, D, *_ in part)
    assert any(na > 64 and na % 64 for *_, na in part)                                   # a last slab that is not 64 anchors long
    assert any(Bg > 64 and lo % 64 and (lo + na) % 64 and lo + na < Bg for Bg, _, lo, na in part)
    assert any(Bg > 256 and lo + na == Bg for Bg, _, lo, na in part) and any(Bg == 1024 for Bg, *_ in part)
    for (Bg, D), ranges in E.RKD_PARTITIONS:
        assert ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == Bg and len({n for _, n in ranges}) == 3
        assert all(a[0] + a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for B, D, rc, _ in E.RKD_ONE_CASES:
        assert (rc == E.OK) == E.rkd_one_wg_fits(B, D), (B, D)
    assert all(E.rkd_one_wg_fits(B, D) for B, D in E.RKD_ONE_VS_TILED)
    pk = E.PKT_CASES
    assert any(B % 4 for B, _ in pk) and any(B > 64 and B % 64 for B, _ in pk) and any(D > 64 and D % 64 for _, D in pk)
    assert any(16 < B for B, _ in pk) and any(B > 1024 for B, _ in pk)
    assert {1023, 1024, 1025, 4096} <= set(E.COX_CASES) and set(E.COX_FUSED) <= set(E.COX_CASES)


def test_one_workgroup_fit_query_is_the_lds_rule():
    """ph_rkd_one_workgroup_fits (host only): the shapes ph_rkd_loss_grad takes; RKDLoss sends the others to the tiled kernels."""
    import multimodal_learning_amd as m
    L = m.lib()
    for B, D, fits in E.RKD_FIT_PAIRS:
        assert L.ph_rkd_one_workgroup_fits(B, D) == fits == int(E.rkd_one_wg_fits(B, D)), (B, D)
    for B in (1, 2, 3, 64, 65, 66, 67, 81, 82, 105, 106, 128, 129, 1024):
        for D in (0, 1, 64, 128, 129, 256, 384, 512, 513):
            assert L.ph_rkd_one_workgroup_fits(B, D) == int(E.rkd_one_wg_fits(B, D)), (B, D)
    assert all(L.ph_rkd_one_workgroup_fits(B, 128) for B in range(2, 129))             # every batch the D = 128 trainers run
    assert L.ph_rkd_one_workgroup_fits(-5, 8) == 0 and L.ph_rkd_one_workgroup_fits(8, -5) == 0
    # a refused shape is PH_EINVAL before any HIP call (this machine may have no device: anything that reached HIP would not be -22)
    import ctypes as C
    p = C.cast((C.c_float * 16)(), C.c_void_p)
    for B, D, fits in E.RKD_FIT_PAIRS:
        if not fits:
            assert L.ph_rkd_loss_grad(p, p, p, p, B, D, 25.0, 50.0, p, None) == E.EINVAL, (B, D)

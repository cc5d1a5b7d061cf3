"""tests/tsvd_emulation.py, the numpy float32 restatement of the tiled t-SVD prox, on the CPU: it reproduces the errors and
sweep counts recorded in tests/golden/tsvd_tiled_restatement.json (which the GPU tolerances are built from), every
recorded sweep count is under the kernel's cap, and the tolerance the device is held to catches the defects such a
kernel can have."""
import functools

import numpy as np
import pytest

from tests import tsvd_emulation as E

SMALL = [s for s in E.SHAPES if s[0] <= 257]


@functools.lru_cache(maxsize=None)
def _case(B, V, D, tau):
    from oracle import variants as OV
    adj = E.make_stack(B, V, D)
    ref, tnn_ref = OV.update_aux(adj, tau)
    return adj.numpy(), ref, tnn_ref


def test_record_covers_every_shape_and_sweeps_stay_under_the_cap():
    rec = E.record()
    assert sorted(rec) == sorted(E.key(*s) for s in E.SHAPES)
    for k, r in rec.items():
        V = int(k.split("x")[1])
        assert len(r["sweeps"]) == V // 2 + 1 and all(1 <= s < E.TB_MAX_SWEEPS for s in r["sweeps"]), (k, r["sweeps"])
        assert r["aux_err"] > 0 and r["tnn_rel"] >= 0


@pytest.mark.parametrize("B,V,D,tau", SMALL)
def test_restatement_reproduces_its_record(B, V, D, tau):
    adj, ref, tnn_ref = _case(B, V, D, tau)
    rec = E.record()[E.key(B, V, D, tau)]
    aux, tnn, sweeps = E.restate(adj, tau)
    ea, et = E.errors(aux, tnn, ref, tnn_ref)
    print(f"\n   {E.key(B, V, D, tau)}: aux err {ea:.3e} (recorded {rec['aux_err']:.3e})  TNN rel {et:.3e} (recorded {rec['tnn_rel']:.3e})  sweeps {sweeps}")
    assert sweeps == rec["sweeps"]
    assert ea <= 2 * rec["aux_err"] and et <= 2 * rec["tnn_rel"] + 1e-7
    assert abs(float(np.abs(ref).max()) - rec["max_ref"]) <= 1e-9 and abs(tnn_ref - rec["tnn_ref"]) <= 1e-9 * abs(tnn_ref)


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_injected_defect_misses_the_aux_tolerance_tenfold(defect):
    """At (129, 2, 32, 0.1) - a partial last block, five block pairs - each defect leaves an aux error at least 10 x the
    tolerance the device is held to at that shape (floors included)."""
    B, V, D, tau = E.SHAPES[0]
    adj, ref, tnn_ref = _case(B, V, D, tau)
    tol_a, tol_t = E.tolerances(E.record()[E.key(B, V, D, tau)])
    aux, tnn, sweeps = E.restate(adj, tau, defect=defect)
    ea, et = E.errors(aux, tnn, ref, tnn_ref)
    print(f"\n   defect {defect}: aux err {ea:.3e} = {ea / tol_a:.0f} x tol {tol_a:.3e};  TNN rel {et:.3e} = {et / tol_t:.1f} x tol {tol_t:.3e};  sweeps {sweeps}")
    assert ea >= 10 * tol_a, (defect, ea, tol_a)

"""The two DSCD entry points of csrc/crd.hip through the C ABI, against tests/dscd_emulation.py.  Every output lives between
NaN- / -7-filled guard bands (the helpers of tests/test_gpu_crd.py): the guards stay intact and nothing in the written region is
left unwritten.

  ph_crd_select_dscd    bit for bit against numpy's stable argsort and the float32 product out * (1 + diff): sel, xs, xt at the
                        shapes dscd_emulation.SELECT_SHAPES (the smallest lists, both parities of P % 4, K longer than the block,
                        P above the block, the shipped sizes, 2 P words above 64 KiB of LDS - that launch must succeed), B in
                        {1, 3}, both directions, both weight settings, `ranks` NULL and given with a repeated rank and rank
                        P - 1; keys from a five-value set with +0 and -0, weights at or below zero included.
  ph_crd_loss_grad_one  dv bitwise equal to the dv2 of ph_crd_loss_grad on the same xt, sel, idx, mem1 and Z_v2 - in the
                        one-workgroup form and in the split form (P2 + K >= 1024: 2 and 5 splits) - at widths 64, 128, 256;
                        loss and dv against float64 within 4 x the float32 restatement's error plus the loss kernel's measured
                        floor (crd_width_emulation.FLOOR["loss_grad"], 4.9e-8 of max |ref|; no other constant).  The mono
                        bank's params layout [P, K, T, Z_v2, momentum] is what the entry is given: index 1 holds K, and T is
                        the argument."""
import numpy as np
import pytest
import torch

from tests import crd_width_emulation as W
from tests import dscd_emulation as DE
from tests.gpu_util import Report
from tests.test_gpu_crd import _api, _collect, _out, _release_operands, _same_bits, _workspace, dev      # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.mark.parametrize("shape", DE.SELECT_SHAPES, ids=lambda s: "P%d_K%d_P2_%d" % s)
def test_select_dscd_exact(shape):
    L, ptr, st = _api()
    bad, n = [], 0
    for c in DE.select_cases():
        if (c["P"], c["K"], c["P2"]) != shape:
            continue
        n += 1
        B, P, K, P2 = c["B"], c["P"], c["K"], c["P2"]
        what = "select_dscd B%d P%d K%d P2 %d asc%d rw%d ranks %s" % (B, P, K, P2, c["asc"], c["rw"], c["ranks"])
        i = DE.select_inputs(c)
        exp = DE.select_ref(i["diff"], i["out1"], i["out2"], i["ranks"], P, K, P2, c["asc"], c["rw"])
        o = {"sel": _out((B, P2 + K), torch.int32), "xs": _out((B, P2 + K)), "xt": _out((B, P2 + K))}
        rc = L.ph_crd_select_dscd(ptr(dev(i["diff"])), ptr(dev(i["out1"])), ptr(dev(i["out2"])), ptr(dev(i["ranks"])), ptr(o["sel"].t),
                                  ptr(o["xs"].t), ptr(o["xt"].t), B, P, K, P2, c["asc"], c["rw"], st)
        assert rc == 0, f"{what}: the launch was refused (rc {rc})"
        got = _collect(what, o, bad)
        for k in ("sel", "xs", "xt"):
            _same_bits(f"{what} {k}", got[k], exp[k], bad)
    assert n >= 4
    if shape[0] == 8200:
        assert 2 * shape[0] * 4 > 64 * 1024
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("D", W.WIDTHS)
def test_loss_grad_one_is_the_half_of_the_two_directional_entry(D):
    L, ptr, st = _api()
    R, bad, splits = Report("ph_crd_loss_grad_one, width %d" % D), [], set()
    excess = 0.0
    for c in DE.LG_ONE_CASES:
        if c["D"] != D:
            continue
        two, one = DE.lg_one_inputs(c)
        B, S2 = two["xt"].shape
        name = "S2 %d P2 %d B%d posw%d T%g" % (S2, c["P2"], B, c["posw"], c["T"])
        splits.add(two["ns"])
        ws = S2 >= 1024
        assert (two["ns"] > 1) == ws
        nbytes = L.ph_crd_loss_grad_workspace_bytes_w(B, D)
        W2, W1 = (_workspace(nbytes), _workspace(nbytes)) if ws else (None, None)
        o2 = {"lossp": _out((B,)), "dv1": _out((B, D)), "dv2": _out((B, D))}
        xt, sel, idx, mem1 = dev(two["xt"]), dev(two["sel"]), dev(two["idx"]), dev(two["mem1"])
        posw = dev(two["posw_t"])
        rc = L.ph_crd_loss_grad(ptr(dev(two["xs"])), ptr(xt), ptr(sel), ptr(idx), None, ptr(dev(two["posw_s"])), ptr(posw), ptr(mem1),
                                ptr(dev(two["mem2"])), ptr(dev(two["params"])), ptr(o2["lossp"].t), ptr(o2["dv1"].t), ptr(o2["dv2"].t),
                                B, two["PK"], two["P2"], two["K2"], D, two["n_data"], two["inv_bnorm"], ptr(W2.t) if ws else None, st)
        assert rc == 0, (name, rc)
        o1 = {"lossp": _out((B,)), "dv": _out((B, D))}
        assert one["params"][1] == two["K2"] and one["params"][2] == F32(c["T"])      # the mono layout: K where the kernels read T
        rc = L.ph_crd_loss_grad_one(ptr(xt), ptr(sel), ptr(idx), ptr(posw), ptr(mem1), ptr(dev(one["params"])), float(c["T"]),
                                    ptr(o1["lossp"].t), ptr(o1["dv"].t), B, one["PK"], one["P2"], one["K2"], D, one["n_data"],
                                    one["inv_bnorm"], ptr(W1.t) if ws else None, st)
        assert rc == 0, (name, rc)
        g2, g1 = _collect(name + " two", o2, bad), _collect(name + " one", o1, bad)
        if ws and not (W1.guards_intact() and W2.guards_intact()):
            bad.append(f"{name}: workspace guard band overwritten")
        _same_bits(f"{name}: dv of the half against dv2 of the two-directional entry", g1["dv"], g2["dv2"], bad)
        ref, rest = DE.loss_grad_one(one, np.float64, D), DE.loss_grad_one(one, F32, D)
        for k in ("lossp", "dv"):
            tol, er, sc = W.tolerance("loss_grad", ref[k], rest[k]), DE.err(ref[k], g1[k]), DE.scale(ref[k])
            excess = max(excess, (er - DE.err(ref[k], rest[k])) / sc)
            R.add(f"{name} {k}", er, sc, tol)
    print(f"   excess over the restatement: {excess:.3e} of max |ref| (floor {W.FLOOR['loss_grad']:.1e})")
    assert splits >= {1, 2, 5}
    try:
        R.finish()
    finally:
        assert not bad, "\n".join(bad)

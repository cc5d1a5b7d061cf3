"""The fusion heads over their option set, on the CPU: constructors against the reference's state_dict layouts, the shapes
that must be refused, and the float64 restatement (tests/fusion_emulation.py) against the golden vectors recorded from the
reference's own classes (tests/golden/make_golden_fusion_options.py -> fusion_options.npz).

Tolerance of the restatement check: the golden is the reference in float32; the fixture also holds, per recorded quantity,
the reference's own float32-vs-float64 distance d (largest absolute difference, same weights, same inputs).  The
restatement runs in float64, so its distance to the golden must be that same d up to float64 rounding: the bound is
2 d + 1e-12 (1 + max |golden|); the factor 2 is margin for nothing but the float64 evaluation order.  The largest d and the
largest distance seen are printed.  The injected defects must each exceed the bound of at least one quantity."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fusion_emulation as FE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_options.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta_json"]))


def _module(kind, width, opts, dropout_rate=0.0):
    import multimodal_learning_amd as m
    cls = dict(bf=m.BilinearFusion, pf=m.PolynomialFusion)[kind]
    return cls(dim1=width, dim2=width, mmhid=width, dropout_rate=dropout_rate, **opts)


def _state_dict(case, seed):
    from oracle import weights as W
    return W.make_state_dict({k: tuple(s) for k, s in case["shapes"]}, seed)


def _inputs(z, width):
    return tuple(torch.as_tensor(z["in_w%d_%s" % (width, n)]) for n in ("v1", "v2", "r"))


def _distances(z, meta, case, defect=None):
    """(name, distance of the float64 restatement to the golden, bound) for every recorded quantity of the case."""
    v1, v2, r = _inputs(z, case["width"])
    res = FE.run_case(case["kind"], case["opts"], _state_dict(case, meta["weight_seed"]), v1, v2, r, defect=defect)
    q = FE.quantities(res, meta["sample_above"], meta["sample_n"])
    rows = []
    for k, d in case["ref_f32_vs_f64"].items():
        g = z[case["tag"] + "|" + k].astype(np.float64)
        dist = float(np.abs(q[k].double().numpy().reshape(g.shape) - g).max())
        rows.append((k, dist, 2.0 * d + 1e-12 * (1.0 + float(np.abs(g).max()))))
    none = sorted(k for k, g in res["grads"].items() if g is None)
    return rows, none


def test_constructors_give_the_reference_state_dict_layout(gold):
    """Fails on a package that refuses any option value: BilinearFusion(skip=1), the reference's own default, must build."""
    z, meta = gold
    assert len(meta["cases"]) == 14
    for case in meta["cases"]:
        net = _module(case["kind"], case["width"], case["opts"])
        got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert got == case["shapes"], case["tag"]
        unused = {id(p) for p in net.unused_parameters()}
        assert sorted(k for k, p in net.named_parameters() if id(p) in unused) == sorted(case["none_grads"]), case["tag"]


def test_define_bifusion_builds_both_heads():
    import multimodal_learning_amd as m
    assert type(m.define_bifusion("pofusion", skip=1, dim1=8, dim2=8, mmhid=8)) is m.BilinearFusion
    assert type(m.define_bifusion("polynomial_fusion", skip=1, dim1=8, dim2=8, mmhid=8)) is m.PolynomialFusion
    with pytest.raises(NotImplementedError):
        m.define_bifusion("concat")
    assert "PolynomialFusion" in m.__all__


def test_shapes_the_reference_cannot_run_are_refused_at_construction(gold):
    z, meta = gold
    assert len(meta["refused"]) == 2
    for ref in meta["refused"]:
        assert ref["exc_type"] == "RuntimeError"
        with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
            _module(ref["kind"], ref["width"], ref["opts"])
    # the other side, and the polynomial head with a gate off and a scale
    with pytest.raises(RuntimeError, match="gate2"):
        _module("bf", 128, dict(skip=0, use_bilinear=1, gate1=1, gate2=0, scale_dim1=1, scale_dim2=2))
    with pytest.raises(RuntimeError, match="encoder2"):
        _module("pf", 64, dict(skip=0, use_bilinear=1, gate1=1, gate2=1, scale_dim1=1, scale_dim2=2))


def test_validate_opt_admits_both_heads_and_refuses_concat():
    import multimodal_learning_amd as m
    from multimodal_learning_amd.train_step import _validate_opt
    _validate_opt(m.stage2_opt(fusion_type="pofusion"), "test")
    _validate_opt(m.stage2_opt(fusion_type="polynomial_fusion"), "test")
    with pytest.raises(NotImplementedError):
        _validate_opt(m.stage2_opt(fusion_type="concat"), "test")


def test_float64_restatement_meets_every_golden(gold):
    z, meta = gold
    worst_d, worst = 0.0, (0.0, "")
    bad = []
    for case in meta["cases"]:
        rows, none = _distances(z, meta, case)
        assert none == sorted(case["none_grads"]), case["tag"]
        assert len(rows) >= 4 + 10
        for k, dist, bound in rows:
            worst_d = max(worst_d, case["ref_f32_vs_f64"][k])
            if dist / bound > worst[0]:
                worst = (dist / bound, case["tag"] + "|" + k)
            if not dist <= bound:
                bad.append("%s|%s: distance %.3e, bound %.3e" % (case["tag"], k, dist, bound))
    print("largest float32-vs-float64 distance of the reference %.3e; largest distance / bound %.3f at %s"
          % (worst_d, worst[0], worst[1]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("defect,tag", [("skip_order", "bf_1111_1x1_w128"), ("no_one", "bf_1111_2x4_w64"),
                                        ("gate_off_gated", "bf_0101_1x1_w128"), ("z_v1_only", "bf_1011_1x1_w128"),
                                        ("kron2_no_one", "pf_0111_1x1_w128")])
def test_injected_defects_fail(gold, defect, tag):
    z, meta = gold
    case = next(c for c in meta["cases"] if c["tag"] == tag)
    rows, _ = _distances(z, meta, case, defect=defect)
    ratio, k = max((dist / bound, k) for k, dist, bound in rows)
    print("%s on %s: largest distance / bound %.3e at %s" % (defect, tag, ratio, k))
    assert ratio > 10.0

"""CPU self-test of tests/crd_width_emulation.py.

  no drift     at D = 128 every function returns what tests/crd_emulation.py returns, bit for bit, on that module's own suite
               inputs, float64 reference and float32 restatement alike.
  accepts      at D = 64 and 256 the float32 restatement is inside its own tolerance by construction (4 x its error): asserted so
               that a restatement returning NaN or another shape is caught here.
  wrong group  a 32-lane reduction at D = 64 (two rows mixed) and at D = 256 (half a row dropped) misses the tolerance of
               ph_crd_score by the printed factor on every case of the GPU sweep.  Smallest factors of this file's run:
               D = 64: 1.9e5 (PK = 1, B = 1, where no neighbouring column exists and only the doubled |v|^2 shows, in diff),
               D = 256: 1.3e6 (PK = 5, B = 1).
  gk_rows      the restatement against float64 within 1e-5 on the three widths (a column sum of at most 5 cosines)."""
import numpy as np
import pytest

from tests import crd_emulation as E
from tests import crd_width_emulation as W

F32, F64 = np.float32, np.float64


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("op", ["score", "loss_grad", "update", "outputs_bwd"])
def test_width_128_is_crd_emulation_bit_for_bit(op):
    fn = {"score": W.score, "loss_grad": W.loss_grad, "update": W.update, "outputs_bwd": W.outputs_bwd}[op]
    entries = E.suite(op)
    if op == "loss_grad":      # (the long lists take minutes in numpy: both split edges, one list per split count below them)
        entries = [e for e in entries if e["inp"]["xs"].shape[1] <= 1537]
    assert entries
    for e in entries:
        for dt, key in ((F64, "ref"), (F32, "rest")):
            got = fn(e["inp"], dt, 128)
            for k, a in e[key].items():
                assert _bits(got[k], a), (op, e["name"], key, k)


def test_width_128_inputs_and_exact_class():
    assert _bits(W.banks(128)[0], E.banks()[0]) and _bits(W.banks(128)[1], E.banks()[1])
    for a, b in zip(W.class_inputs(128), E.class_inputs()):
        assert _bits(a, b)
    bank, members, offsets = E.class_inputs()
    assert _bits(W.class_centers(bank, members, offsets), E.class_centers(bank, members, offsets))
    c = E.LG_CASES[6]
    for k, v in E.lg_inputs(c).items():
        w = W.lg_inputs(c, 128)[k]
        assert (v is None and w is None) or (_bits(v, w) if isinstance(v, np.ndarray) else v == w), k
    i, j = E.update_inputs(E.UPDATE_CASES[4]), W.update_inputs(E.UPDATE_CASES[4]["B"], E.UPDATE_CASES[4]["mom"], 128)
    assert all(_bits(i[k], j[k]) for k in i)


SCORE_CASES = [(PK, B) for PK in (1, 5, 63, 65, 130) for B in (1, 5)]


@pytest.mark.parametrize("D", W.NEW_WIDTHS)
def test_wrong_group_width_misses_by_a_large_factor(D):
    smallest = np.inf
    for n, (PK, B) in enumerate(SCORE_CASES):
        i = W.score_inputs(PK, B, n % 2 == 1, (0.07, 1.0)[(n // 2) % 2], D)
        ref, rest, bad = W.score(i, F64, D), W.score(i, F32, D), W.score(i, F32, D, wrong_group=True)
        worst = 0.0
        for k in ref:
            tol = W.tolerance("score", ref[k], rest[k])
            assert np.isfinite(rest[k]).all() and W.err(ref[k], rest[k]) <= tol
            worst = max(worst, W.err(ref[k], bad[k]) / tol)
        print("D %d PK %d B %d: wrong group width misses by %.3g x the tolerance" % (D, PK, B, worst))
        smallest = min(smallest, worst)
    print("D %d: smallest factor %.3g" % (D, smallest))
    assert smallest >= E.DEFECT_MARGIN


@pytest.mark.parametrize("D", W.WIDTHS)
def test_restatements_are_finite_and_close(D):
    i = W.lg_inputs(dict(S2=70, P2=6, B=2, posw=True, idx2=True, ws=False, T=0.07), D)
    u = W.update_inputs(3, 0.5, D)
    o = W.outputs_bwd_inputs(9, 2, D)
    for fn, inp in ((W.loss_grad, i), (W.update, u), (W.outputs_bwd, o)):
        ref, rest = fn(inp, F64, D), fn(inp, F32, D)
        for k in ref:
            assert rest[k].dtype == F32 and rest[k].shape == ref[k].shape and np.isfinite(rest[k]).all()
            assert W.err(ref[k], rest[k]) <= 1e-5 * W.scale(ref[k]), (fn.__name__, k)
    for ng in (3, 5):
        G = np.random.default_rng([131, ng, D]).standard_normal((ng, 6, D)).astype(F32)
        G[1, 2] = 0      # a zero-norm row: cosine 0, no NaN
        for th in (0, 1):
            ref, rest = W.gk_rows(G, F64, th, 0.05), W.gk_rows(G, F32, th, 0.05)
            assert rest.shape == (6, ng) and np.isfinite(rest).all() and W.err(ref, rest) <= 1e-5 * W.scale(ref)


def test_knn_reference_is_a_stable_sort_and_seeds_are_separated():
    for (n, B, NP) in W.KNN_CASES[:3]:
        for D in W.NEW_WIDTHS:
            i, ref, gap = W.knn_seed(n, B, NP, D)
            assert gap > W.KNN_GAP
            for (rows, sims) in ref:
                assert rows.shape == (B, NP) and (np.diff(sims, axis=1) <= 0).all()
                ties = np.diff(sims, axis=1) == 0
                assert (np.diff(rows, axis=1)[ties] > 0).all()      # equal similarities: the lower row first

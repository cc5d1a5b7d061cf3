"""CPU self-test of tests/dense_emulation.py: the tolerances of the dense sweep (tests/test_gpu_dense.py) accept the float32
restatement of every operator on every case and reject each injected defect by a factor of MARGIN (4) or more; the exact class
notices any one dropped product; the numpy u01 equals the source's formula worked with Python integers; the case tables reach
every value of every axis the sweep is meant to cross."""
import numpy as np
import pytest

from tests import dense_emulation as E

# the defects the tolerances must reject, and the operators whose restatement can be given each
DEFECTS = {"drop_k": "one dropped K element", "drop_row": "one dropped batch row in a BatchNorm sum",
           "biased": "biased instead of unbiased running variance", "no_T": "a missing 1/T factor",
           "nomax": "softmax without max subtraction (wide rows)", "mask_x": "ReLU mask taken from x instead of y",
           "scale_p": "dropout scale 1/p instead of 1/(1-p)"}


@pytest.mark.parametrize("op", E.REAL_OPS)
def test_restatement_inside_and_defects_outside_the_tolerance(op):
    worst_rest, worst_tol, ratios = 0.0, 0.0, {}
    bad = []
    for e in E.suite(op):
        for k, ref in e["ref"].items():
            tol, er, sc = E.entry_tolerance(e, k), E.err(ref, e["rest"][k]), max(E.scale(ref), 1e-300)
            worst_rest, worst_tol = max(worst_rest, er / sc), max(worst_tol, tol / sc)
            if not er <= tol:
                bad.append(f"{e['name']} {k}: restatement {er:.3e} > tol {tol:.3e}")
        for d, outs in e["defects"].items():
            # a defect must show in at least one output array of the case, beyond MARGIN x that array's tolerance
            r = max((E.err(ref, outs[k]) / E.entry_tolerance(e, k)) if E.entry_tolerance(e, k) > 0
                    else (np.inf if E.err(ref, outs[k]) > 0 else 0.0) for k, ref in e["ref"].items())
            ratios[d] = min(ratios.get(d, np.inf), r)
            if not r >= E.MARGIN:
                bad.append(f"{e['name']}: defect {d} only {r:.2f} x the tolerance")
    print(f"\n{op:<18s} restatement {worst_rest:.2e}  tolerance {worst_tol:.2e} (of max |ref|)  smallest defect ratio: "
          + (", ".join(f"{d} {r:.3g}" for d, r in ratios.items()) or "-"))
    assert not bad, "\n".join(bad)


def test_every_listed_defect_is_injected_somewhere():
    seen = set()
    for op in E.REAL_OPS:
        for e in E.suite(op):
            seen |= set(e["defects"])
    assert seen == set(DEFECTS), seen ^ set(DEFECTS)


def test_exact_class_notices_any_dropped_product():
    """Operands of the products are non-zero integers, so leaving one product out changes the int64 result; shown product by
    product on one small case and by the operands' signs on every case of the tables."""
    A, B, _, _, _ = E.gemm_operands(5, 4, 9, "NT", 3)
    full = E.gemm_exact(A, B, None, None, E.ACT_NONE)
    for m in range(5):
        for n in range(4):
            for k in range(9):
                assert full[m, n] - A[m, k] * B[k, n] != full[m, n]
    for c in E.GEMM_CASES + E.SPLITK_CASES:
        A, B, a_s, b_s, _ = E.gemm_operands(c["M"], c["N"], c["K"], c["form"], 1)
        assert (A != 0).all() and (B != 0).all() and np.abs(A).max() <= 4 and np.abs(B).max() <= 4
        # fp32 holds every partial sum exactly: the sum of |products| stays below 2^24
        assert (np.abs(A) @ np.abs(B)).max() < 2 ** 24
    # a chunked float32 accumulation (the split-K order) of the deepest case equals the int64 product
    A, B, _, _, _ = E.gemm_operands(8, 128, 16641, "NT", 1)
    acc = np.zeros((8, 128), dtype=np.float32)
    for k0 in range(0, 16641, 160):
        acc += A[:, k0:k0 + 160].astype(np.float32) @ B[k0:k0 + 160].astype(np.float32)
    assert np.array_equal(acc.astype(np.int64), A @ B)


def _u01_int(seed, idx):
    """dense.hip u01 with Python integers (mod 2^64)."""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z = z ^ (z >> 31)
    return (z >> 40) / 16777216.0


def test_u01_matches_the_formula_in_python_integers():
    for seed in (0, 1, 0x1234567, 0xDEADBEEFCAFE, (1 << 64) - 1):
        idx = [0, 1, 2, 255, 256, (1 << 32) - 1, 1 << 32, (5 << 34) ^ 77777, (1 << 64) - 2, (1 << 64) - 1]
        got = E.u01(seed, np.array(idx, dtype=np.uint64))
        assert got.dtype == np.float32
        assert [float(g) for g in got] == [_u01_int(seed, i) for i in idx]
    # the counter of the graph-replayable form: (step << 34) ^ (offset + i)
    k = E.keep_mask(7, 77777, 4, 0.5, step=5)
    assert list(k) == [_u01_int(7, (5 << 34) ^ (77777 + i)) >= 0.5 for i in range(4)]
    # the kept fraction is 1 - p within 5 standard deviations
    for p in (0.25, 0.5):
        n = 1 << 20
        f = E.keep_mask(99, 0, n, p).mean()
        assert abs(f - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5


def test_tables_reach_every_axis_value_with_every_kernel():
    for kern, Ms, Ks in (("sgemm16", (1, 15, 16, 17, 33), (1, 127, 128, 129, 257)), ("sgemm64", (65, 130), (1, 31, 32, 33, 65))):
        rows = [c for c in E.GEMM_CASES if E.gemm_kernel(c["M"], c["N"]) == kern]
        assert {c["M"] for c in rows} >= set(Ms) and {c["K"] for c in rows} >= set(Ks)
        for key, vals in (("form", E.FORMS), ("bias", (0, 1)), ("acc", (0, 1)), ("pad", (0, 3)), ("act", (0, 1))):
            assert {c[key] for c in rows} == set(vals), (kern, key)
        for K in Ks:                                  # every K remainder through both loader mappings
            assert {c["form"] for c in rows if c["K"] == K} >= {"NT", "GEN"} or kern == "sgemm64", (kern, K)
    assert {(c["M"], c["N"]) for c in E.GEMM_CASES} >= {(128, 128), (129, 128)}
    assert E.gemm_kernel(128, 128) == "sgemm16" and E.gemm_kernel(129, 128) == "sgemm64"
    assert 50 <= len(E.GEMM_CASES) <= 70
    sk = E.SPLITK_CASES
    assert {c["nsplit"] for c in sk} == {1, 3, 4, 5, 32, 128} and {c["form"] for c in sk} == {"NT", "NN"}
    assert {(c["M"], c["N"]) for c in sk} == {(1, 1), (8, 128), (65, 63)} and {c["K"] for c in sk} == {33, 100, 4097, 16641}
    assert any(E.splitk_slabs(c["K"], c["nsplit"]) < c["nsplit"] for c in sk)        # the entry lowers nsplit
    assert E.splitk_slabs(33, 128) == 2 and E.splitk_slabs(16641, 128) == 105 and E.splitk_slabs(100, 3) == 2
    bn = E.BN_CASES
    assert {c["B"] for c in bn} == {1, 2, 15, 16, 17, 33} and {c["C"] for c in bn} == {1, 15, 16, 17, 130}
    for key in ("relu", "running", "dparams"):
        assert {bool(c[key]) for c in bn} == {False, True}
    rc = E.ROW_CASES
    assert {c["B"] for c in rc} == {1, 63, 64, 65, 130} and {c["C"] for c in rc} == {2, 3, 64} and {c["T"] for c in rc} == {1.0, 4.0}

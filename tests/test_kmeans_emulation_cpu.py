"""CPU self-test of tests/kmeans_emulation.py, the yardstick of tests/test_gpu_kmeans.py: on every case the float32 restatement
takes the float64 reference's decisions and its centres sit within float32 rounding of the reference's; every injected defect
changes at least one label or centre element of every case it applies to; and the real-valued cases rest on decisions that are
16 x clear of the restatement's distance error (seeds searched on the CPU, kmeans_emulation.REAL_SEEDS)."""
import numpy as np
import pytest

from tests import kmeans_emulation as E

U = 2.0 ** -24
_CACHE = {}


def _runs(kind, k, T):
    key = (kind, k, T)
    if key not in _CACHE:
        case = {"exact": E.exact_inputs, "real": E.real_inputs}[kind](k) if kind != "fixed" else E.fixed_point_inputs()
        _CACHE[key] = (case, E.kmeans_pair(case, T, False), E.kmeans_pair(case, T, True))
    return _CACHE[key]


CASES = [("exact", k, 1) for k in E.EXACT_K] + [("real", k, T) for k in E.REAL_K for T in E.REAL_ITERS] + [("fixed", 3, 8)]


@pytest.mark.parametrize("kind,k,T", CASES)
def test_restatement_takes_the_reference_decisions(kind, k, T):
    case, ref, rest = _runs(kind, k, T)
    assert np.array_equal(rest["labels"], ref["labels"]) and np.array_equal(rest["counts"], ref["counts"])
    assert ref["counts"].sum() == 2 * case["offsets"][-1]
    if kind == "exact":
        assert np.array_equal(rest["centres"], ref["centres"].astype(E.F32))
    else:
        # 31 + 7 float32 additions in front of the double combination, one rounding of the mean: 40 u max |x| bounds it
        bound = 40 * U * max(np.abs(case["bank1"]).max(), np.abs(case["bank2"]).max())
        assert np.abs(rest["centres"] - ref["centres"]).max() <= bound


def test_exact_case_holds_what_it_is_built_for():
    for k in E.EXACT_K:
        case, ref, _ = _runs("exact", k, 1)
        sizes = case["sizes"]
        assert sizes[7] == k - 1 and sizes[8] == 0 and case["max_rows"] == 513
        cnt = ref["counts"]
        assert (cnt[:, 6, 0] == 40).all() and not cnt[:, 6, 1:].any()          # identical rows: every other cluster empty
        assert not ref["centres"][:, 7, k - 1].any() and not ref["centres"][:, 8].any()      # centres j >= class size: zero rows
        assert (cnt[:, 7].sum(1) == k - 1).all() and not cnt[:, 7, k - 1].any() and not cnt[:, 8].any()
        for b in ("bank1", "bank2"):
            assert np.array_equal(case[b], np.round(case[b])) and len(np.unique(case[b], axis=0)) <= 40
        # ties: some member is equally near to its two nearest centres, some pick has an equal runner-up
        tied_a = tied_p = False
        for tr in ref["trace"][0]:
            for d in tr["dist"]:
                if d.shape[1] > 1:
                    s = np.sort(d, 1); tied_a |= bool((s[:, 0] == s[:, 1]).any())
            for mind in tr["mind"]:
                s = np.sort(mind); tied_p |= len(s) > 1 and s[-1] == s[-2]
        assert tied_a and tied_p


def _applies(defect, kind, k, T):
    if defect in ("tie_high_centre", "tie_high_pos", "empty_zeroed", "expansion"):
        return kind == "exact"
    if defect == "one_iter_less":
        return kind == "real" and T == 5
    return kind != "fixed"


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_every_defect_shows(defect):
    hit = 0
    for kind, k, T in CASES:
        if not _applies(defect, kind, k, T):
            continue
        case, ref, rest = _runs(kind, k, T)
        if defect == "one_iter_less":
            full = [E.stable_from(tr) for b in range(2) for tr in E.kmeans_pair(case, max(E.REAL_ITERS), False)["trace"][b]]
            assert any(s is None or s > T for s in full), "the case has converged by then"
        bad = E.kmeans_pair(case, T, True, defect)
        changed = int((bad["labels"] != rest["labels"]).sum()) + int((bad["centres"] != rest["centres"]).sum())
        print(f"{defect:<20s} {kind} k={k} T={T}: {changed} elements change")
        assert changed >= 1, (defect, kind, k, T)
        hit += 1
    assert hit >= 3


@pytest.mark.parametrize("k", E.REAL_K)
def test_real_cases_decide_clear_of_the_float32_error(k):
    ratio, ref, rest = E.real_margin(E.real_inputs(k))
    print(f"k={k}: smallest decision gap / largest float32 distance error = {ratio:.1f}")
    print("   float64 run stops changing at", [E.stable_from(tr) for b in range(2) for tr in ref["trace"][b]])
    assert ratio >= 16.0


def test_fixed_point_case_converges_by_iteration_6():
    case, ref, rest = _runs("fixed", 3, 8)
    st = [E.stable_from(tr) for b in range(2) for tr in ref["trace"][b]]
    print("fixed-point case: the float64 run stops changing at", st)
    assert all(s is not None and s <= 6 for s in st)
    more = E.kmeans_pair(case, 16, True)
    for key in ("centres", "labels", "counts"):
        assert np.array_equal(more[key].view(np.int32), rest[key].view(np.int32))


def test_planted_bank_is_recovered():
    """The recipe of the reference golden: the algorithm finds the planted blobs (centres equal to the blobs' means up to order)."""
    for P in E.GOLDEN["nce_p"]:
        k = P - 1
        b1, b2, labels, blobs = E.planted_bank(E.GOLDEN["seed"], E.GOLDEN["n_data"], k)
        members, offsets = E.class_lists(labels)
        for b, bank in enumerate((b1, b2)):
            r = E.kmeans(bank, members, offsets, k, 16, True)
            for c in range(3):
                rows = members[offsets[c]:offsets[c + 1]]
                lab = r["labels"][offsets[c]:offsets[c + 1]]
                pairs = set(zip(lab.tolist(), blobs[b, rows].tolist()))
                assert len(pairs) == k and len({p[0] for p in pairs}) == k, (P, b, c, pairs)

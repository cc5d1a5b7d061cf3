"""Records numpy's and scipy's answers for the survival strata into tests/golden/survstrata_scipy.npz, so that the GPU
tests need no scipy:  python tests/golden/make_golden_survstrata.py  (scipy >= 1.11).

Per case `name` (inputs from tests/survstrata_emulation.case): hazard, survtime, event float32 [N], q float64 [K];
cuts = np.percentile(hazard.astype(float64), q) with the reference's patch; group = the first cut above; pvalues [K] =
scipy.stats.logrank of the adjacent strata on CensoredData.right_censored; times = the distinct times; survival [M, K + 1] =
scipy.stats.ecdf(stratum).sf evaluated at `times`, NaN where the stratum is empty."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = (("continuous", 1000, (33, 66)), ("tied_times", 999, (33, 66)), ("tied_hazards", 600, (25, 50, 75)),
         ("continuous", 257, (50,)), ("tied_times", 120, (26, 51, 76)))


def scipy_answers(hazard, survtime, event, q):
    from scipy import stats
    cuts = np.percentile(hazard.astype(np.float64), q)
    if len(cuts) == 2 and cuts[0] == cuts[1]:
        cuts[0] = 2.99997
    h64 = hazard.astype(np.float64)
    group = np.array([next((i for i, c in enumerate(cuts) if h < c), len(cuts)) for h in h64], dtype=np.int32)
    t64, ev = survtime.astype(np.float64), event > 0
    samples = [stats.CensoredData.right_censored(t64[group == g], ~ev[group == g]) for g in range(len(cuts) + 1)]
    pvalues = np.array([stats.logrank(samples[g], samples[g + 1]).pvalue for g in range(len(cuts))], dtype=np.float64)
    times = np.unique(survtime)
    survival = np.full((times.shape[0], len(cuts) + 1), np.nan)
    for g, s in enumerate(samples):
        if (group == g).any():
            survival[:, g] = stats.ecdf(s).sf.evaluate(times.astype(np.float64))
    return cuts, group, pvalues, times, survival


def main():
    from tests import survstrata_emulation as E
    out = {}
    for k, (kind, N, q) in enumerate(CASES):
        hazard, survtime, event = E.case(kind, N, seed=100 + k)
        cuts, group, pvalues, times, survival = scipy_answers(hazard, survtime, event, q)
        name = "c%d" % k
        for key, v in (("hazard", hazard), ("survtime", survtime), ("event", event), ("q", np.asarray(q, dtype=np.float64)),
                       ("cuts", cuts), ("group", group), ("pvalues", pvalues), ("times", times), ("survival", survival)):
            out["%s_%s" % (name, key)] = v
    np.savez_compressed(os.path.join(HERE, "survstrata_scipy.npz"), **out)
    print("wrote", len(CASES), "cases")


if __name__ == "__main__":
    main()

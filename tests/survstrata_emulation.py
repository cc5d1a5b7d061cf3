"""Numpy restatements of ph_surv_strata, ph_surv_table and ph_surv_logrank_km (csrc/survstrata.hip) and
of the host arithmetic behind evaluate.survival_strata_device.

The integer stages are restated by sorting (the kernels count all pairs instead; integers do not depend on the way they are
counted).  The float64 stages are restated in the kernels' own order: the (O - E, V) sums as a tree over each tile of 256
slots, then tile t, t + 256, .. per thread and the same tree; the Kaplan-Meier products as the product of the tiles before,
then the slots of the tile in order.  `defect=` injects one wrong rule at a time; tests/test_survstrata_emulation_cpu.py shows
that each is caught by an independent oracle (numpy's percentile, scipy's logrank and ecdf, utils.cox_log_rank)."""
import math

import numpy as np

OK, EINVAL = 0, -22
TILE = 256
MAX_BLOCKS = 1024                         # SURV_MAX_BLOCKS: N = 262 145 is the first size at which a grid-stride loop wraps
MAX_N, MAX_K, MAX_G, MAX_P = 1 << 20, 7, 8, 28
PATCH = 2.99997
DEFECTS = ("le_group", "count_cuts", "cut_f32", "one_lerp", "gt_at_risk", "cens_as_obs", "var_n", "pooled_n", "split_ties",
           "drop_censor_only")


# ------------------------------------------------------------------------------------------------ ph_surv_strata
def percentile_cuts(hazard, q, defect=None):
    """cuts float64 [K] before the patch: numpy's percentile, method "linear", of the float64 hazards by stable rank."""
    hazard = np.asarray(hazard, dtype=np.float32).reshape(-1)
    N = hazard.shape[0]
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    cuts = np.full(q.shape[0], np.nan, dtype=np.float64)
    if np.isnan(hazard).any():
        return cuts
    vals = hazard[np.argsort(hazard, kind="stable")].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(q.shape[0]):
            frac = np.float64(q[k]) / np.float64(100.0)
            h = np.float64(N - 1) * frac
            fl = np.floor(h)
            lo = min(max(int(fl), 0), N - 1)
            hi = min(lo + 1, N - 1)
            t = h - fl
            a, b = vals[lo], vals[hi]
            if t == 0.0 or a == b:
                c = a
            elif t < 0.5 or defect == "one_lerp":
                prod = (b - a) * t
                c = a + prod
            else:
                prod = (b - a) * (np.float64(1.0) - t)
                c = b - prod
            cuts[k] = np.float64(np.float32(c)) if defect == "cut_f32" else c
    return cuts


def strata_ref(hazard, q, defect=None):
    """(cuts float64 [K], group int32 [N], sizes int32 [K + 1], bad) of ph_surv_strata."""
    hazard = np.asarray(hazard, dtype=np.float32).reshape(-1)
    cuts = percentile_cuts(hazard, q, defect)
    K = cuts.shape[0]
    if K == 2 and cuts[0] == cuts[1]:
        cuts[0] = PATCH
    h64 = hazard.astype(np.float64)
    with np.errstate(invalid="ignore"):
        below = (h64[:, None] <= cuts[None, :]) if defect == "le_group" else (h64[:, None] < cuts[None, :])
    if defect == "count_cuts":
        group = (K - below.sum(axis=1)).astype(np.int32)
    else:
        group = np.where(below.any(axis=1), below.argmax(axis=1), K).astype(np.int32)
    sizes = np.bincount(group, minlength=K + 1).astype(np.int32)
    return cuts, group, sizes, int((~np.isfinite(hazard)).sum())


# ------------------------------------------------------------------------------------------------ ph_surv_table
def table_ref(survtime, event, group, G, defect=None):
    """(times f32 [M], at_risk, observed, censored int32 [M, G], npoints int32 [2]) of ph_surv_table."""
    t = np.asarray(survtime, dtype=np.float32).reshape(-1)
    e = np.asarray(event, dtype=np.float32).reshape(-1)
    g = np.asarray(group).reshape(-1).astype(np.int64)
    ok = (g >= 0) & (g < G) & ~np.isnan(t)
    left_out = int((~ok).sum())
    tt, gg = t[ok], g[ok]
    ev = e[ok] > 0
    if defect == "split_ties":
        order = np.argsort(tt, kind="stable")
        times = tt[order]
        slot = np.empty(tt.shape[0], dtype=np.int64)
        slot[order] = np.arange(tt.shape[0])
    else:
        _, first = np.unique(tt, return_index=True)
        times = tt[first]                              # the bits of the FIRST row that holds the time
        slot = np.searchsorted(times, tt)
    M = times.shape[0]
    observed, censored = np.zeros((M, G), dtype=np.int32), np.zeros((M, G), dtype=np.int32)
    if defect == "cens_as_obs":
        np.add.at(observed, (slot, gg), 1)
    else:
        np.add.at(observed, (slot[ev], gg[ev]), 1)
        np.add.at(censored, (slot[~ev], gg[~ev]), 1)
    at_risk = np.zeros((M, G), dtype=np.int32)
    for c in range(G):
        sg = np.sort(tt[gg == c])
        at_risk[:, c] = sg.shape[0] - np.searchsorted(sg, times, side="right" if defect == "gt_at_risk" else "left")
    if defect == "drop_censor_only":
        keep = observed.sum(axis=1) > 0
        times, at_risk, observed, censored = times[keep], at_risk[keep], observed[keep], censored[keep]
    return times, at_risk, observed, censored, np.array([times.shape[0], left_out], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ ph_surv_logrank_km
def logrank_terms(at_risk, observed, pairs, defect=None):
    """The per-slot terms of (O - E, V) for every pair: two float64 [P, M] arrays, evaluated as utils.cox_log_rank writes them."""
    at_risk, observed = np.asarray(at_risk), np.asarray(observed)
    M = at_risk.shape[0]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    oe, var = np.zeros((pairs.shape[0], M)), np.zeros((pairs.shape[0], M))
    for p, (a, b) in enumerate(pairs):
        na, nb = at_risk[:, a].astype(np.float64), at_risk[:, b].astype(np.float64)
        da, db = observed[:, a].astype(np.float64), observed[:, b].astype(np.float64)
        n, d = na + nb, da + db
        if defect == "pooled_n":
            n = at_risk.sum(axis=1).astype(np.float64)
        has = d > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            oe[p] = np.where(has, da - d * na / n, 0.0)
            den = n * n * n if defect == "var_n" else n * n * (n - 1.0)
            var[p] = np.where(has & (n > 1.0), na * (n - na) * d * (n - d) / den, 0.0)
    return oe, var


def _tile_tree(x):
    """x [.., L] -> [.., tiles]: the fixed tree (red[t] += red[t + o], o = 128 .. 1) over each tile of 256, zero padded."""
    L = x.shape[-1]
    tiles = -(-L // TILE)
    red = np.zeros(x.shape[:-1] + (tiles * TILE,), dtype=np.float64)
    red[..., :L] = x
    red = red.reshape(x.shape[:-1] + (tiles, TILE))
    o = TILE // 2
    while o > 0:
        red[..., :o] = red[..., :o] + red[..., o:2 * o]
        o //= 2
    return red[..., 0]


def kernel_order_sum(x):
    """x [.., M] -> [..]: the sum in the order of surv_terms_kernel and surv_finish_kernel."""
    part = _tile_tree(np.asarray(x, dtype=np.float64))                 # [.., tiles]
    tiles = part.shape[-1]
    rows = -(-tiles // TILE) if tiles else 0
    padded = np.zeros(part.shape[:-1] + (max(rows, 1) * TILE,), dtype=np.float64)
    padded[..., :tiles] = part
    padded = padded.reshape(part.shape[:-1] + (max(rows, 1), TILE))
    v = np.zeros(part.shape[:-1] + (TILE,), dtype=np.float64)
    for r in range(max(rows, 1)):
        v = v + padded[..., r, :]
    return _tile_tree(v)[..., 0]


def km_factors(at_risk, observed):
    n, d = np.asarray(at_risk).astype(np.float64), np.asarray(observed).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, 1.0 - d / n, 1.0)


def km_ref(at_risk, observed):
    """surv float64 [M, G] in the order of the kernels: the product of the tiles before, then the slots of the tile in order."""
    f = km_factors(at_risk, observed)
    M, G = f.shape
    surv = np.empty((M, G), dtype=np.float64)
    pre = np.ones(G, dtype=np.float64)
    for lo in range(0, M, TILE):
        blk = f[lo:lo + TILE]
        surv[lo:lo + TILE] = np.cumprod(np.concatenate([pre[None, :], blk]), axis=0)[1:]
        pre = pre * np.cumprod(blk, axis=0)[-1]
    return surv


def logrank_km_ref(at_risk, observed, pairs, defect=None):
    """(stat float64 [P, 2], surv float64 [M, G]) of ph_surv_logrank_km."""
    oe, var = logrank_terms(at_risk, observed, pairs, defect)
    stat = np.stack([kernel_order_sum(oe), kernel_order_sum(var)], axis=1) if oe.shape[0] else np.zeros((0, 2))
    return stat, km_ref(at_risk, observed)


def pvalue(o_minus_e, var):
    if not var > 0.0:
        return float("nan")
    return math.erfc(math.sqrt(o_minus_e * o_minus_e / var / 2.0))


def chain_ref(hazard, survtime, event, q=(33, 66), group=None, G=None, defect=None):
    """The dict of evaluate.survival_strata_device from the restatements."""
    if group is None:
        cuts, grp, sizes, bad = strata_ref(hazard, q, defect)
        G = cuts.shape[0] + 1
    else:
        grp = np.asarray(group).reshape(-1).astype(np.int32)
        cuts, bad = np.zeros(0), 0
        sizes = np.bincount(grp[(grp >= 0) & (grp < G)], minlength=G)
    times, at_risk, observed, censored, npoints = table_ref(survtime, event, grp, G, defect)
    pairs = [(g, g + 1) for g in range(G - 1)]
    stat, surv = logrank_km_ref(at_risk, observed, pairs, defect)
    return dict(cuts=cuts, group=grp, sizes=sizes.astype(np.int64), stat=stat,
                pvalues=np.array([pvalue(float(s[0]), float(s[1])) for s in stat], dtype=np.float64), times=times,
                at_risk=at_risk, observed=observed, censored=censored, survival=surv, bad=bad + int(npoints[1]))


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("continuous", "tied_times", "tied_hazards", "equal_times", "no_event", "equal_hazards", "nan_inf")


def case(kind, N, seed=0):
    """(hazard f32 [N], survtime f32 [N], event f32 [N]).  continuous: distinct hazards and times; tied_times: integer times
    in 1 .. max(N / 3, 1); tied_hazards: hazards on a grid of 7 values, so that ties straddle every cut; equal_times: one
    time; no_event: every row censored; equal_hazards: one hazard value (with K = 2 the 2.99997 patch puts every row in
    stratum 0); nan_inf: one NaN and a +inf and a -inf hazard.  The hazard correlates with the risk, so that V > 0 and the
    strata differ."""
    r = np.random.RandomState(seed)
    hazard = r.permutation(N).astype(np.float32) / np.float32(N) - np.float32(0.5) + np.float32(0.001) * r.rand(N).astype(np.float32)
    survtime = (np.float32(40.0) * r.rand(N).astype(np.float32) * np.exp(np.float32(-0.5) * hazard)).astype(np.float32) + np.float32(0.5)
    event = (r.rand(N) < 0.7).astype(np.float32)
    if kind == "tied_times":
        survtime = r.randint(1, max(N // 3, 1) + 1, size=N).astype(np.float32)
    elif kind == "tied_hazards":
        hazard = (r.randint(0, 7, size=N).astype(np.float32) - np.float32(3.0)) * np.float32(0.25)
        survtime = np.round(survtime)
    elif kind == "equal_times":
        survtime = np.full(N, 7.0, dtype=np.float32)
    elif kind == "no_event":
        event = np.zeros(N, dtype=np.float32)
    elif kind == "equal_hazards":
        hazard = np.full(N, -0.75, dtype=np.float32)
    elif kind == "nan_inf":
        hazard[N // 2] = np.nan
        hazard[0] = np.inf
        hazard[N - 1] = -np.inf
    elif kind != "continuous":
        raise ValueError(kind)
    return hazard, survtime, event

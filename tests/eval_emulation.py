"""Numpy restatements of the three kernels of csrc/evalmetrics.hip and of the patch geometry of augment.ResidentPatchLoader
(DESIGN.md section 23).  None of the project's code runs here; tests/test_eval_emulation_cpu.py holds these to sklearn and
pandas, tests/test_gpu_evalmetrics.py holds the kernels to these.

Every function takes `defect=`: a named wrong variant of the same computation.  The CPU self-test checks that each one fails
at least one of its checks (a check no defect can fail shows nothing)."""
import numpy as np

TILE = 256          # RANK_TILE of the kernel: pairs per workgroup, j-tile length, width of the summation tree
MAX_M = 1 << 20
OK, EINVAL = 0, -22

DEFECTS = ("gt_for_ge", "ties_dropped", "no_half", "pq_swapped", "last_argmax", "mean_divisor", "max_init_zero",
           "other_group_rows", "order_ignored")


def tree_sum(v):
    """red[t] += red[t + o] for o = 128, 64, .. 1 over TILE float64 values (axis -1)."""
    v = np.array(v, dtype=np.float64)
    o = TILE // 2
    while o:
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def pairs(pred, grade):
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    lab = np.asarray(grade, dtype=np.int64).reshape(N, 1) == np.arange(C).reshape(1, C)
    return pred.reshape(-1), lab.reshape(-1)


def rank_counts_ref(pred, grade, defect=None):
    """(P, concordant, tied, bad, ap_sum) of ph_rank_counts, ap_sum in the kernel's summation order: per block of TILE pairs
    the tree over the per-pair terms (0.0 for a pair that is not positive), then per thread t the blocks t, t + TILE, .. in
    order, then the tree."""
    s, l = pairs(pred, grade)
    C = np.asarray(pred).shape[1]
    g = np.asarray(grade, dtype=np.int64).reshape(-1)
    M = s.shape[0]
    bad = int((~np.isfinite(s)).sum()) + int(((g < 0) | (g >= C)).sum())
    order = np.argsort(s, kind="stable")
    ss, ls = s[order].astype(np.float64), l[order]
    finite = ~np.isnan(ss)
    # counts by rank over the sorted scores (NaN compares false everywhere: such pairs take no part)
    ssf, lsf = ss[finite], ls[finite]
    cum_all = np.arange(1, ssf.shape[0] + 1)
    cum_pos = np.cumsum(lsf)
    cum_neg = cum_all - cum_pos
    left = np.searchsorted(ssf, ssf, side="left")              # #{j: s_j < s_i}
    right = np.searchsorted(ssf, ssf, side="right")            # #{j: s_j <= s_i}
    n_all, n_pos = ssf.shape[0], int(lsf.sum())
    cp = np.concatenate([[0], cum_pos]); cn = np.concatenate([[0], cum_neg])
    ge_all = n_all - (right if defect == "gt_for_ge" else left)
    ge_pos = n_pos - cp[left]
    below_neg = cn[left]
    equal_neg = cn[right] - cn[left]
    pos = lsf.astype(bool)
    P = int(l.sum())
    conc = int(below_neg[pos].sum())
    tied = 0 if defect == "ties_dropped" else int(equal_neg[pos].sum())
    term_sorted = np.zeros(ss.shape[0], dtype=np.float64)
    idx = np.nonzero(finite)[0][pos]
    with np.errstate(divide="ignore", invalid="ignore"):       # (only the `gt_for_ge` defect divides by zero)
        term_sorted[idx] = ge_pos[pos].astype(np.float64) / ge_all[pos].astype(np.float64)
    term = np.zeros(M, dtype=np.float64)
    term[order] = term_sorted
    nb = -(-M // TILE)
    part = tree_sum(np.pad(term, (0, nb * TILE - M)).reshape(nb, TILE))
    k = -(-nb // TILE)
    lanes = np.pad(part, (0, k * TILE - nb)).reshape(k, TILE)
    acc = np.zeros(TILE, dtype=np.float64)
    for row in lanes:
        acc = acc + row
    return P, conc, tied, bad, float(tree_sum(acc))


def rank_metrics(P, conc, tied, ap_sum, M, defect=None):
    """(AUC, AP) from the counts."""
    Q = M - P
    if defect == "pq_swapped":
        return (conc + tied / 2.0) / (float(P) * float(Q)), ap_sum / Q
    half = 1.0 if defect == "no_half" else 2.0
    return (conc + tied / half) / (float(P) * float(Q)), ap_sum / P


def confusion_ref(pred, grade, defect=None):
    """int64 [C, C]: row = label, column = first maximum of the row; rows with a label outside [0, C) left out."""
    pred = np.asarray(pred, dtype=np.float32)
    N, C = pred.shape
    g = np.asarray(grade, dtype=np.int64).reshape(-1)
    arg = C - 1 - np.argmax(pred[:, ::-1], axis=1) if defect == "last_argmax" else np.argmax(pred, axis=1)
    conf = np.zeros((C, C), dtype=np.int64)
    keep = (g >= 0) & (g < C)
    np.add.at(conf, (g[keep], arg[keep]), 1)
    return conf


def f1_from_confusion(conf):
    """(micro F1, per-class F1) = 2 tp / (true + predicted), 0 where that is empty."""
    conf = np.asarray(conf, dtype=np.int64)
    tp = np.diag(conf).astype(np.float64)
    denom = (conf.sum(axis=1) + conf.sum(axis=0)).astype(np.float64)
    per = np.divide(2.0 * tp, denom, out=np.zeros(conf.shape[0]), where=denom > 0)
    return float(2.0 * tp.sum() / (2.0 * float(conf.sum()))), per


def csr(group_of_row, G):
    """offsets int32 [G + 1], order int32 [N]: the rows of a group ascending."""
    g = np.asarray(group_of_row, dtype=np.int64).reshape(-1)
    order = np.argsort(g, kind="stable").astype(np.int32)
    offsets = np.zeros(G + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(g, minlength=G))
    return offsets, order


def group_agg_ref(x, offsets, order, fun, defect=None):
    """f32 [G, C].  mean: float64 running sum over the group's rows in CSR order, one division, one rounding to float32.
    max: exact, from -inf."""
    x = np.asarray(x, dtype=np.float32)
    G = len(offsets) - 1
    out = np.empty((G, x.shape[1]), dtype=np.float32)
    for g in range(G):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        if defect == "other_group_rows":
            hi = min(hi + 1, x.shape[0])
        rows = np.arange(lo, hi) if defect == "order_ignored" else np.asarray(order[lo:hi])
        if fun == "mean":
            acc = np.zeros(x.shape[1], dtype=np.float64)
            for r in rows:
                acc = acc + x[r].astype(np.float64)
            out[g] = (acc / float(len(rows) + (1 if defect == "mean_divisor" else 0))).astype(np.float32)
        elif fun == "max":
            m = np.full(x.shape[1], 0.0 if defect == "max_init_zero" else -np.inf, dtype=np.float32)
            for r in rows:
                m = np.maximum(m, x[r])
            out[g] = m
        else:
            raise ValueError(fun)
    return out


def patch_offsets(extent, S, grid):
    """Offsets of the grid crops along one side: k * (extent - S) / (grid - 1); grid 1 = centre; a non-integer stride raises."""
    if S > extent or S < 1 or grid < 1:
        raise ValueError("crop does not fit")
    if grid == 1:
        return [(extent - S) // 2]
    if (extent - S) % (grid - 1):
        raise ValueError("non-integer stride")
    return [k * (extent - S) // (grid - 1) for k in range(grid)]


def patch_rows(n, SH, SW, S, grid):
    """[(roi, top, left)] in row order: row r = ROI r // grid^2, cell (gy, gx) = divmod(r % grid^2, grid)."""
    tops, lefts = patch_offsets(SH, S, grid), patch_offsets(SW, S, grid)
    rows = []
    for r in range(n * grid * grid):
        gy, gx = divmod(r % (grid * grid), grid)
        rows.append((r // (grid * grid), tops[gy], lefts[gx]))
    return rows


def cut(tiles_u8, roi, top, left, S):
    """f32 [3, S, S] = (u8 / 255 - 0.5) / 0.5 of the crop, in float32 arithmetic."""
    p = np.asarray(tiles_u8)[roi, top:top + S, left:left + S, :].astype(np.float32)
    return ((p / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)


def scores(kind, N, C, seed):
    """The input families of the tests: pred f32 [N, C], grade int64 [N]."""
    rng = np.random.default_rng(seed)
    grade = rng.integers(0, C, N).astype(np.int64)
    if kind == "random":
        pred = rng.standard_normal((N, C)).astype(np.float32)
    elif kind == "distinct":
        pred = (rng.permutation(N * C).astype(np.float32) - np.float32(N * C // 2)).reshape(N, C) / np.float32(8)
    elif kind == "ties":
        pred = rng.integers(0, 3, (N, C)).astype(np.float32) * np.float32(0.5) - np.float32(1)
    elif kind == "equal":
        pred = np.full((N, C), -1.25, dtype=np.float32)
    elif kind == "logprob":
        z = rng.standard_normal((N, C)) * 2
        pred = (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)
        pred = np.round(pred * 16) / np.float32(16) if seed % 2 else pred      # odd seeds: ties among the negatives too
    else:
        raise ValueError(kind)
    return pred, grade

"""numpy restatement of ph_group_quantile (csrc/evalmetrics.hip): the definition, and the stable
rank-count selection the kernels use in place of a sort.

For one (group, column) with n float32 values, s = the values ascending:
    h = (n - 1) q   (float64),  lo = floor(h),  hi = min(lo + 1, n - 1),  t = h - lo,  a = s[lo],  b = s[hi],
    out = float32(a if t == 0 or a == b else a + (b - a) t)      (float64: one product, one sum, one rounding to float32)
A NaN anywhere gives NaN.  The selection: rank_k = #{m : x_m < x_k} + #{m before k : x_m == x_k}; the element of rank lo
hands over a, the one of rank hi hands over b.

`defect=` injects one named mistake (DEFECTS); tests/test_quantile_emulation_cpu.py shows that each of them fails a check."""
import numpy as np

DEFECTS = ("hi_not_clamped", "round_for_floor", "unstable_ties", "le_for_lt", "q_as_percent", "order_ignored", "nan_not_propagated",
           "t0_reads_b")


def select(n, q, defect=None):
    """(lo, hi, t) of n values at the fraction q."""
    q = float(q) / 100.0 if defect == "q_as_percent" else float(q)
    h = float(n - 1) * q
    fl = float(np.round(h)) if defect == "round_for_floor" else float(np.floor(h))
    lo = int(fl)
    hi = lo + 1 if defect == "hi_not_clamped" else min(lo + 1, n - 1)
    return lo, hi, h - fl


def lerp(a, b, t, defect=None):
    """The float32 result from the two order statistics (float32) and t (float64)."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    with np.errstate(invalid="ignore", over="ignore"):
        if defect != "t0_reads_b" and (t == 0.0 or a == b):
            return np.float32(a)
        return np.float32(a + (b - a) * t)


def quantile_sorted(v, q, defect=None):
    """The definition, by sorting: v float32 [n] -> float32."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    if defect != "nan_not_propagated" and np.isnan(v).any():
        return np.float32(np.nan)
    s = np.sort(v)                      # (NaN last, where the defect lets them in)
    lo, hi, t = select(v.shape[0], q, defect)
    return lerp(s[lo], s[hi], t, defect)         # hi_not_clamped: IndexError at q = 1


def stable_ranks(v, defect=None):
    """rank_k = #{m : v_m < v_k} + #{m < k : v_m == v_k}, all pairs (n x n comparisons, as the kernels count them)."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    n = v.shape[0]
    col, row = v[:, None], v[None, :]            # [k, m]: row m against element k
    less = (row <= col) if defect == "le_for_lt" else (row < col)
    before = np.arange(n)[None, :] < np.arange(n)[:, None]
    ties = (row == col) if defect == "unstable_ties" else ((row == col) & before)
    return less.sum(axis=1) + ties.sum(axis=1)


def stable_ranks_by_argsort(v):
    """The same ranks from a stable argsort (for long vectors; equal to stable_ranks when no value is a NaN)."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    rank = np.empty(v.shape[0], dtype=np.int64)
    rank[np.argsort(v, kind="stable")] = np.arange(v.shape[0])
    return rank


def quantile_ranked(v, q, defect=None, ranks=None):
    """The selection the kernels make: exactly one element writes a, one writes b; nothing written stays NaN."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    isn = np.isnan(v)
    if defect != "nan_not_propagated" and isn.any():
        return np.float32(np.nan)
    rank = stable_ranks(v, defect) if ranks is None else ranks(v)
    lo, hi, t = select(v.shape[0], q, defect)
    a = b = np.float32(np.nan)
    wa, wb = np.flatnonzero((rank == lo) & ~isn), np.flatnonzero((rank == hi) & ~isn)
    if wa.size == 1:
        a = v[wa[0]]
    if wb.size == 1:
        b = v[wb[0]]
    return lerp(a, b, t, defect)


def group_quantile(x, offsets, order, q, defect=None, ranks=None):
    """x float32 [N, C] (or [N]); the rows of group g are order[offsets[g] .. offsets[g + 1]) -> float32 [G, C] (or [G])."""
    x = np.asarray(x, dtype=np.float32)
    vec = x.ndim == 1
    x2 = x.reshape(x.shape[0], -1)
    G = len(offsets) - 1
    out = np.empty((G, x2.shape[1]), dtype=np.float32)
    for g in range(G):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        rows = np.arange(lo, hi) if defect == "order_ignored" else np.asarray(order[lo:hi], dtype=np.int64)
        for c in range(x2.shape[1]):
            out[g, c] = quantile_ranked(x2[rows, c], q, defect, ranks)
    return out[:, 0] if vec else out


def csr(group_of_row, num_groups):
    """(offsets int32 [G + 1], order int32 [N]) of one dense group id per row, the rows of a group ascending."""
    g = np.asarray(group_of_row, dtype=np.int64).reshape(-1)
    order = np.argsort(g, kind="stable").astype(np.int32)
    offsets = np.zeros(num_groups + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(g, minlength=num_groups))
    return offsets, order


def values(kind, n, C, seed):
    """The value patterns of the tests, float32 [n, C]: 'neg' negative normals (log-probabilities), 'int3' three integer
    levels (many ties), 'unif' uniform in (0, 1), 'equal' one value everywhere."""
    r = np.random.RandomState(seed)
    if kind == "neg":
        return (-np.abs(r.randn(n, C)) - 1e-3).astype(np.float32)
    if kind == "int3":
        return r.randint(-1, 2, size=(n, C)).astype(np.float32) * np.float32(1.5)
    if kind == "unif":
        return r.rand(n, C).astype(np.float32)
    if kind == "equal":
        return np.full((n, C), -0.625, dtype=np.float32)
    raise ValueError(kind)

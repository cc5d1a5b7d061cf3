"""References of the CRD memory-bank entry points (csrc/crd.hip) for tests/test_gpu_crd.py, and the case tables of that sweep.

Two classes of comparison, as in tests/dense_emulation.py:

  exact   Integer or copy work, compared bit for bit: the columns and the gathered scores of ph_crd_select (numpy's stable
          argsort: descending for the positives, ascending for the negatives, lower column first, -0 == +0), ph_crd_neg_hist
          (np.bincount), the gathered rows of ph_crd_outputs, ph_crd_zsum on integer-valued inputs whose sums stay below 2^24,
          ph_crd_setz on powers of two, ph_crd_class_centers on a bank of integers in [-4, 4] (float32(float64 sum / count), an
          empty class exactly 0), and the zero rows of ph_crd_outputs_bwd under a NULL gradient.

  real    Everything with expf, logf, sqrtf or a float sum.  Each operator is one function of (inputs, dt, defect): dt = float64
          is the reference of the formulas in the header comments of crd.hip and in include/pathomic_hip.h, dt = float32 restates
          the kernel's own grouping (32-lane partial sums over 4 features per lane with the xor butterfly, the 32 half-wave
          strided column walk, the per-split partials added in split order, double accumulation where the kernel uses double,
          fmas where hipcc contracts a multiply-add).  The tolerance of an output array is 4 x the error of the float32
          restatement against the reference on the same inputs, plus FLOOR[operator] x max |ref|.

Inputs: banks and embeddings are unit-norm rows of fixed-seed generators, n_data = 257 unless the case says otherwise; T is 0.07
or 1.0; params = [K, T, Z1, Z2, 0.5, P] with Z1 != Z2 of the size ph_crd_setz would give (mean score x n_data), so swapped Z's
are visible; index lists contain row 0 and row n_data - 1 wherever they have two elements; y holds distinct rows (the
reference's index_copy_ is undefined on duplicates as well).

tests/test_crd_emulation_cpu.py shows that the tolerances accept the restatement on every case and that each of a list of
injected defects misses by a printed factor of at least 100."""
import functools

import numpy as np

from tests.dense_emulation import _fma, err, scale      # noqa: F401  (err / scale are used by the tests through this module)

F32, F64 = np.float32, np.float64
D = 128
MARGIN = 4.0
DEFECT_MARGIN = 100.0
N_DATA = 257
EPS = 1e-7
HIST_BINS, SCAN_CHUNK, LG_SPLIT_MAX, CC_ROWS = 32768, 2048, 8, 256

# Relative floor per operator for the device's own expf / logf, in units of max |ref|: 4 x the largest excess of the MI355X
# result's error over the float32 restatement's on the cases of this file (tests/test_gpu_crd.py prints them on every run and
# lists them in its docstring).  An operator without an entry never exceeded its restatement's error.
FLOOR = {}

REAL_OPS = ("score", "loss_grad", "loss_grad_pos", "scan_neg", "scan_zsum", "update", "outputs", "outputs_bwd", "contrast_loss_v2")


def tolerance(op, ref, rest):
    return MARGIN * err(ref, rest) + FLOOR.get(op, 0.0) * scale(ref)


def entry_tolerance(e, k):
    """Tolerance of output array k of suite entry e."""
    return tolerance(e["op"], e["ref"][k], e["rest"][k])


# ------------------------------------------------------------------------------------------------ inputs
def unit_rows(n, seed):
    r = np.random.default_rng(seed).standard_normal((n, D))
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def banks(n_data=N_DATA):
    return unit_rows(n_data, [11, n_data]), unit_rows(n_data, [12, n_data])


def row_lists(rng, shape, n_data):
    """int64 bank rows in [0, n_data) with row 0 first and row n_data - 1 last."""
    idx = rng.integers(0, n_data, size=shape).astype(np.int64)
    flat = idx.reshape(-1)
    flat[-1] = n_data - 1
    flat[0] = 0 if flat.size > 1 else flat[0]
    return idx


def make_params(K, T, Z1, Z2, P, mom=0.5):
    return np.array([K, T, Z1, Z2, mom, P], dtype=F32)


def _inv_t(T, dt):
    return dt(1) / dt(F32(T))


# ------------------------------------------------------------------------------------------------ lane arithmetic (float32)
def _butterfly(p, width):
    lane = np.arange(width)
    o = width // 2
    while o:
        p = p + p[..., lane ^ o]
        o //= 2
    return p[..., 0]


def _dot4(m, a):
    """sum_k m[..., k] a[..., k] over the 4 features of a lane, as the fma chain d = fma(m_k, a_k, d) from d = 0."""
    d = m[..., 0] * a[..., 0]
    for k in (1, 2, 3):
        d = _fma(m[..., k], a[..., k], d)
    return d


def _half_dot(m, a):
    """Dot products over 128 features as a 32-lane half-wave takes them (4 features per lane, xor butterfly 16..1)."""
    sh = np.broadcast_shapes(m.shape, a.shape)[:-1]
    m, a = np.broadcast_to(m, sh + (D,)), np.broadcast_to(a, sh + (D,))
    return _butterfly(_dot4(m.reshape(sh + (32, 4)), a.reshape(sh + (32, 4))), 32)


def _seq(a, axis):
    """Left-to-right float sum along `axis` starting from 0."""
    a = np.moveaxis(a, axis, 0)
    t = np.zeros(a.shape[1:], dtype=a.dtype)
    for q in range(a.shape[0]):
        t = t + a[q]
    return t


# ------------------------------------------------------------------------------------------------ ph_crd_score
def score(v1, v2, idx, idx2, mem1, mem2, T, dt, defect=None):
    """out1 = exp(mem2[idx2] . v1 / T), out2 = exp(mem1[idx] . v2 / T), diff = cos(mem1[idx], v1) - cos(mem2[idx2], v2)."""
    if idx2 is None or defect == "no_idx2":
        idx2 = idx
    invT = _inv_t(T, dt)
    m1, m2, a1, a2 = mem1[idx].astype(dt), mem2[idx2].astype(dt), v1.astype(dt)[:, None, :], v2.astype(dt)[:, None, :]
    dot = (lambda m, a: (m * a).sum(-1)) if dt is F64 else _half_dot
    n1, n2 = np.sqrt(dot(a1, a1)), np.sqrt(dot(a2, a2))
    d12, d21, d11, d22, q1, q2 = dot(m1, a2), dot(m2, a1), dot(m1, a1), dot(m2, a2), dot(m1, m1), dot(m2, m2)
    out = {"out1": np.exp(d21 * invT), "out2": np.exp(d12 * invT), "diff": d11 / (np.sqrt(q1) * n1) - d22 / (np.sqrt(q2) * n2)}
    if defect == "drop_last_col":
        for a in out.values():
            a[:, -1] = 0
    return out


# ------------------------------------------------------------------------------------------------ ph_crd_select (exact)
def select_ref(diff, out1, out2, ranks, P, K, P2, K2, select_neg, select_pos):
    """numpy's stable argsort: positives descending, negatives ascending, lower column first among equals."""
    B = diff.shape[0]
    sel = np.empty((B, P2 + K2), dtype=np.int32)
    for b in range(B):
        d = diff[b]
        if select_pos:
            order = np.argsort(-d[:P], kind="stable")
            pos = order[np.asarray(ranks) if ranks is not None else np.arange(P2)].copy()
            pos[0] = 0
        else:
            pos = np.arange(P2)
        neg = np.argsort(d[P:P + K], kind="stable")[:K2] if select_neg else np.arange(K2)
        sel[b] = np.concatenate([pos, P + neg])
    return {"sel": sel, "xs": np.take_along_axis(out1, sel.astype(np.int64), 1), "xt": np.take_along_axis(out2, sel.astype(np.int64), 1)}


def _count_rank(lst, vals, descending, reverse_ties):
    w, v = lst[None, :], vals[:, None]
    q, i = np.arange(lst.size)[None, :], np.arange(vals.size)[:, None]
    tie = (q > i) if reverse_ties else (q < i)
    return (((w > v) if descending else (w < v)) | ((w == v) & tie)).sum(1)


def select_count(diff, out1, out2, ranks, P, K, P2, K2, select_neg, select_pos, defect=None):
    """The kernel's rank by counting (slots no rank reaches stay -1).  Defects: `tie_reversed`; `shift_p3` = the sixteen-byte reads
    of the negative list taken from the address rounded down to 16 bytes when P % 4 != 0."""
    B = diff.shape[0]
    sel = np.full((B, P2 + K2), -1, dtype=np.int32)
    rev = defect == "tie_reversed"
    for b in range(B):
        d = diff[b]
        if select_pos:
            r2c = np.full(P, -1)
            r2c[_count_rank(d[:P], d[:P], True, rev)] = np.arange(P)
            pos = r2c[np.asarray(ranks) if ranks is not None else np.arange(P2)].copy()
            pos[0] = 0
        else:
            pos = np.arange(P2)
        sel[b, :P2] = pos
        if select_neg:
            lst = d[P:P + K]
            if defect == "shift_p3" and P & 3:
                K4 = K & ~3
                lst = np.concatenate([d[(P & ~3):(P & ~3) + K4], d[P + K4:P + K]])
            r = _count_rank(lst, d[P:P + K], False, rev)
        else:
            r = np.arange(K)
        for i in np.nonzero(r < K2)[0]:
            sel[b, P2 + r[i]] = P + i
    g = np.clip(sel, 0, None).astype(np.int64)
    return {"sel": sel, "xs": np.take_along_axis(out1, g, 1), "xt": np.take_along_axis(out2, g, 1)}


def _select_table():
    Ps, Ks = (1, 2, 3, 4, 5, 7, 8, 101, 1030), (1, 3, 4, 5, 37, 1025, 2051)
    pick = lambda n, c: (1, max(1, n // 2), n)[c % 3]
    out = []
    for n, P in enumerate(Ps):
        for m, (sp, sn) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
            K = Ks[(n + 2 * m) % len(Ks)]
            P2 = pick(P, n + m) if sp else P
            K2 = pick(K, n + m + 1) if sn else K
            if sn and P & 3 and K >= 4 and K2 == 1:      # (the one smallest value can survive a shifted list: K2 = 1 is met at P % 4 == 0)
                K2 = K // 2
            out.append(dict(B=1 if P * K > 100000 else 2, P=P, K=K, P2=P2, K2=K2, sp=sp, sn=sn, ranks=bool(sp and (n + m) % 2 == 0),
                            ties=False))
    # every K with a ranked negative side at both parities of P % 4
    for n, K in enumerate(Ks):
        P = (4, 5, 8, 7, 101, 3, 2)[n]
        K2 = pick(K, n + 1)
        out.append(dict(B=2, P=P, K=K, P2=pick(P, n), K2=K // 2 if (P & 3 and K >= 4 and K2 == 1) else K2, sp=1, sn=1, ranks=n % 2 == 1,
                        ties=False))
    for (P, K) in ((5, 37), (8, 37), (7, 5), (101, 1025), (4, 3)):
        for rk in (False, True):
            out.append(dict(B=2, P=P, K=K, P2=max(1, P // 2), K2=max(1, K // 2), sp=1, sn=1, ranks=rk, ties=True))
    return out


SELECT_CASES = _select_table()
SELECT_COPY_CASE = dict(B=1, P=4, K=70000, P2=4, K2=70000, sp=0, sn=0, ranks=False, ties=False)          # no LDS: any list length
SELECT_BIG_LDS_CASE = dict(B=1, P=4, K=20000, P2=2, K2=8, sp=1, sn=1, ranks=False, ties=False)           # 80 032 bytes of LDS
TIE_VALUES = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], dtype=F32)


def select_inputs(c, n):
    rng = np.random.default_rng([21, n, c["P"], c["K"]])
    B, P, K, PK = c["B"], c["P"], c["K"], c["P"] + c["K"]
    diff = TIE_VALUES[rng.integers(0, 6, size=(B, PK))] if c["ties"] else rng.standard_normal((B, PK)).astype(F32)
    # the gathered scores name their column: distinct values per (sample, column), different in the two arrays
    out1 = (1.0 + np.arange(B * PK, dtype=F64).reshape(B, PK)).astype(F32)
    out2 = (0.5 + 2.0 * np.arange(B * PK, dtype=F64).reshape(B, PK)).astype(F32)
    ranks = None
    if c["ranks"]:
        # distinct ranks with rank P - 1 in slot 1 (slot 0 is forced to column 0 whatever its rank)
        others = rng.permutation(P - 1)[:max(c["P2"] - 1, 1)] if P > 1 else np.zeros(1, dtype=np.int64)
        ranks = (np.concatenate([others[:1], [P - 1], others[1:]]) if c["P2"] > 1 else others[:1]).astype(np.int32)
        assert ranks.size == c["P2"]
    return dict(diff=diff, out1=out1, out2=out2, ranks=ranks)


# ------------------------------------------------------------------------------------------------ ph_crd_zsum / ph_crd_setz (exact)
ZSUM_N = (1, 63, 64, 1023, 1024, 1025, 5000)
SETZ_CASES = ((-1.0, 8.0), (4.0, -1.0), (-1.0, -1.0), (4.0, 8.0))       # (Z1, Z2) before the call


def zsum_inputs(n):
    rng = np.random.default_rng([31, n])
    return rng.integers(0, 9, size=n).astype(F32), rng.integers(0, 9, size=n).astype(F32)


def setz_exact(params, sums, count, n_data):
    p = params.copy()
    if p[2] < 0:
        p[2] = F32(F32(sums[0]) / F32(count)) * F32(n_data)
    if p[3] < 0:
        p[3] = F32(F32(sums[1]) / F32(count)) * F32(n_data)
    return p


# ------------------------------------------------------------------------------------------------ ph_crd_loss_grad / _pos
def lg_splits(S2, workspace=True):
    return min(max(S2 // 512, 1), LG_SPLIT_MAX) if workspace else 1


def _nce(m_neg, n_data, dt):
    mPn = dt(m_neg) / dt(F32(n_data))
    return mPn, dt(mPn + dt(F32(EPS)))


def loss_grad(i, dt, defect=None):
    """lossp[b] = -inv_bnorm (sum_p w_p (log(x1/(x1+c)) + log(x2/(x2+c))) + sum_n (log(mPn/(x1+c)) + log(mPn/(x2+c)))),
    dv1[b] = sum_j c1_j mem2[idx2[b][sel_j]], dv2[b] = sum_j c2_j mem1[idx[b][sel_j]]; x1 = xs / Z1, x2 = xt / Z2, c = m / n_data +
    eps, c_j = -(c / (x + c)) w / T inv_bnorm for a positive, (x / (x + c)) / T inv_bnorm for a negative."""
    xs, xt, sel, idx, P2, K2 = i["xs"], i["xt"], i["sel"].astype(np.int64), i["idx"], i["P2"], i["K2"]
    B, S2 = xs.shape
    idx2 = idx if (i["idx2"] is None or defect == "no_idx2") else i["idx2"]
    posw_s, posw_t = (None, None) if defect == "uniform_posw" else (i["posw_s"], i["posw_t"])
    par = i["params"]
    Z1, Z2 = (par[3], par[2]) if defect == "swap_z" else (par[2], par[3])
    invT, Z1, Z2, ib = dt(1) / dt(par[1]), dt(Z1), dt(Z2), dt(F32(i["inv_bnorm"]))
    mPn, c = _nce(K2 if defect == "mpn_k2" else i["m_neg"], i["n_data"], dt)
    w1, w2 = np.full((B, S2), dt(1) / dt(P2), dtype=dt), np.full((B, S2), dt(1) / dt(P2), dtype=dt)
    if posw_s is not None:
        w1[:, :P2], w2[:, :P2] = posw_s, posw_t
    pos = (np.arange(S2) < P2)[None, :]
    x1, x2 = xs.astype(dt) / Z1, xt.astype(dt) / Z2
    with np.errstate(divide="ignore", invalid="ignore"):
        A, Bq = np.log(x1 / (x1 + c)), np.log(x2 / (x2 + c))
        lpos = (A * w1 + Bq * w2) if dt is F64 else _fma(A, w1, Bq * w2)
        lt = np.where(pos, lpos, np.log(mPn / (x1 + c)) + np.log(mPn / (x2 + c))).astype(dt)
    c1 = np.where(pos, -(c / (x1 + c)) * invT * ib * w1, (x1 / (x1 + c)) * invT * ib).astype(dt)
    c2 = np.where(pos, -(c / (x2 + c)) * invT * ib * w2, (x2 / (x2 + c)) * invT * ib).astype(dt)
    rows, rows2 = np.take_along_axis(idx, sel, 1), np.take_along_axis(idx2, sel, 1)
    mem1, mem2 = i["mem1"], i["mem2"]
    if dt is F64:
        dv1 = np.einsum("bj,bjd->bd", c1, mem2[rows2].astype(F64))
        dv2 = np.einsum("bj,bjd->bd", c2, mem1[rows].astype(F64))
        return {"lossp": -lt.sum(1) * ib, "dv1": dv1, "dv2": dv2}
    # 32 half-waves per split walk the columns j = 32 y + hw, stepping by 32 ns; the half-waves are added in order, then the splits
    ns = i["ns"]
    j0 = (np.arange(ns)[:, None] * 32 + np.arange(32)[None, :])                      # [ns][32]
    g1, g2 = np.zeros((B, ns, 32, D), dtype=F32), np.zeros((B, ns, 32, D), dtype=F32)
    ls = np.zeros((B, ns, 32), dtype=F32)
    bb = np.arange(B)[:, None, None]
    for s in range(-(-S2 // (32 * ns))):
        j = j0 + s * 32 * ns
        ok = (j < S2)[None, :, :]
        jc = np.minimum(j, S2 - 1)[None, :, :]
        ls = np.where(ok, ls + lt[bb, jc], ls)
        g1 = np.where(ok[..., None], _fma(c1[bb, jc][..., None], mem2[rows2[bb, jc]], g1), g1)
        g2 = np.where(ok[..., None], _fma(c2[bb, jc][..., None], mem1[rows[bb, jc]], g2), g2)
    keep = ns - 1 if (defect == "drop_last_split" and ns > 1) else ns
    t1, t2, tl = _seq(g1, 2)[:, :keep], _seq(g2, 2)[:, :keep], _seq(ls, 2)[:, :keep]
    return {"lossp": -_seq(tl, 1) * ib, "dv1": _seq(t1, 1), "dv2": _seq(t2, 1)}


LG_S2 = (5, 31, 32, 33, 511, 512, 1023, 1024, 1025, 1537, 2600, 3600, 4096, 4608, 5000)     # (2600, 3600: 5 and 7 splits)


def _lg_table():
    out = []
    for n, S2 in enumerate(LG_S2):
        P2 = (1, 6, 20)[n % 3] if S2 > 6 else 1
        out.append(dict(S2=S2, P2=P2, B=(1, 3)[n % 2], posw=n % 2 == 1, idx2=(n // 2) % 2 == 1, ws=True, T=(0.07, 1.0)[(n // 2) % 2]))
    out.append(dict(S2=1537, P2=20, B=3, posw=True, idx2=True, ws=False, T=0.07))
    out.append(dict(S2=33, P2=20, B=3, posw=False, idx2=False, ws=True, T=1.0))
    out.append(dict(S2=1025, P2=6, B=1, posw=True, idx2=False, ws=True, T=0.07))
    return out


LG_CASES = _lg_table()
LG_POS_CASES = [dict(P=P, m_neg=m, B=3, posw=(n + k) % 2 == 0, idx2=k == 0, T=(0.07, 1.0)[(n + k) % 2])
                for n, P in enumerate((1, 6, 8)) for k, m in enumerate((1, 4096))]


def _posw(rng, B, P2):
    w = 0.2 + rng.random((B, P2))
    return (w / w.sum(1, keepdims=True)).astype(F32)


def lg_inputs(c, pos_only=False):
    """Scores of real embeddings against the bank rows of a permutation sample of the index list."""
    if pos_only:
        P2, K2, B, m_neg = c["P"], 0, c["B"], c["m_neg"]
        S2 = PK = P2
    else:
        S2, P2, B = c["S2"], c["P2"], c["B"]
        K2, PK, m_neg = S2 - P2, S2 + 7, S2 - P2
    rng = np.random.default_rng([41, S2, P2, B, int(pos_only), m_neg])
    mem1, mem2 = banks()
    v1, v2 = unit_rows(B, [42, S2, B]), unit_rows(B, [43, S2, B])
    idx = row_lists(rng, (B, PK), N_DATA)
    idx2 = row_lists(rng, (B, PK), N_DATA) if c["idx2"] else None
    sel = np.stack([rng.permutation(PK)[:S2] for _ in range(B)]).astype(np.int32)
    sc = score(v1, v2, idx, idx2, mem1, mem2, c["T"], F64)
    xs = np.take_along_axis(sc["out1"], sel.astype(np.int64), 1).astype(F32)
    xt = np.take_along_axis(sc["out2"], sel.astype(np.int64), 1).astype(F32)
    Z1, Z2 = xs.astype(F64).mean() * N_DATA, xt.astype(F64).mean() * N_DATA * 1.25      # (apart by a quarter at least)
    return dict(xs=xs, xt=xt, sel=sel, idx=idx, idx2=idx2, posw_s=_posw(rng, B, P2) if c["posw"] else None,
                posw_t=_posw(rng, B, P2) if c["posw"] else None, mem1=mem1, mem2=mem2,
                params=make_params(max(K2, 1), c["T"], Z1, Z2, P2), B=B, PK=PK, P2=P2, K2=K2, m_neg=m_neg, n_data=float(N_DATA),
                inv_bnorm=1.0 / B, ns=lg_splits(S2, c.get("ws", False)), ws=c.get("ws", False))


# ------------------------------------------------------------------------------------------------ ph_crd_neg_hist (exact)
def _hist_table():
    ns, Ks, c0s = (1, 100, 32767, 32768, 32769, 65541), (1, 1023, 1024, 1025, 3000), (0, 1, 7)
    out = [dict(n_data=n, K=Ks[(k + 1) % 5], col0=c0s[k % 3], B=(1, 3)[k % 2]) for k, n in enumerate(ns)]
    out += [dict(n_data=65541, K=1, col0=1, B=3), dict(n_data=32769, K=3000, col0=7, B=1), dict(n_data=100, K=1024, col0=0, B=3)]
    return out


HIST_CASES = _hist_table()


def hist_inputs(c):
    n, K, col0, B = c["n_data"], c["K"], c["col0"], c["B"]
    rng = np.random.default_rng([51, n, K, col0, B])
    stride = col0 + K + 3
    idx = rng.integers(0, n + 3, size=(B, stride)).astype(np.int64)      # rows at or above n_data are centre rows: ignored
    edges = [r for r in (n - 1, 0, HIST_BINS - 1, HIST_BINS, 2 * HIST_BINS - 1, 2 * HIST_BINS, n, n + 2) if r < n + 3]
    for k, r in enumerate(edges[:K]):          # the chunk edges and the first centre row, at the front of the window
        idx[:, col0 + k] = r
    return idx, stride


def neg_hist(idx, col0, K, n_data, defect=None):
    out = np.zeros((idx.shape[0], n_data), dtype=np.int32)
    for b in range(idx.shape[0]):
        r = idx[b, col0:col0 + K]
        out[b] = np.bincount(r[r < n_data], minlength=n_data)
    if defect == "hist_edge":                  # the last row of every chunk left to nobody
        out[:, HIST_BINS - 1::HIST_BINS] = 0
        out[:, n_data - 1] = 0
    return out


# ------------------------------------------------------------------------------------------------ ph_crd_scan_neg
def scan_neg(i, dt, defect=None):
    """loss_neg[b] = -inv_bnorm sum_r mult (log(mPn/(x1+c)) + log(mPn/(x2+c))), x = exp(S / T) / Z; S := inv_bnorm mult (x/(x+c)) / T;
    zsum_only: zsums[k] += sum_b sum_r mult exp(S_k / T).  float32: per 2048-row chunk sums in double rounded to float, the
    chunks added in double."""
    S1, S2, mult, par = i["S1"], i["S2"], i["mult"], i["params"]
    B, n = S1.shape
    Z1, Z2 = (par[3], par[2]) if defect == "swap_z" else (par[2], par[3])
    invT, Z1, Z2, ib = dt(1) / dt(par[1]), dt(Z1), dt(Z2), dt(F32(i["inv_bnorm"]))
    mPn, c = _nce(i["m_neg"], n, dt)
    live = np.ones(n, dtype=bool)
    if defect == "scan_tail":                 # the rows behind the last full 256-row stride of the last chunk
        r0 = (n - 1) // SCAN_CHUNK * SCAN_CHUNK
        live[r0 + (n - r0) // 256 * 256:] = False
    e1, e2 = np.exp(S1.astype(dt) * invT), np.exp(S2.astype(dt) * invT)
    fm = mult.astype(dt)
    chunks = [slice(r, min(r + SCAN_CHUNK, n)) for r in range(0, n, SCAN_CHUNK)]
    csum = lambda a: np.stack([(a[:, ch].astype(F64) * live[ch]).sum(1) for ch in chunks], 1).astype(dt)     # [B][chunks]
    if i["zsum_only"]:
        z = [csum(mult.astype(F64) * e.astype(F64)).astype(F64).sum() for e in (e1, e2)]
        return {"zsums": np.array([dt(i["zsums0"][k]) + dt(z[k]) for k in range(2)], dtype=dt)}
    x1, x2 = e1 / Z1, e2 / Z2
    t1, t2 = fm * np.log(mPn / (x1 + c)), fm * np.log(mPn / (x2 + c))
    loss = -((csum(t1).astype(F64) + csum(t2).astype(F64)).sum(1)).astype(dt) * ib
    k1, k2 = fm * (x1 / (x1 + c)) * invT * ib, fm * (x2 / (x2 + c)) * invT * ib
    return {"loss_neg": loss, "S1": np.where(live, k1, S1.astype(dt)), "S2": np.where(live, k2, S2.astype(dt))}


SCAN_CASES = [dict(n_data=n, B=3) for n in (1, 255, 256, 257, 2047, 2048, 2049, 4097)] + [dict(n_data=257, B=B) for B in (1, 64, 65)]


def scan_inputs(c, zsum_only, T=None):
    n, B = c["n_data"], c["B"]
    T = T if T is not None else (0.07, 1.0)[(n + B) % 2]
    rng = np.random.default_rng([61, n, B])
    mem1, mem2 = banks(n)
    v1, v2 = unit_rows(B, [62, n, B]), unit_rows(B, [63, n, B])
    S1, S2 = (v1.astype(F64) @ mem2.astype(F64).T).astype(F32), (v2.astype(F64) @ mem1.astype(F64).T).astype(F32)
    mult = rng.integers(0, 4, size=(B, n)).astype(np.int32)
    mult[:, 0], mult[:, -1] = (2, 3) if n > 1 else (3, 3)
    if n > 2:
        mult[:, 1] = 0
    m_neg = max(1, int(mult[0].sum()))
    Z1 = (mult * np.exp(S1.astype(F64) / T)).sum() / mult.sum() * n
    Z2 = (mult * np.exp(S2.astype(F64) / T)).sum() / mult.sum() * n * 1.25
    return dict(S1=S1, S2=S2, mult=mult, params=make_params(m_neg, T, Z1, Z2, 1), m_neg=m_neg, inv_bnorm=1.0 / B, zsum_only=zsum_only,
                zsums0=np.array([3.5, 0.625], dtype=F32), mem1=mem1, mem2=mem2, v1=v1, v2=v2, T=T, B=B, n_data=n)


# ------------------------------------------------------------------------------------------------ ph_crd_update
UPDATE_CASES = [dict(B=B, mom=m) for B in (1, 2, 3, 5) for m in (0.5, 0.0)]


def update_inputs(c):
    B = c["B"]
    rng = np.random.default_rng([71, B])
    y = (1 + rng.permutation(N_DATA - 2)[:B]).astype(np.int64)      # distinct rows
    y[0] = 0
    if B > 1:
        y[-1] = N_DATA - 1
    assert len(set(y.tolist())) == B
    mem1, mem2 = banks()
    return dict(mem1=mem1, mem2=mem2, v1=unit_rows(B, [72, B]), v2=unit_rows(B, [73, B]), y=y, params=make_params(16, 0.07, 300.0, 400.0, 1, c["mom"]))


def update(i, dt, defect=None):
    """mem[y[b]] = normalize(momentum mem[y[b]] + (1 - momentum) v[b]); the new rows of both banks."""
    mom = dt(i["params"][4])
    out = {}
    for k, (mem, v) in enumerate(((i["mem1"], i["v1"]), (i["mem2"], i["v2"]))):
        old, v = mem[i["y"]].astype(dt), v.astype(dt)
        if dt is F64:
            a = old * mom + v * (1 - mom)
            n = np.sqrt((a * a).sum(1))
        else:
            a = _fma(old, np.broadcast_to(mom, old.shape), v * (F32(1) - mom))
            n = np.sqrt(_butterfly(_fma(a[:, :64], a[:, :64], a[:, 64:] * a[:, 64:]), 64))
        out["rows%d" % (k + 1)] = a if defect == "no_renorm" else a / n[:, None]
    return out


# ------------------------------------------------------------------------------------------------ ph_crd_class_centers (exact)
CLASS_SIZES = (2, 255, 0, 513, 1, 256, 257)
CLASS_MAX_ROWS = (513, 1026)


def class_inputs():
    rng = np.random.default_rng([81])
    n = sum(CLASS_SIZES)
    bank = rng.integers(-4, 5, size=(n, D)).astype(F32)
    members = rng.permutation(n).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(CLASS_SIZES)]).astype(np.int32)
    return bank, members, offsets


def class_centers(bank, members, offsets, defect_rows=None):
    out = np.zeros((len(offsets) - 1, D), dtype=F32)
    for c in range(len(offsets) - 1):
        m = members[offsets[c]:offsets[c + 1]]
        if m.size:
            out[c] = (bank[m].astype(F64).sum(0) / (defect_rows or m.size)).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ ph_crd_outputs / _bwd
OUTPUTS_S2 = (1, 7, 8, 9, 17)
OUTPUTS_BWD_CASES = [dict(S2=S2, g1=g[0], g2=g[1]) for S2, g in zip((1, 7, 8, 9, 100, 100), ((1, 1), (1, 0), (0, 1), (1, 1), (1, 1), (0, 1)))]


def outputs(i, dt, defect=None):
    par = i["params"]
    Z1, Z2 = (par[3], par[2]) if defect == "swap_z" else (par[2], par[3])
    return {"out1": i["xs"].astype(dt) / dt(Z1), "out2": i["xt"].astype(dt) / dt(Z2)}


def outputs_rows(i):
    sel = i["sel"].astype(np.int64)
    idx2 = i["idx"] if i["idx2"] is None else i["idx2"]
    return i["mem1"][np.take_along_axis(i["idx"], sel, 1)], i["mem2"][np.take_along_axis(idx2, sel, 1)]


def outputs_bwd_inputs(c):
    S2, B = c["S2"], 3
    i = lg_inputs(dict(S2=S2, P2=1, B=B, posw=False, idx2=True, ws=False, T=(0.07, 1.0)[S2 % 2]))
    rng = np.random.default_rng([91, S2])
    o = outputs(i, F64)
    rows1, rows2 = outputs_rows(i)
    return dict(g1=rng.standard_normal((B, S2)).astype(F32) if c["g1"] else None,
                g2=rng.standard_normal((B, S2)).astype(F32) if c["g2"] else None, out1=o["out1"].astype(F32), out2=o["out2"].astype(F32),
                rows1=rows1, rows2=rows2, T=float(i["params"][1]), B=B, S2=S2)


def outputs_bwd(i, dt, defect=None):
    """dv1 = sum_j g1 out1 / T rows2, dv2 = sum_j g2 out2 / T rows1; float32: 8 half-waves stride the columns, added in order."""
    invT = _inv_t(i["T"], dt)
    res = {}
    for name, g, out, rows in (("dv1", i["g1"], i["out1"], i["rows2"]), ("dv2", i["g2"], i["out2"], i["rows1"])):
        B, S2 = out.shape
        c = (g.astype(dt) if g is not None else np.zeros((B, S2), dtype=dt)) * out.astype(dt) * invT
        if dt is F64:
            res[name] = np.einsum("bj,bjd->bd", c, rows.astype(F64))
            continue
        acc = np.zeros((B, 8, D), dtype=F32)
        for j in range(S2):
            acc[:, j % 8] = _fma(np.broadcast_to(c[:, j, None], (B, D)), rows[:, j], acc[:, j % 8])
        res[name] = _seq(acc, 1)
    return res


# ------------------------------------------------------------------------------------------------ ph_contrast_loss_v2
CL2_CASES = [dict(S=S, P=P) for S in (2, 255, 256, 257, 1000) for P in sorted({1, S // 2, S - 1})]


def cl2_inputs(c):
    rng = np.random.default_rng([101, c["S"], c["P"]])
    return dict(x=(np.exp(1.3 * rng.standard_normal((3, c["S"]))) / N_DATA).astype(F32), P=c["P"], n_data=float(N_DATA))


def contrast_loss_v2(i, dt, defect=None):
    """rows[b] = -(sum_p log(x/(x+c)) / P + sum_n log(mPn/(x+c))), dx = -c/(x (x+c))/P | 1/(x+c); m = S - P, c = m / n_data + eps."""
    x, P = i["x"].astype(dt), i["P"]
    S = x.shape[1]
    mPn, c = _nce(S - P, i["n_data"], dt)
    pos = (np.arange(S) < P)[None, :]
    lt = np.where(pos, np.log(x / (x + c)).astype(F64) / P, np.log(mPn / (x + c)).astype(F64))      # (the kernel sums in double)
    dx = np.where(pos, -(c / (x * (x + c))) / dt(P), dt(1) / (x + c))
    return {"rows": -(lt.sum(1).astype(dt)), "dx": dx.astype(dt)}


# ------------------------------------------------------------------------------------------------ the real-valued suite
def _entry(op, name, inp, fn, defects=()):
    return dict(op=op, name=name, inp=inp, ref=fn(inp, F64), rest=fn(inp, F32), defects={d: fn(inp, F32, d) for d in defects})


SCORE_PK = (1, 7, 8, 9, 63, 64, 65, 129, 200)


def score_inputs(PK, B, second, T):
    rng = np.random.default_rng([1, PK, B])
    mem1, mem2 = banks()
    return dict(v1=unit_rows(B, [2, PK, B]), v2=unit_rows(B, [3, PK, B]), idx=row_lists(rng, (B, PK), N_DATA),
                idx2=row_lists(rng, (B, PK), N_DATA) if second else None, mem1=mem1, mem2=mem2, T=T, B=B, PK=PK)


def _score_fn(i, dt, defect=None):
    return score(i["v1"], i["v2"], i["idx"], i["idx2"], i["mem1"], i["mem2"], i["T"], dt, defect)


@functools.lru_cache(maxsize=None)
def suite(op):
    out = []
    if op == "score":
        for n, PK in enumerate(SCORE_PK):
            for k, B in enumerate((1, 3)):
                second, T = (n + k) % 2 == 1, (0.07, 1.0)[(n // 2 + k) % 2]
                dfs = (("drop_last_col",) if PK % 64 else ()) + (("no_idx2",) if second else ())
                out.append(_entry(op, f"PK{PK} B{B} idx2 {int(second)} T{T}", score_inputs(PK, B, second, T), _score_fn, dfs))
    elif op == "loss_grad":
        for c in LG_CASES:
            i = lg_inputs(c)
            dfs = ["swap_z"] + (["drop_last_split"] if i["ns"] > 1 else []) + (["uniform_posw"] if c["posw"] and c["P2"] > 1 else []) \
                + (["no_idx2"] if c["idx2"] else [])
            out.append(_entry(op, "S2 %d P2 %d B%d posw%d idx2 %d ws%d T%g" % (c["S2"], c["P2"], c["B"], c["posw"], c["idx2"], c["ws"], c["T"]),
                              i, loss_grad, dfs))
    elif op == "loss_grad_pos":
        for c in LG_POS_CASES:
            out.append(_entry(op, "P%d m_neg %d posw%d idx2 %d T%g" % (c["P"], c["m_neg"], c["posw"], c["idx2"], c["T"]),
                              lg_inputs(c, pos_only=True), loss_grad, ("mpn_k2", "swap_z")))
    elif op in ("scan_neg", "scan_zsum"):
        for c in SCAN_CASES:
            n = c["n_data"]
            dfs = (("scan_tail",) if n % 256 else ()) + (("swap_z",) if op == "scan_neg" else ())
            out.append(_entry(op, "n_data %d B%d" % (n, c["B"]), scan_inputs(c, int(op == "scan_zsum")), scan_neg, dfs))
    elif op == "update":
        for c in UPDATE_CASES:
            out.append(_entry(op, "B%d momentum %g" % (c["B"], c["mom"]), update_inputs(c), update, ("no_renorm",) if c["mom"] else ()))
    elif op == "outputs":
        for S2 in OUTPUTS_S2:
            i = lg_inputs(dict(S2=S2, P2=1, B=3 if S2 != 8 else 1, posw=False, idx2=S2 % 2 == 1, ws=False, T=0.07))
            out.append(_entry(op, "S2 %d" % S2, i, outputs, ("swap_z",)))
    elif op == "outputs_bwd":
        for c in OUTPUTS_BWD_CASES:
            out.append(_entry(op, "S2 %d g1 %d g2 %d" % (c["S2"], c["g1"], c["g2"]), outputs_bwd_inputs(c), outputs_bwd))
    elif op == "contrast_loss_v2":
        for c in CL2_CASES:
            out.append(_entry(op, "S%d P%d" % (c["S"], c["P"]), cl2_inputs(c), contrast_loss_v2))
    else:
        raise KeyError(op)
    return out

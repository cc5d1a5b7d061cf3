"""The kernels' grouping of csrc/crd.hip and of ph_gk_rows restated with the row width D as a parameter (64, 128, 256), for
tests/test_gpu_crd_width.py; the counterpart of tests/crd_emulation.py, which is the same restatement at D = 128 alone.

A bank row is D/4 lanes of 4 features: a GROUP of 16, 32 or 64 lanes.  What changes with D:
  score        dot products as 4-feature fma chains per lane, xor butterfly from D/8 down to 1 inside the group
  loss_grad    1024 / (D/4) = 64, 32 or 16 row groups stride the columns of a split, added in group order, then the splits
  update       one wave per row, D/64 elements per lane: |a|^2 per lane as a^2 | fma(a0, a0, a1^2) | the sum of two such pairs,
               then the 64-lane butterfly
  outputs_bwd  1024 / D = 16, 8 or 4 row groups stride the columns, added in group order
  gk_rows      one wave per sample, D/64 products per lane summed as in update, the 64-lane butterfly per pair of gradients
Every function takes the input dictionaries of tests/crd_emulation.py (the width is read from D, the arrays must agree with it);
tests/test_crd_width_emulation_cpu.py shows that at D = 128 they return crd_emulation's results bit for bit on that module's own
inputs, in both dt = float64 (the reference) and dt = float32 (the restatement), so the two files cannot drift.

`wrong_group`: the defect a width-templated kernel can have - the half-wave (32-lane) reduction kept at another width.  At D = 64
a 32-lane butterfly adds the partial sums of the NEIGHBOURING 16-lane group, i.e. of the column the neighbour walks (column j ^ 4:
a group walks 4 consecutive columns; nothing is added where that column is past the list) and doubles |v|^2; at D = 256 it stops
half way and lane 0 holds features 0 .. 127 alone.  The CPU test records by what factor these miss the tolerance.

Tolerance (the project's rule): 4 x the error of the float32 restatement against float64 on the same inputs, plus
FLOOR[operator] x max |ref|.

FLOOR: 4 x the largest excess of the MI355X result's error over the float32 restatement's, in units of max |ref|, measured on the
first run of tests/test_gpu_crd_width.py (which prints them on every run): score 9.447e-08 (one ulp of expf on the one-element case
PK = 1, B = 1 at width 256, where the restatement happens to be within 9e-9), loss_grad 1.231e-08, update 9.184e-09, gk_rows
6.191e-08; outputs and outputs_bwd never exceeded their restatements.  All are below 1e-5 of max |ref| by a factor of 25 or more."""
import functools

import numpy as np

from tests import crd_emulation as E
from tests.crd_emulation import _butterfly, _dot4, _fma, _seq, err, scale      # noqa: F401

F32, F64 = np.float32, np.float64
WIDTHS = (64, 128, 256)
NEW_WIDTHS = (64, 256)
MARGIN = E.MARGIN
N_DATA = E.N_DATA

FLOOR = {"score": 3.8e-7, "loss_grad": 4.9e-8, "update": 3.7e-8, "gk_rows": 2.5e-7}


def tolerance(op, ref, rest):
    return MARGIN * err(ref, rest) + FLOOR.get(op, 0.0) * scale(ref)


# ------------------------------------------------------------------------------------------------ inputs
def unit_rows(n, seed, D):
    r = np.random.default_rng(seed).standard_normal((n, D))
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def banks(D, n_data=N_DATA):
    return unit_rows(n_data, [11, n_data], D), unit_rows(n_data, [12, n_data], D)


# ------------------------------------------------------------------------------------------------ ph_crd_score
def _group_dot(m, a, D, wrong_group=False, cols=None):
    sh = np.broadcast_shapes(m.shape, a.shape)[:-1]
    m, a = np.broadcast_to(m, sh + (D,)), np.broadcast_to(a, sh + (D,))
    G = D // 4
    lane = _dot4(m.reshape(sh + (G, 4)), a.reshape(sh + (G, 4)))
    if not wrong_group:
        return _butterfly(lane, G)
    if G == 64:                                   # the butterfly stops at 32 lanes
        return _butterfly(lane[..., :32], 32)
    assert G == 16                                # 32 lanes = this group and its neighbour (column j ^ 4 of the same walk)
    own = _butterfly(lane, 16)
    if cols is None:                              # a query norm: both groups hold the same vector
        return own + own
    PK = own.shape[-1]
    other = np.arange(PK) ^ 4
    return own + np.where(other < PK, own[..., np.minimum(other, PK - 1)], F32(0))


def score(i, dt, D, wrong_group=False):
    """crd_emulation.score at width D."""
    v1, v2, idx, idx2, mem1, mem2 = i["v1"], i["v2"], i["idx"], i["idx2"], i["mem1"], i["mem2"]
    assert mem1.shape[1] == D and v1.shape[1] == D
    idx2 = idx if idx2 is None else idx2
    invT = E._inv_t(i["T"], dt)
    m1, m2, a1, a2 = mem1[idx].astype(dt), mem2[idx2].astype(dt), v1.astype(dt)[:, None, :], v2.astype(dt)[:, None, :]
    if dt is F64:
        dot = ndot = lambda m, a: (m * a).sum(-1)
    else:
        dot = lambda m, a: _group_dot(m, a, D, wrong_group, cols=True)
        ndot = lambda m, a: _group_dot(m, a, D, wrong_group)
    n1, n2 = np.sqrt(ndot(a1, a1)), np.sqrt(ndot(a2, a2))
    d12, d21, d11, d22, q1, q2 = dot(m1, a2), dot(m2, a1), dot(m1, a1), dot(m2, a2), dot(m1, m1), dot(m2, m2)
    return {"out1": np.exp(d21 * invT), "out2": np.exp(d12 * invT), "diff": d11 / (np.sqrt(q1) * n1) - d22 / (np.sqrt(q2) * n2)}


def score_inputs(PK, B, second, T, D):
    rng = np.random.default_rng([1, PK, B])
    mem1, mem2 = banks(D)
    return dict(v1=unit_rows(B, [2, PK, B], D), v2=unit_rows(B, [3, PK, B], D), idx=E.row_lists(rng, (B, PK), N_DATA),
                idx2=E.row_lists(rng, (B, PK), N_DATA) if second else None, mem1=mem1, mem2=mem2, T=T, B=B, PK=PK)


# ------------------------------------------------------------------------------------------------ ph_crd_loss_grad
def loss_grad(i, dt, D):
    """crd_emulation.loss_grad at width D: NHW = 4096 / D row groups per split."""
    xs, xt, sel, idx, P2, K2 = i["xs"], i["xt"], i["sel"].astype(np.int64), i["idx"], i["P2"], i["K2"]
    B, S2 = xs.shape
    idx2 = idx if i["idx2"] is None else i["idx2"]
    posw_s, posw_t = i["posw_s"], i["posw_t"]
    par = i["params"]
    invT, Z1, Z2, ib = dt(1) / dt(par[1]), dt(par[2]), dt(par[3]), dt(F32(i["inv_bnorm"]))
    mPn, c = E._nce(i["m_neg"], i["n_data"], dt)
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
    assert mem1.shape[1] == D
    if dt is F64:
        dv1 = np.einsum("bj,bjd->bd", c1, mem2[rows2].astype(F64))
        dv2 = np.einsum("bj,bjd->bd", c2, mem1[rows].astype(F64))
        return {"lossp": -lt.sum(1) * ib, "dv1": dv1, "dv2": dv2}
    ns, NHW = i["ns"], 4096 // D
    j0 = (np.arange(ns)[:, None] * NHW + np.arange(NHW)[None, :])                    # [ns][NHW]
    g1, g2 = np.zeros((B, ns, NHW, D), dtype=F32), np.zeros((B, ns, NHW, D), dtype=F32)
    ls = np.zeros((B, ns, NHW), dtype=F32)
    bb = np.arange(B)[:, None, None]
    for s in range(-(-S2 // (NHW * ns))):
        j = j0 + s * NHW * ns
        ok = (j < S2)[None, :, :]
        jc = np.minimum(j, S2 - 1)[None, :, :]
        ls = np.where(ok, ls + lt[bb, jc], ls)
        g1 = np.where(ok[..., None], _fma(c1[bb, jc][..., None], mem2[rows2[bb, jc]], g1), g1)
        g2 = np.where(ok[..., None], _fma(c2[bb, jc][..., None], mem1[rows[bb, jc]], g2), g2)
    t1, t2, tl = _seq(g1, 2), _seq(g2, 2), _seq(ls, 2)
    return {"lossp": -_seq(tl, 1) * ib, "dv1": _seq(t1, 1), "dv2": _seq(t2, 1)}


def lg_inputs(c, D):
    """crd_emulation.lg_inputs at width D (the gathered form: S2 columns out of PK = S2 + 7)."""
    S2, P2, B = c["S2"], c["P2"], c["B"]
    K2, PK, m_neg = S2 - P2, S2 + 7, S2 - P2
    rng = np.random.default_rng([41, S2, P2, B, 0, m_neg])
    mem1, mem2 = banks(D)
    v1, v2 = unit_rows(B, [42, S2, B], D), unit_rows(B, [43, S2, B], D)
    idx = E.row_lists(rng, (B, PK), N_DATA)
    idx2 = E.row_lists(rng, (B, PK), N_DATA) if c["idx2"] else None
    sel = np.stack([rng.permutation(PK)[:S2] for _ in range(B)]).astype(np.int32)
    sc = score(dict(v1=v1, v2=v2, idx=idx, idx2=idx2, mem1=mem1, mem2=mem2, T=c["T"]), F64, D)
    xs = np.take_along_axis(sc["out1"], sel.astype(np.int64), 1).astype(F32)
    xt = np.take_along_axis(sc["out2"], sel.astype(np.int64), 1).astype(F32)
    Z1, Z2 = xs.astype(F64).mean() * N_DATA, xt.astype(F64).mean() * N_DATA * 1.25
    return dict(xs=xs, xt=xt, sel=sel, idx=idx, idx2=idx2, posw_s=E._posw(rng, B, P2) if c["posw"] else None,
                posw_t=E._posw(rng, B, P2) if c["posw"] else None, mem1=mem1, mem2=mem2,
                params=E.make_params(max(K2, 1), c["T"], Z1, Z2, P2), B=B, PK=PK, P2=P2, K2=K2, m_neg=m_neg, n_data=float(N_DATA),
                inv_bnorm=1.0 / B, ns=E.lg_splits(S2, c.get("ws", False)), ws=c.get("ws", False))


# ------------------------------------------------------------------------------------------------ ph_crd_update / ph_gk_rows
def _lane_pairs(x, y, D):
    """sum_e x[.., e * 64 + lane] y[.., e * 64 + lane] per lane: x0 y0 | fma(x0, y0, x1 y1) | (that of 0, 1) + (that of 2, 3)."""
    e = D // 64
    xs, ys = [x[..., k * 64:(k + 1) * 64] for k in range(e)], [y[..., k * 64:(k + 1) * 64] for k in range(e)]
    if e == 1:
        return xs[0] * ys[0]
    pair = lambda a: _fma(xs[a], ys[a], xs[a + 1] * ys[a + 1])
    return pair(0) if e == 2 else pair(0) + pair(2)


def update(i, dt, D):
    """crd_emulation.update at width D."""
    mom = dt(i["params"][4])
    out = {}
    for k, (mem, v) in enumerate(((i["mem1"], i["v1"]), (i["mem2"], i["v2"]))):
        assert mem.shape[1] == D
        old, v = mem[i["y"]].astype(dt), v.astype(dt)
        if dt is F64:
            a = old * mom + v * (1 - mom)
            n = np.sqrt((a * a).sum(1))
        else:
            a = _fma(old, np.broadcast_to(mom, old.shape), v * (F32(1) - mom))
            n = np.sqrt(_butterfly(_lane_pairs(a, a, D), 64))
        out["rows%d" % (k + 1)] = a / n[:, None]
    return out


def update_inputs(B, mom, D):
    rng = np.random.default_rng([71, B])
    y = (1 + rng.permutation(N_DATA - 2)[:B]).astype(np.int64)
    y[0] = 0
    if B > 1:
        y[-1] = N_DATA - 1
    mem1, mem2 = banks(D)
    return dict(mem1=mem1, mem2=mem2, v1=unit_rows(B, [72, B], D), v2=unit_rows(B, [73, B], D), y=y,
                params=E.make_params(16, 0.07, 300.0, 400.0, 1, mom))


def gk_rows(G, dt, use_thresh, thresh):
    """all_scale[b][j] = sum_i (cos(G[i][b], G[j][b]) > thresh) or max(cos, 0); zero-norm rows give cosine 0.  G [ng][B][D]."""
    ng, B, D = G.shape
    g = G.astype(dt)
    if dt is F64:
        gram = np.einsum("ibd,jbd->bij", g, g)
    else:
        gram = np.zeros((B, ng, ng), dtype=F32)
        for a in range(ng):
            for b in range(a, ng):
                gram[:, a, b] = gram[:, b, a] = _butterfly(_lane_pairs(g[a], g[b], D), 64)
    dg = np.sqrt(np.einsum("bii->bi", gram))
    den = dg[:, :, None] * dg[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(den > 0, gram / den, dt(0)).astype(dt)
    t = (c > dt(F32(thresh))).astype(dt) if use_thresh else np.where(c > 0, c, dt(0))
    return _seq(np.moveaxis(t, 1, 0), 0) if dt is F32 else t.sum(1)


# ------------------------------------------------------------------------------------------------ ph_crd_outputs_bwd
def outputs_bwd(i, dt, D):
    """crd_emulation.outputs_bwd at width D: 1024 / D row groups."""
    invT = E._inv_t(i["T"], dt)
    NGRP = 1024 // D
    res = {}
    for name, g, out, rows in (("dv1", i["g1"], i["out1"], i["rows2"]), ("dv2", i["g2"], i["out2"], i["rows1"])):
        B, S2 = out.shape
        assert rows.shape[2] == D
        c = (g.astype(dt) if g is not None else np.zeros((B, S2), dtype=dt)) * out.astype(dt) * invT
        if dt is F64:
            res[name] = np.einsum("bj,bjd->bd", c, rows.astype(F64))
            continue
        acc = np.zeros((B, NGRP, D), dtype=F32)
        for j in range(S2):
            acc[:, j % NGRP] = _fma(np.broadcast_to(c[:, j, None], (B, D)), rows[:, j], acc[:, j % NGRP])
        res[name] = _seq(acc, 1)
    return res


def outputs_bwd_inputs(S2, B, D):
    i = lg_inputs(dict(S2=S2, P2=1, B=B, posw=False, idx2=True, ws=False, T=(0.07, 1.0)[S2 % 2]), D)
    rng = np.random.default_rng([91, S2])
    o = E.outputs(i, F64)
    rows1, rows2 = E.outputs_rows(i)
    return dict(g1=rng.standard_normal((B, S2)).astype(F32), g2=rng.standard_normal((B, S2)).astype(F32), out1=o["out1"].astype(F32),
                out2=o["out2"].astype(F32), rows1=rows1, rows2=rows2, T=float(i["params"][1]), B=B, S2=S2)


# ------------------------------------------------------------------------------------------------ ph_crd_class_centers (exact)
def class_inputs(D):
    rng = np.random.default_rng([81])
    n = sum(E.CLASS_SIZES)
    bank = rng.integers(-4, 5, size=(n, D)).astype(F32)
    members = rng.permutation(n).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(E.CLASS_SIZES)]).astype(np.int32)
    return bank, members, offsets


def class_centers(bank, members, offsets):
    out = np.zeros((len(offsets) - 1, bank.shape[1]), dtype=F32)
    for c in range(len(offsets) - 1):
        m = members[offsets[c]:offsets[c + 1]]
        if m.size:
            out[c] = (bank[m].astype(F64).sum(0) / m.size).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ ph_crd_bank_topk
KNN_CASES = ((77, 3, 2), (33, 33, 8), (257, 65, 1), (5000, 100, 8))       # (n_data, B, num_pos)
KNN_BIG_CASE = (65536, 64, 6)
KNN_CLASSES = 3
# float32 rounding of a cosine of D Gaussian features: each of the D products and sums rounds by 2^-24 of a term of size ~1/D,
# about sqrt(D) 2^-24 / sqrt(D) ~ 1e-7 in all for the dot product and the same again for the two norms; 1e-5 is 50 x that and
# still leaves most seeds usable (the best similarities of a query are ~1e-2 apart)
KNN_GAP = 1e-5


def knn_inputs(n, B, NP, D, seed):
    """Both banks, the class of every row, the queries' own rows idx[b][0] (PK = 5 columns as in the callers) and their classes."""
    rng = np.random.default_rng([121, n, B, NP, D, seed])
    mem = [(rng.standard_normal((n, D)) * (0.5 + rng.random((n, 1)))).astype(F32) for _ in range(2)]
    labels = rng.integers(0, KNN_CLASSES, size=n).astype(np.int32)
    idx = rng.integers(0, n, size=(B, 5)).astype(np.int64)
    idx[0, 0], idx[-1, 0] = n - 1, 0
    return dict(mem1=mem[0], mem2=mem[1], labels=labels, idx=idx, batch_label=labels[idx[:, 0]].astype(np.int64))


def knn_reference(i, NP):
    """Per bank: rows [B][NP] and float64 similarities of a stable descending sort of cos(bank[idx[b][0]], bank[r]) x
    (class(r) == class of the query), and the smallest gap between unequal neighbours among the first NP + 1 of any query."""
    out, gap = [], np.inf
    for mem in (i["mem1"], i["mem2"]):
        m = mem.astype(F64)
        mn = m / np.linalg.norm(m, axis=1, keepdims=True)
        sim = mn[i["idx"][:, 0]] @ mn.T
        sim = np.where(i["labels"][None, :] == i["batch_label"][:, None], sim, 0.0)
        order = np.argsort(-sim, axis=1, kind="stable")[:, :NP + 1]
        top = np.take_along_axis(sim, order, 1)
        d = -np.diff(top, axis=1)
        if (d > 0).any():
            gap = min(gap, d[d > 0].min())
        out.append((order[:, :NP].astype(np.int64), top[:, :NP]))
    return out, gap


def knn_seed(n, B, NP, D):
    """The first seed whose float64 similarities around rank NP are apart by more than KNN_GAP for every query (or exactly equal:
    masked rows, ordered by row)."""
    for seed in range(64):
        i = knn_inputs(n, B, NP, D, seed)
        ref, gap = knn_reference(i, NP)
        if gap > KNN_GAP:
            return i, ref, gap
    raise AssertionError("no separated seed")

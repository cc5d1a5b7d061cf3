"""References of the DSCD criteria of the MIA-2022 tree (CL_utils/CRD_loss_v2.py: CRDLoss over ContrastMemory_v4, CRDLoss_v2 over
ContrastMemory_mono) and of the two entry points they add to csrc/crd.hip, for tests/test_gpu_dscd.py, tests/test_gpu_dscd_modules.py
and tests/test_dscd_emulation_cpu.py.  Scores, loss and gradient are the functions of tests/crd_width_emulation.py (dt = float64:
the reference of the formulas; dt = float32: the kernels' own grouping) - with x = w exp(s / T) / Z they hold unchanged; what is
new sits in the selection.

  exact   ph_crd_select_dscd: `select_ref` - numpy's stable argsort of the P positive keys (ascending = v4, descending = mono, the
          lower column first among equal keys, -0 == +0), P2 of them at `ranks`, slot 0 forced to column 0, then all K negatives in
          order; under neg_reweight the gathered negative scores are float32 out * (float32(1) + diff): one rounded add, one
          rounded multiply.
  real    `chain`: score -> selection -> weights -> Z (first call) -> loss and gradient, for one call on normalised embeddings;
          `loss_grad_one`: the one-directional half.  Tolerance: crd_width_emulation.tolerance - 4 x the float32 restatement's
          error against float64 on the same inputs plus that file's measured floor of the loss kernel.
  module  `criterion_calls`: the two consecutive calls of a case of tests/golden/dscd_forward.npz from f_s / f_t through the Embed
          layers (linear + L2 norm, forward and backward) and the momentum update of the banks.

The selection of `chain` is always made on the float32 discrepancies, also under dt = float64 (a float64 sort can order two keys
1e-8 apart the other way; the selection itself belongs to the exact class), everything behind it runs in dt.
`defect`: one of DEFECTS - what the kernels or the host mirror could get wrong; tests/test_dscd_emulation_cpu.py shows that each
misses the tolerance by a printed factor of at least 100."""
import numpy as np

from tests import crd_emulation as E
from tests import crd_width_emulation as W
from tests.crd_emulation import _fma, _seq, err, scale      # noqa: F401

F32, F64 = np.float32, np.float64
N_DATA = 2048          # bank rows of the chain cases: every index list (up to 100 + 1024 columns) is drawn without replacement
DEFECT_MARGIN = 100.0
TIE_KEYS = np.array([-1.5, -0.0, 0.0, 0.25, 1.0], dtype=F32)      # five values, +0 and -0 among them

DEFECTS = {
    "descending": "v4's positives ranked descending (v3's direction)",
    "weight_minus": "weight 1 - diff",
    "weight_one_side": "the weight applied to the student's direction only",
    "weight_positives": "the weight applied to the positives as well",
    "slot0_free": "slot 0 not forced to column 0",
    "tie_higher": "ties broken by the higher column",
    "m_k2": "m = K2 in the noise constant",
    "z_unweighted": "Z from the unweighted scores",
    "mono_z_v1": "mono reading Z from index 2 of its params (T there)",
    "mono_mid_v4": "mono's `mid` ranks drawn by v4's rule",
    "mono_ascending": "mono's positives ranked ascending",
}


# ------------------------------------------------------------------------------------------------ selection (exact)
def select_ref(diff, out1, out2, ranks, P, K, P2, ascending, neg_reweight, defect=None):
    """sel [B][P2 + K] int32, xs / xt the gathered (and weighted) float32 scores."""
    B = diff.shape[0]
    sel = np.empty((B, P2 + K), dtype=np.int32)
    rk = np.asarray(ranks) if ranks is not None else np.arange(P2)
    for b in range(B):
        key = diff[b, :P] + F32(0)                            # (-0 == +0 in the comparison either way)
        key = key if ascending else -key
        if defect == "tie_higher":
            order = (P - 1 - np.argsort(key[::-1], kind="stable"))
        else:
            order = np.argsort(key, kind="stable")
        pos = order[rk].copy()
        if defect != "slot0_free":
            pos[0] = 0
        sel[b] = np.concatenate([pos, P + np.arange(K)])
    g = sel.astype(np.int64)
    xs, xt = np.take_along_axis(out1, g, 1).astype(F32), np.take_along_axis(out2, g, 1).astype(F32)
    if neg_reweight:
        w = (F32(1) + np.take_along_axis(diff, g, 1).astype(F32)).astype(F32)
        xs[:, P2:] = xs[:, P2:] * w[:, P2:]
        xt[:, P2:] = xt[:, P2:] * w[:, P2:]
    return {"sel": sel, "xs": xs, "xt": xt}


def select_count(diff, P, ranks, P2, ascending):
    """The kernel's rank by counting over the negated-when-ascending keys: the positive columns alone."""
    B = diff.shape[0]
    out = np.empty((B, P2), dtype=np.int32)
    rk = np.asarray(ranks) if ranks is not None else np.arange(P2)
    for b in range(B):
        k = -diff[b, :P] if ascending else diff[b, :P]
        r2c = np.zeros(P, dtype=np.int64)
        r2c[E._count_rank(k, k, True, False)] = np.arange(P)
        out[b] = r2c[rk]
        out[b, 0] = 0
    return out


# (P, K, P2) of the device sweep: the smallest lists, both parities of P % 4, a K longer than the block, a P above the block
# (strided walk), the shipped sizes, and a list whose 2 P words pass 64 KiB of LDS
SELECT_SHAPES = ((1, 1, 1), (3, 5, 3), (4, 7, 2), (5, 1, 1), (100, 512, 20), (300, 1024, 20), (1025, 3, 64), (100, 4096, 20),
                 (8200, 1, 8))


def select_cases():
    out = []
    for n, (P, K, P2) in enumerate(SELECT_SHAPES):
        for B in (1, 3):
            for asc in (1, 0):
                for rw in (0, 1):
                    for rk in ((None, "given") if P > 1 else (None,)):
                        if P >= 1025 and (B == 3) != (asc == rw):      # (the long lists: half of the crossings)
                            continue
                        out.append(dict(P=P, K=K, P2=P2, B=B, asc=asc, rw=rw, ranks=rk, n=n))
    return out


def select_inputs(c):
    """Keys from TIE_KEYS (ties decide, weights 1 + diff at or below zero occur); scores that name their column."""
    P, K, P2, B = c["P"], c["K"], c["P2"], c["B"]
    PK = P + K
    rng = np.random.default_rng([61, c["n"], B, c["asc"], c["rw"]])
    diff = TIE_KEYS[rng.integers(0, TIE_KEYS.size, size=(B, PK))]
    out1 = (1.0 + np.arange(B * PK, dtype=F64).reshape(B, PK) / 8).astype(F32)
    out2 = (0.5 + np.arange(B * PK, dtype=F64).reshape(B, PK) / 4).astype(F32)
    ranks = None
    if c["ranks"] == "given":      # a repeated rank and rank P - 1 (slot 0 is forced whatever its rank)
        r = rng.integers(0, P, size=P2)
        if P2 > 1:
            r[1] = P - 1
        if P2 > 2:
            r[2] = r[1]
        ranks = r.astype(np.int32)
    return dict(diff=diff, out1=out1, out2=out2, ranks=ranks)


# ------------------------------------------------------------------------------------------------ the one-directional half
def loss_grad_one(i, dt, D, z_index=3):
    """lossp and dv of ph_crd_loss_grad_one: the xt / mem1 / Z_v2 half of crd_width_emulation.loss_grad, T = i["T"], Z =
    params[z_index] of the mono layout [P, K, T, Z_v2, momentum]."""
    par = i["params"]
    two = dict(i, xs=i["xt"], params=np.array([i["K2"], F32(i["T"]), par[z_index], par[z_index], 0.5, i["P2"]], dtype=par.dtype),
               posw_s=i.get("posw"), posw_t=i.get("posw"), idx2=None, mem2=i["mem1"])
    full = W.loss_grad(two, dt, D)
    # (with xs = xt and Z1 = Z2 the two directions are the same numbers: dv2 is the half, the loss needs its own sum)
    xt, P2, K2 = i["xt"], i["P2"], i["K2"]
    B, S2 = xt.shape
    Z, ib = dt(par[z_index]), dt(F32(i["inv_bnorm"]))
    mPn, c = E._nce(i["m_neg"], i["n_data"], dt)
    w = np.full((B, S2), dt(1) / dt(P2), dtype=dt)
    if i.get("posw") is not None:
        w[:, :P2] = i["posw"]
    x = xt.astype(dt) / Z
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = np.where((np.arange(S2) < P2)[None, :], np.log(x / (x + c)) * w, np.log(mPn / (x + c))).astype(dt)
    if dt is F64:
        return {"lossp": -lt.sum(1) * ib, "dv": full["dv2"]}
    ns, NHW = i["ns"], 4096 // D
    j0 = np.arange(ns)[:, None] * NHW + np.arange(NHW)[None, :]
    ls = np.zeros((B, ns, NHW), dtype=F32)
    bb = np.arange(B)[:, None, None]
    for s in range(-(-S2 // (NHW * ns))):
        j = j0 + s * NHW * ns
        ls = np.where((j < S2)[None], ls + lt[bb, np.minimum(j, S2 - 1)[None]], ls)
    return {"lossp": -_seq(_seq(ls, 2), 1) * ib, "dv": full["dv2"]}


LG_ONE_CASES = [dict(S2=S2, P2=P2, B=B, posw=pw, T=T, D=D)
                for D in W.WIDTHS for (S2, P2, B, pw, T) in ((33, 4, 3, False, 0.07), (532, 20, 2, True, 0.07), (1023, 20, 1, False, 1.0),
                                                             (1044, 20, 3, False, 0.07), (2600, 6, 1, True, 0.07))]


def lg_one_inputs(c):
    """The inputs of crd_width_emulation.lg_inputs, read by both entries: `two` for ph_crd_loss_grad, `one` for the half."""
    two = W.lg_inputs(dict(S2=c["S2"], P2=c["P2"], B=c["B"], posw=c["posw"], idx2=False, T=c["T"], ws=True), c["D"])
    par = two["params"]
    one = dict(xt=two["xt"], sel=two["sel"], idx=two["idx"], posw=two["posw_t"], mem1=two["mem1"], T=c["T"],
               params=np.array([two["P2"], two["K2"], c["T"], par[3], 0.5], dtype=F32), B=two["B"], PK=two["PK"], P2=two["P2"],
               K2=two["K2"], m_neg=two["m_neg"], n_data=two["n_data"], inv_bnorm=two["inv_bnorm"], ns=two["ns"])
    return two, one


# ------------------------------------------------------------------------------------------------ one call of a criterion
def _z(xs, n_data, dt):
    """Z of the first call: mean x n_data (float32: the double sum rounded to float, then the float divide and multiply of ph_crd_setz)."""
    if dt is F64:
        return xs.astype(F64).mean() * n_data
    return F32(F32(F32(xs.astype(F64).sum()) / F32(xs.size)) * F32(n_data))


def chain(c, dt, defect=None):
    """One call on normalised embeddings.  c: kind ("v4" / "mono"), v1, v2 [B, D] float32, idx [B, P + K], mem1, mem2, T, P, K,
    P2, K2 (stored, never read), ranks, neg_reweight, n_data, Z (None: the first call, else (Z1, Z2)), inv_bnorm.  Returns loss,
    dv1 (None for mono), dv2, Z1, Z2, sel."""
    D = c["v1"].shape[1]
    mono = c["kind"] == "mono"
    P, K, P2 = c["P"], c["K"], c["P2"]
    si = dict(v1=c["v1"], v2=c["v2"], idx=c["idx"], idx2=None, mem1=c["mem1"], mem2=c["mem2"], T=c["T"])
    sc, sc32 = W.score(si, dt, D), W.score(si, F32, D)
    diff32 = c.get("diff", sc32["diff"]).astype(F32)
    diff = diff32.astype(dt) if "diff" in c else sc["diff"]
    asc = not mono
    if defect == "descending" or defect == "mono_ascending":
        asc = not asc
    ranks = c["ranks"]
    if defect == "mono_mid_v4":
        ranks = c["ranks_v4"]
    sel = select_ref(diff32, sc32["out1"], sc32["out2"], ranks, P, K, P2, asc, False, defect)["sel"]
    g = sel.astype(np.int64)
    xs, xt = np.take_along_axis(sc["out1"], g, 1).astype(dt), np.take_along_axis(sc["out2"], g, 1).astype(dt)
    xs_raw, xt_raw = xs.copy(), xt.copy()
    if c["neg_reweight"] and not mono:
        d = np.take_along_axis(diff, g, 1).astype(dt)
        w = (dt(1) - d) if defect == "weight_minus" else (dt(1) + d)
        lo = 0 if defect == "weight_positives" else P2
        xs[:, lo:] = xs[:, lo:] * w[:, lo:]
        if defect != "weight_one_side":
            xt[:, lo:] = xt[:, lo:] * w[:, lo:]
    if c["Z"] is None:
        zs, zt = (xs_raw, xt_raw) if defect == "z_unweighted" else (xs, xt)
        Z1, Z2 = _z(zs, c["n_data"], dt), _z(zt, c["n_data"], dt)
    else:
        Z1, Z2 = dt(c["Z"][0]), dt(c["Z"][1])
    m_neg = c["K2"] if defect == "m_k2" else K
    S2 = P2 + K
    base = dict(sel=sel, idx=c["idx"], mem1=c["mem1"], P2=P2, K2=K, m_neg=m_neg, n_data=float(c["n_data"]),
                inv_bnorm=c["inv_bnorm"], ns=E.lg_splits(S2, S2 >= 1024), B=xs.shape[0], PK=P + K)
    if mono:
        par = np.array([P, K, F32(c["T"]), Z2, 0.5], dtype=dt)
        o = loss_grad_one(dict(base, xt=xt.astype(dt), T=c["T"], params=par), dt, D, z_index=2 if defect == "mono_z_v1" else 3)
        return dict(loss=o["lossp"].astype(dt).sum(), dv1=None, dv2=o["dv"], Z1=None, Z2=Z2, sel=sel)
    par = np.array([K, F32(c["T"]), Z1, Z2, 0.5, P], dtype=dt)
    o = W.loss_grad(dict(base, xs=xs.astype(dt), xt=xt.astype(dt), idx2=None, posw_s=None, posw_t=None, mem2=c["mem2"], params=par),
                    dt, D)
    return dict(loss=o["lossp"].astype(dt).sum(), dv1=o["dv1"], dv2=o["dv2"], Z1=Z1, Z2=Z2, sel=sel)


def chain_tolerances(ref, rest):
    """Per output of `chain`: crd_width_emulation.tolerance under the loss kernel's floor."""
    return {k: W.tolerance("loss_grad", np.asarray(ref[k], dtype=F64), np.asarray(rest[k], dtype=F64))
            for k in ("loss", "dv1", "dv2", "Z1", "Z2") if ref[k] is not None}


# (kind, D, P, K, P2, K2, neg_reweight, mode, first call, ties): what the chain is checked on - both criteria, the three widths,
# both weight settings, host-drawn ranks, a second call with Z given, the split form P2 + K >= 1024, a tie case
CHAIN_CASES = (
    ("v4", 128, 100, 512, 20, 64, True, "hard", True, False),
    ("v4", 128, 100, 512, 20, 64, False, "hard", True, False),
    ("v4", 128, 100, 512, 20, 64, True, "mid", False, False),
    ("v4", 64, 12, 40, 4, 8, True, "hard", True, False),
    ("v4", 256, 12, 40, 4, 8, True, "hard", False, False),
    ("v4", 128, 100, 1024, 20, 512, True, "hard", True, False),
    ("v4", 128, 24, 90, 6, 16, True, "hard", True, True),
    ("mono", 128, 100, 512, 20, 64, False, "hard", True, False),
    ("mono", 128, 100, 512, 20, 64, False, "mid", True, False),
    ("mono", 256, 12, 40, 4, 8, False, "hard", False, False),
    ("mono", 64, 100, 1024, 20, 512, False, "hard", True, False),
    ("mono", 128, 24, 90, 6, 16, False, "hard", True, True),
)


def draw_ranks(kind, mode, P2, rng):
    """The host draws of the reference: v4 `mid` = choice(arange(30, 100), P2, replace=False), mono `mid` = randint(50, 100, P2)."""
    if mode == "hard":
        return None
    return (rng.choice(np.arange(30, 100), P2, replace=False) if kind == "v4" else rng.randint(50, 100, P2)).astype(np.int32)


def chain_inputs(case, n):
    kind, D, P, K, P2, K2, rw, mode, first, ties = case
    rng = np.random.default_rng([71, n])
    mem1, mem2 = W.banks(D, N_DATA)
    B = 3
    v1, v2 = W.unit_rows(B, [72, n], D), W.unit_rows(B, [73, n], D)
    idx = np.stack([rng.permutation(N_DATA)[:P + K] for _ in range(B)]).astype(np.int64)
    c = dict(kind=kind, v1=v1, v2=v2, idx=idx, mem1=mem1, mem2=mem2, T=0.07, P=P, K=K, P2=P2, K2=K2, neg_reweight=rw,
             n_data=N_DATA, inv_bnorm=1.0 / B, Z=None,
             ranks=draw_ranks(kind, mode, P2, np.random.RandomState(5)), ranks_v4=draw_ranks("v4", mode, P2, np.random.RandomState(5)))
    if ties:      # keys of the positives from the tie set (scaled into the range of a cosine difference), the negatives' as scored
        d = W.score(dict(v1=v1, v2=v2, idx=idx, idx2=None, mem1=mem1, mem2=mem2, T=0.07), F32, D)["diff"].copy()
        d[:, :P] = TIE_KEYS[rng.integers(0, TIE_KEYS.size, size=(B, P))] * F32(0.25)
        d[:, 1] = d[:, 0]                                     # column 0 tied with column 1: the forced slot matters
        c["diff"] = d
    if not first:
        z = chain(c, F64)
        c["Z"] = (F32(z["Z1"] if z["Z1"] is not None else 1.0) * F32(1.1), F32(z["Z2"]) * F32(0.9))
    return c


# which defects apply to which cases
def defects_of(case):
    kind, D, P, K, P2, K2, rw, mode, first, ties = case
    out = []
    if kind == "v4":
        out += ["descending", "m_k2"]
        if rw:
            out += ["weight_minus", "weight_one_side", "weight_positives"]
            if first:
                out += ["z_unweighted"]
    else:
        out += ["mono_ascending", "m_k2", "mono_z_v1"]
        if mode == "mid":
            out += ["mono_mid_v4"]
    if ties:
        out += ["tie_higher", "slot0_free"]
    return out


# ------------------------------------------------------------------------------------------------ the criteria on the fixture
def _embed(f, Wt, b, dt):
    z = f.astype(dt) @ Wt.astype(dt).T + b.astype(dt)
    n = np.sqrt((z * z).sum(1, keepdims=True))
    return z / n, n


def _embed_bwd(f, Wt, v, n, dv, dt):
    dz = (dv - v * (v * dv).sum(1, keepdims=True)) / n
    return dz @ Wt.astype(dt), dz.T @ f.astype(dt), dz.sum(0)


def _update(mem, y, v, mom, dt):
    a = mem[y].astype(dt) * dt(mom) + v.astype(dt) * (dt(1) - dt(mom))
    mem = mem.copy()
    mem[y] = (a / np.sqrt((a * a).sum(1, keepdims=True))).astype(mem.dtype)
    return mem


def criterion_calls(g, name, embed_s, embed_t, banks, dt, defect=None):
    """The two consecutive calls of case `name` of dscd_forward.npz: per call loss, g_fs, g_ws, g_bs, g_wt (v4), sel, Z, the
    updated bank rows.  embed_s / embed_t: (weight, bias) (embed_t None for the one-directional criterion); banks: (mem1, mem2)."""
    D, P, P2, K = (int(v) for v in g[name + ".dims"])
    mono = str(g[name + ".crit"]) == "CRDLoss_v2"
    mem1, mem2 = (b.astype(dt) for b in banks)
    Z, out = None, []
    for it in range(2):
        f_s, f_t, y, idx = (g["%s.%s%d" % (name, k, it)] for k in ("f_s", "f_t", "index", "sidx"))
        vs, ns_ = _embed(f_s, embed_s[0], embed_s[1], dt)
        if mono:
            ft = f_t.astype(dt)
            vt = ft / np.sqrt((ft * ft).sum(1, keepdims=True))
            v1, v2 = vt, vs                                   # the bank is called with (teacher, student)
        else:
            vt, nt = _embed(f_t, embed_t[0], embed_t[1], dt)
            v1, v2 = vs, vt
        ranks = g[name + ".ranks"][it].astype(np.int32) if str(g[name + ".mode"]) == "mid" else None
        c = dict(kind="mono" if mono else "v4", v1=v1.astype(F32) if dt is F32 else v1, v2=v2.astype(F32) if dt is F32 else v2,
                 idx=idx, mem1=mem1, mem2=mem2, T=0.07, P=P, K=K, P2=P2, K2=K, neg_reweight=str(g[name + ".neg_reweight"]) == "True",
                 n_data=int(g["n_data"]), inv_bnorm=1.0 / f_s.shape[0], Z=Z, ranks=ranks, ranks_v4=ranks)
        o = chain(c, dt, defect)
        Z = (o["Z1"] if o["Z1"] is not None else 1.0, o["Z2"])
        r = dict(loss=o["loss"], sel=o["sel"], Z1=o["Z1"], Z2=o["Z2"])
        if mono:
            r["g_fs"], r["g_ws"], r["g_bs"] = _embed_bwd(f_s, embed_s[0], vs, ns_, o["dv2"].astype(dt), dt)
        else:
            r["g_fs"], r["g_ws"], r["g_bs"] = _embed_bwd(f_s, embed_s[0], vs, ns_, o["dv1"].astype(dt), dt)
            r["g_wt"] = _embed_bwd(f_t, embed_t[0], vt, nt, o["dv2"].astype(dt), dt)[1]
        mem1, mem2 = _update(mem1, y, v1, 0.5, dt), _update(mem2, y, v2, 0.5, dt)
        r["bank_v1_rows"], r["bank_v2_rows"] = mem1[y], mem2[y]
        out.append(r)
    return out

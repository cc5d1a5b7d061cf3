"""References of the GK-Refine loss weights (csrc/optim.hip), the masks of the MIA-2023 masking teacher (csrc/superpixel.hip) and the
flat-buffer updates and reductions (csrc/optim.hip, csrc/surv.hip, csrc/tsvd.hip) for tests/test_gpu_head.py, and the case tables of
that sweep.  The layout is that of tests/dense_emulation.py.

Every operator is one function of (inputs, dt, defect): dt = float64 is the reference of the documented formula, dt = float32 restates
the kernel, in its summation order where it has one (ph_gram: per-thread strided sums of 1024 threads, the 64-lane butterfly, the 16
wave sums one after the other; ph_sqdiff_sum: the 1024-wide tree; ph_l1_sum: 256-thread blocks, butterfly, the four wave sums in
pairs, the partials added in double; ph_superpixel_mask: the 64-bit fixed point under its power-of-two scale).  An output array of a
case is compared in one of two classes:

  exact   named in the entry's `exact`: the float64 and the float32 form agree bit for bit (integers below 2^24, 0/1 masks, counts of
          cosines that are exact ties or at least 1e-3 away from the threshold, sums of binary fractions) and the device must equal them.
  real    everything else: within MARGIN (4) x the float32 restatement's error against float64 on the same inputs, plus
          FLOOR[operator] x max |ref| (4 x the largest excess of the MI355X over the restatement; the figures are in the docstring of
          tests/test_gpu_head.py, which prints them on every run).

tests/test_head_emulation_cpu.py shows that the tolerances accept the restatement and reject every injected defect by a factor of 4
or more (an exact array rejects by not being equal)."""
import numpy as np

from tests.dense_emulation import err, scale, _fma      # noqa: F401  (err / scale are part of this module's interface)

F32, F64 = np.float32, np.float64
MARGIN = 4.0
EINVAL = -22

# Relative floor per operator, in units of max |ref|: 4 x the measured excess of the device's error over the restatement's (the
# kernels' `a * b + c` are contracted to fmas where hipcc chooses, their expf / sqrtf / division are the device's).  An operator
# without an entry never exceeded its restatement.
FLOOR = {"adam": 4 * 3.57e-8, "adagrad": 4 * 1.096e-8}


def tolerance(op, ref, rest):
    return MARGIN * err(ref, rest) + FLOOR.get(op, 0.0) * scale(ref)


def entry_tolerance(e, k):
    return tolerance(e["op"], e["ref"][k], e["rest"][k])


def _butterfly(w):
    """The xor butterfly of wave_sum over the last axis (64 lanes): every lane ends with the same sum."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    return w


def _madd(a, b, c, dt):
    """a * b + c as the kernels' `t += a * b` compiles: one fma in float32 (hipcc contracts by default), plain in float64."""
    return _fma(np.asarray(a), np.asarray(b), np.asarray(c))[()] if dt is F32 else a * b + c


def _tree(p):
    """sh[t] += sh[t + o] for o = 512 .. 1 over 1024 per-thread values."""
    p = p.copy()
    o = 512
    while o > 0:
        p[:o] = p[:o] + p[o:2 * o]
        o >>= 1
    return p[0]


def _strided(vals, T, dt, fma_with=None):
    """Per-thread sums of T threads: thread t adds elements t, t + T, .. in that order (zero padding adds nothing).  fma_with: the
    second factor of a product accumulated by one fma per element (`acc += a * b` as hipcc contracts it)."""
    n = len(vals)
    pad = -n % T
    a = np.concatenate([vals, np.zeros(pad, dt)]).reshape(-1, T)
    b = None if fma_with is None else np.concatenate([fma_with, np.zeros(pad, dt)]).reshape(-1, T)
    acc = np.zeros(T, dt)
    for r in range(a.shape[0]):
        acc = (acc + a[r]) if b is None else _fma(a[r], b[r], acc)
    return acc


# ------------------------------------------------------------------------------------------------ ph_gram
GRAM_NG, GRAM_N = (2, 3, 4, 5), (1, 63, 64, 65, 1023, 1024, 1025, 4099, 16384)
_LEAD = np.array([1, 2, 3, -1, -2])


def gram_inputs(ng, n, real):
    """G [ng][n].  Integer class: non-zero integers in [-3, 3] (every Gram entry below 2^24, a dropped element always shows), the
    first column 1, 2, 3, -1, -2; real class: row i is a normal row scaled by 1 + i / 2.  Either way no two rows can be swapped
    without changing the Gram matrix (asserted by the self-test)."""
    rng = np.random.default_rng([61, ng, n, int(real)])
    if real:
        G = rng.standard_normal((ng, n)) * (1.0 + 0.5 * np.arange(ng))[:, None]
    else:
        G = rng.integers(1, 4, size=(ng, n)) * rng.choice([-1, 1], size=(ng, n))
        G[:, 0] = _LEAD[:ng]
    return G.astype(F32)


def gram(G, dt, defect=None):
    G = G.astype(dt)
    if defect == "drop_tail":
        G = G[:, :-1]
    ng = G.shape[0]
    if dt is F64:
        return {"gram": G @ G.T}
    out = np.zeros((ng, ng), F32)
    for i in range(ng):
        for j in range(i, ng):
            w = _butterfly(_strided(G[i], 1024, F32, fma_with=G[j]).reshape(16, 64))[:, 0]
            s = F32(0)
            for k in range(16):
                s = s + w[k]
            out[i, j] = out[j, i] = s
    return {"gram": out}


# ------------------------------------------------------------------------------------------------ the GK weights
INT2EXT = (0, 1, 3, 4, 2)      # ext2int of the kernels: the trainer's order [div1, div2, kd1, kd2, CE] in internal indices


def _real_gram(ng, seed):
    """The float32 Gram matrix of ng correlated real rows (cosines spread over (-1, 1), norms over a decade)."""
    rng = np.random.default_rng([67, ng, seed])
    G = rng.standard_normal((ng, 40)) + 0.8 * rng.standard_normal(40)[None, :]
    G = G * (1.0 + np.arange(ng))[:, None]
    return (G @ G.T).astype(F32)


# integer rows whose norms are perfect squares: r1 = 2 r0 (cosine exactly 1), r2 and r3 orthogonal to r0, r1 and to each other
# (cosine exactly 0), r4 at cosines 0.7, 0.7, 17/26, 0.1 - every cosine is an exact tie with a threshold of 0 or 1 or at least
# 0.1 away from 0, 0.5 and 1, and every square root and quotient of the kernel is exact or far from the threshold
_TROWS = np.array([[3, 4, 0, 0], [6, 8, 0, 0], [0, 0, 5, 12], [4, -3, 0, 0], [1, 1, 1, 1]], dtype=np.int64)
_TPICK3 = ((0, 1, 2), (0, 3, 4), (1, 4, 2))
_TPICK5 = ((0, 1, 2, 3, 4), (4, 0, 2, 1, 3), (2, 3, 1, 4, 0))
THRESHES = (0.0, 1.0, 0.5)


def _tie_gram(ng, call):
    rows = _TROWS[list((_TPICK3 if ng == 3 else _TPICK5)[call])]
    return (rows @ rows.T).astype(F32)


def _cos_sums(g, dt, idx, mult=None, thresh=None, ge=False):
    """Row sums of the cosine matrix of Gram g over the index list idx, added one after the other as the kernels do."""
    g = g.astype(dt)
    d = np.sqrt(np.diag(g))
    out = np.zeros(len(idx), dt)
    for a, i in enumerate(idx):
        s = dt(0)
        for j in idx:
            if mult is not None:
                r = g[i, j] * dt(F32(mult)) / (d[i] * d[j])
            else:
                r = g[i, j] / (d[i] * d[j])
            if thresh is not None:
                t = dt(F32(thresh))
                r = dt(1) if (r >= t if ge else r > t) else dt(0)
            s = s + r
        out[a] = s
    return out


def gk_scale(inp, dt, defect=None):
    ng, mult = inp["ng"], (1.0 if defect == "no_mult" else inp["mult"])
    s = _cos_sums(inp["gram"], dt, range(ng), mult=mult)
    out = {"scale": s}
    if inp["losses"] is not None:
        t = dt(0)
        for i in range(inp["nl"]):
            t = _madd(s[i], inp["losses"].astype(dt)[i], t, dt)
        out["total"] = np.array([t])
    return out


def gk_finish(inp, dt, defect=None):
    mult = 1.0 if defect == "no_mult" else inp["mult"]
    s = _cos_sums(inp["gram"], dt, range(5), mult=mult)
    L, coef, add, logc = (inp[k].astype(dt) for k in ("losses", "coef", "add", "logc"))
    w = add + s * coef
    t = dt(0)
    for i in range(5):
        t = _madd(w[i], L[i], t, dt)
    ext = s if defect == "ext_internal" else s[list(INT2EXT)]
    return {"scale_int": s, "w": w, "total": np.array([t]), "scaled": L * logc, "scale_ext": ext}


def _momentum(state, s, first, mom, dt, defect):
    if first and defect != "mom_first":
        return s
    m = dt(F32(mom))
    return m * state + (dt(1) - m) * s


def gk_scale_momentum(inp, dt, defect=None):
    """The calls of one case on the persistent state (NaN before the first call: a first call must not read it).  Output
    "mo<c>" = the state after call c."""
    ng, out = inp["ng"], {}
    state, init = np.full(ng, np.nan, dt), 0
    for c, g in enumerate(inp["grams"]):
        first = inp["mo_init"] is None or init == 0
        s = _cos_sums(g, dt, range(ng), thresh=inp["thresh"] if inp["use_thresh"] else None, ge=defect == "ge_thresh")
        state = _momentum(state, s, first, inp["momentum"], dt, defect)
        init = 1
        out["mo%d" % c] = state
    if inp["mo_init"] is not None:
        out["init"] = np.array([1], dtype=np.int32)
    return out


def gk_finish_momentum(inp, dt, defect=None):
    """Per call c: mo<c> (= scale_ext<c>) in the trainer's order, w<c> / scaled<c> in internal order, total<c>, and "wce<c>" = the
    CE weight, which is lam itself."""
    out = {}
    state, init = np.full(5, np.nan, dt), 0
    e = dt(1) if inp["e_dev"] is None else dt(F32(inp["e_dev"]))
    al, be, lam = dt(F32(inp["alpha"])), dt(F32(inp["beta"])), dt(F32(inp["lam"]))
    mult = dt(1) if defect == "no_mult" else dt(F32(inp["mult"]))
    c_int = np.array([al, al, dt(1), be * e, be * e], dt)
    for c, (g, L) in enumerate(zip(inp["grams"], inp["losses"])):
        first = inp["mo_init"] is None or init == 0
        idx = range(5) if defect == "ext_internal" else INT2EXT
        s = _cos_sums(g, dt, idx, thresh=inp["thresh"] if inp["use_thresh"] else None, ge=defect == "ge_thresh")
        state = _momentum(state, s, first, inp["momentum"], dt, defect)
        init = 1
        L = L.astype(dt)
        w, t = np.zeros(5, dt), dt(0)
        for ie, i in enumerate(INT2EXT):
            w[i] = lam if i == 2 else mult * state[ie] * c_int[i]
            t = _madd(w[i], L[i], t, dt)
        out.update({"mo%d" % c: state, "scale_ext%d" % c: state, "w%d" % c: w, "wce%d" % c: w[2:3], "total%d" % c: np.array([t]),
                    "scaled%d" % c: L * c_int})
    if inp["mo_init"] is not None:
        out["init"] = np.array([1], dtype=np.int32)
    return out


def _five(seed, lo=0.3):
    """Five distinct positive values (a wrong index always changes a result)."""
    v = lo + np.random.default_rng([71, seed]).random(5) + 0.37 * np.arange(5)
    return v.astype(F32)


# ------------------------------------------------------------------------------------------------ ph_superpixel_mask
SP_GAP = 1e-4      # least separation (of max |mean|) between the K-th and the (K + 1)-th mean of a case that is no built tie


def _sp_means64(grad, lab, N):
    B = grad.shape[0]
    m = np.zeros((B, N))
    for b in range(B):
        ok = (lab[b] >= 0) & (lab[b] < N)
        s = np.bincount(lab[b][ok], weights=grad[b].astype(F64).sum(0)[ok], minlength=N)
        m[b] = s / (np.bincount(lab[b][ok], minlength=N) + 1e-9)
    return m


def sp_gap(means, K):
    """Smallest gap between the K-th and (K + 1)-th largest mean over the images, in units of the largest |mean| (inf for K = N)."""
    N = means.shape[1]
    if K >= N:
        return np.inf
    s = -np.sort(-means, axis=1)
    return float(((s[:, K - 1] - s[:, K]) / max(np.abs(means).max(), 1e-300)).min())


def superpixel(inp, dt, defect=None):
    grad, lab, N, K = inp["grad"], inp["lab"], inp["N"], inp["K"]
    B, C, HW = grad.shape
    means, mask = np.zeros((B, N), dt), np.zeros((B, HW), F32)
    for b in range(B):
        g, l = grad[b], lab[b]
        if defect == "clamp_label":
            l = np.clip(l, 0, N - 1)
        ok = (l >= 0) & (l < N)
        area = np.bincount(l[ok], minlength=N)
        if dt is F64:
            sums = np.bincount(l[ok], weights=g.astype(F64).sum(0)[ok], minlength=N)
            mean = sums / (area + 1e-9)
        else:
            mx, ex = np.abs(g).max(), 0
            if mx > 0:
                ex = 61 - int(np.frexp(mx)[1]) - int(np.frexp(F32(C) * F32(HW))[1])
            hi, lo = np.ldexp(F32(1), min(ex, 126)), np.ldexp(F32(1), ex - 126 if ex > 126 else 0)
            q = np.rint((g * hi) * lo).astype(np.int64).sum(0)
            isum = np.zeros(N, np.int64)
            np.add.at(isum, l[ok], q[ok])
            sums = (isum.astype(F64) / (F64(hi) * F64(lo))).astype(F32)
            mean = sums / (area.astype(F32) + F32(1e-9))
        if defect == "no_area":
            mean = sums.astype(dt)
        idx = np.arange(N)
        order = np.lexsort((-idx if defect == "tie_high" else idx, -mean))      # largest mean first, then the lowest index
        sel = np.zeros(N, bool)
        sel[order[:K]] = True
        means[b] = mean
        mask[b] = (ok & sel[np.clip(l, 0, N - 1)]).astype(F32)
    out = {"mask": mask}
    if inp["want_mean"]:
        out["mean"] = means
    return out


def _sp_case(name, B, C, H, W, N, K, want_mean, kind="real", scale2=0):
    """kind: real (normal gradients, labels uniform in [0, N)), oob (labels -1 and N among them), empty (all gradients negative,
    three labels unused), tie (integer gradients, two superpixels of equal sum and area at the K-th place), zero.  K "mid": the K
    in [N / 3, 2 N / 3] with the widest gap behind it.  A case that is no built tie has at least SP_GAP behind its K-th mean."""
    HW = H * W
    for seed in range(50):
        rng = np.random.default_rng([73, B, C, HW, N, seed])
        lab = rng.integers(0, N, size=(B, HW)).astype(np.int64)
        grad = rng.standard_normal((B, C, HW)).astype(F32)
        if kind == "oob":
            lab[:, ::7], lab[:, 3::11] = -1, N
        elif kind == "empty":
            lab = (2 + lab % (N - 3)).astype(np.int64)          # labels 0, 1 and N - 1 stay empty
            grad = -np.abs(grad) - F32(0.5)
        elif kind == "tie":
            # superpixels 1 and 3 take the same integers in another order: equal area, bit-identical sums
            grad = rng.integers(-3, 4, size=(B, C, HW)).astype(F32)
            lab = (np.arange(HW) % N)[None, :].repeat(B, 0).astype(np.int64)
            a = (HW // N) * N
            blk = grad[:, :, :a].reshape(B, C, -1, N)
            blk[..., 3] = blk[:, :, ::-1, 1]
            blk[..., 1] += 2                                    # both well above the others
            blk[..., 3] += 2
            grad[:, :, :a] = blk.reshape(B, C, a)
            lab[:, a:] = 0
        elif kind == "zero":
            grad[:] = 0
        if scale2:
            grad = np.ldexp(grad, scale2).astype(F32)
        m = _sp_means64(grad, lab, N)
        k = K
        if K == "mid":
            cand = range(max(1, N // 3), max(2, 2 * N // 3 + 1))
            k = max(cand, key=lambda q: sp_gap(m, q))
        if kind in ("tie", "zero") or sp_gap(m, k) > SP_GAP:
            return dict(name=name, B=B, C=C, H=H, W=W, N=N, K=int(k), want_mean=want_mean, kind=kind, grad=grad, lab=lab, scale2=scale2)
    raise AssertionError("no seed separates the K-th mean of " + name)


def _sp_table():
    T = [_sp_case("B1 C1 HW1 N1 K1", 1, 1, 1, 1, 1, 1, True),
         _sp_case("B3 C3 HW1023 N2 K1", 3, 3, 1023, 1, 2, 1, False),
         _sp_case("B1 C3 HW1024 N2 K2", 1, 3, 1024, 1, 2, 2, True),
         _sp_case("B3 C1 HW1025 N1024 Kmid", 3, 1, 1025, 1, 1024, "mid", True),
         _sp_case("B1 C1 48x40 N1025 Kmid", 1, 1, 48, 40, 1025, "mid", False),
         _sp_case("B3 C3 48x40 N2048 KN", 3, 3, 48, 40, 2048, 2048, True),
         _sp_case("B1 C3 48x40 N2048 K1", 1, 3, 48, 40, 2048, 1, False),
         _sp_case("B1 C1 HW1025 N1024 K1024", 1, 1, 1025, 1, 1024, 1024, False),
         _sp_case("oob B3 C1 HW1025 N5 K2", 3, 1, 1025, 1, 5, 2, True, "oob"),
         _sp_case("empty B3 C3 HW1023 N8 K4", 3, 3, 1023, 1, 8, 4, True, "empty"),
         _sp_case("tie B3 C3 HW1024 N6 K1", 3, 3, 1024, 1, 6, 1, True, "tie"),
         _sp_case("tie B1 C1 HW1023 N6 K1", 1, 1, 1023, 1, 6, 1, False, "tie"),
         _sp_case("zero B3 C1 HW1025 N4 K2", 3, 1, 1025, 1, 4, 2, True, "zero"),
         _sp_case("2^-100 B3 C3 HW1023 N7 Kmid", 3, 3, 1023, 1, 7, "mid", True, "real", -100),
         _sp_case("2^+100 B1 C3 HW1025 N7 Kmid", 1, 3, 1025, 1, 7, "mid", True, "real", 100)]
    return T


# ------------------------------------------------------------------------------------------------ ph_topk_threshold_mask
def topk_mask(inp, dt, defect=None):
    x, K = inp["x"].astype(dt), inp["K"]
    kth = -np.sort(-x, axis=1)[:, K - 1:K]
    return {"mask": ((x > kth) if defect == "gt_kth" else (x >= kth)).astype(F32)}


def _topk_table():
    """Values from a few small integers, so that runs of equal values straddle every K; "zero": +0.0 and -0.0 at the K-th place;
    "inf": both infinities present."""
    T = []
    for i, D in enumerate((1, 2, 255, 256, 257, 16384)):
        for j, K in enumerate((1, "mid", D)):
            if D <= 2 and K == "mid":
                continue
            B = (1, 3)[(i + j) % 2]
            rng = np.random.default_rng([79, D, j])
            x = rng.integers(-3, 4, size=(B, D)).astype(F32)
            k = D // 2 + 1 if K == "mid" else K
            if K == "mid":                  # a row whose run of equal values ends at the K-th place gets one more of them
                for row in x:
                    kth = -np.sort(-row)[k - 1]
                    if (row >= kth).sum() == k:
                        row[np.nonzero(row < kth)[0][0]] = kth
            T.append(dict(name="B%d D%d K%d" % (B, D, k), B=B, D=D, K=k, x=x, kind="ties"))
    rng = np.random.default_rng([79, 0])
    x = rng.choice(np.array([-2.0, -0.0, 0.0, 0.0, -0.0, 3.0], F32), size=(3, 257))
    x[:, :4] = np.array([0.0, -0.0, 3.0, -2.0], F32)
    k = int((x > 0).sum(1).max()) + 1                            # the K-th largest is a zero in every row
    T.append(dict(name="zero B3 D257 K%d" % k, B=3, D=257, K=k, x=x, kind="zero"))
    x = np.random.default_rng([79, 1]).standard_normal((3, 255)).astype(F32)
    x[:, 5], x[:, 17], x[:, 100], x[0, 101] = np.inf, -np.inf, np.inf, np.inf
    for k in (2, 3, 255):
        T.append(dict(name="inf B3 D255 K%d" % k, B=3, D=255, K=k, x=x, kind="inf"))
    return T


# ------------------------------------------------------------------------------------------------ ph_apply_mask
APPLY_CASES = ((1, 1, 1), (2, 3, 85), (3, 1, 257))


def apply_mask(inp, dt, defect=None):
    x, m = inp["x"].astype(dt), inp["mask"].astype(dt)
    return {"out": x * (m if defect == "no_sub" else dt(1) - m)[:, None, :]}


# ------------------------------------------------------------------------------------------------ Adam, Adagrad, EMA
UPD_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)
LR, BETA1, BETA2, ADAM_EPS, ADAGRAD_EPS, EMA_ALPHA, WD = 0.01, 0.9, 0.999, 1e-8, 0.01, 0.95, 4e-4


def hyper_record(step, lr=LR, b1=BETA1, b2=BETA2, alpha=EMA_ALPHA):
    """The device record of ph_adam_ema_step_dev, the doubles the host form computes rounded to float once."""
    h = np.zeros(12, F32)
    h[:5] = [lr, 1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step), alpha, 1.0 - alpha]
    h[8:12] = [b1, 1.0 - b1, b2, 1.0 - b2]
    return h


def _upd_inputs(n, seed):
    """p, g, m, v (>= 0), ema of n elements; the elements 2 and 1024 (where they exist: vector body and scalar tail) have g = m = v = 0."""
    rng = np.random.default_rng([83, n, seed])
    d = dict(p=rng.standard_normal(n), g=rng.standard_normal(n), m=0.3 * rng.standard_normal(n), v=0.1 + rng.random(n),
             ema=rng.standard_normal(n))
    for z in (2, 1024):
        if z < n:
            d["g"][z] = d["m"][z] = d["v"][z] = 0.0
    return {k: a.astype(F32) for k, a in d.items()}


def adam(inp, dt, defect=None):
    """hyper, eps, wd are float32 inputs (the kernels' arguments); every operation in dt."""
    h = inp["hyper"].astype(dt)
    lr, bc1, bc2s, al, oma, b1, omb1, b2, omb2 = h[0], h[1], h[2], h[3], h[4], h[8], h[9], h[10], h[11]
    eps, wd = dt(F32(inp["eps"])), dt(F32(inp["wd"]))
    p, g, m, v = (inp[k].astype(dt) for k in "pgmv")
    gg = g if defect == "wd_after" else g + wd * p
    m = b1 * m + omb1 * gg
    v = b2 * v + omb2 * gg * gg
    den = np.sqrt(v) / (bc2s * bc2s if defect == "bc2_nosqrt" else bc2s) + eps
    pn = p - (lr / bc1) * m / den
    if defect == "wd_after":
        pn = pn - lr * wd * p
    out = {"p": pn, "m": m, "v": v}
    if inp["use_ema"]:
        out["ema"] = al * inp["ema"].astype(dt) + oma * (p if defect == "ema_old_p" else pn)
    return out


def adagrad(inp, dt, defect=None):
    h = inp["hyper"].astype(dt)
    lr, al, oma = h[0], h[3], h[4]
    eps, wd = dt(F32(inp["eps"])), dt(F32(inp["wd"]))
    p, g, s = (inp[k].astype(dt) for k in "pgv")
    gg = g + wd * p
    s = s + gg * gg
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(s + eps) if defect == "eps_in_sqrt" else np.sqrt(s) + eps
        pn = p - lr * gg / den
    out = {"p": pn, "v": s}
    if inp["use_ema"]:
        out["ema"] = al * inp["ema"].astype(dt) + oma * (p if defect == "ema_old_p" else pn)
    return out


def _upd_table():
    T = []
    for i, n in enumerate(UPD_N):
        for e in (0, 1):
            step = (1, 1000)[(i + e) % 2]
            T.append(dict(n=n, use_ema=bool(e), wd=(0.0, WD)[(i // 2 + e) % 2], step=step, hyper=hyper_record(step)))
    return T


UPD_CASES = _upd_table()
ELT_N = (1, 255, 256, 257, 1025)


def ema_update(inp, dt, defect=None):
    """ph_ema_update (alpha an argument, 1 - alpha taken in dt) and ph_ema_update_dev (hyper[3], hyper[4])."""
    if inp["dev"]:
        a, b = inp["hyper"].astype(dt)[3], inp["hyper"].astype(dt)[4]
    else:
        a = dt(F32(inp["alpha"]))
        b = dt(1) - a
    if defect == "swap_rate":
        a, b = b, a
    return {"ema": a * inp["ema"].astype(dt) + b * inp["p"].astype(dt)}


def scaled_diff(inp, dt, defect=None):
    gs, al = inp["gs"].astype(dt)[0], dt(F32(inp["alpha"]))
    return {"out": (gs if defect == "no_alpha" else gs * al) * (inp["a"].astype(dt) - inp["b"].astype(dt))}


def l1_sign_axpy(inp, dt, defect=None):
    """g += c sgn(w), sgn(+-0) = 0; c and the entries of g are binary fractions: exact."""
    w, c = inp["w"].astype(dt), dt(F32(inp["coef"]))
    if inp["coef_dev"] is not None:
        c = c * dt(F32(inp["coef_dev"]))
    sg = np.where(w > 0, dt(1), np.where(w < 0, dt(-1), dt(1) if defect == "sign0_plus" else dt(0)))
    return {"g": inp["g"].astype(dt) + c * sg}


# ------------------------------------------------------------------------------------------------ reductions
L1_N = (1, 255, 256, 2047, 2048, 2049, 2097152, 2097153)
L1_REAL_N = (1, 255, 2049, 5000)
RED_N = (1, 1023, 1024, 1025, 5000)


def l1_blocks(n):
    return min(max((n + 2047) // 2048, 1), 1024)


def l1_sum(inp, dt, defect=None):
    """sum |w| (+ the prior out[0] when accumulate).  float32: block b's thread t adds elements (k nb + b) 256 + t for k = 0, 1, ..,
    the butterfly, (sh0 + sh1) + (sh2 + sh3) per block, the partials in double, rounded once, then the prior value."""
    w = np.abs(inp["w"].astype(dt))
    if defect == "drop_tail":
        w = w[:-1]
    prior = dt(F32(inp["prior"])) if inp["accumulate"] else dt(0)
    if dt is F64:
        return {"out": np.array([w.sum() + prior])}
    nb = l1_blocks(len(inp["w"]))
    acc = _strided(w, nb * 256, F32).reshape(nb, 4, 64)
    sh = _butterfly(acc)[:, :, 0]
    parts = (sh[:, 0] + sh[:, 1]) + (sh[:, 2] + sh[:, 3])
    v = F32(parts.astype(F64).sum())
    return {"out": np.array([prior + v if inp["accumulate"] else v])}


def sqdiff_sum(inp, dt, defect=None):
    d = inp["a"].astype(dt) - inp["b"].astype(dt)
    if defect == "drop_tail":
        d = d[:-1]
    sc = dt(F32(inp["scale"]))
    if dt is F64:
        return {"out": np.array([sc * (d * d).sum()])}
    return {"out": np.array([sc * _tree(_strided(d, 1024, F32, fma_with=d))])}


def maxnorm_mix(inp, dt, defect=None):
    a, b = inp["a"].astype(dt), inp["b"].astype(dt)
    ma, mb = a.max(), b.max()          # (a maximum does not depend on the order of the tree)
    if defect == "max_init0":
        ma, mb = max(ma, dt(0)), max(mb, dt(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"out": dt(F32(inp["wa"])) * (a / ma) + dt(F32(inp["wb"])) * (b / mb)}


# ------------------------------------------------------------------------------------------------ sigmoid-range head
SIG_N = (1, 255, 256, 257)
SIG_SPECIAL = (100.0, 0.0, -100.0, 20.0, -20.0)


def sigmoid_range_fwd(inp, dt, defect=None):
    with np.errstate(over="ignore"):
        s = dt(1) / (dt(1) + np.exp(-inp["h"].astype(dt)))
    r, sh = inp["range"].astype(dt)[0], inp["shift"].astype(dt)[0]
    return {"sigma": s, "pred": s * r + (dt(0) if defect == "no_shift" else sh)}


def sigmoid_range_bwd(inp, dt, defect=None):
    """sigma is the float32 array the forward kept; "dh_sat" = the entries where it is 0 or 1, which are exactly 0."""
    s, r = inp["sigma"].astype(dt), (dt(1) if defect == "no_range" else inp["range"].astype(dt)[0])
    dh = inp["dpred"].astype(dt) * r * s * (dt(1) - s)
    return {"dh": dh, "dh_sat": dh[(inp["sigma"] == 0) | (inp["sigma"] == 1)]}


# ------------------------------------------------------------------------------------------------ the suite
def _entry(op, name, inp, fn, defects=(), exact=()):
    """One case of one operator: inputs, float64 reference, float32 restatement, the restatement with each defect; `exact` names the
    output arrays of the exact class (all of them: True)."""
    ref = fn(inp, F64)
    return dict(op=op, name=name, inp=inp, ref=ref, rest=fn(inp, F32), defects={d: fn(inp, F32, d) for d in defects},
                exact=set(ref) if exact is True else set(exact))


def _suite(op):
    out = []
    if op in ("gram_exact", "gram"):
        for ng in GRAM_NG:
            for n in GRAM_N:
                inp = dict(ng=ng, n=n, G=gram_inputs(ng, n, op == "gram"))
                out.append(_entry(op, "ng%d n%d" % (ng, n), inp, lambda i, dt, d=None: gram(i["G"], dt, d),
                                  ("drop_tail",) if n % 1024 and n > 1 else (), True if op == "gram_exact" else ()))
    elif op == "gk_scale":
        for ng in (3, 5):
            for nl in (0, ng - 1):
                for mult in (1.0, 4.0):
                    inp = dict(ng=ng, nl=nl, mult=mult, gram=_real_gram(ng, nl), losses=_five(ng)[:nl] if nl else None)
                    out.append(_entry(op, "ng%d nl%d mult%g" % (ng, nl, mult), inp, gk_scale, ("no_mult",) if mult != 1 else ()))
    elif op == "gk_finish":
        for s, mult in enumerate((1.0, 4.0, 4.0)):
            inp = dict(mult=mult, gram=_real_gram(5, 10 + s), losses=_five(s), coef=_five(20 + s), add=_five(40 + s, 0.0),
                       logc=_five(60 + s))
            out.append(_entry(op, "gram%d mult%g" % (s, mult), inp, gk_finish, ("ext_internal",) + (("no_mult",) if mult != 1 else ())))
    elif op in ("gk_scale_momentum", "gk_finish_momentum"):
        fin = op == "gk_finish_momentum"
        r = 0
        for ng in ((5,) if fin else (3, 5)):
            for has_init in (1, 0):
                for ut in (0, 1):
                    for mom in (0.0, 0.9):
                        for e_dev, mult in (((None, 1.0), (0.37, 4.0), (0.37, 1.0), (None, 4.0)) if fin else ((None, None),)):
                            th = THRESHES[r % 3]
                            r += 1
                            grams = [_tie_gram(ng, c) if ut else _real_gram(ng, 100 + 3 * r + c) for c in range(3)]
                            inp = dict(ng=ng, mo_init=0 if has_init else None, use_thresh=ut, thresh=th, momentum=mom, grams=grams)
                            name = "ng%d init%d thr%d(%g) mom%g" % (ng, has_init, ut, th, mom)
                            dfs = (("ge_thresh",) if ut and th != 0.5 else ()) + ("mom_first",)
                            # the thresholded counts are integers: exact on a first call and under momentum 0 (0 * state + 1 * s)
                            every_first = not has_init
                            ex = ["mo%d" % c for c in range(3) if ut and (c == 0 or every_first or mom == 0.0)]
                            if has_init:
                                ex.append("init")
                            if fin:
                                inp.update(e_dev=e_dev, mult=mult, alpha=0.7, beta=1.3, lam=0.45, losses=[_five(r + c) for c in range(3)])
                                name += " e%s mult%g" % (e_dev, mult)
                                if not (ut and th == 1.0):      # (no cosine exceeds 1: every weight of such a case is 0)
                                    dfs += ("ext_internal",) + (("no_mult",) if mult != 1 else ())
                                ex += [k.replace("mo", "scale_ext") for k in ex if k.startswith("mo")] + ["wce%d" % c for c in range(3)]
                            out.append(_entry(op, name, inp, gk_finish_momentum if fin else gk_scale_momentum, dfs, ex))
    elif op == "superpixel":
        for c in _sp_table():
            dfs = {"real": ("no_area",) if c["want_mean"] and c["N"] > 1 else (), "oob": ("clamp_label",), "empty": (),
                   "tie": ("tie_high",), "zero": ("tie_high",)}[c["kind"]]
            out.append(_entry(op, c["name"], c, superpixel, dfs, ("mask",)))
    elif op == "topk_mask":
        for c in _topk_table():
            out.append(_entry(op, c["name"], c, topk_mask, ("gt_kth",), True))
    elif op == "apply_mask":
        for (B, C, P) in APPLY_CASES:
            rng = np.random.default_rng([89, B, C, P])
            inp = dict(B=B, C=C, P=P, x=(rng.integers(-4096, 4097, size=(B, C, P)) / 1024.0).astype(F32),
                       mask=rng.choice(np.array([0, 1, 0.25, 0.5, 0.75], F32), size=(B, P)))
            inp["mask"][0, 0] = 0.25
            out.append(_entry(op, "B%d C%d P%d" % (B, C, P), inp, apply_mask, ("no_sub",), True))
    elif op in ("adam", "adagrad"):
        for c in UPD_CASES:
            inp = dict(_upd_inputs(c["n"], int(op == "adam")), **c)
            inp["eps"] = ADAM_EPS if op == "adam" else ADAGRAD_EPS
            name = "n%d ema%d wd%g step%d" % (c["n"], c["use_ema"], c["wd"], c["step"])
            dfs = ("bc2_nosqrt",) + (("wd_after",) if c["wd"] else ()) if op == "adam" else ("eps_in_sqrt",)
            if c["use_ema"]:
                dfs += ("ema_old_p",)
            out.append(_entry(op, name, inp, adam if op == "adam" else adagrad, dfs))
    elif op in ("ema_update", "ema_update_dev", "scaled_diff", "l1_sign_axpy"):
        for i, n in enumerate(ELT_N):
            rng = np.random.default_rng([97, n])
            if op.startswith("ema"):
                inp = dict(n=n, dev=op.endswith("dev"), alpha=0.97, hyper=hyper_record(7, alpha=0.97),
                           ema=rng.standard_normal(n).astype(F32), p=(3 + rng.standard_normal(n)).astype(F32))
                out.append(_entry(op, "n%d" % n, inp, ema_update, ("swap_rate",)))
            elif op == "scaled_diff":
                inp = dict(n=n, alpha=0.3, gs=np.array([1.7], F32), a=rng.standard_normal(n).astype(F32), b=rng.standard_normal(n).astype(F32))
                out.append(_entry(op, "n%d" % n, inp, scaled_diff, ("no_alpha",)))
            else:
                for cd in (None, 0.5):
                    w = rng.choice(np.array([-1.5, -0.0, 0.0, 2.0, 0.25], F32), size=n)
                    w[0] = (0.0, -0.0)[i % 2]
                    inp = dict(n=n, coef=0.25, coef_dev=cd, w=w, g=(rng.integers(-64, 65, size=n) / 8.0).astype(F32))
                    out.append(_entry(op, "n%d coef_dev %s" % (n, cd), inp, l1_sign_axpy, ("sign0_plus",), True))
    elif op in ("l1_sum_exact", "l1_sum"):
        ex = op == "l1_sum_exact"
        for i, n in enumerate(L1_N if ex else L1_REAL_N):
            for acc in (0, 1):
                if ex and n > 2049 and acc != i % 2:      # the two large cases once each, one with and one without accumulate
                    continue
                rng = np.random.default_rng([101, n])
                w = rng.integers(1, 4, size=n) * rng.choice([-1, 1], size=n) if ex else rng.standard_normal(n)
                inp = dict(n=n, accumulate=acc, prior=5.0, w=w.astype(F32))
                out.append(_entry(op, "n%d acc%d" % (n, acc), inp, l1_sum, ("drop_tail",), True if ex else ()))
    elif op in ("sqdiff_sum", "maxnorm_mix"):
        for i, n in enumerate(RED_N):
            rng = np.random.default_rng([103, n])
            a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
            if op == "sqdiff_sum":
                inp = dict(n=n, a=a, b=b, scale=0.5 / n)
                out.append(_entry(op, "n%d" % n, inp, sqdiff_sum, ("drop_tail",) if n > 1 else ()))
            else:
                neg = i % 2 == 0
                if neg:
                    b = (-np.abs(b) - F32(0.25)).astype(F32)      # every entry negative: the maximum is negative
                inp = dict(n=n, a=(a + F32(3)).astype(F32) if n == 1 else a, b=b, wa=0.6, wb=0.4, neg=neg)
                out.append(_entry(op, "n%d neg%d" % (n, neg), inp, maxnorm_mix, ("max_init0",) if neg else ()))
    elif op in ("sigmoid_range_fwd", "sigmoid_range_bwd"):
        for n in SIG_N:
            rng = np.random.default_rng([107, n])
            h = (2 * rng.standard_normal(n)).astype(F32)
            k = min(n, len(SIG_SPECIAL))
            h[:k] = SIG_SPECIAL[:k]
            inp = dict(n=n, h=h, range=np.array([6.0], F32), shift=np.array([-3.0], F32), dpred=(1 + rng.random(n)).astype(F32))
            if op == "sigmoid_range_fwd":
                out.append(_entry(op, "n%d" % n, inp, sigmoid_range_fwd, ("no_shift",)))
            else:
                inp["sigma"] = sigmoid_range_fwd(inp, F64)["sigma"].astype(F32)
                out.append(_entry(op, "n%d" % n, inp, sigmoid_range_bwd, ("no_range",) if n > 1 else (), ("dh_sat",)))
    else:
        raise KeyError(op)
    return out


OPS = ("gram_exact", "gram", "gk_scale", "gk_finish", "gk_scale_momentum", "gk_finish_momentum", "superpixel", "topk_mask",
       "apply_mask", "adam", "adagrad", "ema_update", "ema_update_dev", "scaled_diff", "l1_sign_axpy", "l1_sum_exact", "l1_sum",
       "sqdiff_sum", "maxnorm_mix", "sigmoid_range_fwd", "sigmoid_range_bwd")
_cache = {}


def suite(op):
    """The cases of one operator (computed once per process; treat the arrays as read-only)."""
    if op not in _cache:
        _cache[op] = _suite(op)
    return _cache[op]

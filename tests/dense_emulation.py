"""References of the dense fp32 operators (csrc/dense.hip) for tests/test_gpu_dense.py, and the case tables of that sweep.

Two classes of comparison:

  exact   Sums of products (both GEMMs, ph_outer / ph_outer_bwd, ph_sum, the ADD / MUL / RELU / RELU_BWD / copy ops of ph_eltwise)
          run on integer operands in [-4, 4] stored as float32.  Every product and partial sum is an integer below 2^24, so fp32
          accumulation in any order is exact and the device result must equal the int64 numpy result bit for bit.  The operands
          of the products are non-zero, so one dropped (or doubled) product always changes the result.

  real    Everything with a division, a root or a transcendental runs on seeded real-valued operands.  Each operator is one
          function of (inputs, dt): dt = float64 is the reference of the documented formula, dt = float32 restates the kernel
          (its operation order where the source states one; sums the kernels keep in fp64 stay in fp64).  The tolerance of an
          output array is 4 x the largest error of the float32 restatement against the reference on the same inputs, plus
          FLOOR[operator] x max |ref| for the device's own expf / logf / expm1f / rsqrtf (see FLOOR).

The dropout generator (u01, a splitmix64 finaliser over seed + golden * (index + 1)) is restated on numpy uint64.

tests/test_dense_emulation_cpu.py shows that the tolerances accept the restatement and reject each of a list of injected defects
by a factor of 4 or more."""
import numpy as np

F32, F64 = np.float32, np.float64
ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3
EW_RELU, EW_GATE, EW_RELU_BWD, EW_ADD, EW_ELU_BWD, EW_MUL, EW_COPY = 0, 1, 2, 3, 4, 5, 6      # (6: any other code copies a)
MARGIN = 4.0

# Relative floor per operator for the device's transcendentals (expf, logf, expm1f, rsqrtf), in units of max |ref|: 4 x the
# largest excess of the MI355X result's error over the float32 restatement's error on the cases of this file (the figures are in
# the docstring of tests/test_gpu_dense.py, which prints them on every run).  No table of the ULP bounds of the HIP math functions
# ships with the toolchain, so the floor is the measured one.  An operator with a transcendental and no entry never exceeded its
# restatement's error; the others (fp64 sqrt, correctly rounded sqrtf and division) have no floor by construction.
FLOOR = {"sgemm_act": 4 * 9.1e-8, "bn1d_eval": 4 * 4.2e-8, "bn1d_eval_bwd": 4 * 2.1e-8, "log_softmax": 4 * 4.1e-10,
         "kl_bwd": 4 * 6.5e-8, "kl_rows_fwd": 4 * 1.06e-6, "kl_rows_bwd": 4 * 5.5e-8, "conf_discrepancy": 4 * 4.2e-7}


# ------------------------------------------------------------------------------------------------ the dropout generator
_G, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def u01(seed, idx):
    """dense.hip u01 on a uint64 array of counters: float32 in [0, 1) with 24 random bits."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(_G) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)


def keep_mask(seed, offset, n, p, step=0):
    """The keep mask of ph_dropout (step 0) / ph_dropout_dev: counter = (step << 34) ^ (offset + i), keep = u01 >= p."""
    ctr = (np.uint64(step) << np.uint64(34)) ^ (np.uint64(offset) + np.arange(n, dtype=np.uint64))
    return u01(seed, ctr) >= F32(p)


ALPHA_P = -1.7580993408473766      # -selu_alpha * selu_scale (nn.AlphaDropout)


def dropout(x, keep, p, alpha, dt, defect=None):
    """Forward of nn.Dropout / nn.AlphaDropout given the keep mask."""
    x, p = x.astype(dt), dt(F32(p))
    if not alpha:
        scale = p if defect == "scale_p" else dt(1) - p
        return np.where(keep, x / scale, dt(0))
    ap = dt(F32(ALPHA_P)) if dt is F32 else F64(ALPHA_P)
    a = dt(1) / np.sqrt((dt(1) - p) * (dt(1) + p * ap * ap))
    b = -a * ap * p
    return a * np.where(keep, x, ap) + b


def dropout_bwd(g, keep, p, alpha, dt):
    g, p = g.astype(dt), dt(F32(p))
    if not alpha:
        return np.where(keep, g / (dt(1) - p), dt(0))
    ap = dt(F32(ALPHA_P)) if dt is F32 else F64(ALPHA_P)
    a = dt(1) / np.sqrt((dt(1) - p) * (dt(1) + p * ap * ap))
    return np.where(keep, a * g, dt(0))


# ------------------------------------------------------------------------------------------------ error and tolerance
def err(ref, got):
    """max |got - ref| in float64; a NaN or an infinity where the reference has none counts as an infinite error."""
    ref, got = np.asarray(ref, dtype=F64), np.asarray(got, dtype=F64)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref)
    d = np.where(ref == got, 0.0, d)          # (equal infinities)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


def scale(ref):
    r = np.abs(np.asarray(ref, dtype=F64))
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


def tolerance(op, ref, rest, alts=()):
    """Tolerance of one output array: MARGIN x the restatement's error + the operator's floor.  `alts`: the same array from further
    float32 restatements (other summation orders of a one-block reduction, whose single output is otherwise right or wrong by a
    rounding's chance; the uncontracted form of the BatchNorm forward); the largest error of them all counts."""
    return MARGIN * max([err(ref, rest)] + [err(ref, a) for a in alts]) + FLOOR.get(op, 0.0) * scale(ref)


def entry_tolerance(e, k):
    """Tolerance of output array k of suite entry e."""
    return tolerance(e["op"], e["ref"][k], e["rest"][k], [a[k] for a in e.get("alts", ())])


# ------------------------------------------------------------------------------------------------ exact class: GEMM
FORMS = ("NT", "NN", "TN", "BCAST", "GEN")


def _ints(rng, shape, nonzero):
    if nonzero:
        return (rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.int64)
    return rng.integers(-4, 5, size=shape).astype(np.int64)


def gemm_operands(M, N, K, form, seed, real=False):
    """Logical A [M][K], B [K][N] and their float32 storage with the strides of `form`:
        NT     A [M][K], B stored [N][K]            (ops.py linear_fwd: x @ w^T)
        NN     A [M][K], B [K][N]                   (ops.py dX = dY @ W; memory_new.py coef @ bank)
        TN     A stored [K][M], B [K][N]            (ops.py dW = dY^T @ X)
        BCAST  A one row [K] read by every m (sam = 0), B [K][N]      (ops.py db = 1^T dY)
        GEN    no unit stride: A [M][2K], B [K][2N], every second element (the loaders' other branch)
    Returns (A, B, a_store, b_store, (sam, sak, sbk, sbn)); the gaps of GEN hold 7 (never a legal operand)."""
    rng = np.random.default_rng([seed, M, N, K, FORMS.index(form)])

    def vals(shape):
        return rng.standard_normal(shape).astype(F32) if real else _ints(rng, shape, True)

    if form == "BCAST":
        a_store = vals((K,))
        A = np.broadcast_to(a_store, (M, K))
        sam, sak = 0, 1
    else:
        A = vals((M, K))
        if form == "TN":
            a_store, sam, sak = np.ascontiguousarray(A.T), 1, M
        elif form == "GEN":
            a_store = np.full((M, 2 * K), 7, dtype=A.dtype)
            a_store[:, ::2] = A
            sam, sak = 2 * K, 2
        else:
            a_store, sam, sak = A, K, 1
    B = vals((K, N))
    if form == "NT":
        b_store, sbk, sbn = np.ascontiguousarray(B.T), 1, K
    elif form == "GEN":
        b_store = np.full((K, 2 * N), 7, dtype=B.dtype)
        b_store[:, ::2] = B
        sbk, sbn = 2 * N, 2
    else:
        b_store, sbk, sbn = B, N, 1
    return A, B, a_store.astype(F32), b_store.astype(F32), (sam, sak, sbk, sbn)


def gemm_exact(A, B, bias, prior, act):
    """int64: act(A @ B + bias) + prior, act none or ReLU."""
    v = A.astype(np.int64) @ B.astype(np.int64)
    if bias is not None:
        v = v + bias.astype(np.int64)[None, :]
    if act == ACT_RELU:
        v = np.maximum(v, 0)
    if prior is not None:
        v = v + prior.astype(np.int64)
    assert np.abs(v).max() < 2 ** 24
    return v


def gemm_real(A, B, bias, act, dt, defect=None):
    """act(A @ B + bias) in dt; defect "drop_k": the product of the middle k is left out of every output."""
    A, B = A.astype(dt), B.astype(dt)
    if defect == "drop_k":
        k = np.arange(A.shape[1]) != A.shape[1] // 2
        A, B = A[:, k], B[k, :]
    v = A @ B
    if bias is not None:
        v = v + bias.astype(dt)[None, :]
    if act == ACT_RELU:
        v = np.maximum(v, dt(0))
    elif act == ACT_ELU:
        v = np.where(v > 0, v, np.expm1(np.minimum(v, dt(0))))
    elif act == ACT_SIGMOID:
        v = dt(1) / (dt(1) + np.exp(-v))
    return v


def gemm_kernel(M, N):
    """The kernel ph_sgemm picks (DISPATCH_FAMILIES name)."""
    return "sgemm16" if M * N <= 128 * 128 else "sgemm64"


def _gemm_table():
    rows = []

    def add(M, N, K, form, r):
        rows.append(dict(M=M, N=N, K=K, form=form, bias=r % 2, acc=(r // 2) % 2, pad=3 * ((r // 3) % 2), act=(r // 4) % 2))

    S, KS = (1, 15, 16, 17, 33), (1, 127, 128, 129, 257)
    r = 0
    for i, M in enumerate(S):                       # the 16-wide kernel: 25 rows, every M x N once, K and form cycling
        for j, N in enumerate(S):
            add(M, N, KS[(i + j) % 5], FORMS[(i + 2 * j) % 5], r)
            r += 1
    for q, K in enumerate(KS):                      # ... every K with every form
        for f, form in enumerate(FORMS):
            if (q + f) % 2 == 0:
                add(S[(q + 1) % 5], S[(f + 2) % 5], K, form, r)
                r += 1
    add(128, 128, 129, "NT", 1)                      # either side of the size rule
    add(128, 128, 1, "TN", 6)
    add(129, 128, 33, "NT", 1)
    add(129, 128, 65, "NN", 6)
    KL = (1, 31, 32, 33, 65)
    for a, (M, N) in enumerate(((65, 257), (130, 127))):   # the 64-wide kernel
        for q, K in enumerate(KL):
            for c in range(2):
                add(M, N, K, FORMS[(a + q + 3 * c) % 5], r)
                r += 1
    return rows


GEMM_CASES = _gemm_table()
# ELU and sigmoid in the epilogue, two shapes per kernel: (M, N, K, form, act, bias)
GEMM_REAL_CASES = [(17, 33, 129, "NT", ACT_ELU, 1), (16, 15, 257, "GEN", ACT_SIGMOID, 1), (33, 17, 128, "TN", ACT_SIGMOID, 0),
                   (65, 257, 33, "NT", ACT_ELU, 1), (130, 127, 65, "NN", ACT_SIGMOID, 1), (65, 257, 31, "GEN", ACT_ELU, 0)]


def _splitk_table():
    rows, NS = [], (1, 3, 4, 5, 32, 128)
    for a, (M, N) in enumerate(((1, 1), (8, 128), (65, 63))):
        for b, K in enumerate((33, 100, 4097, 16641)):
            for c in range(2):
                rows.append(dict(M=M, N=N, K=K, nsplit=NS[(a + 2 * b + 3 * c) % 6], form=("NT", "NN")[(a + b + c) % 2],
                                 bias=(a + c) % 2, act=(b + c) % 2, pad=3 * ((a + b) % 2)))
    rows.append(dict(M=8, N=128, K=33, nsplit=128, form="NT", bias=1, act=0, pad=0))      # nsplit far above K / 32
    rows.append(dict(M=65, N=63, K=16641, nsplit=128, form="NT", bias=1, act=0, pad=0))   # the fusion encoder's call
    rows.append(dict(M=65, N=63, K=4097, nsplit=32, form="NN", bias=0, act=0, pad=0))     # the bank GEMM's call
    return rows


SPLITK_CASES = _splitk_table()
SPLITK_REAL_CASES = [(8, 128, 4097, 32, "NT", ACT_ELU), (65, 63, 100, 3, "NN", ACT_SIGMOID)]      # the finish kernel's epilogue


def splitk_slabs(K, nsplit):
    """The number of slabs ph_sgemm_splitk runs for a requested nsplit (slab depth: a multiple of 32)."""
    kchunk = -(-(-(-K // nsplit)) // 32) * 32
    return -(-K // kchunk)


# ------------------------------------------------------------------------------------------------ exact class: the rest
def outer_exact(o1, o2, append_one):
    if append_one:
        o1 = np.concatenate([o1, np.ones((o1.shape[0], 1), o1.dtype)], 1)
        o2 = np.concatenate([o2, np.ones((o2.shape[0], 1), o2.dtype)], 1)
    return (o1[:, :, None] * o2[:, None, :]).reshape(o1.shape[0], -1)


def outer_bwd_exact(g, o1, o2, append_one):
    B, D1, D2 = o1.shape[0], o1.shape[1], o2.shape[1]
    g = g.reshape(B, D1 + append_one, D2 + append_one)
    if append_one:
        o1 = np.concatenate([o1, np.ones((B, 1), o1.dtype)], 1)
        o2 = np.concatenate([o2, np.ones((B, 1), o2.dtype)], 1)
    do1 = np.einsum("bij,bj->bi", g, o2)[:, :D1]
    do2 = np.einsum("bij,bi->bj", g, o1)[:, :D2]
    return do1, do2


def eltwise(a, b, op, dt):
    """ph_eltwise; exact for integer operands and the ops without a transcendental."""
    a, b = a.astype(dt), b.astype(dt)
    if op == EW_RELU:
        return np.where(a > 0, a, dt(0))
    if op == EW_GATE:
        return (dt(1) / (dt(1) + np.exp(-a))) * b
    if op == EW_RELU_BWD:
        return np.where(b > 0, a, dt(0))
    if op == EW_ADD:
        return a + b
    if op == EW_ELU_BWD:
        return np.where(b > 0, a, a * (b + dt(1)))
    if op == EW_MUL:
        return a * b
    return a


EW_EXACT = (EW_RELU, EW_RELU_BWD, EW_ADD, EW_MUL, EW_COPY)
EW_REAL = (EW_GATE, EW_ELU_BWD)
ELTWISE_N = (1, 255, 256, 257, 1000003)
OUTER_CASES = [(B, D1, D2, ap) for (D1, D2) in ((5, 7), (32, 32), (1, 129)) for B in (1, 3) for ap in (0, 1)]
SUM_N = (1, 63, 64, 65, 255, 256, 257, 5000)


def gate_bwd(g, z, h, dt):
    g, z, h = g.astype(dt), z.astype(dt), h.astype(dt)
    s = dt(1) / (dt(1) + np.exp(-z))
    return {"dz": g * h * s * (dt(1) - s), "dh": g * s}


# ------------------------------------------------------------------------------------------------ BatchNorm1d
BN_EPS, BN_MOM = 1e-5, 0.1


def _bn_table():
    rows, Bs, Cs = [], (1, 2, 15, 16, 17, 33), (1, 15, 16, 17, 130)
    r = 0
    for i, B in enumerate(Bs):
        for j, C in enumerate(Cs):
            if (i + j) % 2 == 0 or C == 130 or B == 33:
                rows.append(dict(B=B, C=C, relu=r % 2, running=(r // 2) % 2 == 0, dparams=(r // 3) % 2 == 0))
                r += 1
    return rows


BN_CASES = _bn_table()


def bn_inputs(case):
    """x [B][C]; where C >= 2, column 0 is constant (variance 0) and column 1 has mean 1000 and unit spread."""
    B, C = case["B"], case["C"]
    rng = np.random.default_rng([11, B, C, case["relu"]])
    x = rng.standard_normal((B, C)).astype(F32)
    if C >= 2:
        x[:, 0] = F32(0.3)
        x[:, 1] += F32(1000.0)
    return dict(x=x, gamma=(1.0 + 0.5 * rng.standard_normal(C)).astype(F32), beta=rng.standard_normal(C).astype(F32),
                rm=rng.standard_normal(C).astype(F32), rv=(0.5 + rng.random(C)).astype(F32), nbt=np.int64(3),
                g=rng.standard_normal((B, C)).astype(F32))


def bn_split(out):
    """Takes the mean-1000 column (column 1, where C >= 2) of the [B][C] and [C] outputs out as arrays of their own ("y@1000"): its
    intrinsic error, u |m| |sc|, is a thousand times the other columns' and would set the tolerance of the whole array."""
    res = {}
    for k, v in out.items():
        if v.shape[-1] >= 2:
            res[k] = np.delete(v, 1, axis=-1)
            res[k + "@1000"] = v[..., 1:2]
        else:
            res[k] = v
    return res


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64, the sum is rounded once (to float64 and then to
    float32: a double rounding that differs from a true fma in about one case in 2^29)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def bn_fwd(inp, relu, dt, defect=None, contract=True):
    """nn.BatchNorm1d in training mode.  float64: the two-pass formula.  float32: bn1d_fwd_kernel - fp64 sums of x and x^2,
    var = s2 / B - m^2 clamped at 0, y = x * sc + (beta - m * sc) with sc = gamma * invstd, all of that in float32.  The source
    writes the two multiply-adds as `a * b + c`, which hipcc contracts to one fma each by default (-ffp-contract=fast): `contract`
    restates them so; without it each product is rounded first.  The error is u |m| |sc| either way, but it is the same in every
    row of a column, so the two forms are two draws of it, not one draw and its noise: the tolerance takes both (suite: alts).
    defect "drop_row": the sums leave out the last batch row; "biased": the running variance is not unbiased."""
    x, gamma, beta = inp["x"], inp["gamma"], inp["beta"]
    B = x.shape[0]
    xd = x.astype(F64)
    rows = xd[:-1] if defect == "drop_row" else xd
    eps, mom = F64(F32(BN_EPS)), dt(F32(BN_MOM))
    m = rows.sum(0) / B
    if dt is F64:
        var = ((rows - m) ** 2).sum(0) / B
        istd = 1.0 / np.sqrt(var + eps)
        y = (xd - m) * istd * gamma.astype(F64) + beta.astype(F64)
    else:
        var = np.maximum((rows * rows).sum(0) / B - m * m, 0.0)
        istd = (1.0 / np.sqrt(var + eps)).astype(F32)
        sc = gamma * istd
        if contract:
            y = _fma(x, sc[None, :], _fma(-m.astype(F32), sc, beta)[None, :])
        else:
            y = x * sc + (beta - m.astype(F32) * sc)
    if relu:
        y = np.maximum(y, dt(0))
    unb = var * B / (B - 1.0) if (B > 1 and defect != "biased") else var
    out = {"mean": m.astype(dt), "invstd": istd.astype(dt), "y": y}
    out["running_mean"] = (dt(1) - mom) * inp["rm"].astype(dt) + mom * m.astype(dt)
    out["running_var"] = (dt(1) - mom) * inp["rv"].astype(dt) + mom * unb.astype(dt)
    return out


def bn_eval(inp, relu, dt):
    x, eps = inp["x"].astype(dt), dt(F32(BN_EPS))
    y = (x - inp["rm"].astype(dt)) * (dt(1) / np.sqrt(inp["rv"].astype(dt) + eps)) * inp["gamma"].astype(dt) + inp["beta"].astype(dt)
    return {"y": np.maximum(y, dt(0)) if relu else y}


def bn_eval_bwd(inp, y, relu, dt):
    s = inp["gamma"].astype(dt) * (dt(1) / np.sqrt(inp["rv"].astype(dt) + dt(F32(BN_EPS))))
    dx = inp["g"].astype(dt) * s
    return {"dx": np.where(y > 0, dx, dt(0)) if relu else dx}


def bn_bwd_autograd(inp, relu):
    """float64 autograd of y = relu?(batch_norm(x)): dx, dgamma, dbeta for the upstream gradient inp["g"]."""
    import torch
    x = torch.from_numpy(inp["x"].astype(F64)).requires_grad_()
    gamma = torch.from_numpy(inp["gamma"].astype(F64)).requires_grad_()
    beta = torch.from_numpy(inp["beta"].astype(F64)).requires_grad_()
    m = x.mean(0)
    var = ((x - m) ** 2).mean(0)
    y = (x - m) / torch.sqrt(var + float(F32(BN_EPS))) * gamma + beta
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(inp["g"].astype(F64)))
    return {"dx": x.grad.numpy(), "dgamma": gamma.grad.numpy(), "dbeta": beta.grad.numpy()}


def bn_bwd(inp, fwd, relu, defect=None):
    """bn1d_bwd_kernel in float32 (fp64 sums) from the float32 mean / invstd / y of the forward (`fwd`: float32 arrays).
    defect "mask_x": the ReLU mask is taken from x instead of y."""
    x, g, gamma = inp["x"], inp["g"], inp["gamma"]
    mu, istd, y = fwd["mean"].astype(F32), fwd["invstd"].astype(F32), fwd["y"].astype(F32)
    B = x.shape[0]
    dz = np.where((x if defect == "mask_x" else y) > 0, g, F32(0)) if relu else g
    xh = (x - mu) * istd
    s1 = dz.astype(F64).sum(0)
    s2 = (dz.astype(F64) * xh.astype(F64)).sum(0)
    c1, c2, sc = (s1 / B).astype(F32), (s2 / B).astype(F32), gamma * istd
    return {"dx": sc * (dz - c1 - xh * c2), "dgamma": s2.astype(F32), "dbeta": s1.astype(F32)}


# ------------------------------------------------------------------------------------------------ row operators [B][C <= 64]
def _row_table():
    rows, Bs, Cs = [], (1, 63, 64, 65, 130), (2, 3, 64)
    for i, B in enumerate(Bs):
        for j, C in enumerate(Cs):
            if (i + j) % 2 == 0 or B == 130:
                rows.append(dict(B=B, C=C, T=(1.0, 4.0)[(i + j // 2) % 2]))
    rows.append(dict(B=65, C=3, T=4.0))
    return rows


ROW_CASES = _row_table()
SOFTMAX_EXTRA = [dict(B=65, C=1, T=1.0), dict(B=1, C=1, T=1.0)]            # C = 1 for the softmax alone
BLOCK_EXTRA = [dict(B=257, C=3, T=4.0), dict(B=600, C=64, T=1.0), dict(B=600, C=2, T=4.0), dict(B=257, C=64, T=1.0)]   # single-block reductions
SPREAD = 1e4


def row_inputs(case, wide=True):
    """Student / teacher logits [B][C], labels, upstream gradients.  Every fourth row (from row 1) is `wide`: one logit 1e4 above
    the others, so that exp(x - max) underflows to 0 everywhere else and exp(x) without the max subtraction overflows."""
    B, C = case["B"], case["C"]
    rng = np.random.default_rng([23, B, C, int(case["T"])])
    d = {k: (2.0 * rng.standard_normal((B, C))).astype(F32) for k in ("ys", "yt", "yt2")}
    if wide and C > 1:
        for k, shift in (("ys", 0), ("yt", 1), ("yt2", 2)):
            r = wide_rows(B)
            d[k][r, (r + shift) % C] += F32(SPREAD)
    d["grade"] = rng.integers(0, C, size=B).astype(np.int64)
    d["g"] = rng.standard_normal((B, C)).astype(F32)
    d["grow"] = rng.standard_normal(B).astype(F32)
    d["gs"] = np.array([0.75], dtype=F32) + rng.random(1).astype(F32)
    d["wide"] = wide and C > 1 and B > 1
    return d


def wide_rows(B):
    return np.arange(1, B, 4)


def row_split(out, inp):
    """Takes the wide rows of the per-row outputs out as arrays of their own ("y@wide"): their values, and so their rounding
    errors, are 1e4 times the other rows' and would set the tolerance of the whole array."""
    if not inp["wide"]:
        return out
    B, res = inp["B"], {}
    for k, v in out.items():
        if v.shape[0] == B:
            res[k] = np.delete(v, wide_rows(B), axis=0)
            res[k + "@wide"] = v[wide_rows(B)]
        else:
            res[k] = v
    return res


def _seqsum(a):
    """Sum over the last axis, one element after the other (the kernels' `for c` loops)."""
    s = np.zeros(a.shape[:-1], dtype=a.dtype)
    for c in range(a.shape[-1]):
        s = s + a[..., c]
    return s


ORDERS = ("seq", "rev", "pair")      # further float32 summation orders of a one-block reduction (tolerance: see `tolerance`)


def block_sum(v, dt, threads=256, order="kernel"):
    """block_sum of per-row values as the one-block kernels do: thread t adds rows t, t + 256, ..; a 64-lane xor butterfly;
    the waves' sums one after the other.  float64: a plain sum.  order "seq" / "rev" / "pair": one after the other, the same
    backwards, numpy's pairwise sum."""
    v = np.asarray(v, dtype=dt)
    if dt is F64:
        return F64(v.sum())
    if order == "pair":
        return v.sum(dtype=dt)
    if order in ("seq", "rev"):
        return (v[::-1] if order == "rev" else v).cumsum(dtype=dt)[-1]
    p = np.zeros(threads, dtype=dt)
    for s in range(0, len(v), threads):
        c = v[s:s + threads]
        p[:len(c)] = p[:len(c)] + c
    w = p.reshape(-1, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    t = dt(0)
    for i in range(w.shape[0]):
        t = t + w[i, 0]
    return t


def _lse(x, nomax=False):
    """(max, sum exp(x - max)) of each row; nomax: the defect of leaving the max subtraction out."""
    mx = np.zeros(x.shape[0], dtype=x.dtype) if nomax else x.max(1)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - mx[:, None])
    return mx, e, _seqsum(e)


def log_softmax(x, dt, defect=None):
    x = x.astype(dt)
    mx, _, s = _lse(x, defect == "nomax")
    with np.errstate(invalid="ignore"):
        return {"y": x - (mx + np.log(s))[:, None]}


def log_softmax_bwd(g, y, dt):
    g, y = g.astype(dt), y.astype(dt)
    return {"dx": g - np.exp(y) * _seqsum(g)[:, None]}


def nll_fwd(pred, grade, inv_bnorm, dt, order="kernel"):
    v = -pred.astype(dt)[np.arange(len(grade)), grade]
    return {"loss": np.array([block_sum(v, dt, order=order) * dt(F32(inv_bnorm))])}


def nll_bwd(gs, grade, C, inv_bnorm, dt):
    d = np.zeros((len(grade), C), dtype=dt)
    d[np.arange(len(grade)), grade] = -gs.astype(dt)[0] * dt(F32(inv_bnorm))
    return {"dpred": d}


def _kl_parts(ys, yt, T, dt, defect):
    T = dt(F32(T))
    a, b = (ys.astype(dt), yt.astype(dt)) if defect == "no_T" else (ys.astype(dt) / T, yt.astype(dt) / T)
    nomax = defect == "nomax"
    ms, es, ss = _lse(a, nomax)
    mt, et, st = _lse(b, nomax)
    return T, a, b, (ms, es, ss), (mt, et, st)


def kl_rows(ys, yt, T, dt, defect=None):
    """Per-row sum_c p_t (log p_t - log p_s) of the temperature softmaxes (before the T^2 factor)."""
    T, a, b, (ms, _, ss), (mt, _, st) = _kl_parts(ys, yt, T, dt, defect)
    with np.errstate(invalid="ignore", over="ignore"):
        lps, lpt = a - (ms + np.log(ss))[:, None], b - (mt + np.log(st))[:, None]
        pt = np.exp(lpt)
        term = np.where(pt > 0, pt * (lpt - lps), dt(0))
    return _seqsum(term), T


def kl_fwd(ys, yt, T, inv_bnorm, dt, defect=None, order="kernel"):
    r, T = kl_rows(ys, yt, T, dt, defect)
    return {"loss": np.array([block_sum(r, dt, order=order) * T * T * dt(F32(inv_bnorm))])}


def kl_rows_fwd(ys, yt, T, dt, defect=None):
    r, T = kl_rows(ys, yt, T, dt, defect)
    return {"sample_loss": r * T * T}


def _kl_grad(ys, yt, T, dt, defect):
    T, _, _, (_, es, ss), (_, et, st) = _kl_parts(ys, yt, T, dt, defect)
    with np.errstate(invalid="ignore", over="ignore"):
        return T, es / ss[:, None] - et / st[:, None]


def kl_bwd(gs, ys, yt, T, inv_bnorm, dt, defect=None):
    T, d = _kl_grad(ys, yt, T, dt, defect)
    return {"dys": (gs.astype(dt)[0] * T * dt(F32(inv_bnorm))) * d}


def kl_rows_bwd(g, ys, yt, T, dt, defect=None):
    T, d = _kl_grad(ys, yt, T, dt, defect)
    return {"dys": (g.astype(dt) * T)[:, None] * d}


def conf_discrepancy(ls, lt, gt, cap, dt):
    """min(max(conf_t - conf_s, 0), cap), conf = log p_gt - log max_{c != gt} p_c; fmax / fmin drop a NaN as fmaxf / fminf do."""
    conf = []
    rows = np.arange(len(gt))
    with np.errstate(divide="ignore", invalid="ignore"):
        for y in (ls.astype(dt), lt.astype(dt)):
            _, e, s = _lse(y)
            p = e / s[:, None]
            other = p.copy()
            other[rows, gt] = dt(0)
            conf.append(np.log(p[rows, gt]) - np.log(other.max(1)))
        return {"out": np.fmin(np.fmax(conf[1] - conf[0], dt(0)), dt(F32(cap)))}


def conf_inputs(case):
    """The logits of row_inputs with the label on the student's argmax in even rows and off it in odd rows.  With CONF_CAPS[0]
    the cap is reached in some rows (every wide row whose difference is +inf among them) and not in others; CONF_CAPS[1] is
    never reached by a finite difference."""
    d = row_inputs(case)
    B, C = case["B"], case["C"]
    am = d["ys"].argmax(1)
    d["grade"] = np.where(np.arange(B) % 2 == 0, am, (am + 1) % C).astype(np.int64)
    return d


CONF_CAPS = (1.0, 1e9)


# ------------------------------------------------------------------------------------------------ L2 normalise rows
L2_CASES = [(B, D) for B in (1, 3, 4, 5, 9) for D in (1, 63, 64, 65, 128, 200)]


def _wave_rowsum(a, dt):
    """Row sums as a 64-lane wave takes them: lane l adds elements l, l + 64, .., then the xor butterfly."""
    if dt is F64:
        return a.sum(1)
    B, D = a.shape
    pad = np.zeros((B, -(-D // 64) * 64), dtype=dt)
    pad[:, :D] = a
    p = np.zeros((B, 64), dtype=dt)
    for j in range(pad.shape[1] // 64):
        p = p + pad[:, 64 * j:64 * j + 64]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ o]
    return p[:, 0]


def l2_inputs(B, D):
    rng = np.random.default_rng([31, B, D])
    return dict(x=rng.standard_normal((B, D)).astype(F32), g=rng.standard_normal((B, D)).astype(F32),
                r=(0.5 + rng.random(B)).astype(F32))


def l2norm_fwd(x, dt):
    x = x.astype(dt)
    n = np.sqrt(_wave_rowsum(x * x, dt))
    return {"y": x / n[:, None], "nrm": n}


def l2norm_bwd(g, y, nrm, dt):
    g, y, nrm = g.astype(dt), y.astype(dt), nrm.astype(dt)
    s = _wave_rowsum(g * y, dt)
    return {"dx": (g - y * s[:, None]) * (dt(1) / nrm)[:, None]}


def row_invnorm_scale(x, eps, dt):
    x = x.astype(dt)
    r = dt(1) / (np.sqrt(_wave_rowsum(x * x, dt)) + dt(F32(eps)))
    return {"y": x * r[:, None], "inv": r}


def row_scale(x, r, dt):
    return {"y": x.astype(dt) * r.astype(dt)[:, None]}


# ------------------------------------------------------------------------------------------------ the real-valued suite
def _entry(op, name, inp, fn, defects=(), orders=()):
    """One case of one operator: inputs, float64 reference, float32 restatement, the restatement with each defect and (one-block
    reductions) in each further summation order."""
    return dict(op=op, name=name, inp=inp, ref=fn(F64, None), rest=fn(F32, None), defects={d: fn(F32, d) for d in defects},
                alts=[fn(F32, None, order=o) for o in orders])


def _suite(op):
    out = []
    if op in ("sgemm_act", "splitk_act"):
        cases = [(M, N, K, 0, f, a, b) for (M, N, K, f, a, b) in GEMM_REAL_CASES] if op == "sgemm_act" else \
                [(M, N, K, ns, f, a, 1) for (M, N, K, ns, f, a) in SPLITK_REAL_CASES]
        for (M, N, K, ns, form, act, hb) in cases:
            A, B, a_s, b_s, st = gemm_operands(M, N, K, form, 5, real=True)
            # (operands of unit variance over K: pre-activations of a few units, the range where ELU and the sigmoid bend)
            b_s = (b_s / np.sqrt(K)).astype(F32)
            B = b_s.T if form == "NT" else (b_s[:, ::2] if form == "GEN" else b_s)
            bias = np.random.default_rng([6, M, N]).standard_normal(N).astype(F32) if hb else None
            inp = dict(M=M, N=N, K=K, nsplit=ns, form=form, act=act, a=a_s, b=b_s, bias=bias, strides=st)
            out.append(_entry(op, f"{M}x{N}x{K} {form} act{act}", inp,
                              lambda dt, d, A=A, B=B, bias=bias, act=act: {"c": gemm_real(A, B, bias, act, dt, d)}, ("drop_k",)))
    elif op in ("bn1d_fwd", "bn1d_eval", "bn1d_bwd", "bn1d_eval_bwd"):
        for case in BN_CASES:
            inp = dict(bn_inputs(case), **case)
            relu, name = case["relu"], "B%d C%d relu%d" % (case["B"], case["C"], case["relu"])
            if op == "bn1d_fwd":
                dfs = ("drop_row", "biased") if case["B"] > 1 else ()
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, relu=relu, order="kernel":
                                  bn_split(bn_fwd(inp, relu, dt, d, order != "unfused")), dfs, ("unfused",)))
            elif op == "bn1d_eval":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, relu=relu: bn_split(bn_eval(inp, relu, dt))))
            elif op == "bn1d_eval_bwd":
                y = bn_eval(inp, relu, F64)["y"].astype(F32)
                inp["y"] = y
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, relu=relu, y=y: bn_split(bn_eval_bwd(inp, y, relu, dt))))
            else:
                fwd = {k: v.astype(F32) for k, v in bn_fwd(inp, relu, F64).items()}
                inp.update(mean=fwd["mean"], invstd=fwd["invstd"], y=fwd["y"])
                ref = bn_split(bn_bwd_autograd(inp, relu))
                e = dict(op=op, name=name, inp=inp, ref=ref, rest=bn_split(bn_bwd(inp, fwd, relu)), defects={})
                if relu and case["B"] > 1:
                    e["defects"]["mask_x"] = bn_split(bn_bwd(inp, fwd, relu, "mask_x"))
                out.append(e)
    elif op in ("log_softmax", "log_softmax_bwd", "nll_fwd", "nll_bwd", "kl_fwd", "kl_bwd", "kl_rows_fwd", "kl_rows_bwd",
                "conf_discrepancy"):
        cases = list(ROW_CASES)
        if op == "log_softmax":
            cases += SOFTMAX_EXTRA
        if op in ("nll_fwd", "kl_fwd"):
            cases += BLOCK_EXTRA
        for case in cases:
            B, C, T = case["B"], case["C"], case["T"]
            inp = dict(conf_inputs(case) if op == "conf_discrepancy" else row_inputs(case), **case)
            inv = 1.0 / B
            inp["inv_bnorm"] = inv
            name = "B%d C%d T%g" % (B, C, T)
            ys, yt = inp["ys"], inp["yt"]
            wide = ("nomax",) if inp["wide"] else ()
            kdef = wide + (("no_T",) if T != 1.0 else ())
            if op == "log_softmax":
                out.append(_entry(op, name, inp, lambda dt, d, ys=ys, inp=inp: row_split(log_softmax(ys, dt, d), inp), wide))
                continue
            pred = log_softmax(ys, F64)["y"].astype(F32)
            inp["pred"] = pred
            if op == "log_softmax_bwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, pred=pred: row_split(log_softmax_bwd(inp["g"], pred, dt), inp)))
            elif op == "nll_fwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, pred=pred, inv=inv, order="kernel":
                                  nll_fwd(pred, inp["grade"], inv, dt, order), (), ORDERS))
            elif op == "nll_bwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, C=C, inv=inv: row_split(nll_bwd(inp["gs"], inp["grade"], C, inv, dt), inp)))
            elif op == "kl_fwd":
                out.append(_entry(op, name, inp, lambda dt, d, ys=ys, yt=yt, T=T, inv=inv, order="kernel":
                                  kl_fwd(ys, yt, T, inv, dt, d, order), kdef, ORDERS))
            elif op == "kl_bwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, ys=ys, yt=yt, T=T, inv=inv:
                                  row_split(kl_bwd(inp["gs"], ys, yt, T, inv, dt, d), inp), kdef))
            elif op == "kl_rows_fwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, ys=ys, yt=yt, T=T: row_split(kl_rows_fwd(ys, yt, T, dt, d), inp), kdef))
            elif op == "kl_rows_bwd":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, ys=ys, yt=yt, T=T:
                                  row_split(kl_rows_bwd(inp["grow"], ys, yt, T, dt, d), inp), kdef))
            else:
                for cap in CONF_CAPS:
                    i2 = dict(inp, cap=cap)
                    out.append(_entry(op, name + " cap%g" % cap, i2, lambda dt, d, i2=i2, cap=cap:
                                      row_split(conf_discrepancy(i2["ys"], i2["yt"], i2["grade"], cap, dt), i2)))
    elif op in ("l2norm_fwd", "l2norm_bwd", "row_invnorm_scale", "row_scale"):
        for (B, D) in L2_CASES:
            inp = dict(l2_inputs(B, D), B=B, D=D, eps=1e-8 if D % 2 else 0.25)
            name, x = "B%d D%d" % (B, D), inp["x"]
            if op == "l2norm_fwd":
                out.append(_entry(op, name, inp, lambda dt, d, x=x: l2norm_fwd(x, dt)))
            elif op == "l2norm_bwd":
                f = {k: v.astype(F32) for k, v in l2norm_fwd(x, F64).items()}
                inp.update(y=f["y"], nrm=f["nrm"])
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp: l2norm_bwd(inp["g"], inp["y"], inp["nrm"], dt)))
            elif op == "row_invnorm_scale":
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, x=x: row_invnorm_scale(x, inp["eps"], dt)))
            else:
                out.append(_entry(op, name, inp, lambda dt, d, inp=inp, x=x: row_scale(x, inp["r"], dt)))
    elif op in ("eltwise_real", "gate_bwd"):
        for n in ELTWISE_N:
            rng = np.random.default_rng([41, n])
            inp = dict(n=n, a=(2 * rng.standard_normal(n)).astype(F32), b=(2 * rng.standard_normal(n)).astype(F32),
                       g=rng.standard_normal(n).astype(F32))
            if op == "gate_bwd":
                out.append(_entry(op, "n%d" % n, inp, lambda dt, d, inp=inp: gate_bwd(inp["g"], inp["a"], inp["b"], dt)))
            else:
                for code in EW_REAL:
                    i2 = dict(inp, code=code)
                    if code == EW_ELU_BWD:      # b = ELU(x): above -1
                        i2["b"] = np.where(inp["b"] > 0, inp["b"], np.expm1(np.minimum(inp["b"], 0))).astype(F32)
                    out.append(_entry(op, "n%d op%d" % (n, code), i2, lambda dt, d, i2=i2, code=code:
                                      {"o": eltwise(i2["a"], i2["b"], code, dt)}))
    elif op == "dropout":
        n, x = 100003, np.random.default_rng([51]).standard_normal(100003).astype(F32)
        for (p, seed, offset, step) in DROPOUT_CASES:
            keep = keep_mask(seed, offset, n, p, step)
            for alpha in (0, 1):
                inp = dict(n=n, x=x, p=p, seed=seed, offset=offset, step=step, alpha=alpha, keep=keep)
                out.append(_entry(op, "p%g seed%d off%d step%d alpha%d" % (p, seed % 1000, offset, step, alpha), inp,
                                  lambda dt, d, inp=inp: {"y": dropout(inp["x"], inp["keep"], inp["p"], inp["alpha"], dt, d),
                                                          "dg": dropout_bwd(inp["x"], inp["keep"], inp["p"], inp["alpha"], dt)},
                                  ("scale_p",) if (p != 0.5 and not alpha) else ()))
    else:
        raise KeyError(op)
    return out


DROPOUT_CASES = [(0.25, 0x1234567, 0, 0), (0.5, 0xDEADBEEFCAFE, 0, 0), (0.25, 0xDEADBEEFCAFE, 77777, 5), (0.5, 0x1234567, 1 << 33, 5)]
REAL_OPS = ("sgemm_act", "splitk_act", "bn1d_fwd", "bn1d_eval", "bn1d_bwd", "bn1d_eval_bwd", "log_softmax", "log_softmax_bwd",
            "nll_fwd", "nll_bwd", "kl_fwd", "kl_bwd", "kl_rows_fwd", "kl_rows_bwd", "conf_discrepancy", "l2norm_fwd", "l2norm_bwd",
            "row_invnorm_scale", "row_scale", "eltwise_real", "gate_bwd", "dropout")
_cache = {}


def suite(op):
    """The cases of one real-valued operator (computed once per process; treat the arrays as read-only)."""
    if op not in _cache:
        _cache[op] = _suite(op)
    return _cache[op]

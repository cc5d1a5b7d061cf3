"""References of the relational and survival loss kernels - PKT, the one-workgroup RKD and Cox (csrc/zoo.hip), the anchor-partitioned
tiled RKD (csrc/zoo_rkd.hip) - for tests/test_gpu_zoo_sweep.py, the case tables of that sweep and its tolerance rule.  The layout is
that of tests/bn_emulation.py.

Every operator has two statements, both on the CPU in torch, both returning {"loss": [1], "dx": [B, D]} as numpy arrays:

  *_ref   float64, from the definition and differentiated by autograd: RKD.py:15-58 restricted to an anchor range
          (`rkd_part_torch`, the contract of a part; the whole batch is the range [0, B)), PKT.py:17-46, and the Cox negative partial
          log-likelihood of utils.py:361-376.  tests/test_zoo_emulation_cpu.py pins them against the committed goldens of the
          reference's own classes.
  *_f32   float32, the kernel's own algebra with its closed-form gradient: zoo.hip's RKD takes the distances from the Gram matrix
          (g_ii + g_jj - 2 g_ij) and normalises each difference vector by its own norm; zoo_rkd.hip sums the squared differences
          and takes every norm from that matrix; PKT normalises with / (norm + eps), uses (S + 1) / 2, row-normalises and carries
          eps = 1e-7 inside the log; Cox compares the survival times with >= (ties belong to the risk set).  `defect=` injects one
          of the mistakes listed in DEFECTS into the restatement.

Degenerate conventions (stated here once; the kernels and both statements follow them):
  * coinciding student rows carry no gradient through their zero difference vector (its unit vector is 0, and the gradient of that
    entry is dropped instead of being divided by the clamp 1e-12) or through their clamped distance (sqrt(max(d^2, 1e-12)) is a
    constant where the clamp is active);
  * an all-zero PKT row i has k = 0 in dx_i = ds_i / (n_i + eps) - x_i k: no gradient through its norm.

Tolerance rule (tolerance()): the device's error against float64 is at most MARGIN (4) x the float32 restatement's error against
float64 on the same inputs, plus FLOOR[(operator, output)] x max |ref|; both errors are max-norm.  The loss and the gradient are
judged separately.  The floors are 4 x the largest excess of the MI355X over the restatement (a kernel's serial chain of up to 4096
terms against torch's blocked sums, fma contraction, the device's sqrtf / logf / expf / division); the measured figures are in the
docstring of tests/test_gpu_zoo_sweep.py, which prints them on every run.
A case whose reference is identically zero (RKD with two rows, Cox with one, PKT at D = 1) has no max |ref|; its absolute allowance is
reasoned at ZERO_REF.

Inputs are randn(..).relu_() as the goldens' (|randn| at D = 1, where a ReLU leaves half of the rows zero); the seeds in the tables
are the first ones for which no row of the student or of the teacher is all zero."""
import numpy as np
import torch

from tests.dense_emulation import err, scale      # noqa: F401  (part of this module's interface)

F32, F64 = torch.float32, torch.float64
MARGIN = 4.0
OK, EINVAL = 0, -22
W_D, W_A = 25.0, 50.0                              # RKDLoss's defaults (RKD.py:8)
RKD_EPS = 1e-12
PKT_EPS = float(np.float32(1e-7))                  # the kernels' 1e-7f
RKD_ONE_WG_LDS = 150 * 1024                        # bytes of LDS the one-workgroup angle kernel may ask for

# (operator, "loss" | "dx") -> floor in units of max |ref|: 4 x the measured excess of the device's error over the restatement's
# (the cases are named in the docstring of tests/test_gpu_zoo_sweep.py).
FLOOR = {("rkd_part", "loss"): 4 * 6.57e-8, ("rkd_part", "dx"): 4 * 3.35e-7, ("rkd", "loss"): 4 * 3.43e-7, ("rkd", "dx"): 4 * 5.88e-7,
         ("pkt", "loss"): 4 * 1.52e-6, ("pkt", "dx"): 4 * 3.79e-7, ("cox", "loss"): 4 * 5.82e-8, ("cox", "dx"): 4 * 1.18e-6}

DEFECTS = {
    "rkd_part": {"drop_j_tail": "the last partial row tile j dropped", "drop_k_tail": "the last partial row tile k dropped",
                 "drop_de_cols": "the columns past the last whole 64-chunk dropped from dE",
                 "skip_65th_anchor": "the 65th anchor of a part skipped", "no_anchor_self": "the anchor's own -sum_j dv_ij missing",
                 "corr_once": "2 corr taken as corr in the part's distance gradient",
                 "part_mean": "the mean distance taken over the part's rows only"},
    "rkd": {"rows_ge16": "rows >= 16 never revisited in the j = wave; j += 16 loop", "cols_ge64": "columns >= 64 dropped from g[q]"},
    "pkt": {"rowsum_64": "the row sums stopping at the last multiple of 64", "finish_16rows": "pkt_finish visiting only the first 16 rows",
            "no_proj": "the -x_i (x_i . ds_i) term missing"},
    "cox": {"gt": "> for >=", "rows_ge1024": "rows >= 1024 left out of the outer loop"},
}


def tolerance(op, out, ref, rest, absolute=0.0):
    return MARGIN * err(ref, rest) + FLOOR.get((op, "dx" if out == "dx_live" else out), 0.0) * scale(ref) + absolute


def rkd_one_wg_fits(B, D):
    """The host rule of ph_rkd_one_workgroup_fits: E [B][D + 1], A [B][B + 1] and the B norms in at most 150 KiB of LDS."""
    return 2 <= B <= 128 and 1 <= D <= 512 and (B * (D + 1) + B * (B + 1) + B) * 4 <= RKD_ONE_WG_LDS


# ------------------------------------------------------------------------------------------------ inputs
def rows(seed, B, D):
    """(f_s, f_t) float32 [B, D]: randn.relu_() (|randn| at D = 1), no all-zero row (asserted: the seed tables are chosen for it)."""
    g = torch.Generator().manual_seed(seed)
    f_s, f_t = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    for f in (f_s, f_t):
        f.abs_() if D == 1 else f.relu_()
        assert bool((f.abs().sum(1) > 0).all()), ("an all-zero row", seed, B, D)
    return f_s, f_t


def first_seed(B, D, start=0, tries=100000):
    """The first seed >= start for which rows() has no all-zero row (how the tables below were filled)."""
    for s in range(start, start + tries):
        try:
            rows(s, B, D)
            return s
        except AssertionError:
            continue
    raise ValueError((B, D))


def cox_inputs(seed, B, censored=False):
    """theta ~ N(0, 1); survival times from about B / 3 distinct values (ties everywhere); about 60 % of the rows with an event."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(B, generator=g)
    t = torch.randint(0, max(B // 3, 1), (B,), generator=g).float() * 0.5 + 1.0
    c = (torch.rand(B, generator=g) < 0.6).float()
    if censored:
        c.zero_()
    return theta, t, c


def _np(loss, dx):
    return {"loss": loss.detach().reshape(1).double().numpy(), "dx": dx.detach().double().numpy()}


def _huber(z):
    az = z.abs()
    return torch.where(az < 1, 0.5 * z * z, az - 0.5)


# ------------------------------------------------------------------------------------------------ RKD: the contract of a part
def rkd_part_torch(g_s, g_t, anchor_lo, n_anchors, w_d, w_a):
    """The contract of ph_rkd_loss_grad_part in torch (RKD.py:15-58 restricted to an anchor range): the rows
    [lo, lo + n) of the distance matrix and the anchors [lo, lo + n) of the angle tensor, with the mean distances and the
    normalisers Bg^2 / Bg^3 of ALL rows, in the dtype of its inputs.  Returns (loss_part [1], dx_part [Bg, D]).  A zero difference
    vector has the unit vector 0 and passes no gradient (the module's convention; F.normalize would divide it by the clamp)."""
    def pdist(e):
        sq = (e[:, None, :] - e[None, :, :]).pow(2).sum(2)
        d = sq.clamp(min=RKD_EPS).sqrt()
        return d * (1.0 - torch.eye(e.shape[0], dtype=e.dtype))

    def angles(e, sl):
        v = e[None, :, :] - e[sl, None, :]                       # [n, Bg, D]: v[a, j] = x_j - x_(lo + a)
        n = v.norm(dim=2, keepdim=True)
        u = v / n.clamp(min=RKD_EPS) * (n > RKD_EPS).to(e.dtype)
        return torch.bmm(u, u.transpose(1, 2))

    huber = torch.nn.functional.smooth_l1_loss
    x = g_s.detach().clone().requires_grad_(True)
    t = g_t.detach()
    Bg = x.shape[0]
    sl = slice(anchor_lo, anchor_lo + n_anchors)
    with torch.no_grad():
        t_d = pdist(t)
        t_d = t_d / t_d[t_d > 0].mean()
        t_a = angles(t, sl)
    with torch.enable_grad():                 # (grad mode is off inside an autograd Function's forward)
        d = pdist(x)
        d = d / d[d > 0].mean()
        loss_d = huber(d[sl], t_d[sl], reduction="sum") / float(Bg * Bg)
        loss_a = huber(angles(x, sl), t_a, reduction="sum") / float(Bg) ** 3
        loss = w_d * loss_d + w_a * loss_a
        dx, = torch.autograd.grad(loss, x)
    return loss.detach().reshape(1), dx


def rkd_part_ref(f_s, f_t, lo, na, w_d=W_D, w_a=W_A):
    return _np(*rkd_part_torch(torch.as_tensor(f_s).double(), torch.as_tensor(f_t).double(), lo, na, w_d, w_a))


def rkd_ref(f_s, f_t, w_d=W_D, w_a=W_A):
    return rkd_part_ref(f_s, f_t, 0, int(f_s.shape[0]), w_d, w_a)


def _tail(n):
    """Start of the last partial tile of 64 (n if there is none)."""
    return (n // 64) * 64 if n % 64 else n


def rkd_part_f32(f_s, f_t, lo, na, w_d=W_D, w_a=W_A, defect=None):
    """zoo_rkd.hip: N2 from the squared differences, every norm and distance from N2, the distance rows and the anchors of the part,
    the closed-form gradient (the file's header comment); float32."""
    x, t = torch.as_tensor(f_s, dtype=F32), torch.as_tensor(f_t, dtype=F32)
    Bg, D = x.shape
    sl = slice(lo, lo + na)
    f = lambda v: torch.tensor(v, dtype=F32)
    off = 1.0 - torch.eye(Bg, dtype=F32)
    n2 = lambda e: (e[None, :, :] - e[:, None, :]).pow(2).sum(2)            # [i][k] = |x_k - x_i|^2
    N2s, N2t = n2(x), n2(t)
    d_s, d_t = N2s.clamp(min=RKD_EPS).sqrt() * off, N2t.clamp(min=RKD_EPS).sqrt() * off
    N = f(Bg) * f(Bg - 1)
    if defect == "part_mean":
        md, mt = d_s[sl].sum() / (f(na) * f(Bg - 1)), d_t[sl].sum() / (f(na) * f(Bg - 1))
    else:
        md, mt = d_s.sum(1).sum() / N, d_t.sum(1).sum() / N
    dh, th = d_s / md, d_t / mt
    z = dh - th                                                             # (0 on the diagonal: huber 0, clip 0)
    inv_n2, inv_n3 = 1.0 / (f(Bg) * f(Bg)), 1.0 / (f(Bg) * f(Bg) * f(Bg))
    loss_d = w_d * _huber(z[sl]).sum(1).sum() / (f(Bg) * f(Bg))
    corr = (z[sl].clamp(-1, 1) * dh[sl]).sum(1).sum() * inv_n2 / N
    inpart = torch.zeros(Bg, dtype=F32)
    inpart[sl] = 1.0
    cnt = inpart[:, None] + inpart[None, :]
    act = (N2s > RKD_EPS) & (off > 0)
    dr = N2s.sqrt()
    c2 = corr if defect == "corr_once" else 2.0 * corr
    W = torch.where(act, w_d * (z.clamp(-1, 1) * inv_n2 * cnt - c2) / md / torch.where(act, dr, torch.ones_like(dr)), torch.zeros_like(dr))
    dx = (W[:, :, None] * (x[:, None, :] - x[None, :, :])).sum(1)
    # angle term of the anchors [lo, lo + na)
    ns, nt = N2s[sl].sqrt(), N2t[sl].sqrt()                                 # [na][Bg]
    Es = (x[None, :, :] - x[sl, None, :]) * (1.0 / ns.clamp(min=RKD_EPS))[:, :, None]
    Et = (t[None, :, :] - t[sl, None, :]) * (1.0 / nt.clamp(min=RKD_EPS))[:, :, None]
    z = torch.bmm(Es, Es.transpose(1, 2)) - torch.bmm(Et, Et.transpose(1, 2))          # [a][j][k]
    if defect == "drop_j_tail":
        z[:, _tail(Bg):, :] = 0.0
    if defect == "drop_k_tail":
        z[:, :, _tail(Bg):] = 0.0
    if defect == "skip_65th_anchor" and na > 64:
        z[64] = 0.0
    loss_a = w_a * inv_n3 * _huber(z).sum((1, 2)).sum()
    dE = torch.bmm(z.clamp(-1, 1) * inv_n3, Es)
    if defect == "drop_de_cols":
        dE[:, :, _tail(D):] = 0.0
    dot = (Es * dE).sum(2, keepdim=True)
    notself = torch.ones(na, Bg, dtype=torch.bool)
    notself[torch.arange(na), torch.arange(lo, lo + na)] = False
    live = notself & (ns > RKD_EPS)
    inv_b = torch.where(live, 1.0 / torch.where(live, ns, torch.ones_like(ns)), torch.zeros_like(ns))
    dv = 2.0 * w_a * (dE - Es * dot) * inv_b[:, :, None]
    dx = dx + dv.sum(0)
    if defect != "no_anchor_self":
        dx[sl] -= dv.sum(1)
    return _np(loss_d + loss_a, dx)


def rkd_f32(f_s, f_t, w_d=W_D, w_a=W_A, defect=None):
    """zoo.hip: the distances from the Gram matrices, one anchor at a time with the difference vectors normalised by their own norm,
    dx_j = sum_i dv[i][j] - sum_k dv[j][k] + 2 sum_k W_jk (x_j - x_k); float32."""
    x, t = torch.as_tensor(f_s, dtype=F32), torch.as_tensor(f_t, dtype=F32)
    B, D = x.shape
    f = lambda v: torch.tensor(v, dtype=F32)
    off = 1.0 - torch.eye(B, dtype=F32)

    def gram_res(e):
        g = e @ e.t()
        dg = g.diagonal()
        return dg[:, None] + dg[None, :] - 2.0 * g
    res_s, res_t = gram_res(x), gram_res(t)
    d_s, d_t = res_s.clamp(min=RKD_EPS).sqrt() * off, res_t.clamp(min=RKD_EPS).sqrt() * off
    N = f(B) * f(B - 1)
    md, mt = d_s.sum() / N, d_t.sum() / N
    dh, th = d_s / md, d_t / mt
    z = dh - th
    inv_n2, inv_n3 = 1.0 / f(B * B), 1.0 / (f(B) * f(B) * f(B))
    loss_d = w_d * (_huber(z).sum() * inv_n2)
    corr = (z.clamp(-1, 1) * dh).sum() * inv_n2 / N
    act = (res_s > RKD_EPS) & (off > 0)
    dr = torch.where(act, res_s, torch.ones_like(res_s)).sqrt()
    W = torch.where(act, w_d * (z.clamp(-1, 1) * inv_n2 - corr) / md / dr, torch.zeros_like(dr))
    dxd = 2.0 * (W[:, :, None] * (x[:, None, :] - x[None, :, :])).sum(1)

    def dirs(e):
        v = e[None, :, :] - e[:, None, :]                                   # [i][j] = x_j - x_i
        n = v.pow(2).sum(2).sqrt()
        return v * (1.0 / n.clamp(min=RKD_EPS))[:, :, None], n
    Et, _ = dirs(t)
    Es, ns = dirs(x)
    z = torch.bmm(Es, Es.transpose(1, 2)) - torch.bmm(Et, Et.transpose(1, 2))
    loss_a = (w_a * _huber(z).sum((1, 2)) * inv_n3).sum()
    G = torch.bmm(z.clamp(-1, 1) * inv_n3, Es) * (2.0 * w_a)
    if defect == "cols_ge64":
        G[:, :, 64:] = 0.0
    dot = (G * Es).sum(2, keepdim=True)
    live = (off > 0) & (ns > RKD_EPS)
    inv = torch.where(live, 1.0 / torch.where(live, ns, torch.ones_like(ns)), torch.zeros_like(ns))
    dv = (G - Es * dot) * inv[:, :, None]
    if defect == "rows_ge16":
        dv[:, 16:, :] = 0.0
    return _np(loss_d + loss_a, (dv.sum(0) - dv.sum(1)) + dxd)


# ------------------------------------------------------------------------------------------------ PKT
def _safe_norm(x):
    """Row norms whose gradient at an all-zero row is 0 (the module's convention)."""
    sq = x.pow(2).sum(1, keepdim=True)
    pos = sq > 0
    return torch.where(pos, sq, torch.ones_like(sq)).sqrt() * pos.to(x.dtype)


def pkt_ref(f_s, f_t):
    """PKT.py:17-46 (cosine_similarity_loss) in float64, autograd."""
    x = torch.as_tensor(f_s).double().clone().requires_grad_(True)
    t = torch.as_tensor(f_t).double()
    eps = PKT_EPS
    s, tt = x / (_safe_norm(x) + eps), t / (_safe_norm(t) + eps)
    P, Q = (s @ s.t() + 1.0) / 2.0, (tt @ tt.t() + 1.0) / 2.0
    P, Q = P / P.sum(1, keepdim=True), Q / Q.sum(1, keepdim=True)
    loss = (Q * torch.log((Q + eps) / (P + eps))).mean()
    dx, = torch.autograd.grad(loss, x)
    return _np(loss, dx)


def pkt_f32(f_s, f_t, defect=None):
    """zoo.hip's three PKT kernels around the GEMMs (their header comments); float32."""
    x, t = torch.as_tensor(f_s, dtype=F32), torch.as_tensor(f_t, dtype=F32)
    B, D = x.shape
    eps = torch.tensor(PKT_EPS, dtype=F32)
    ns, nt = x.pow(2).sum(1).sqrt(), t.pow(2).sum(1).sqrt()
    s, tt = x * (1.0 / (ns + eps))[:, None], t * (1.0 / (nt + eps))[:, None]
    M, Mq = (s @ s.t() + 1.0) * 0.5, (tt @ tt.t() + 1.0) * 0.5
    upto = (B // 64) * 64 if defect == "rowsum_64" else B
    r, rq = M[:, :upto].sum(1, keepdim=True), Mq[:, :upto].sum(1, keepdim=True)
    P, Q = M / r, Mq / rq
    inv_bb = 1.0 / (torch.tensor(B, dtype=F32) * torch.tensor(B, dtype=F32))
    loss = (Q * torch.log((Q + eps) / (P + eps))).sum(1).sum() / (torch.tensor(B, dtype=F32) * torch.tensor(B, dtype=F32))
    g = -Q / (P + eps) * inv_bb
    c = (g * P).sum(1, keepdim=True)
    H = 0.5 * (g - c) / r
    ds = H @ s + H.t() @ s
    dot = (x * ds).sum(1)
    ne = ns + eps
    k = torch.where(ns > 0, dot / torch.where(ns > 0, ns * ne * ne, torch.ones_like(ns)), torch.zeros_like(ns))
    if defect == "no_proj":
        k = torch.zeros_like(k)
    dx = ds / ne[:, None] - x * k[:, None]
    if defect == "finish_16rows":
        dx[16:] = 0.0
    return _np(loss, dx)


# ------------------------------------------------------------------------------------------------ Cox
def cox_ref(theta, t, c):
    """utils.py:361-376 in float64, autograd: -mean_i c_i (theta_i - log sum_j [t_j >= t_i] exp(theta_j))."""
    th = torch.as_tensor(theta).double().reshape(-1).clone().requires_grad_(True)
    t, c = torch.as_tensor(t).double().reshape(-1), torch.as_tensor(c).double().reshape(-1)
    R = (t[None, :] >= t[:, None]).double()
    loss = -((th - torch.log((R * torch.exp(th)[None, :]).sum(1))) * c).mean()
    dth, = torch.autograd.grad(loss, th)
    return _np(loss, dth)


def cox_f32(theta, t, c, defect=None):
    """cox_kernel of zoo.hip: S_i, w_i = c_i / S_i, the closed-form gradient; float32."""
    th, t, c = (torch.as_tensor(v, dtype=F32).reshape(-1) for v in (theta, t, c))
    B = th.shape[0]
    e = torch.exp(th)
    R = (t[None, :] > t[:, None]) if defect == "gt" else (t[None, :] >= t[:, None])              # [i][j]: j in the risk set of i
    S = (R.float() * e[None, :]).sum(1)
    w = c / S
    li = (th - torch.log(S)) * c
    n = min(B, 1024) if defect == "rows_ge1024" else B
    w = torch.cat([w[:n], torch.zeros(B - n)])
    loss = -li[:n].sum() / torch.tensor(B, dtype=F32)
    a = (R.t().float() * w[None, :]).sum(1)                                                       # sum_i [t_k >= t_i] w_i
    d = -(c - e * a) * (1.0 / torch.tensor(B, dtype=F32))
    d = torch.cat([d[:n], torch.zeros(B - n)])
    return _np(loss, d)


# ------------------------------------------------------------------------------------------------ case tables
# (B, D) -> seed of rows(): the first one without an all-zero row (first_seed) and, for PKT at (2, 3), with rows that are not parallel
SEEDS = {(1024, 8): 4113, (2, 3): 3, (3, 2): 3}
# (Bg, D, anchor_lo, n_anchors).  Two rows are a fixed point of RKD (the one normalised distance is 1, the one angle cosine is 1: loss and
# gradient are identically zero, see ZERO_REF), so three rows stand next to them as the smallest case that has a gradient.
RKD_PART_CASES = (
    (2, 3, 0, 2), (3, 2, 1, 2), (63, 33, 0, 63), (64, 64, 0, 64), (65, 65, 0, 65), (65, 65, 64, 1), (130, 129, 0, 130), (130, 200, 37, 70),
    (100, 256, 0, 100), (70, 257, 3, 67), (66, 512, 0, 66), (257, 40, 250, 7), (1024, 8, 1000, 24), (1024, 8, 0, 1),
)
# uneven three-way partitions whose parts, summed in rank order, meet the float64 full-range result
RKD_PARTITIONS = (((130, 200), ((0, 37), (37, 70), (107, 23))), ((257, 40), ((0, 64), (64, 186), (250, 7))))
# (B, D, the return code the LDS rule gives, whether the gradient is compared).  (15, 1): at D = 1 the Gram form g_ii + g_jj - 2 g_ij
# cancels (the float32 restatement's own gradient is 12 % off there); the loss alone is compared.
RKD_ONE_CASES = (
    (2, 3, OK, True), (3, 3, OK, True), (15, 1, OK, False), (16, 63, OK, True), (17, 64, OK, True), (17, 65, OK, True), (33, 512, OK, True),
    (66, 512, OK, True), (67, 512, EINVAL, False), (105, 256, OK, True), (106, 256, EINVAL, False), (128, 128, OK, True),
)
RKD_ONE_VS_TILED = ((66, 512), (105, 256), (128, 128))
RKD_FIT_PAIRS = ((128, 128, 1), (105, 256, 1), (106, 256, 0), (128, 256, 0), (81, 384, 1), (82, 384, 0), (66, 512, 1), (67, 512, 0))
# degenerate RKD input: rows 3 and 64 of a 70 x 48 student equal while the teacher's differ, and student row 10 all zero
RKD_DEGENERATE = (70, 48)
PKT_CASES = ((2, 3), (5, 1), (63, 64), (65, 65), (66, 200), (17, 512), (130, 128), (1030, 24))
PKT_ZERO_ROW = (66, 40, 9)                  # (B, D, the all-zero student row)
COX_CASES = (1, 2, 64, 1023, 1024, 1025, 4096)
COX_CENSORED = 70                           # every row censored: loss 0, gradient 0
COX_FUSED = (1023, 1025, 4096)

# Absolute allowances of the cases whose reference is identically zero or pure cancellation (max |ref| gives no unit there):
#   RKD at two rows: d / mean_d is exactly 1 on both sides (the mean of two equal numbers).  With u = 2^-24, a unit vector's components
#     carry <= 4 u (sum of squares, sqrt, reciprocal, product), the one cosine e.e is 1 +- 11 u on either side, so |z| <= 22 u = 1.3e-6:
#     loss <= w_a z^2 / 16 = 5.3e-12, and dv = (G - e (e.G)) / |v| with G = 2 w_a (z / 8) e parallel to e leaves |G| (11 u + 3 u) / |v| =
#     1.6e-5 * 8.4e-7 / |v| <= 5e-11 for |v| >= 0.3 (the case's rows are 0.8 and 1.5 apart);
#   Cox at one row: theta - log(exp(theta)) and 1 - e (1 / e) are each within 4 ulp32 of their operands max(|theta|, 1) and 1;
#   PKT at D = 1 (positive rows): every cosine is 1 within an ulp, P and Q are both 1 / B within a few ulp32, so the loss - a mean of
#     Q log((Q + eps) / (P + eps)), each term within 8 ulp32 / B of zero - and ds = H s + H^T s with |H| <= 4 ulp32 / B^2 are rounding
#     noise around a float64 value of 1e-16; dx_i = (ds_i / ne_i)(1 - n_i / ne_i) is smaller still.  8 ulp32 for both.
ULP32 = 2.0 ** -23
ZERO_REF = {"rkd2": {"loss": 1e-11, "dx": 5e-11}, "pkt_d1": 8 * ULP32}


def seed_of(B, D):
    return SEEDS.get((B, D), 0)


def live_rows(dx):
    """The gradient rows of the PKT_ZERO_ROW case without the all-zero row's."""
    return np.delete(np.asarray(dx), PKT_ZERO_ROW[2], 0)


def rkd_degenerate_rows():
    B, D = RKD_DEGENERATE
    f_s, f_t = rows(seed_of(B, D), B, D)
    f_s[64] = f_s[3]
    f_s[10] = 0.0
    return f_s, f_t


_CACHE = {}


def case(op, key):
    """{"inp", "ref", "rest", "abs": {"loss", "dx"}} of one case, computed once per process and shared (read only).
    op: "rkd_part" (Bg, D, lo, na) | "rkd_part_deg" (lo, na) | "rkd" (B, D) | "pkt" (B, D) | "pkt_zero_row" () | "cox" B | "cox_censored" ()."""
    k = (op, key)
    if k in _CACHE:
        return _CACHE[k]
    ab = {"loss": 0.0, "dx": 0.0}
    if op in ("rkd_part", "rkd_part_deg"):
        if op == "rkd_part":
            Bg, D, lo, na = key
            f_s, f_t = rows(seed_of(Bg, D), Bg, D)
        else:
            (lo, na), (f_s, f_t) = key, rkd_degenerate_rows()
            Bg, D = f_s.shape
        ref, rest = rkd_part_ref(f_s, f_t, lo, na), rkd_part_f32(f_s, f_t, lo, na)
        inp = dict(f_s=f_s, f_t=f_t, lo=lo, na=na)
        if Bg == 2:
            ab = dict(ZERO_REF["rkd2"])
    elif op == "rkd":
        B, D = key
        f_s, f_t = rows(seed_of(B, D), B, D)
        ref, rest, inp = rkd_ref(f_s, f_t), rkd_f32(f_s, f_t), dict(f_s=f_s, f_t=f_t)
        if B == 2:
            ab = dict(ZERO_REF["rkd2"])
    elif op in ("pkt", "pkt_zero_row"):
        if op == "pkt":
            B, D = key
            f_s, f_t = rows(seed_of(B, D), B, D)
        else:
            B, D, z = PKT_ZERO_ROW
            f_s, f_t = rows(seed_of(B, D), B, D)
            f_s[z] = 0.0
        ref, rest, inp = pkt_ref(f_s, f_t), pkt_f32(f_s, f_t), dict(f_s=f_s, f_t=f_t)
        if D == 1:
            ab = {"loss": ZERO_REF["pkt_d1"], "dx": ZERO_REF["pkt_d1"]}
        if op == "pkt_zero_row":             # the zero row's ds / eps dwarfs every other row: those are judged on their own as well
            ab["dx_live"] = 0.0
            for o in (ref, rest):
                o["dx_live"] = live_rows(o["dx"])
    elif op in ("cox", "cox_censored"):
        B = key if op == "cox" else COX_CENSORED
        theta, t, c = cox_inputs(B, B, censored=op == "cox_censored")
        if B == 1:
            c.fill_(1.0)
            ab = {"loss": 4 * ULP32 * max(1.0, float(theta.abs().max())), "dx": 4 * ULP32}
        ref, rest, inp = cox_ref(theta, t, c), cox_f32(theta, t, c), dict(theta=theta, t=t, c=c)
    else:
        raise KeyError(op)
    _CACHE[k] = dict(inp=inp, ref=ref, rest=rest, abs=ab)
    return _CACHE[k]


def base_op(op):
    return {"rkd_part_deg": "rkd_part", "pkt_zero_row": "pkt", "cox_censored": "cox"}.get(op, op)


def case_tolerance(op, e, out):
    return tolerance(base_op(op), out, e["ref"][out], e["rest"][out], e["abs"][out])

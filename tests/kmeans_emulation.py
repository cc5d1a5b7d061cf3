"""numpy statements of the device k-means class centres (csrc/crd_kmeans.hip, ph_crd_kmeans_centers).

  kmeans(..., f32=False)  the float64 reference of the algorithm: farthest-point initialisation from list position 0 (lowest
                          position among equal values), T rounds of assignment (direct-form distance, lowest centre index among
                          equal distances) and mean update (a centre without members keeps its value; centres j >= class size are
                          zero rows without members).
  kmeans(..., f32=True)   the float32 restatement with the kernel's grouping: the distance of a row is 32 lanes x 4 features,
                          ((t0^2 + t1^2) + t2^2) + t3^2 per lane, every operation rounded, then the xor butterfly 16, 8, 4, 2, 1;
                          the partial sums of a 256-row chunk are 8 running sums (rows h, h + 8, ..) added in the order 0 .. 7;
                          chunks are combined in double in chunk order and divided by the count in double.
  DEFECTS                 what tests/test_kmeans_emulation_cpu.py injects into the restatement.
  exact_inputs / real_inputs / fixed_point_inputs / planted_bank     the case tables of the CPU and GPU tests and the recipe of
                          the reference golden (tests/golden/make_golden_mia2023_kmeans.py)."""
import numpy as np

D = 128
ROWS = 256          # KM_ROWS
HW = 8              # half-waves of a workgroup
KMAX = 8
F32, F64 = np.float32, np.float64

DEFECTS = ("tie_high_centre", "tie_high_pos", "drop_chunk_last", "mean_over_capacity", "empty_zeroed", "banks_swapped",
           "one_iter_less", "expansion")
_XOR = [np.arange(32) ^ o for o in (16, 8, 4, 2, 1)]


def dist32(X, Cn):
    """[m, 128] x [k, 128] float32 -> [m, k] float32 distances in the kernel's grouping."""
    X, Cn = np.asarray(X, F32), np.asarray(Cn, F32)
    t = X[:, None, :] - Cn[None, :, :]
    q = (t * t).reshape(X.shape[0], Cn.shape[0], 32, 4)
    s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    for p in _XOR:
        s = s + s[..., p]
    assert s.dtype == F32
    return s[..., 0]


def dist32_expansion(X, Cn):
    """The |x|^2 - 2 x.y + |y|^2 form in float32 (a defect: the algorithm fixes the direct form)."""
    X, Cn = np.asarray(X, F32), np.asarray(Cn, F32)
    xx = (X * X).sum(1, dtype=F32)
    cc = (Cn * Cn).sum(1, dtype=F32)
    return (xx[:, None] - F32(2) * (X @ Cn.T).astype(F32)) + cc[None, :]


def dist64(X, Cn):
    t = np.asarray(X, F64)[:, None, :] - np.asarray(Cn, F64)[None, :, :]
    return (t * t).sum(2)


def _first_max(v, high=False):
    return int(len(v) - 1 - np.argmax(v[::-1])) if high else int(np.argmax(v))


def _update32(X, lab, k, old, defect):
    m = X.shape[0]
    nch = -(-m // ROWS)
    Xp = np.zeros((nch * ROWS, D), F32); Xp[:m] = X
    oh = np.zeros((nch * ROWS, k), bool); oh[np.arange(m), lab] = True
    if defect == "drop_chunk_last":
        oh[[min(m, (q + 1) * ROWS) - 1 for q in range(nch)]] = False
    Xp = Xp.reshape(nch, ROWS // HW, HW, D); oh = oh.reshape(nch, ROWS // HW, HW, k)
    acc = np.zeros((nch, HW, k, D), F32)
    for i in range(ROWS // HW):
        acc = acc + np.where(oh[:, i, :, :, None], Xp[:, i, :, None, :], F32(0))
    part = acc[:, 0]
    for h in range(1, HW):
        part = part + acc[:, h]
    assert part.dtype == F32
    s = np.zeros((k, D), F64)
    for q in range(nch):
        s += part[q].astype(F64)
    cnt = oh.reshape(-1, k).sum(0).astype(np.int32)
    div = np.full(k, nch * ROWS, F64) if defect == "mean_over_capacity" else np.maximum(cnt, 1).astype(F64)
    new = (s / div[:, None]).astype(F32)
    keep = np.zeros_like(old) if defect == "empty_zeroed" else old
    return np.where((cnt > 0)[:, None], new, keep), cnt


def _update64(X, lab, k, old):
    new, cnt = old.copy(), np.bincount(lab, minlength=k).astype(np.int32)
    for j in range(k):
        if cnt[j]:
            new[j] = X[lab == j].mean(0)
    return new, cnt


def class_run(X, k, T, f32, defect=None):
    """One class of one bank.  -> centres [k, 128], labels [m], counts [k], trace (the running minimum before every pick after
    the first, the distance table and the labels of every iteration)."""
    ft = F32 if f32 else F64
    X = np.asarray(X, F32).astype(ft)
    m = X.shape[0]
    dist = (dist32_expansion if defect == "expansion" else dist32) if f32 else dist64
    keff = min(k, m)
    cen = np.zeros((k, D), ft)
    tr = dict(mind=[], dist=[], labels=[])
    if m == 0:
        return cen, np.zeros(0, np.int32), np.zeros(k, np.int32), tr
    pos, mind = 0, None
    for j in range(keff):
        if j:
            tr["mind"].append(mind.copy())
            pos = _first_max(mind, defect == "tie_high_pos")
        cen[j] = X[pos]
        d = dist(X, X[pos:pos + 1])[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
    lab, cnt = np.zeros(m, np.int32), np.zeros(k, np.int32)
    for _ in range(T):
        d = dist(X, cen[:keff])
        lab = (keff - 1 - np.argmin(d[:, ::-1], 1) if defect == "tie_high_centre" else np.argmin(d, 1)).astype(np.int32)
        cen, cnt = _update32(X, lab, k, cen, defect) if f32 else _update64(X, lab, k, cen)
        tr["dist"].append(d); tr["labels"].append(lab)
    return cen, lab, cnt, tr


def kmeans(bank, members, offsets, k, T, f32, defect=None):
    """One bank, all classes.  -> dict(centres [C, k, 128], labels [offsets[-1]], counts [C, k], trace [C])."""
    C = len(offsets) - 1
    if defect == "one_iter_less":
        T, defect = T - 1, None
    out = dict(centres=np.zeros((C, k, D), F32 if f32 else F64), labels=np.zeros(int(offsets[-1]), np.int32),
               counts=np.zeros((C, k), np.int32), trace=[])
    for c in range(C):
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        cen, lab, cnt, tr = class_run(bank[members[lo:hi]], k, T, f32, defect)
        out["centres"][c], out["labels"][lo:hi], out["counts"][c] = cen, lab, cnt
        out["trace"].append(tr)
    return out


def kmeans_pair(case, T, f32, defect=None):
    """Both banks of a case, the layout of the C entry: centres [2, C, k, 128], labels [2, total], counts [2, C, k]."""
    r = [kmeans(case[b], case["members"], case["offsets"], case["k"], T, f32, None if defect == "banks_swapped" else defect)
         for b in ("bank1", "bank2")]
    if defect == "banks_swapped":
        r = r[::-1]
    return dict(centres=np.stack([x["centres"] for x in r]), labels=np.stack([x["labels"] for x in r]),
                counts=np.stack([x["counts"] for x in r]), trace=[x["trace"] for x in r])


def stable_from(trace):
    """The first iteration (1-based) of a class trace whose assignment repeats the one before: from there on nothing changes.
    None if the trace ends before."""
    L = trace["labels"]
    for t in range(1, len(L)):
        if np.array_equal(L[t], L[t - 1]):
            return t + 1
    return None


def margins(ref_trace, rest_trace):
    """Over the picks and the iterations of one class: (smallest gap between best and second best in the float64 run, largest
    distance difference between the restatement and the reference), for the assignments and for the picks."""
    ga, ea, gp, ep = np.inf, 0.0, np.inf, 0.0
    for d64, d32 in zip(ref_trace["dist"], rest_trace["dist"]):
        if d64.shape[1] > 1:
            s = np.sort(d64, 1)
            ga = min(ga, float((s[:, 1] - s[:, 0]).min()))
        ea = max(ea, float(np.abs(d32.astype(F64) - d64).max()))
    for m64, m32 in zip(ref_trace["mind"], rest_trace["mind"]):
        if len(m64) > 1:
            s = np.sort(m64)
            gp = min(gp, float(s[-1] - s[-2]))
        ep = max(ep, float(np.abs(m32.astype(F64) - m64).max()))
    return ga, ea, gp, ep


# ------------------------------------------------------------------------------------------------ the cases
def _lists(sizes, n_data, rng):
    perm = rng.permutation(n_data).astype(np.int32)
    offsets = np.zeros(len(sizes) + 1, np.int32)
    offsets[1:] = np.cumsum(sizes)
    assert offsets[-1] <= n_data
    return perm[:offsets[-1]].copy(), offsets


EXACT_K = (2, 3, 8)
EXACT_OFFSET = 1024.0     # every row of the last class carries it: the direct form stays exact, the expansion form does not


def exact_sizes(k):
    """Class sizes of the exact case: the edges of the 256-row chunk, the smallest classes, one of identical rows (every cluster
    but the first is empty after the first assignment), one smaller than k, an empty one, one of offset rows."""
    return [k, k + 1, 255, 256, 257, 513, 40, k - 1, 0, 300]


def exact_inputs(k):
    """Integer banks in [-4, 4] drawn from a pool of 16 rows that differ in eight features: duplicate rows and equal distances
    everywhere, every sum exact in float32.  iters = 1."""
    rng = np.random.RandomState(700 + k)
    sizes = exact_sizes(k)
    n_data = sum(sizes) + 37
    members, offsets = _lists(sizes, n_data, rng)
    case = dict(k=k, members=members, offsets=offsets, max_rows=max(sizes), n_data=n_data, sizes=sizes)
    for b in ("bank1", "bank2"):
        pool = np.tile(rng.randint(-4, 5, (1, D)), (16, 1))
        pool[:, :8] = 0
        pool[np.arange(8), np.arange(8)] = 4                 # eight rows at one distance from each other: distinct rows tie
        pool[8:, :8] = rng.randint(-2, 3, (8, 8))
        bank = pool[rng.randint(0, 16, n_data)].astype(F32)
        ident = members[offsets[6]:offsets[7]]
        bank[ident] = bank[ident[0]]
        bank[members[offsets[9]:offsets[10]]] += F32(EXACT_OFFSET)
        case[b] = bank
    return case


REAL_SIZES = (257, 513, 1030)
REAL_K = (2, 3, 7)
REAL_ITERS = (1, 5, 16)
# seeds at which the float64 run's decisions are 16 x clear of the restatement's distance error over all 16 iterations
# (searched on the CPU with real_margin below; tests/test_kmeans_emulation_cpu.py asserts the condition)
REAL_SEEDS = {2: 5, 3: 38, 7: 38}


def real_inputs(k, seed=None):
    """Bank rows as ContrastMemory initialises them (uniform in +-1 / sqrt(128 / 3)), three classes of REAL_SIZES rows."""
    rng = np.random.RandomState(REAL_SEEDS[k] if seed is None else seed)
    n_data = sum(REAL_SIZES) + 24
    members, offsets = _lists(list(REAL_SIZES), n_data, rng)
    stdv = 1.0 / np.sqrt(D / 3.0)
    case = dict(k=k, members=members, offsets=offsets, max_rows=max(REAL_SIZES), n_data=n_data)
    for b in ("bank1", "bank2"):
        case[b] = ((rng.rand(n_data, D) * 2 - 1) * stdv).astype(F32)
    return case


def real_margin(case, T=max(REAL_ITERS)):
    """(smallest decision gap of the float64 run) / (largest distance error of the restatement), over both banks, all classes,
    picks and assignments; the runs themselves."""
    ref, rest = kmeans_pair(case, T, False), kmeans_pair(case, T, True)
    ratio = np.inf
    for b in range(2):
        for tr64, tr32 in zip(ref["trace"][b], rest["trace"][b]):
            ga, ea, gp, ep = margins(tr64, tr32)
            ratio = min(ratio, ga / max(ea, 1e-300), gp / max(ep, 1e-300))
    return ratio, ref, rest


def planted_bank(seed, n_data, k, C=3, noise=0.02):
    """The planted bank: every class is exactly k tight blobs of unequal size - a unit direction plus `noise` per feature,
    renormalised.  -> bank1, bank2 [n_data, 128] float32, labels [n_data] (class), blobs [2, n_data] (blob of the row in its
    class, per bank).  Any k-means finds this partition."""
    rng = np.random.RandomState(seed)
    labels = rng.permutation(np.arange(n_data) % C).astype(np.int64)
    banks, blobs = [], np.zeros((2, n_data), np.int64)
    for b in range(2):
        bank = np.zeros((n_data, D), F64)
        for c in range(C):
            rows = np.nonzero(labels == c)[0]
            w = np.arange(2, k + 2, dtype=F64)
            sizes = np.floor(len(rows) * w / w.sum()).astype(int)
            sizes[-1] += len(rows) - sizes.sum()
            bl = rng.permutation(np.repeat(np.arange(k), sizes))
            dirs = rng.randn(k, D); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            x = dirs[bl] + noise * rng.randn(len(rows), D)
            bank[rows] = x / np.linalg.norm(x, axis=1, keepdims=True)
            blobs[b, rows] = bl
        banks.append(bank.astype(F32))
    return banks[0], banks[1], labels, blobs


def class_lists(labels, C=3):
    lists = [np.nonzero(labels == c)[0].astype(np.int32) for c in range(C)]
    offsets = np.zeros(C + 1, np.int32)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    return np.concatenate(lists), offsets


FIXED_POINT = dict(seed=5, n_data=1500, k=3)     # 500 rows per class: two chunks each


def fixed_point_inputs():
    """A planted bank: the float64 run stops changing within 6 iterations (asserted on the CPU)."""
    b1, b2, labels, _ = planted_bank(FIXED_POINT["seed"], FIXED_POINT["n_data"], FIXED_POINT["k"])
    members, offsets = class_lists(labels)
    return dict(k=FIXED_POINT["k"], members=members, offsets=offsets, max_rows=int(np.diff(offsets).max()),
                n_data=FIXED_POINT["n_data"], bank1=b1, bank2=b2)


GOLDEN = dict(seed=31, n_data=384, nce_p=(3, 4))   # the bank of tests/golden/mia2023_crd_v10_kmeans.npz

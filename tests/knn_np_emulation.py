"""numpy statement of the rank-window rule of ph_crd_bank_topk for num_pos > 8 (csrc/crd.hip), on the
kernel's own uint64 keys.

A key is (monotone bits of the float32 similarity, -0 folded onto +0) << 32 | ~row: larger = earlier in a stable descending
sort, unique per row, 0 = an empty slot.  Per query and bank:

  group maxima   the sample pass: the largest key of each of 2 x stiles disjoint row sets (every tstride-th tile of 32 rows, the
                 two half-waves' 16 rows each);
  thr[p]         the 8 (p + 1)-th largest group maximum, 0 with fewer groups;
  ub[0]          all ones; ub[p + 1] = the eighth key of window p, 0 (exhausted) when the window held fewer than eight;
  window p       the eight largest keys k with thr[p] <= k < ub[p] -> ranks 8 p .. 8 p + 7.

`defect` injects one of DEFECTS, for tests/test_knn_np_cpu.py to show that the comparison sees each of them."""
import numpy as np

F32, F64, U64 = np.float32, np.float64, np.uint64
W = 8                               # TOPK_MAX: keys per window
MAX_POS = 64
SAMPLE_TILES = 128                  # KNN_SAMPLE_TILES
EMPTY_ROW = 0x7fffffff
ALL_ONES = U64(0xffffffffffffffff)
DEFECTS = ("ub_inclusive", "thr_of_first_window", "no_exhausted_state", "rank_offset_zero")


def keys_of(sim32):
    """knn_key of every bank row of one query: sim32 float32 [n]."""
    u = (sim32.astype(F32) + F32(0.0)).view(np.uint32).astype(U64)
    u = np.where(u & U64(0x80000000), u ^ U64(0xffffffff), u ^ U64(0x80000000))
    row = np.arange(sim32.shape[0], dtype=np.uint32)
    return (u << U64(32)) | (~row).astype(U64)


def key_row(key):
    return np.where(key == 0, np.int64(EMPTY_ROW), (~key.astype(np.uint32)).astype(np.int64))


def key_value(key):
    u = (key >> U64(32)).astype(np.uint32)
    v = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(F32)
    return np.where(key == 0, F32(-np.inf), v)


def group_maxima(keys):
    """The sample pass: [2 * stiles] keys, group 2 s + h = rows 8 q + 4 h .. 8 q + 4 h + 3 (q = 0 .. 3) of tile s * tstride."""
    n = keys.shape[0]
    ntiles = (n + 31) // 32
    stiles = min(ntiles, SAMPLE_TILES)
    tstride = ntiles // stiles
    out = np.zeros(2 * stiles, dtype=U64)
    m = np.arange(32)
    for s in range(stiles):
        rows = s * tstride * 32 + m
        for h in range(2):
            r = rows[((m >> 2) & 1) == h]
            r = r[r < n]
            if r.size:
                out[2 * s + h] = keys[r].max()
    return out


def thresholds(gmax, npass, defect=None):
    g = np.sort(gmax[gmax != 0])[::-1]
    thr = np.zeros(npass, dtype=U64)
    for p in range(npass):
        k = W * (1 if defect == "thr_of_first_window" else p + 1)
        if g.size >= k:
            thr[p] = g[k - 1]
    return thr


def window_topk(keys, NP, defect=None):
    """The NP keys the windows leave for one query, in rank order; 0 = an empty slot, None-filled slots (rank_offset_zero) = -1."""
    npass = (NP + W - 1) // W
    thr = thresholds(group_maxima(keys), npass, defect)
    out = np.full(NP, ALL_ONES, dtype=U64)          # "never written"
    ub = ALL_ONES
    for p in range(npass):
        below = keys <= ub if defect == "ub_inclusive" and p > 0 else keys < ub
        win = np.sort(keys[(keys >= thr[p]) & below])[::-1][:W]
        win = np.concatenate([win, np.zeros(W - win.size, dtype=U64)])
        r0 = 0 if defect == "rank_offset_zero" else W * p
        cnt = min(W, NP - W * p)
        out[r0:r0 + cnt] = win[:cnt]
        ub = win[W - 1]
        if ub == 0 and defect == "no_exhausted_state":
            ub = ALL_ONES
    return out


def masked_cosine(i):
    """float64 class-masked cosine of every query with every row, per bank (the formula of crd_width_emulation.knn_reference)."""
    out = []
    for mem in (i["mem1"], i["mem2"]):
        m = mem.astype(F64)
        mn = m / np.linalg.norm(m, axis=1, keepdims=True)
        sim = mn[i["idx"][:, 0]] @ mn.T
        out.append(np.where(i["labels"][None, :] == i["batch_label"][:, None], sim, 0.0))
    return out


def knn_windows(i, NP, defect=None):
    """Per bank: rows [B][NP] int64 (EMPTY_ROW = an empty slot, -1 = never written) and float32 similarities."""
    res = []
    for sim in masked_cosine(i):
        k = np.stack([window_topk(keys_of(s.astype(F32)), NP, defect) for s in sim])
        rows = np.where(k == ALL_ONES, np.int64(-1), key_row(k))
        res.append((rows, key_value(k)))
    return res


def stable_sort_f32(i, NP):
    """Per bank: rows of a stable descending sort of the float32-rounded similarities, EMPTY_ROW past the end of the bank."""
    res = []
    for sim in masked_cosine(i):
        s32 = sim.astype(F32) + F32(0.0)
        order = np.argsort(-s32, axis=1, kind="stable")[:, :NP].astype(np.int64)
        pad = np.full((order.shape[0], NP - order.shape[1]), EMPTY_ROW, dtype=np.int64)
        res.append(np.concatenate([order, pad], axis=1))
    return res


def workspace_bytes(old_bytes, B, NP):
    """ph_crd_bank_topk_workspace_bytes_np from the value of ph_crd_bank_topk_workspace_bytes: one record
    [thr bank 0 | thr bank 1 | ub bank 0 | ub bank 1][min(B, 64)] of u64 per window in place of thr [2][min(B, 64)]."""
    if not 1 <= NP <= MAX_POS:
        return 0
    npass = (NP + W - 1) // W
    return old_bytes + (2 * min(B, 64) * (2 * npass - 1) * 8 if npass > 1 else 0)

"""numpy restatement of csrc/epochrec.hip: the epoch record, the row store and the similarity audit,
with the float64 reference of the audit and the defects the GPU cases of tests/test_gpu_epoch.py must see.

Record: float32 values widened to float64 and added in call order - Python's `acc += t.item()`; exact counts.
Audit: rows scaled by the float32 of 1 / sqrt(float64 sum of squares), float32 products accumulated in float32 over the
columns (three orders: one column at a time, the MFMA's two columns per instruction, numpy's matmul), float64 sums grouped as
the kernel groups them - per workgroup (tile of 64 rows i, j tiles by, by + split, ..), then over the workgroups.  Inside a
workgroup numpy's pairwise float64 sum stands in for the lane order: float64 re-association moves a sum by 1e-16 of its terms.

Tolerances (the house rule: 4 x the error of the float32 restatement + a floor):
  audit sums    4 x the largest error of the three restatements + 4 * 2^-24 * sqrt(D) * sqrt(pairs in the sum).  The floor is
                reasoning, not a measurement: the kernel and the restatement share every rounding except the ORDER of the D
                float32 additions of one similarity, |partial sums| <= 1 by Cauchy-Schwarz, so an element moves by a random
                walk of at most sqrt(D) half-ulps of 1 (2^-24 sqrt(D)), independently per pair - sqrt(pairs) of that over a
                sum, times the margin 4.
  softmax rows  4 x the float32 restatement's error + 8 * 2^-24: expf within 1 ulp of a value <= 1 (the HIP math
                library's documented bound), the float32 sum of <= 4096 such values re-associated, one division."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = 4.0
TILE, CHUNK, MAX_SPLIT = 64, 32, 16
REC_ADD, REC_ADD_POSITIVE = 0, 1
SUMS = ("teacher_intra", "teacher_inter", "student_intra", "student_inter", "absdiff")


# ------------------------------------------------------------------------------------------------ the record
def first_argmax(row, last=False):
    """The kernel's arg-max: a strict `>` scan from column 0 (the FIRST maximum; a NaN never wins).  last: the defect `>=`."""
    best, arg = row[0], 0
    for c in range(1, len(row)):
        if (row[c] >= best) if last else (row[c] > best):
            best, arg = row[c], c
    return arg


def record_emulate(calls, defect=None):
    """calls: dicts with optional keys scalars (float32 values), modes, wvec, pred [B, C], grade [B], rows (<= 2 vectors).
    -> dict(sums [16], added [16], wvec [16], rowmeans [2], correct, bad, steps, rows) as the device record holds them."""
    sums, added, wv, rm = [0.0] * 16, [0] * 16, [0.0] * 16, [0.0] * 2
    correct = bad = steps = rows = 0
    for c in calls:
        for k, (v, mode) in enumerate(zip(c.get("scalars", ()), c.get("modes", ()))):
            v = F32(v)
            take = mode == REC_ADD or (v >= 0.0 if defect == "ge_zero" else v > 0.0)
            if take:
                sums[k] += float(v)                      # `acc += t.item()`
                added[k] += 1
        for k, v in enumerate(c.get("wvec", ())):
            wv[k] += float(F32(v))
        if c.get("pred") is not None:
            pred, grade = np.asarray(c["pred"], dtype=F32), np.asarray(c["grade"], dtype=np.int64)
            B, C = pred.shape
            for b in range(B):
                if grade[b] < 0 or grade[b] >= C:
                    bad += 1
                elif first_argmax(pred[b], last=defect == "last_max") == grade[b]:
                    correct += 1
            rows += B
        for k, r in enumerate(c.get("rows", ())):
            r = np.asarray(r, dtype=F32).astype(F64)
            rm[k] += math.fsum(r.tolist()) / r.size     # (float32 values of one binade range: every order is exact)
        steps += 1
    return dict(sums=sums, added=added, wvec=wv, rowmeans=rm, correct=correct, bad=bad, steps=steps, rows=rows)


# ------------------------------------------------------------------------------------------------ the row store
def softmax_rows(x, dt):
    x = np.asarray(x, dtype=F32).astype(dt)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True, dtype=dt)


def store_emulate(store, index, rows, softmax=False, dt=F32, defect=None):
    """store[index] = rows as the kernel resolves it: the LAST of equal indices wins (defect "first_writer": the first), an
    index outside the store is skipped.  -> (store, skipped)."""
    out = np.array(store, dtype=dt)
    vals = softmax_rows(rows, dt) if softmax else np.asarray(rows, dtype=F32).astype(dt)
    index = np.asarray(index, dtype=np.int64)
    skipped, seen = 0, set()
    order = range(len(index)) if defect != "first_writer" else range(len(index) - 1, -1, -1)
    for b in order:                                      # (ascending: a later row overwrites; descending = first writer wins)
        i = int(index[b])
        if i < 0 or i >= out.shape[0]:
            skipped += 1
            continue
        out[i] = vals[b]
        seen.add(i)
    return out, skipped


SOFTMAX_FLOOR = 8 * 2.0 ** -24


def softmax_tolerance(ref64, rest32):
    return MARGIN * float(np.abs(rest32.astype(F64) - ref64).max()) + SOFTMAX_FLOOR


# ------------------------------------------------------------------------------------------------ the audit
def inv_norms(x):
    """float32(1 / sqrt(float64 sum of squares)); 0 for a zero row."""
    s = (np.asarray(x, dtype=F32).astype(F64) ** 2).sum(axis=1)
    with np.errstate(divide="ignore"):
        return np.where(s > 0.0, 1.0 / np.sqrt(s), 0.0).astype(F32)


def audit_reference(F, P, labels=None):
    """float64 throughout: normalised rows (a zero row stays zero), both Gram matrices, the reference's three formulas
    ("MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":162-188) as SUMS and counts."""
    def sim(x):
        x = np.asarray(x, dtype=F32).astype(F64)
        nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        x = x / np.where(nrm == 0.0, 1.0, nrm)
        return x @ x.T
    Sf, Sp = sim(F), sim(P)
    n = Sf.shape[0]
    lab = np.zeros(n, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    same = lab[:, None] == lab[None, :]
    sums = dict(teacher_intra=Sf[same].sum(), teacher_inter=Sf[~same].sum(), student_intra=Sp[same].sum(),
                student_inter=Sp[~same].sum(), absdiff=np.abs(Sf - Sp).sum())
    return sums, (int(same.sum()), int((~same).sum()))


def _gram_tile(xi, xj, order):
    """float32 Gram tile xi xj^T of two normalised row tiles [., D] (D a multiple of the chunk, zero padded)."""
    if order == "matmul":
        return xi @ xj.T
    acc = np.zeros((xi.shape[0], xj.shape[0]), dtype=F32)
    if order == "seq":
        for d in range(xi.shape[1]):
            acc = acc + np.outer(xi[:, d], xj[:, d])
    else:                                                # "pair": the 32x32x2 instruction's two columns, then the accumulator
        for d in range(0, xi.shape[1], 2):
            acc = acc + (np.outer(xi[:, d], xj[:, d]) + np.outer(xi[:, d + 1], xj[:, d + 1]))
    return acc


def audit_emulate(F, P, labels=None, order="seq", defect=None):
    """The kernel's arithmetic and grouping -> (sums dict, (intra pairs, inter pairs)).  defect: "no_diagonal",
    "drop_last_row_tile" (the last partial tile of rows i), "drop_last_chunk" (the last column chunk of a D that is no multiple
    of 32), "transposed_class_test" (the labels of tile position (jl, il) instead of (il, jl))."""
    n = np.asarray(F).shape[0]
    lab = np.zeros(n, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if order == "matmul" and defect is None:
        # whole matrices at once (the float64 grouping moves nothing a float32 product order does not): fast at n = 4096
        sf, sp = [(lambda xn: xn @ xn.T)(np.asarray(x, dtype=F32) * inv_norms(x)[:, None]) for x in (F, P)]
        same = lab[:, None] == lab[None, :]
        sf64, sp64 = sf.astype(F64), sp.astype(F64)
        sums = [sf64[same].sum(), sf64[~same].sum(), sp64[same].sum(), sp64[~same].sum(), np.abs(sf - sp).astype(F64).sum()]
        return dict(zip(SUMS, (float(v) for v in sums))), (int(same.sum()), int((~same).sum()))
    ntiles = -(-n // TILE)
    split = min(ntiles, MAX_SPLIT)
    npad = ntiles * TILE
    mats = []
    for x in (F, P):
        x = np.asarray(x, dtype=F32)
        D = x.shape[1]
        nc = -(-D // CHUNK)
        if defect == "drop_last_chunk" and D % CHUNK:
            nc -= 1
        xn = np.zeros((npad, max(nc, 0) * CHUNK), dtype=F32)
        keep = min(D, nc * CHUNK)
        xn[:n, :keep] = (x * inv_norms(x)[:, None])[:, :keep]
        mats.append(xn)
    labp = np.full(npad, -1, dtype=np.int64)
    labp[:n] = lab
    valid = np.arange(npad) < n
    parts = np.zeros((ntiles, split, 5), dtype=F64)
    cnt = np.zeros((ntiles, split, 2), dtype=np.int64)
    for bx in range(ntiles):
        if defect == "drop_last_row_tile" and bx == ntiles - 1 and n % TILE:
            continue
        ri = slice(bx * TILE, bx * TILE + TILE)
        for by in range(split):
            acc = np.zeros(5, dtype=F64)
            for jt in range(by, ntiles, split):
                rj = slice(jt * TILE, jt * TILE + TILE)
                sf = _gram_tile(mats[0][ri], mats[0][rj], order) if mats[0].shape[1] else np.zeros((TILE, TILE), F32)
                sp = _gram_tile(mats[1][ri], mats[1][rj], order) if mats[1].shape[1] else np.zeros((TILE, TILE), F32)
                ok = valid[ri][:, None] & valid[rj][None, :]
                if defect == "no_diagonal" and bx == jt:
                    ok = ok & ~np.eye(TILE, dtype=bool)
                if defect == "transposed_class_test":
                    same = labp[ri][None, :] == labp[rj][:, None]      # element (il, jl) tests lab_i[jl] against lab_j[il]
                else:
                    same = labp[ri][:, None] == labp[rj][None, :]
                sf64, sp64 = sf.astype(F64), sp.astype(F64)
                acc += [sf64[ok & same].sum(), sf64[ok & ~same].sum(), sp64[ok & same].sum(), sp64[ok & ~same].sum(),
                        np.abs(sf - sp)[ok].astype(F64).sum()]
                cnt[bx, by] += [(ok & same).sum(), (ok & ~same).sum()]
            parts[bx, by] = acc
    flat = parts.reshape(-1, 5)
    total = [math.fsum(flat[:, k].tolist()) for k in range(5)]
    return dict(zip(SUMS, total)), (int(cnt[..., 0].sum()), int(cnt[..., 1].sum()))


def audit_tolerance(F, P, labels=None, orders=("seq", "pair", "matmul")):
    """-> (reference sums, counts, tolerance per sum): MARGIN x the largest error of the three float32 restatements + the floor
    of this file's docstring."""
    ref, counts = audit_reference(F, P, labels)
    rests = [audit_emulate(F, P, labels, order=o)[0] for o in orders]
    D = max(np.asarray(F).shape[1], np.asarray(P).shape[1])
    pairs = dict(teacher_intra=counts[0], teacher_inter=counts[1], student_intra=counts[0], student_inter=counts[1],
                 absdiff=counts[0] + counts[1])
    tol = {k: MARGIN * max(abs(r[k] - ref[k]) for r in rests) + MARGIN * 2.0 ** -24 * math.sqrt(D) * math.sqrt(pairs[k])
           for k in SUMS}
    return ref, counts, tol


def means(sums, counts):
    """The host's divisions: the reference's five numbers (NaN where a selection is empty)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        i, o = F64(counts[0]), F64(counts[1])
        return dict(teacher_intra=F64(sums["teacher_intra"]) / i, teacher_inter=F64(sums["teacher_inter"]) / o,
                    student_intra=F64(sums["student_intra"]) / i, student_inter=F64(sums["student_inter"]) / o,
                    similarity_diff=F64(sums["absdiff"]) / (i + o))


def planted_exact(n, Df, Dp, classes=3):
    """Rows whose every similarity is exact in float32: one-hot rows scaled by a power of two (norms are powers of two, the
    normalised rows one-hot, every product 0 or 1).  -> (F, P, labels); F and P differ in which column a row takes."""
    i = np.arange(n)
    F = np.zeros((n, Df), dtype=F32)
    P = np.zeros((n, Dp), dtype=F32)
    F[i, (i * 7) % Df] = (2.0 ** ((i % 5) - 2)).astype(F32)
    P[i, (i * 3 + 1) % Dp] = (2.0 ** ((i % 3) - 1)).astype(F32) * np.where(i % 4 == 0, -1, 1).astype(F32)
    return F, P, (i % classes).astype(np.int64)

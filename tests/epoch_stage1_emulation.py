"""numpy restatement of ph_stage1_record_add (csrc/epochrec.hip): the stage-1 record and the survival
store, the all-pairs C-index under the ph_cindex_counts rule, and the defects the GPU cases of tests/test_gpu_epoch_stage1.py
must see.

Record: float32 values widened to float64 and added in call order - Python's `acc += t.item()`; exact counts; per head the
FIRST maximum; a label outside [0, C) counted once and left out of every head.  Store: row b of a call goes to column
cursor + b while that is < cap, the rest is dropped and counted; the cursor is read before it is advanced.  Everything is exact
(bitwise or integer): no tolerance."""
import numpy as np

from tests.epoch_emulation import REC_ADD, REC_ADD_POSITIVE, first_argmax

F32, F64 = np.float32, np.float64
COLUMNS = ("h_fuse", "h_path", "h_omic", "censor", "survtime")
DEFECTS = ("last_max", "ge_zero", "positive_takes_negzero", "positive_takes_nan", "bad_per_head", "cursor_advanced_first",
           "write_at_cap", "overflow_uncounted", "columns_swapped", "f32_accumulation", "heads_share_count")


def stage1_emulate(calls, cap=0, store=None, defect=None):
    """calls: dicts with optional keys scalars (float32 values), modes, heads (1-3 arrays [B, C]), grade [B], cols (five
    vectors [B], COLUMNS order).  store: float32 [5, cap + 1] when given - the extra column stands for the memory behind the
    store, which only the defect "write_at_cap" touches.
    -> dict(sums [16], added [16], correct [3], bad, steps, rows, cursor, overflow, store)."""
    sums, added = [0.0] * 16, [0] * 16
    if defect == "f32_accumulation":
        sums = [F32(0.0)] * 16
    correct = [0, 0, 0]
    bad = steps = rows = cursor = overflow = 0
    st = None if store is None else np.array(store, dtype=F32)
    for c in calls:
        for k, (v, mode) in enumerate(zip(c.get("scalars", ()), c.get("modes", ()))):
            v = F32(v)
            take = mode == REC_ADD or v > 0.0
            if mode == REC_ADD_POSITIVE:
                if defect == "ge_zero":
                    take = v >= 0.0
                elif defect == "positive_takes_negzero":
                    take = v > 0.0 or (v == 0.0 and np.signbit(v))
                elif defect == "positive_takes_nan":
                    take = not (v <= 0.0)
            if take:
                sums[k] = F32(sums[k] + v) if defect == "f32_accumulation" else sums[k] + float(v)     # `acc += t.item()`
                added[k] += 1
        B = None
        if c.get("heads"):
            heads = [np.asarray(h, dtype=F32) for h in c["heads"]]
            grade = np.asarray(c["grade"], dtype=np.int64)
            B, C = heads[0].shape
            for b in range(B):
                if grade[b] < 0 or grade[b] >= C:
                    bad += len(heads) if defect == "bad_per_head" else 1
                    continue
                for h, p in enumerate(heads):
                    if first_argmax(p[b], last=defect == "last_max") == grade[b]:
                        correct[0 if defect == "heads_share_count" else h] += 1
        if c.get("cols") is not None:
            cols = [np.asarray(x, dtype=F32).reshape(-1) for x in c["cols"]]
            if defect == "columns_swapped":
                cols[3], cols[4] = cols[4], cols[3]
            B = cols[0].shape[0]
            cur = cursor
            limit = cap + 1 if defect == "write_at_cap" else cap
            fit = min(B, max(limit - cur, 0))
            if defect == "cursor_advanced_first":
                cur = cursor + min(B, max(cap - cursor, 0))           # the rows land behind the step's own advance
                fit = min(B, max(limit - cur, 0))
            for k in range(5):
                st[k, cur:cur + fit] = cols[k][:fit]
            good = min(B, max(cap - cursor, 0))
            cursor += good
            if defect != "overflow_uncounted":
                overflow += B - good
        if B is not None:
            rows += B
        steps += 1
    return dict(sums=[float(s) for s in sums], added=added, correct=correct, bad=bad, steps=steps, rows=rows, cursor=cursor,
                overflow=overflow, store=st)


def reference_accumulation(steps, task):
    """The reference's statements written out literally ("MIA 2022/train_test_tSVD.py":455-467, :478-491; MIA-2023
    train_test_MT_SP_Masking.py:324-325) over per-step dicts of numpy float32 scalars / arrays: loss, loss_fuse, loss_path,
    loss_omic, loss_tsvd, loss_CRD, loss_pred_KD, pred_KD_masking_loss, pred / pred_path / pred_omic, grade | censor, survtime."""
    loss_epoch, loss_fuse_epoch, loss_path_epoch, loss_omic_epoch = 0, 0, 0, 0
    grad_acc_epoch, grad_path_epoch, grad_omic_epoch = 0, 0, 0
    loss_CRD_epoch, loss_KD_epoch = 0, 0
    loss_tsvd_epoch = 0
    loss_pred_KD_masking_epoch = 0
    risk_pred_all, risk_path_all, risk_omic_all = np.array([]), np.array([]), np.array([])
    censor_all, survtime_all = np.array([]), np.array([])
    for s in steps:
        loss_epoch += s["loss"].item()
        loss_fuse_epoch += (0 + s["loss_fuse"]).item()
        loss_path_epoch += (0 + s["loss_path"]).item()
        loss_omic_epoch += (0 + s["loss_omic"]).item()
        if s["loss_tsvd"] > 0.0:
            loss_tsvd_epoch += s["loss_tsvd"].item()
        if s["loss_CRD"] > 0.0:
            loss_CRD_epoch += s["loss_CRD"].item()
        if s["loss_pred_KD"] > 0.0:
            loss_KD_epoch += s["loss_pred_KD"].item()
        if s["pred_KD_masking_loss"] > 0.0:
            loss_pred_KD_masking_epoch += s["pred_KD_masking_loss"].item()
        if task == "surv":
            risk_pred_all = np.concatenate((risk_pred_all, s["pred"].reshape(-1)))
            risk_path_all = np.concatenate((risk_path_all, s["pred_path"].reshape(-1)))
            risk_omic_all = np.concatenate((risk_omic_all, s["pred_omic"].reshape(-1)))
            censor_all = np.concatenate((censor_all, s["censor"].reshape(-1)))
            survtime_all = np.concatenate((survtime_all, s["survtime"].reshape(-1)))
        elif task == "grad":
            grade = s["grade"]
            pred = s["pred"].argmax(axis=1).reshape(-1, 1)
            grad_acc_epoch += (pred == grade.reshape(pred.shape)).sum().item()
            pred_path = s["pred_path"].argmax(axis=1).reshape(-1, 1)
            grad_path_epoch += (pred_path == grade.reshape(pred_path.shape)).sum().item()
            pred_omic = s["pred_omic"].argmax(axis=1).reshape(-1, 1)
            grad_omic_epoch += (pred_omic == grade.reshape(pred_omic.shape)).sum().item()
    return dict(sums=[loss_epoch, loss_fuse_epoch, loss_path_epoch, loss_omic_epoch, loss_tsvd_epoch, loss_CRD_epoch,
                      loss_KD_epoch, loss_pred_KD_masking_epoch],
                correct=[grad_acc_epoch, grad_path_epoch, grad_omic_epoch],
                cols=[risk_pred_all, risk_path_all, risk_omic_all, censor_all, survtime_all])


def cindex_all_pairs(hazards, labels, survtime):
    """The ph_cindex_counts rule over all ordered pairs: (i, j) is comparable iff labels_i = 1 and (t_i < t_j, or t_i == t_j and
    labels_j = 0); concordant iff hazards_i > hazards_j, 0.5 on a tie (lifelines' concordance_index(t, -h, e))."""
    h, e, t = (np.asarray(a, dtype=F64).reshape(-1) for a in (hazards, labels, survtime))
    comp = (e[:, None] == 1) & ((t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & (e[None, :] == 0)))
    np.fill_diagonal(comp, False)
    conc = int((comp & (h[:, None] > h[None, :])).sum())
    tied = int((comp & (h[:, None] == h[None, :])).sum())
    n = int(comp.sum())
    if n == 0:
        raise ZeroDivisionError("No admissable pairs in the dataset.")
    return (conc + 0.5 * tied) / n


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
SPECIAL = [0.0, -0.0, -1.5, float("nan"), 2.5e-3, 1.0e30, 3.0]


def kernel_case(B, C, nh, ns, rng, cap=None):
    """Five calls on one record: the special values under both modes, tied maxima whose FIRST carries the label, labels -1 and
    C, heads that disagree; with `cap` the five survival columns as well (the heads stay: the entry takes both)."""
    calls = []
    for s in range(5):
        vals = [SPECIAL[(s + k) % len(SPECIAL)] if (k + s) % 2 else float(rng.standard_normal()) for k in range(ns)]
        modes = [1 if s % 2 else k % 2 for k in range(ns)]           # (ns = 1: -0.0 and the NaN meet the `> 0.0` mode)
        c = dict(scalars=vals, modes=modes)
        if nh:
            heads = [rng.standard_normal((B, C)).astype(F32) for _ in range(nh)]
            grade = rng.integers(0, C, size=B).astype(np.int64)
            if C > 1:
                p = heads[0]
                first = p[::2, :C - 1].argmax(axis=1)
                p[::2, C - 1] = p[::2, :C - 1].max(axis=1)           # the maximum again in the last column
                grade[::2] = first
            grade[1::7] = -1
            grade[3::11] = C
            c.update(heads=heads, grade=grade)
        if cap is not None:
            c["cols"] = [(100.0 * (s + 1) + 10.0 * k + rng.random(B)).astype(F32) for k in range(5)]
        calls.append(c)
    return calls

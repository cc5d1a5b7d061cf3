"""tests/epoch_stage1_emulation.py against the reference's accumulation statements written out literally and an all-pairs
numpy C-index, and the injected defects: each is caught on the very cases tests/test_gpu_epoch_stage1.py runs on the device."""
import math

import numpy as np
import pytest

from tests import epoch_stage1_emulation as S

F32 = np.float32
BS, CS = (1, 2, 63, 64, 65, 257), (1, 3, 16)


def _same(a, b):
    return len(a) == len(b) and all((x == y and math.copysign(1, x) == math.copysign(1, y)) or (x != x and y != y)
                                    for x, y in zip(a, b))


def _steps(task, n, B, rng, C=3):
    out = []
    for s in range(n):
        d = dict(loss=F32(rng.standard_normal() * 3), loss_fuse=F32(rng.random()), loss_path=F32(rng.random()),
                 loss_omic=F32(rng.random()), loss_tsvd=F32([0.0, 0.37, -0.0][s % 3]), loss_CRD=F32([7.25, 0.0][s % 2]),
                 loss_pred_KD=F32(rng.random() * 1e-3), pred_KD_masking_loss=F32([0.0, 0.0, 1.5][s % 3]))
        if task == "grad":
            d.update(pred=rng.standard_normal((B, C)).astype(F32), pred_path=rng.standard_normal((B, C)).astype(F32),
                     pred_omic=rng.standard_normal((B, C)).astype(F32), grade=rng.integers(0, C, size=B).astype(np.int64))
            d["pred"][0, :] = 1.0                                    # a full tie: numpy's argmax takes column 0 as well
        else:
            d.update(pred=rng.random((B, 1)).astype(F32), pred_path=rng.random((B, 1)).astype(F32),
                     pred_omic=rng.random((B, 1)).astype(F32), censor=(rng.random(B) > 0.3).astype(F32),
                     survtime=rng.integers(1, 9, size=B).astype(F32))
        out.append(d)
    return out


def _calls(steps, task):
    calls = []
    for s in steps:
        c = dict(scalars=[s[k] for k in ("loss", "loss_fuse", "loss_path", "loss_omic", "loss_tsvd", "loss_CRD", "loss_pred_KD",
                                         "pred_KD_masking_loss")], modes=[0] * 4 + [1] * 4)
        if task == "grad":
            c.update(heads=[s["pred"], s["pred_path"], s["pred_omic"]], grade=s["grade"])
        else:
            c["cols"] = [s["pred"], s["pred_path"], s["pred_omic"], s["censor"], s["survtime"]]
        calls.append(c)
    return calls


@pytest.mark.parametrize("task", ["grad", "surv"])
def test_restatement_equals_the_reference_statements(task):
    rng = np.random.default_rng(11)
    B, n = 7, 6
    steps = _steps(task, n, B, rng)
    ref = S.reference_accumulation(steps, task)
    cap = n * B
    got = S.stage1_emulate(_calls(steps, task), cap=cap, store=np.zeros((5, cap + 1), F32))
    assert _same(got["sums"][:8], [float(v) for v in ref["sums"]])
    assert got["steps"] == n and got["rows"] == n * B and got["overflow"] == 0
    if task == "grad":
        assert got["correct"] == ref["correct"] and got["bad"] == 0
    else:
        assert got["cursor"] == cap
        for k in range(5):
            assert np.array_equal(got["store"][k, :cap].astype(np.float64), ref["cols"][k])
        # the C-index of the stored columns under the ph_cindex_counts rule, against a plain double loop
        h, e, t = got["store"][0, :cap], got["store"][3, :cap], got["store"][4, :cap]
        conc = comp = 0.0
        for i in range(cap):
            for j in range(cap):
                if i != j and e[i] == 1 and (t[i] < t[j] or (t[i] == t[j] and e[j] == 0)):
                    comp += 1
                    conc += 1.0 if h[i] > h[j] else (0.5 if h[i] == h[j] else 0.0)
        assert S.cindex_all_pairs(h, e, t) == conc / comp
    # the TNN columns: added on the steps that ran the update only, no test on the value, divided by every step later
    calls = _calls(steps, task)
    tnn = [F32(3.5), F32(-0.0), F32(2.25)]
    want, k = 0, 0
    for s, c in enumerate(calls):
        if s % 2 == 0:
            c["scalars"] = c["scalars"] + [tnn[k], tnn[k]]
            c["modes"] = c["modes"] + [0, 0]
            want += float(tnn[k])
            k += 1
    got = S.stage1_emulate(calls, cap=cap, store=np.zeros((5, cap + 1), F32))
    assert got["sums"][8] == want == got["sums"][9] and got["added"][8] == 3 and got["added"][0] == n


def _caught(got, want, cap):
    """Whether a defective restatement differs from the right one in what the GPU test compares."""
    for k in ("added", "correct", "bad", "steps", "rows", "cursor", "overflow"):
        if got[k] != want[k]:
            return True
    if not _same(got["sums"], want["sums"]):
        return True
    return want["store"] is not None and not np.array_equal(got["store"], want["store"])        # guard column included


def test_every_defect_is_caught_by_the_gpu_cases():
    """The grid of tests/test_gpu_epoch_stage1.py: B x C x heads x scalars, and the store cases cap = B, cap = 3 B + 1."""
    seen = {d: 0 for d in S.DEFECTS}
    total = 0
    for B in BS:
        for C in CS:
            for nh, ns in ((1, 0), (2, 1), (3, 16)):
                for cap in (None, B, 3 * B + 1):
                    rng = np.random.default_rng(1000 * B + 10 * C + nh)
                    calls = S.kernel_case(B, C, nh, ns, rng, cap)
                    store = None if cap is None else np.full((5, cap + 1), -7.0, F32)
                    want = S.stage1_emulate(calls, cap or 0, store)
                    total += 1
                    for d in S.DEFECTS:
                        seen[d] += _caught(S.stage1_emulate(calls, cap or 0, store, defect=d), want, cap)
    print("\ncases %d, caught per defect: %s" % (total, seen))
    assert len(S.DEFECTS) >= 10 and all(v > 0 for v in seen.values()), seen
    # and where a defect must show on EVERY case that can show it
    for B in BS:
        rng = np.random.default_rng(B)
        calls = S.kernel_case(B, 3, 3, 16, rng, 3 * B + 1)
        store = np.full((5, 3 * B + 2), -7.0, F32)
        want = S.stage1_emulate(calls, 3 * B + 1, store)
        assert want["overflow"] == 2 * B - 1 and want["cursor"] == 3 * B + 1 and (want["store"][:, -1] == -7.0).all()
        for d in ("ge_zero", "positive_takes_negzero", "positive_takes_nan", "cursor_advanced_first", "write_at_cap",
                  "overflow_uncounted", "columns_swapped", "f32_accumulation", "heads_share_count"):
            assert _caught(S.stage1_emulate(calls, 3 * B + 1, store, defect=d), want, 3 * B + 1), (B, d)
        if B >= 12:                                                   # (a label outside [0, C) needs row 1 or 3; a tie row 0)
            assert _caught(S.stage1_emulate(calls, 3 * B + 1, store, defect="bad_per_head"), want, 3 * B + 1)
        assert _caught(S.stage1_emulate(calls, 3 * B + 1, store, defect="last_max"), want, 3 * B + 1) or B < 2

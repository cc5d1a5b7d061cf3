"""The three kernels of csrc/evalmetrics.hip through the C ABI against their numpy restatements (tests/eval_emulation.py, itself
held to sklearn and pandas by tests/test_eval_emulation_cpu.py).  Every output - and the workspace, exactly
ph_rank_counts_workspace_bytes long - lies between sentinel guard bands (gpu_util.Guarded).

ph_rank_counts: the integer counts bit for bit; ap_sum within M * 2^-52 of the restatement (which adds in the kernel's order,
so the difference is expected to be 0) and bitwise equal between two runs; a NaN score sets the flag and nothing else goes
wrong.  ph_confusion_counts and ph_group_agg (max and mean): bit for bit."""
import numpy as np
import pytest
import torch

from tests import eval_emulation as E
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

T = E.TILE
I64, F64, F32, I32 = torch.int64, torch.float64, torch.float32, torch.int32


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def _rank(pred, grade):
    """Two runs of ph_rank_counts on fresh guarded buffers -> (counts [4] list, ap_sum float) of the first; asserts the
    guards and the bitwise equality of the two runs."""
    L, ptr, st = _api()
    N, C = pred.shape
    nbytes = L.ph_rank_counts_workspace_bytes(N, C)
    assert nbytes == 8 * (-(-N * C // T))
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
    runs = []
    for _ in range(2):
        counts, ap, ws = Guarded((4,), I64, fill=-7), Guarded((1,), F64), Guarded((nbytes // 8,), F64)
        assert L.ph_rank_counts(ptr(dp), ptr(dg), N, C, ptr(counts.t), ptr(ap.t), ptr(ws.t), st) == E.OK
        torch.cuda.synchronize()
        assert counts.guards_intact() and ap.guards_intact() and ws.guards_intact()
        assert not bool(torch.isnan(ws.t).any()), "a block partial was never written"
        runs.append((counts.t.cpu().tolist(), ap.t.cpu().numpy().copy()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1].view(np.int64)[0] == runs[1][1].view(np.int64)[0], "ap_sum differs between two runs"
    return runs[0][0], float(runs[0][1][0])


# M = 2, 3, T - 1, T, T + 1, 3 T + 1, 12 288; C = 3 where 3 divides M, else 2 or (odd M) 1
RANK_SHAPES = ((1, 2), (1, 3), (85, 3), (128, 2), (257, 1), (769, 1), (4096, 3))


@pytest.mark.parametrize("N,C", RANK_SHAPES)
def test_rank_counts_vs_restatement(N, C):
    M = N * C
    assert M in (2, 3, T - 1, T, T + 1, 3 * T + 1, 12288)
    for k, kind in enumerate(("distinct", "ties", "equal", "logprob")):
        pred, grade = E.scores(kind, N, C, seed=100 + 2 * k + 1)
        if C == 1:
            grade = (np.arange(N) % 3 == 1).astype(np.int64)       # label = (grade == 0); the rows of "class 1" are flagged
        if kind == "logprob":
            assert pred.max() <= 0
        P, conc, tied, bad, ap_sum = E.rank_counts_ref(pred, grade)
        counts, got_ap = _rank(pred, grade)
        print(f"M={M} C={C} {kind}: counts {counts} ap_sum {got_ap!r} (restatement {ap_sum!r})")
        assert counts == [P, conc, tied, bad], (kind, counts, (P, conc, tied, bad))
        assert abs(got_ap - ap_sum) <= M * 2.0 ** -52, (kind, got_ap, ap_sum)


def test_rank_counts_nan_score_sets_the_flag():
    pred, grade = E.scores("logprob", 300, 3, seed=8)
    pred[17, int(grade[17])] = np.nan          # a positive pair
    pred[40, int((grade[40] + 1) % 3)] = np.inf  # and an infinite negative one
    P, conc, tied, bad, ap_sum = E.rank_counts_ref(pred, grade)
    counts, got_ap = _rank(pred, grade)
    assert bad == 2 and counts == [P, conc, tied, 2]
    assert np.isfinite(got_ap) and abs(got_ap - ap_sum) <= 900 * 2.0 ** -52
    grade2 = grade.copy(); grade2[5] = 3; grade2[6] = -1
    clean, _ = E.scores("logprob", 300, 3, seed=8)
    counts, _ = _rank(clean, grade2)
    assert counts == list(E.rank_counts_ref(clean, grade2)[:4]) and counts[3] == 2


@pytest.mark.parametrize("N", (1, 255, 256, 257))
def test_confusion_counts_vs_restatement(N):
    L, ptr, st = _api()
    for C, kind in ((3, "ties"), (3, "logprob"), (16, "ties"), (1, "equal")):
        pred, grade = E.scores(kind, N, C, seed=N + C)
        if kind == "ties":
            assert N == 1 or (np.sort(pred, axis=1)[:, -1] == np.sort(pred, axis=1)[:, -2]).any()      # ties for the maximum
        if N > 1:
            grade[N // 2] = C                      # one label out of range: the row is left out
        dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
        conf = Guarded((C, C), I64, fill=-7)
        assert L.ph_confusion_counts(ptr(dp), ptr(dg), N, C, ptr(conf.t), st) == E.OK
        torch.cuda.synchronize()
        assert conf.guards_intact()
        ref = E.confusion_ref(pred, grade)
        assert np.array_equal(conf.t.cpu().numpy(), ref), (N, C, kind)
        assert int(ref.sum()) == N - (1 if N > 1 else 0)


def _agg(x, offsets, order, fun):
    L, ptr, st = _api()
    N, C = x.shape
    G = len(offsets) - 1
    dx, do, dr = torch.from_numpy(x).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(order).cuda()
    out = Guarded((G, C), F32)
    rc = L.ph_group_agg(ptr(dx), ptr(do), ptr(dr), offsets.ctypes.data, N, C, G, {"mean": 0, "max": 1}[fun], ptr(out.t), st)
    assert rc == E.OK
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.t.cpu().numpy()


def _group_cases(N):
    rng = np.random.default_rng(N)
    cases = {"one group holding all rows": np.zeros(N, dtype=np.int64), "groups of one row": rng.permutation(N)}
    if N >= 9:
        G = 4 if N == 9 else 29
        g = rng.integers(1, G, N)
        g[:G - 1] = rng.permutation(G - 1) + 1      # interleaved, none empty ...
        g[N // 2] = 0                                # ... and group 0 has exactly one row, in the middle
        cases["interleaved groups, one of a single row"] = g
    return cases


@pytest.mark.parametrize("N", (1, 9, 257))
def test_group_agg_vs_restatement(N):
    for what, g in _group_cases(N).items():
        G = int(g.max()) + 1
        offsets, order = E.csr(g, G)
        for C, seed in ((3, 1), (5, 2)):
            x, _ = E.scores("logprob", N, C, seed=seed)
            x = x - np.float32(0.0625)
            assert x.max() < 0                        # all negative: a maximum started at 0 would show
            for fun in ("max", "mean"):
                got, ref = _agg(x, offsets, order, fun), E.group_agg_ref(x, offsets, order, fun)
                assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (what, N, C, fun, np.abs(got - ref).max())


def test_wrappers_and_grading_metrics_device_vs_sklearn():
    """ops.rank_counts / confusion_counts / group_agg and evaluate.grading_metrics_device: sklearn's four numbers within
    M * 2^-52 (F1 exactly); the refusals of the Python layer."""
    import multimodal_learning_amd as m
    from sklearn import metrics as skm
    pred, grade = E.scores("logprob", 301, 3, seed=3)
    M = pred.size
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
    got = m.evaluate.grading_metrics_device(dp, dg)
    onehot = np.eye(3, dtype=np.int64)[grade]
    arg = pred.argmax(axis=1)
    ref = (skm.roc_auc_score(onehot, pred, average="micro"), skm.average_precision_score(onehot, pred, average="micro"),
           skm.f1_score(grade, arg, average="micro"), skm.f1_score(grade, arg, average=None)[2])
    print("device", got, "sklearn", ref)
    assert abs(got[0] - ref[0]) <= M * 2.0 ** -52 and abs(got[1] - ref[1]) <= M * 2.0 ** -52
    assert got[2] == ref[2] and got[3] == ref[3]
    assert np.allclose(got, m.evaluate.grading_metrics(onehot, pred), rtol=0, atol=M * 2.0 ** -52)
    bad = dp.clone(); bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        m.evaluate.grading_metrics_device(bad, dg)
    with pytest.raises(ValueError):
        m.evaluate.grading_metrics_device(dp[:, :1].contiguous(), torch.zeros_like(dg))       # no negative pair
    offsets, order = m.ops.group_csr(np.arange(301) % 7, 7)
    ref_off, ref_ord = E.csr(np.arange(301) % 7, 7)
    assert np.array_equal(offsets, ref_off) and np.array_equal(order, ref_ord)
    do, dr = torch.from_numpy(offsets).cuda(), torch.from_numpy(order).cuda()
    out = m.ops.group_agg(dp, do, dr, offsets, "max").cpu().numpy()
    assert np.array_equal(out, E.group_agg_ref(pred, offsets, order, "max"))
    with pytest.raises(ValueError, match="mean.*max"):
        m.ops.group_agg(dp, do, dr, offsets, "p0.75")
    empty = offsets.copy(); empty[3] = empty[2]
    with pytest.raises(ValueError):
        m.ops.group_agg(dp, do, dr, empty, "max")

"""ph_rank_counts_classes and ph_roc_points through the C ABI against their numpy restatements (tests/evalavg_emulation.py,
itself held to sklearn by tests/test_evalavg_emulation_cpu.py), and the layers above them: ops.rank_counts_classes /
roc_points, evaluate.grading_metrics_device(avg=...), roc_curve_device, and the avg= / curves= forms of test_patches and
test_teacher_patches.

The kernels: counts, the BITS of ap_sum (the restatement adds in the kernel's order), the points and npoints are equal to the
restatement exactly, and two runs of ph_rank_counts_classes agree bitwise.  Every output and the workspace - exactly as long as the workspace query
says - lie between sentinel guard bands (gpu_util.Guarded); the tail of the point arrays past npoints[0] keeps its fill value.
The wrappers against sklearn: floats within M * 2^-52 (M = N per class, N * C for an average over the classes - the rule of
tests/test_evalavg_emulation_cpu.py), curves as equal arrays."""
import numpy as np
import pytest
import torch

from tests import eval_emulation as E0
from tests import evalavg_emulation as E
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

T = E.TILE
I64, F64, F32, I32 = torch.int64, torch.float64, torch.float32, torch.int32
EPS = 2.0 ** -52
THR_FILL = -12345.0


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def _classes(pred, grade):
    """Two runs of ph_rank_counts_classes on fresh guarded buffers -> (counts int64 [C, 4], ap_sum float64 [C]) of the first;
    asserts the guards and the bitwise equality of the two runs."""
    L, ptr, st = _api()
    N, C = pred.shape
    nbytes = L.ph_rank_counts_classes_workspace_bytes(N, C)
    assert nbytes == 8 * C * (-(-N // T))
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
    runs = []
    for _ in range(2):
        counts, ap, ws = Guarded((C, 4), I64, fill=-7), Guarded((C,), F64), Guarded((nbytes // 8,), F64)
        assert L.ph_rank_counts_classes(ptr(dp), ptr(dg), N, C, ptr(counts.t), ptr(ap.t), ptr(ws.t), st) == E.OK
        torch.cuda.synchronize()
        assert counts.guards_intact() and ap.guards_intact() and ws.guards_intact()
        assert not bool(torch.isnan(ws.t).any()), "a block partial was never written"
        runs.append((counts.t.cpu().numpy().copy(), ap.t.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1].view(np.int64), runs[1][1].view(np.int64)), "ap_sum differs between two runs"
    return runs[0]


def _roc(pred, grade, cls):
    """ph_roc_points on guarded buffers -> (fps, tps, thr of the npoints[0] points, bad); asserts the guards and that the tail
    of the three arrays keeps its fill value."""
    L, ptr, st = _api()
    N, C = pred.shape
    M = N if cls >= 0 else N * C
    nbytes = L.ph_roc_points_workspace_bytes(N, C)
    assert nbytes == 12 * N * C
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
    fps, tps, thr = Guarded((M,), I32, fill=-7), Guarded((M,), I32, fill=-7), Guarded((M,), F32, fill=THR_FILL)
    npts, ws = Guarded((2,), I32, fill=-7), Guarded((nbytes // 4,), I32, fill=-7)
    assert L.ph_roc_points(ptr(dp), ptr(dg), N, C, cls, ptr(fps.t), ptr(tps.t), ptr(thr.t), ptr(npts.t), ptr(ws.t), st) == E.OK
    torch.cuda.synchronize()
    for g in (fps, tps, thr, npts, ws):
        assert g.guards_intact()
    K, bad = npts.t.cpu().tolist()
    assert 0 <= K <= M
    f, t, h = fps.t.cpu().numpy(), tps.t.cpu().numpy(), thr.t.cpu().numpy()
    assert (f[K:] == -7).all() and (t[K:] == -7).all() and (h[K:] == np.float32(THR_FILL)).all(), "the unwritten tail was written"
    return f[:K].copy(), t[:K].copy(), h[:K].copy(), bad


def _check_classes(pred, grade):
    counts, ap = _classes(pred, grade)
    ref_counts, ref_ap = E.rank_counts_classes_ref(pred, grade)
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    assert np.array_equal(ap.view(np.int64), ref_ap.view(np.int64)), (ap, ref_ap)
    return counts, ap


def _check_roc(pred, grade, cls):
    got, ref = _roc(pred, grade, cls), E.roc_points_ref(pred, grade, cls)
    for what, a, b in zip(("fps", "tps", "thr"), got[:3], ref[:3]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), (cls, what)
    assert got[3] == ref[3], cls
    return got


@pytest.mark.parametrize("N", (1, 2, 255, 256, 257, 513, 1025))
def test_kernels_vs_restatement(N):
    """N at one element and at the tile edge 256 from both sides; with C = 2, 3, 16 the micro problem M = N * C crosses
    tile edges that N does not."""
    for C in (1, 2, 3, 16):
        for k, kind in enumerate(("decimal", "continuous")):
            pred, grade = E.scores(kind, N, C, seed=1000 + 10 * C + k)
            counts, _ = _check_classes(pred, grade)
            assert int(counts[:, 0].sum()) == N and not counts[:, 3].any()
            for cls in [-1] + list(range(C)):
                fps, tps, thr, bad = _check_roc(pred, grade, cls)
                M = N if cls >= 0 else N * C
                assert bad == 0 and fps[-1] + tps[-1] == M and tps[-1] == (counts[cls, 0] if cls >= 0 else N)


def test_special_inputs():
    # a class that no label has
    pred, grade = E.scores("decimal", 300, 4, seed=1)
    grade[grade == 2] = 3
    counts, ap = _check_classes(pred, grade)
    assert counts[2].tolist() == [0, 0, 0, 0] and ap[2] == 0.0
    fps, tps, thr, bad = _check_roc(pred, grade, 2)
    assert not tps.any() and fps[-1] == 300 and bad == 0
    # all scores equal: one point
    pred, grade = E.scores("equal", 300, 3, seed=2)
    counts, ap = _check_classes(pred, grade)
    assert not counts[:, 1].any() and counts[:, 2].tolist() == [int(p * (300 - p)) for p in counts[:, 0]]
    for cls in (-1, 1):
        fps, tps, thr, bad = _check_roc(pred, grade, cls)
        assert thr.tolist() == [-1.25] and fps[0] + tps[0] == (300 if cls >= 0 else 900)
    # strictly increasing scores: M points
    pred, grade = E.scores("increasing", 300, 3, seed=3)
    _check_classes(pred, grade)
    for cls in (-1, 0, 2):
        fps, tps, thr, bad = _check_roc(pred, grade, cls)
        M = 300 if cls >= 0 else 900
        assert thr.shape[0] == M and (np.diff(thr) < 0).all() and (fps + tps == np.arange(1, M + 1)).all()
    # a NaN in one column: flagged in that class only, the other classes as without it
    clean, grade = E.scores("decimal", 300, 3, seed=4)
    pred = clean.copy()
    pred[17, 1] = np.nan
    pred[40, 1] = np.inf
    counts, ap = _check_classes(pred, grade)
    ref_counts, ref_ap = E.rank_counts_classes_ref(clean, grade)
    assert counts[:, 3].tolist() == [0, 2, 0]
    for c in (0, 2):
        assert np.array_equal(counts[c], ref_counts[c]) and ap[c] == ref_ap[c]
    fps, tps, thr, bad = _check_roc(pred, grade, 1)
    assert bad == 2 and fps[-1] + tps[-1] == 299 and thr[0] == np.inf
    assert _check_roc(pred, grade, 0)[3] == 0 and _check_roc(pred, grade, -1)[3] == 2
    # labels outside [0, C): counted once, in class 0; the rows are negatives of every class
    grade2 = grade.copy(); grade2[5] = 3; grade2[6] = -1
    counts, ap = _check_classes(clean, grade2)
    assert counts[:, 3].tolist() == [2, 0, 0] and int(counts[:, 0].sum()) == 298
    for cls in (-1, 0, 2):
        assert _check_roc(clean, grade2, cls)[3] == 2


def test_many_blocks():
    """N = 20 000, C = 3: 79 row blocks (the finish kernel adds 79 partials per class), 235 blocks of the micro problem."""
    pred, grade = E.scores("decimal", 20000, 3, seed=7)
    _check_classes(pred, grade)
    _check_roc(pred, grade, -1)
    _check_roc(pred, grade, 1)
    pred, grade = E.scores("continuous", 20000, 3, seed=8)
    _check_classes(pred, grade)
    fps, tps, thr, bad = _check_roc(pred, grade, 2)
    assert thr.shape[0] == np.unique(pred[:, 2]).shape[0]


def test_wrappers_vs_sklearn():
    import multimodal_learning_amd as m
    from sklearn import metrics as skm
    EV = m.evaluate
    pred, grade = E.scores("decimal", 301, 3, seed=3)
    N, C = pred.shape
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(grade).cuda()
    onehot, arg, s64 = np.eye(3, dtype=np.int64)[grade], pred.argmax(axis=1), pred.astype(np.float64)
    f1_iv = skm.f1_score(grade, arg, average=None)[2]
    for avg in ("macro", "weighted", None):
        got = EV.grading_metrics_device(dp, dg, avg)
        ref = (skm.roc_auc_score(onehot, s64, average=avg), skm.average_precision_score(onehot, s64, average=avg),
               skm.f1_score(grade, arg, average=avg))
        print(avg, "device", got, "sklearn", ref)
        tol = (N if avg is None else N * C) * EPS
        for a, b in zip(got[:3], ref):
            assert np.abs(np.asarray(a) - np.asarray(b)).max() <= tol, (avg, a, b)
        assert got[3] == f1_iv
    # micro: the call it was, bit for bit
    assert EV.grading_metrics_device(dp, dg, "micro") == EV.grading_metrics_device(dp, dg)
    micro = m.ops.rank_counts(dp, dg).cpu().tolist()
    per = m.ops.rank_counts_classes(dp, dg).cpu()
    ref_counts, ref_ap = E.rank_counts_classes_ref(pred, grade)
    assert np.array_equal(per[:12].view(3, 4).numpy(), ref_counts) and np.array_equal(per[12:].numpy(), ref_ap.view(np.int64))
    assert int(per[:12].view(3, 4)[:, 0].sum()) == micro[0] == N
    out = torch.full((17,), -1, device="cuda", dtype=I64)
    m.ops.rank_counts_classes(dp, dg, out=out[1:16])
    assert out[0].item() == -1 and out[16].item() == -1 and torch.equal(out[1:16].cpu(), per)
    # the curves
    auc_c = EV.grading_metrics_device(dp, dg, None)[0]
    for cls in (0, 1, 2, "micro"):
        s, l = (pred[:, cls], grade == cls) if cls != "micro" else (pred.reshape(-1), onehot.reshape(-1) == 1)
        for drop in (True, False):
            got = EV.roc_curve_device(dp, dg, cls, drop_intermediate=drop)
            ref = skm.roc_curve(l.astype(np.int64), s, drop_intermediate=drop)
            for a, b in zip(got, ref):
                assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b), (cls, drop)
            area = EV.roc_auc_from_curve(got[0], got[1])
            assert area == skm.auc(ref[0], ref[1])
            if cls != "micro":
                assert abs(area - auc_c[cls]) <= N * EPS
    assert EV.roc_curve_device(dp, dg)[0].shape == EV.roc_curve_device(dp, dg, "micro")[0].shape
    buf, again = m.ops.roc_points(dp, dg, -1).cpu(), m.ops.roc_points(dp, dg, "micro").cpu()
    M, K = N * C, int(buf[0])
    assert buf.dtype == I32 and buf.shape == (2 + 3 * M,) and K == np.unique(pred).shape[0]
    for at in (0, 2, 2 + M, 2 + 2 * M):                      # (the entries past the K points are left unwritten)
        assert torch.equal(buf[at:at + (2 if at == 0 else K)], again[at:at + (2 if at == 0 else K)])
    fps, tps, thr, _ = E.roc_points_ref(pred, grade, -1)
    assert np.array_equal(buf[2:2 + K].numpy(), fps) and np.array_equal(buf[2 + M:2 + M + K].numpy(), tps)
    assert np.array_equal(buf[2 + 2 * M:2 + 2 * M + K].view(F32).numpy(), thr)
    # refusals
    with pytest.raises(ValueError, match="avg"):
        EV.grading_metrics_device(dp, dg, "samples")
    nan = dp.clone(); nan[3, 1] = float("nan")
    for avg in ("macro", "weighted", None):
        with pytest.raises(ValueError, match="non-finite"):
            EV.grading_metrics_device(nan, dg, avg)
    with pytest.raises(ValueError, match="non-finite"):
        EV.roc_curve_device(nan, dg, 1)
    absent = dg.clone(); absent[absent == 1] = 0
    with pytest.raises(ValueError, match="class 1"):
        EV.grading_metrics_device(dp, absent, "macro")
    with pytest.raises(ValueError, match="class 1"):
        EV.roc_curve_device(dp, absent, 1)
    for cls in (3, -2, "macro"):
        with pytest.raises(ValueError):
            m.ops.roc_points(dp, dg, cls)
    with pytest.raises(ValueError):
        m.ops.rank_counts_classes(torch.zeros(4, 17, device="cuda"), torch.zeros(4, device="cuda", dtype=I64))


# ---- the avg= / curves= forms of the patch passes, on the tiny networks and loader of tests/test_gpu_eval_patches.py
N_ROI, SH, S = 4, 96, 64
PATIENTS = ["TCGA-a", "TCGA-a", "TCGA-b", "TCGA-c"]
GRADES = [2, 2, 0, 1]


def _opt(**kw):
    from oracle.step import default_opt
    return default_opt(dropout_rate=0.25, input_size_path=S, batch_size=16, **kw)


@pytest.fixture(scope="module")
def setup():
    import multimodal_learning_amd as m
    from oracle import weights as W
    g = torch.Generator().manual_seed(11)
    tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8)
    omic = torch.randn(N_ROI, 320, generator=g)
    opt = _opt()
    student = m.define_net(opt, 1, path_only=True); teacher = m.define_net(opt, 1)
    student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    ld = m.augment.ResidentPatchLoader(opt, tiles.cuda(), omic, torch.tensor(GRADES), patient=PATIENTS)
    return opt, student.cuda(), teacher.cuda(), ld


def _same_curves(got, y_pred, ld):
    import multimodal_learning_amd as m
    dev = torch.from_numpy(y_pred).cuda()
    assert list(got) == [0, 1, 2, "micro"]
    for cls, curve in got.items():
        want = m.evaluate.roc_curve_device(dev, ld.patient_grade, cls)
        assert len(curve) == 3 and all(np.array_equal(a, b) for a, b in zip(curve, want)), cls


def test_patches_avg_and_curves(setup):
    import multimodal_learning_amd as m
    EV = m.evaluate
    opt, student, teacher, ld = setup
    base_patch, base = EV.test_patches(opt, teacher, student, ld, "cuda")
    keys = {"patients", "y_label", "y_pred_path", "y_pred_fuse", "metrics_path", "metrics_fuse", "agg"}
    assert set(base) == keys
    patch, pat = EV.test_patches(opt, teacher, student, ld, "cuda", avg="macro", curves=True)
    assert set(pat) == keys | {"avg", "roc_path", "roc_fuse"} and pat["avg"] == "macro"
    assert np.array_equal(pat["y_pred_path"], base["y_pred_path"]) and np.array_equal(patch[6][6], base_patch[6][6])
    for name, rows in (("path", patch[6][6]), ("fuse", patch[6][5])):
        y_pred = pat["y_pred_" + name]
        assert pat["metrics_" + name] == list(EV.grading_metrics_device(torch.from_numpy(y_pred).cuda(), ld.patient_grade, "macro"))
        sk = EV.grading_metrics(pat["y_label"], y_pred, avg="macro")
        assert np.abs(np.asarray(pat["metrics_" + name]) - np.asarray(sk, dtype=np.float64)).max() <= 9 * EPS, name
        _same_curves(pat["roc_" + name], y_pred, ld)
    d_grade = torch.tensor(GRADES).repeat_interleave(9).cuda()
    assert patch[5] == list(EV.grading_metrics_device(torch.from_numpy(patch[6][6]).cuda(), d_grade, "macro"))
    # per class: three arrays and the F1 of grade IV; student-only: no fuse branch, no curve for it
    patch, pat = EV.test_patches(opt, None, student, ld, "cuda", avg=None, curves=True)
    assert pat["avg"] is None and "roc_fuse" not in pat and pat["metrics_fuse"] is None
    assert [np.shape(v) for v in pat["metrics_path"]] == [(3,), (3,), (3,), ()]
    with pytest.raises(ValueError, match="avg"):
        EV.test_patches(opt, None, student, ld, "cuda", avg="samples")


def test_teacher_patches_avg_and_curves(setup):
    import multimodal_learning_amd as m
    EV = m.evaluate
    opt, student, teacher, ld = setup
    names = ("fuse", "path", "omic")
    keys = {"patients", "y_label", "agg"} | {p + n for p in ("y_pred_", "metrics_") for n in names}
    base_patch, base = EV.test_teacher_patches(opt, teacher, ld, "cuda")
    assert set(base) == keys
    patch, pat = EV.test_teacher_patches(opt, teacher, ld, "cuda", avg="macro", curves=True)
    assert set(pat) == keys | {"avg"} | {"roc_" + n for n in names} and pat["avg"] == "macro"
    d_grade = torch.tensor(GRADES).repeat_interleave(9).cuda()
    for k, name in enumerate(names):
        y_pred = pat["y_pred_" + name]
        assert np.array_equal(y_pred, base["y_pred_" + name])
        assert pat["metrics_" + name] == list(EV.grading_metrics_device(torch.from_numpy(y_pred).cuda(), ld.patient_grade, "macro"))
        _same_curves(pat["roc_" + name], y_pred, ld)
        rows = torch.from_numpy(patch[13][5 + k]).cuda()
        assert patch[12][4 * k:4 * k + 4] == list(EV.grading_metrics_device(rows, d_grade, "macro"))
    with pytest.raises(ValueError, match="avg"):
        EV.test_teacher_patches(opt, teacher, ld, "cuda", avg="samples")

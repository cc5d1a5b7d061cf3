"""The patch-level test pass: augment.ResidentPatchLoader, evaluate.test_patches,
aggregate_by_patient and grading_metrics_device on 4 ROIs of 96 x 96, S = 64, grid 3 (stride 16): 36 rows, batches of
16, 16, 4; three patients (2 + 1 + 1 ROIs); a small student and a teacher.

References: the numpy cut (tests/eval_emulation.py), evaluate.test on the same loader, pandas' groupby and sklearn on the
copied rows.  Metric tolerance M * 2^-52 (M = rows x classes of the split scored), the aggregated rows exact for max and
within one float32 ulp for mean."""
import numpy as np
import pytest
import torch

from tests import eval_emulation as E
from tests.gpu_util import count_host_reads

pytestmark = pytest.mark.gpu

N_ROI, SH, S, GRID = 4, 96, 64, 3
PATIENTS = ["TCGA-a", "TCGA-a", "TCGA-b", "TCGA-c"]
GRADES = [2, 2, 0, 1]


def _opt(**kw):
    from oracle.step import default_opt
    return default_opt(dropout_rate=0.25, input_size_path=S, batch_size=16, **kw)


@pytest.fixture(scope="module")
def store():
    g = torch.Generator().manual_seed(11)
    tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8)
    omic = torch.randn(N_ROI, 320, generator=g)
    return tiles, omic, torch.tensor(GRADES)


@pytest.fixture(scope="module")
def nets():
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt = _opt()
    student = m.define_net(opt, 1, path_only=True); teacher = m.define_net(opt, 1)
    student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    return student.cuda(), teacher.cuda()


def _loader(store, opt=None, **kw):
    import multimodal_learning_amd as m
    tiles, omic, grade = store
    kw.setdefault("patient", PATIENTS)
    return m.augment.ResidentPatchLoader(opt or _opt(), tiles.cuda(), omic, grade, **kw)


@pytest.fixture(scope="module")
def passes(store, nets):
    """One test_patches pass per aggregation and one evaluate.test pass over the same loader, shared by the tests below."""
    import multimodal_learning_amd as m
    student, teacher = nets
    opt = _opt()
    ld = _loader(store, opt)
    ref = m.evaluate.test(opt, teacher, student, ld, "cuda")
    out = {agg: m.evaluate.test_patches(opt, teacher, student, ld, "cuda", agg=agg) for agg in ("max", "mean")}
    return ld, ref, out


def test_loader_geometry_and_attributes(store):
    ld = _loader(store)
    assert len(ld) == 3 and len(ld.dataset) == 36 and ld.num_patients == 3 and ld.patients == ["TCGA-a", "TCGA-b", "TCGA-c"]
    assert ld.row_patient.dtype == torch.int64 and ld.row_patient.is_cuda
    assert ld.row_patient.cpu().tolist() == [0] * 18 + [1] * 9 + [2] * 9
    assert ld.patient_grade.cpu().tolist() == [2, 0, 1] and ld.patient_grade.dtype == torch.int64
    one = _loader(store, patient=None)
    assert one.num_patients == 4 and one.patients == [0, 1, 2, 3] and one.row_patient.cpu().tolist() == sum(([k] * 9 for k in range(4)), [])


def test_every_patch_equals_the_numpy_cut(store):
    tiles, omic, grade = store
    ld = _loader(store)
    batches = list(ld)
    assert [b[0].shape[0] for b in batches] == [16, 16, 4]
    for b in batches:
        assert len(b) == 6 and b[0].dtype == torch.float32 and tuple(b[0].shape[1:]) == (3, S, S)
    x = torch.cat([b[0] for b in batches]).cpu().numpy()
    rows = E.patch_rows(N_ROI, SH, SH, S, GRID)
    assert len(rows) == 36
    t8 = tiles.numpy()
    for r, (roi, top, left) in enumerate(rows):
        assert np.array_equal(x[r].view(np.int32), E.cut(t8, roi, top, left, S).view(np.int32)), (r, roi, top, left)
    # by hand: row 2 = ROI 0, cell (0, 2): top 0, left 32 (a corner); row 9 + 4 = ROI 1, cell (1, 1): top 16, left 16 (the centre)
    hand = lambda roi, top, left: ((t8[roi, top:top + S, left:left + S].astype(np.float32) / np.float32(255) - np.float32(0.5))
                                   / np.float32(0.5)).transpose(2, 0, 1)
    assert np.array_equal(x[2], hand(0, 0, 32)) and np.array_equal(x[13], hand(1, 16, 16))
    assert np.array_equal(x[35], hand(3, 32, 32))
    assert torch.equal(torch.cat([b[2] for b in batches]).cpu(), omic.float().repeat_interleave(9, 0))
    assert torch.cat([b[5] for b in batches]).cpu().tolist() == sum(([g] * 9 for g in GRADES), [])
    # grid 1: the centre crop
    c = _loader(store, grid=1)
    xb = torch.cat([b[0] for b in c]).cpu().numpy()
    assert len(c.dataset) == 4 and np.array_equal(xb[3], hand(3, 16, 16))


def test_patch_result_is_evaluate_test_bit_for_bit(passes):
    ld, ref, out = passes
    patch, _ = out["max"]
    assert len(patch) == 9 and patch[0] == ref[0] and patch[4] == ref[4] and patch[1:4] == (None, None, None)
    for k in (5, 6, 8):
        assert patch[6][k].dtype == ref[6][k].dtype and np.array_equal(patch[6][k], ref[6][k]), k
    assert np.array_equal(patch[8][1], ref[8][1]) and np.array_equal(patch[8][3], ref[8][3])
    assert patch[6][6].shape == (36, 3) and patch[7] == [None, None, None]
    M = 36 * 3
    print("patch metrics: device", patch[5], "sklearn", ref[5])
    assert np.abs(np.asarray(patch[5]) - np.asarray(ref[5], dtype=np.float64)).max() <= M * 2.0 ** -52


@pytest.mark.parametrize("agg", ("max", "mean"))
def test_patient_result_vs_pandas_and_sklearn(passes, agg):
    import pandas as pd
    import multimodal_learning_amd as m
    ld, ref, out = passes
    patch, pat = out[agg]
    assert set(pat) == {"patients", "y_label", "y_pred_path", "y_pred_fuse", "metrics_path", "metrics_fuse", "agg"}
    assert pat["patients"] == ["TCGA-a", "TCGA-b", "TCGA-c"] and pat["agg"] == agg
    assert np.array_equal(pat["y_label"], np.eye(3, dtype=np.float32)[[2, 0, 1]])
    ids = np.repeat(np.asarray(PATIENTS), 9)
    for key, mkey, probs in (("y_pred_path", "metrics_path", patch[6][6]), ("y_pred_fuse", "metrics_fuse", patch[6][5])):
        df = pd.DataFrame(probs if agg == "max" else probs.astype(np.float64))
        want = df.groupby(ids).agg(agg).to_numpy().astype(np.float32)          # (sorted ids = order of first appearance here)
        got = pat[key]
        assert got.dtype == np.float32 and got.shape == (3, 3)
        if agg == "max":
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), key
        else:
            assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), key
        sk = m.evaluate.grading_metrics(pat["y_label"], got)
        print(agg, key, "device", pat[mkey], "sklearn", sk)
        assert np.abs(np.asarray(pat[mkey]) - np.asarray(sk, dtype=np.float64)).max() <= 9 * 2.0 ** -52, (key, pat[mkey], sk)
    dev = m.evaluate.aggregate_by_patient(ld, torch.from_numpy(patch[6][6]).cuda(), agg)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), pat["y_pred_path"])


def test_stage1_evaluation_consumes_the_loader(store, nets):
    """evaluate.test_teacher (the stage-1 trainers' test()) over the same loader: its 16-tuple, 36 rows per branch."""
    import multimodal_learning_amd as m
    out = m.evaluate.test_teacher(_opt(), nets[1], _loader(store), "cuda")
    assert len(out) == 16 and all(out[13][k].shape == (36, 3) for k in (5, 6, 7)) and len(out[12]) == 12
    assert out[13][8].tolist() == sum(([float(g)] * 9 for g in GRADES), [])


def test_student_only_form(passes, nets):
    import multimodal_learning_amd as m
    ld, ref, out = passes
    patch, pat = m.evaluate.test_patches(_opt(), None, nets[0], ld, "cuda")
    assert patch[6][5] is None and pat["y_pred_fuse"] is None and pat["metrics_fuse"] is None
    assert np.array_equal(patch[6][6], ref[6][6]) and patch[0] == ref[0]
    assert pat["metrics_path"] == out["max"][1]["metrics_path"]


def test_host_reads_do_not_depend_on_the_number_of_batches(store, nets, monkeypatch):
    import multimodal_learning_amd as m
    student, teacher = nets
    calls = count_host_reads(monkeypatch)
    reads = {}
    for bs in (36, 8):
        opt = _opt()
        opt.batch_size = bs
        ld = _loader(store, opt)
        assert len(ld) == -(-36 // bs)
        calls["n"] = 0
        m.evaluate.test_patches(opt, teacher, student, ld, "cuda")
        reads[bs] = calls["n"]
    print("host reads per call:", reads)
    assert reads[36] == reads[8] and reads[36] > 0


def test_refusals(store, nets):
    import multimodal_learning_amd as m
    tiles, omic, grade = store
    with pytest.raises(ValueError, match="different grades"):
        m.augment.ResidentPatchLoader(_opt(), tiles.cuda(), omic, torch.tensor([2, 1, 0, 1]), patient=PATIENTS)
    with pytest.raises(ValueError, match="stride"):
        m.augment.ResidentPatchLoader(_opt(), tiles.cuda(), omic, grade, grid=4)          # 32 / 3
    big = _opt(); big.input_size_path = 128
    with pytest.raises(ValueError):
        m.augment.ResidentPatchLoader(big, tiles.cuda(), omic, grade)
    ld = _loader(store)
    with pytest.raises(ValueError, match="mean.*max"):
        m.evaluate.test_patches(_opt(), None, nets[0], ld, "cuda", agg="p0.75")
    with pytest.raises(ValueError, match="mean.*max"):
        m.evaluate.aggregate_by_patient(ld, torch.zeros(36, 3, device="cuda"), agg="p0.75")
    with pytest.raises(NotImplementedError):
        m.evaluate.test_patches(_opt(task="surv"), None, nets[0], ld, "cuda")

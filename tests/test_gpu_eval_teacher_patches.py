"""The patient-level test pass of the stage-1 teacher (evaluate.test_teacher_patches) for the grading
and the survival task, the survival columns of augment.ResidentPatchLoader, and the order-statistic aggregations
("median", ("quantile", q)) - on the fixture of tests/test_gpu_eval_patches.py: 4 ROIs of 96 x 96, S = 64, grid 3: 36 rows
in batches of 16, 16, 4; three patients (2 + 1 + 1 ROIs).

References: evaluate.test_teacher on the same loader (bit for bit), pandas' groupby on the copied rows (max exact; mean,
median and quantile within one float32 ulp of pandas' float64 value), sklearn within G * C * 2^-52 for the patient metrics
(36 * 3 * 2^-52 for the patch metrics), utils.CIndex_lifeline / cox_log_rank / accuracy_cox on the copied patient vectors."""
import numpy as np
import pytest
import torch

from tests.gpu_util import assert_same, count_host_reads

pytestmark = pytest.mark.gpu

N_ROI, SH, S, GRID = 4, 96, 64, 3
PATIENTS = ["TCGA-a", "TCGA-a", "TCGA-b", "TCGA-c"]
GRADES = [2, 2, 0, 1]
CENSOR = [1.0, 1.0, 0.0, 1.0]
SURVTIME = [5.0, 5.0, 9.0, 2.0]
IDS = np.repeat(np.asarray(PATIENTS), 9)
AGGS = ("max", "mean", "median", ("quantile", 0.009))


def _opt(**kw):
    from oracle.step import default_opt
    return default_opt(dropout_rate=0.25, input_size_path=S, batch_size=16, **kw)


def _surv_opt():
    return _opt(task="surv", act_type="Sigmoid", label_dim=1)


@pytest.fixture(scope="module")
def store():
    g = torch.Generator().manual_seed(11)
    tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8)
    omic = torch.randn(N_ROI, 320, generator=g)
    return tiles.cuda(), omic, torch.tensor(GRADES)


def _loader(store, opt=None, **kw):
    import multimodal_learning_amd as m
    tiles, omic, grade = store
    kw.setdefault("patient", PATIENTS)
    return m.augment.ResidentPatchLoader(opt or _opt(), tiles, omic, grade, **kw)


def _ulp_close(got, want64):
    """got float32 within one float32 ulp of the float64 reference."""
    want32 = want64.astype(np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(want32)).astype(np.float64)))


def _pandas_agg(rows, agg):
    import pandas as pd
    gb = pd.DataFrame(rows if agg == "max" else rows.astype(np.float64)).groupby(IDS)
    if isinstance(agg, tuple):
        return gb.quantile(agg[1]).to_numpy()
    return gb.agg(agg).to_numpy()


# ------------------------------------------------------------------------------------------------ grading
@pytest.fixture(scope="module")
def grad_passes(store):
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt = _opt()
    teacher = m.define_net(opt, 1)
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    teacher = teacher.cuda()
    ld = _loader(store, opt)
    ref = m.evaluate.test_teacher(opt, teacher, ld, "cuda")
    out = {agg: m.evaluate.test_teacher_patches(opt, teacher, ld, "cuda", agg=agg) for agg in AGGS}
    out[None] = m.evaluate.test_teacher_patches(opt, teacher, ld, "cuda")
    return opt, teacher, ld, ref, out


def test_grading_patch_result_is_test_teacher(grad_passes):
    opt, teacher, ld, ref, out = grad_passes
    patch, pat = out[None]
    assert len(patch) == 16 and pat["agg"] == "max"
    for k in range(16):
        if k != 12:
            assert_same(patch[k], ref[k], "patch[%d]" % k)
    assert len(patch[12]) == 12 and all(isinstance(v, float) for v in patch[12])
    print("teacher patch metrics: device", patch[12], "sklearn", ref[12])
    assert np.abs(np.asarray(patch[12]) - np.asarray(ref[12], dtype=np.float64)).max() <= 36 * 3 * 2.0 ** -52
    assert_same(out["max"][0], patch)


@pytest.mark.parametrize("agg", AGGS, ids=str)
def test_grading_patient_rows_vs_pandas_and_sklearn(grad_passes, agg):
    import multimodal_learning_amd as m
    opt, teacher, ld, ref, out = grad_passes
    patch, pat = out[agg]
    assert set(pat) == {"patients", "y_label", "agg"} | {p + n for p in ("y_pred_", "metrics_") for n in ("fuse", "path", "omic")}
    assert pat["patients"] == ["TCGA-a", "TCGA-b", "TCGA-c"] and pat["agg"] == agg
    assert np.array_equal(pat["y_label"], np.eye(3, dtype=np.float32)[[2, 0, 1]])
    for name, probs in (("fuse", patch[13][5]), ("path", patch[13][6]), ("omic", patch[13][7])):
        got, want = pat["y_pred_" + name], _pandas_agg(probs, agg)
        assert got.dtype == np.float32 and got.shape == (3, 3)
        if agg == "max":
            assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32)), name
        else:
            assert _ulp_close(got, want.astype(np.float64)), (name, agg, got, want)
        sk = m.evaluate.grading_metrics(pat["y_label"], got)
        print(agg, name, "device", pat["metrics_" + name], "sklearn", sk)
        assert np.abs(np.asarray(pat["metrics_" + name]) - np.asarray(sk, dtype=np.float64)).max() <= 9 * 2.0 ** -52, name


def test_aggregate_by_patient_names_and_vector_form(grad_passes):
    import multimodal_learning_amd as m
    from tests import quantile_emulation as E
    opt, teacher, ld, ref, out = grad_passes
    rows = out["max"][0][13][6]
    d = torch.from_numpy(rows).cuda()
    med = m.evaluate.aggregate_by_patient(ld, d, "median")
    assert torch.equal(med, m.evaluate.aggregate_by_patient(ld, d, ("quantile", 0.5))) and tuple(med.shape) == (3, 3)
    want = E.group_quantile(rows, ld.group_offsets_host, ld.group_order.cpu().numpy(), 0.5)
    assert np.array_equal(med.cpu().numpy().view(np.int32), want.view(np.int32))
    for agg in AGGS:
        vec = m.evaluate.aggregate_by_patient(ld, d[:, 1].contiguous(), agg)
        assert tuple(vec.shape) == (3,) and torch.equal(vec, m.evaluate.aggregate_by_patient(ld, d, agg)[:, 1])
    for bad in ("p0.75", "min", ("quantile", 1.5), ("quantile", -0.1), ("quantile", float("nan")), ("quantile", "0.5"),
                ("percentile", 0.5), 0.5, None):
        with pytest.raises(ValueError, match="mean.*max"):
            m.evaluate.aggregate_by_patient(ld, d, bad)
    with pytest.raises(ValueError, match=r"np\.percentile\(x, 0\.90\).*\(\"quantile\", 0\.009\)"):
        m.evaluate.aggregate_by_patient(ld, d, "p0.75")


def test_test_patches_median_vs_pandas(store, grad_passes):
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt, teacher, ld, ref, out = grad_passes
    student = m.define_net(opt, 1, path_only=True)
    student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    patch, pat = m.evaluate.test_patches(opt, teacher, student.cuda(), ld, "cuda", agg="median")
    assert pat["agg"] == "median"
    assert set(pat) == {"patients", "y_label", "y_pred_path", "y_pred_fuse", "metrics_path", "metrics_fuse", "agg"}
    for key, probs in (("y_pred_path", patch[6][6]), ("y_pred_fuse", patch[6][5])):
        assert _ulp_close(pat[key], _pandas_agg(probs, "median").astype(np.float64)), key
    sk = m.evaluate.grading_metrics(pat["y_label"], pat["y_pred_path"])
    assert np.abs(np.asarray(pat["metrics_path"]) - np.asarray(sk, dtype=np.float64)).max() <= 9 * 2.0 ** -52


def test_host_reads_do_not_depend_on_the_number_of_batches(store, grad_passes, monkeypatch):
    import multimodal_learning_amd as m
    teacher = grad_passes[1]
    calls = count_host_reads(monkeypatch)
    reads = {}
    for bs in (36, 8):
        opt = _opt()
        opt.batch_size = bs
        ld = _loader(store, opt)
        calls["n"] = 0
        m.evaluate.test_teacher_patches(opt, teacher, ld, "cuda")
        reads[bs] = calls["n"]
    print("host reads per call:", reads)
    assert reads[36] == reads[8] and reads[36] > 0


# ------------------------------------------------------------------------------------------------ survival
@pytest.fixture(scope="module")
def surv_passes(store):
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt = _surv_opt()
    teacher = m.define_net(opt, 1)
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3))
    teacher = teacher.cuda()
    ld = _loader(store, opt, censor=CENSOR, survtime=torch.tensor(SURVTIME))
    ref = m.evaluate.test_teacher(opt, teacher, ld, "cuda")
    out = {agg: m.evaluate.test_teacher_patches(opt, teacher, ld, "cuda", agg=agg) for agg in ("mean", "median", "max")}
    out[None] = m.evaluate.test_teacher_patches(opt, teacher, ld, "cuda")
    return opt, teacher, ld, ref, out


def test_loader_survival_columns(store):
    ld = _loader(store, censor=CENSOR, survtime=SURVTIME)
    batches = list(ld)
    assert [b[0].shape[0] for b in batches] == [16, 16, 4] and all(len(b) == 6 for b in batches)
    c, t = torch.cat([b[3] for b in batches]), torch.cat([b[4] for b in batches])
    assert c.is_cuda and t.is_cuda and c.dtype == torch.float32 and t.dtype == torch.float32
    assert c.cpu().tolist() == sum(([v] * 9 for v in CENSOR), []) and t.cpu().tolist() == sum(([v] * 9 for v in SURVTIME), [])
    assert ld.patient_censor.cpu().tolist() == [1.0, 0.0, 1.0] and ld.patient_survtime.cpu().tolist() == [5.0, 9.0, 2.0]
    assert ld.patient_censor.dtype == torch.float32 and ld.patient_censor.is_cuda and ld.patient_survtime.is_cuda
    assert ld.patient_censor_host.tolist() == [1.0, 0.0, 1.0] and ld.patient_survtime_host.tolist() == [5.0, 9.0, 2.0]
    # the default is the loader of before: zeros at positions 3 and 4, no survival attributes
    plain = _loader(store)
    for a, b in zip(plain, ld):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[5], b[5])
        assert not a[3].any() and not a[4].any() and a[3].dtype == torch.float32 and a[3].is_cuda
    assert not hasattr(plain, "patient_censor") and not plain.has_survival


def test_loader_survival_refusals(store):
    with pytest.raises(ValueError, match="both or neither"):
        _loader(store, censor=CENSOR)
    with pytest.raises(ValueError, match="both or neither"):
        _loader(store, survtime=SURVTIME)
    with pytest.raises(ValueError, match="different survival"):
        _loader(store, censor=CENSOR, survtime=[5.0, 6.0, 9.0, 2.0])
    with pytest.raises(ValueError, match="different survival"):
        _loader(store, censor=[1.0, 0.0, 0.0, 1.0], survtime=SURVTIME)
    with pytest.raises(ValueError):
        _loader(store, censor=CENSOR[:3], survtime=SURVTIME[:3])


def test_survival_patch_result_is_test_teacher(surv_passes):
    opt, teacher, ld, ref, out = surv_passes
    patch, pat = out[None]
    assert pat["agg"] == "mean" and len(patch) == 16
    assert_same(patch, ref, "patch")
    assert patch[13][0].shape == (36,) and patch[12] is None and patch[4] is not None
    assert_same(out["mean"][0], patch)


@pytest.mark.parametrize("agg", ("mean", "median", "max"))
def test_survival_patient_level(surv_passes, agg):
    import pandas as pd
    from multimodal_learning_amd import utils as U
    opt, teacher, ld, ref, out = surv_passes
    patch, pat = out[agg]
    names = ("fuse", "path", "omic")
    assert set(pat) == {"patients", "agg", "survtime", "censor", "pvalue", "surv_acc"} | {p + n for p in ("hazard_", "cindex_") for n in names}
    assert pat["patients"] == ["TCGA-a", "TCGA-b", "TCGA-c"] and pat["agg"] == agg
    assert pat["survtime"].tolist() == [5.0, 9.0, 2.0] and pat["censor"].tolist() == [1.0, 0.0, 1.0]
    for k, name in enumerate(names):
        rows = patch[13][k]                                             # float64 copies of the float32 hazards
        got = pat["hazard_" + name]
        assert got.dtype == np.float32 and got.shape == (3,)
        table = pd.DataFrame({"h": rows}).groupby(IDS).agg(["mean", "median", "max"])["h"]
        want = table[agg].to_numpy().astype(np.float64)
        if agg == "max":
            assert np.array_equal(got, want.astype(np.float32)), name
        else:
            assert _ulp_close(got, want), (name, agg, got, want)
        assert pat["cindex_" + name] == U.CIndex_lifeline(got, pat["censor"], pat["survtime"]), name
    h64 = pat["hazard_fuse"].astype(np.float64)
    assert_same(pat["pvalue"], U.cox_log_rank(h64, pat["censor"], pat["survtime"]))
    assert pat["surv_acc"] == U.accuracy_cox(h64, pat["censor"])
    print(agg, "C-index", [pat["cindex_" + n] for n in names], "p", pat["pvalue"], "acc", pat["surv_acc"])


def test_survival_refusals(store, surv_passes):
    import multimodal_learning_amd as m
    opt, teacher = surv_passes[0], surv_passes[1]
    with pytest.raises(ValueError, match="censor"):
        m.evaluate.test_teacher_patches(opt, teacher, _loader(store, opt), "cuda")
    tiles, omic, grade = store
    one = m.augment.ResidentPatchLoader(opt, tiles, omic, torch.tensor([1, 1, 1, 1]), patient=["p"] * 4, censor=[1.0] * 4,
                                        survtime=[3.0] * 4)
    with pytest.raises(ValueError, match="1048576"):                  # one patient: ph_cindex_counts takes 2 .. 1048576
        m.evaluate.test_teacher_patches(opt, teacher, one, "cuda")
    with pytest.raises(ValueError, match="mean.*max"):
        m.evaluate.test_teacher_patches(opt, teacher, surv_passes[2], "cuda", agg="p0.75")
    with pytest.raises(NotImplementedError):
        m.evaluate.test_patches(opt, None, teacher, surv_passes[2], "cuda", agg="median")

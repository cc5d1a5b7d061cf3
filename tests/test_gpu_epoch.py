"""The epoch record, the row store, the similarity audit and train() on the GPU (csrc/epochrec.hip,
epoch.py, trainers.py) against tests/epoch_emulation.py: record sums bit for bit equal to Python's accumulation of the same
float32 values, counts exact; the store against numpy's `a[index] = rows` between guard bands; the audit against float64 within
the tolerances measured in tests/test_epoch_emulation_cpu.py (a planted exact case bit for bit, two runs bitwise); the record
inside the step - eager and replayed - against a step without one and against the reference's accumulation statements;
no host synchronisation while stepping (torch's sync debug mode, which this build honours: the test first shows that an
.item() raises under it); train() against a hand loop.

Figures (MI355X; printed by every run):  see DESIGN.md section 30."""
import math
import os

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

from tests import epoch_emulation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_process_as_found():
    """train() seeds the global generators as the reference does (:145-149) and the step tests build whole steps with their
    captured graphs: a test of this file hands the process on as it found it - the host and device generator states, the
    arithmetic mode and the sync debug mode put back, its steps and graphs collected and their cached blocks released."""
    import gc
    import random
    from multimodal_learning_amd import ops
    states = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all())
    mode = (ops._precision, ops._fwd_only_precision, ops._backward_precision)
    yield
    torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    ops._precision, ops._fwd_only_precision, ops._backward_precision = mode
    random.setstate(states[0]); np.random.set_state(states[1]); torch.set_rng_state(states[2])
    torch.cuda.set_rng_state_all(states[3])


def _rec_dict(buf):
    w = buf.cpu().numpy()
    f = w.view(np.float64)
    return dict(sums=f[0:16].tolist(), wvec=f[16:32].tolist(), rowmeans=f[32:34].tolist(), correct=int(w[34]), bad=int(w[35]),
                steps=int(w[36]), rows=int(w[37]), added=w[40:56].tolist())


def _same_floats(a, b):
    return len(a) == len(b) and all((x == y and math.copysign(1, x) == math.copysign(1, y)) or (x != x and y != y)
                                    for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the record kernel alone
def _record_case(B, C, ns, rng):
    """Five calls on one record: special values under both modes, tied maxima, labels -1 and C, 0-2 rows, one call without
    predictions, one without a weight vector."""
    special = [0.0, -0.0, -1.5, float("nan"), 2.5e-3, 1.0e30, 3.0]
    calls = []
    for s in range(5):
        vals = [special[(s + k) % len(special)] if (k + s) % 2 else float(rng.standard_normal()) for k in range(ns)]
        modes = [1 if s % 2 else k % 2 for k in range(ns)]           # (ns = 1: -0.0 and the NaN meet the `> 0.0` mode)
        pred = rng.standard_normal((B, C)).astype(np.float32)
        grade = rng.integers(0, C, size=B).astype(np.int64)
        if C > 1:
            # every second row: its maximum copied into the last column and the label on the FIRST maximum - a last-maximum
            # rule loses exactly these rows
            first = pred[::2, :C - 1].argmax(axis=1)
            pred[::2, C - 1] = pred[::2, :C - 1].max(axis=1)
            grade[::2] = first
        grade[1::7] = -1
        grade[3::11] = C
        c = dict(scalars=vals, modes=modes, pred=pred, grade=grade,
                 rows=[(1.0 + rng.random(B)).astype(np.float32) for _ in range(s % 3)])
        if s != 2:
            c["wvec"] = rng.standard_normal(1 + (s + ns) % 16).astype(np.float32).tolist()
        if s == 4:                                                    # a call without predictions
            c.pop("pred"); c.pop("grade")
        calls.append(c)
    return calls


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1024])
def test_record_kernel_bitwise_against_python_accumulation(B):
    from multimodal_learning_amd import epoch
    rng = np.random.default_rng(B)
    for C in (1, 3, 16):
        for ns in (1, 16):
            buf = torch.zeros(epoch.REC_WORDS, device="cuda", dtype=torch.int64)
            calls = _record_case(B, C, ns, rng)
            for c in calls:
                dev = [torch.tensor([v], dtype=torch.float32, device="cuda") for v in c["scalars"]]
                epoch.record_add(buf, dev, c["modes"],
                                 torch.tensor(c["wvec"], dtype=torch.float32, device="cuda") if "wvec" in c else None,
                                 torch.tensor(c["pred"], device="cuda") if "pred" in c else None,
                                 torch.tensor(c["grade"], device="cuda") if "pred" in c else None,
                                 [torch.tensor(r, device="cuda") for r in c["rows"]])
            got, want = _rec_dict(buf), E.record_emulate(calls)
            for k in ("sums", "wvec", "rowmeans"):
                assert _same_floats(got[k], want[k]), (B, C, ns, k, got[k], want[k])
            for k in ("correct", "bad", "steps", "rows", "added"):
                assert got[k] == want[k], (B, C, ns, k, got[k], want[k])
            # the defects of tests/test_epoch_emulation_cpu.py are visible on these inputs
            assert E.record_emulate(calls, defect="ge_zero")["added"] != want["added"]
            if C > 1:
                assert E.record_emulate(calls, defect="last_max")["correct"] < want["correct"]


def test_record_add_refusals_write_nothing():
    from multimodal_learning_amd import epoch
    buf = torch.zeros(epoch.REC_WORDS, device="cuda", dtype=torch.int64)
    one = torch.ones(1, device="cuda")
    with pytest.raises(ValueError):
        epoch.record_add(buf)                                         # nothing to add
    with pytest.raises(ValueError):
        epoch.record_add(buf, [one], [2])                             # an unknown mode
    with pytest.raises(ValueError):
        epoch.record_add(buf, pred=torch.zeros(4, 17, device="cuda"), grade=torch.zeros(4, device="cuda", dtype=torch.int64))
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ------------------------------------------------------------------------------------------------ ph_store_rows
@pytest.mark.parametrize("D", [3, 32, 33, 128, 256])
@pytest.mark.parametrize("softmax", [False, True])
def test_store_rows_between_guard_bands(D, softmax):
    from multimodal_learning_amd import epoch
    rng = np.random.default_rng(D)
    n, B, guard = 37, 70, 64
    whole = torch.full(((n + 2) * D + 2 * guard,), -7.0, device="cuda")
    store = whole[guard + D:guard + D + n * D].view(n, D)
    store.fill_(0.5)
    rows = (3.0 * rng.standard_normal((B, D))).astype(np.float32)
    index = rng.integers(0, n, size=B).astype(np.int64)
    index[5], index[40], index[69] = 11, 11, 11                       # a triple duplicate: position 69 wins
    index[7], index[8], index[9] = -1, n, 1 << 40                     # out of range
    skipped = torch.zeros(1, device="cuda", dtype=torch.int64)
    epoch.store_rows(store, torch.tensor(index, device="cuda"), torch.tensor(rows, device="cuda"), skipped, softmax=softmax)
    got = store.cpu().numpy()
    base = np.full((n, D), 0.5, dtype=np.float32)
    assert int(skipped.item()) == 3
    w = whole.cpu().numpy()
    assert (w[:guard + D] == -7.0).all() and (w[guard + D + n * D:] == -7.0).all(), "a write outside the store"
    if not softmax:
        want, _ = E.store_emulate(base, index, rows)
        ref = base.copy()
        ok = (index >= 0) & (index < n)
        ref[index[ok]] = rows[ok]                                     # numpy's own rule
        assert np.array_equal(want, ref) and np.array_equal(got, ref)
        assert not np.array_equal(E.store_emulate(base, index, rows, defect="first_writer")[0], ref)
        return
    ref64, _ = E.store_emulate(base, index, rows, softmax=True, dt=np.float64)
    rest, _ = E.store_emulate(base, index, rows, softmax=True, dt=np.float32)
    tol = E.softmax_tolerance(ref64, rest)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print("\nstore_rows softmax D %d: max error %.3e (restatement %.3e, tolerance %.3e)"
          % (D, err, float(np.abs(rest - ref64).max()), tol))
    assert err <= tol
    touched = np.unique(index[(index >= 0) & (index < n)])
    assert np.allclose(got[touched].sum(axis=1), 1.0, atol=1e-5)
    bad64, _ = E.store_emulate(base, index, rows, softmax=True, dt=np.float64, defect="first_writer")
    assert float(np.abs(bad64 - ref64).max()) > 4 * tol


# ------------------------------------------------------------------------------------------------ the audit
WIDTHS = [3, 31, 32, 33, 128, 256]


def _audit_case(n, Df, Dp, classes, seed, zero_rows=False):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, Df)).astype(np.float32)
    P = (0.5 * F[:, :1] + rng.standard_normal((n, Dp))).astype(np.float32)
    if zero_rows:
        F[0] = 0.0
        P[n // 2] = 0.0
    return F, P, rng.integers(0, classes, size=n).astype(np.int64)


def _device_audit(F, P, lab):
    from multimodal_learning_amd import epoch
    w = epoch.sim_audit(torch.tensor(F, device="cuda"), torch.tensor(P, device="cuda"),
                        None if lab is None else torch.tensor(lab, device="cuda")).cpu().numpy()
    return dict(zip(E.SUMS, w[:5].view(np.float64).tolist())), (int(w[5]), int(w[6])), w


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 200])
def test_audit_against_float64(n):
    worst = 0.0
    for k, Df in enumerate(WIDTHS):
        Dp = WIDTHS[(k + 2) % len(WIDTHS)]                            # (the two stores differ in width, as features do)
        classes = 1 + k % 3
        F, P, lab = _audit_case(n, Df, Dp, classes, 100 * n + k, zero_rows=(k == 3 and n > 2))
        ref, counts, tol = E.audit_tolerance(F, P, lab)
        got, c, w1 = _device_audit(F, P, lab)
        _, _, w2 = _device_audit(F, P, lab)
        assert np.array_equal(w1[:7], w2[:7]), "two runs differ"
        assert c == counts, (n, Df, Dp, c, counts)
        for s in E.SUMS:
            if tol[s] > 0.0:                                          # (an empty selection: sum, reference and tolerance are 0)
                worst = max(worst, abs(got[s] - ref[s]) / tol[s])
            assert abs(got[s] - ref[s]) <= tol[s], (n, Df, Dp, s, got[s], ref[s], tol[s])
        # planted: every similarity exact, all five sums bit for bit
        Fp, Pp, labp = E.planted_exact(n, Df, Dp, classes)
        refp, cp = E.audit_reference(Fp, Pp, labp)
        gotp, cgp, _ = _device_audit(Fp, Pp, labp)
        assert cgp == cp and all(gotp[s] == refp[s] for s in E.SUMS), (n, Df, Dp, gotp, refp)
    print("\naudit n %d: largest error / tolerance %.3f" % (n, worst))


def test_audit_functions_single_class_and_logits():
    import multimodal_learning_amd as m
    F, P, _ = _audit_case(65, 33, 3, 1, 5)
    lab = np.zeros(65, dtype=np.int64)
    d = m.evaluate.feature_audit_device(torch.tensor(F, device="cuda"), torch.tensor(P, device="cuda"), torch.tensor(lab))
    ref, counts, tol = E.audit_tolerance(F, P, lab)
    want = E.means(ref, counts)
    assert (d["intra_pairs"], d["inter_pairs"]) == (65 * 65, 0)
    assert math.isnan(d["teacher_inter"]) and math.isnan(d["student_inter"])
    assert abs(d["teacher_intra"] - want["teacher_intra"]) <= tol["teacher_intra"] / counts[0]
    diff = m.evaluate.logit_audit_device(torch.tensor(F, device="cuda"), torch.tensor(P, device="cuda"))
    assert abs(diff - want["similarity_diff"]) <= tol["absdiff"] / (65 * 65) and diff == d["similarity_diff"]
    for bad in (torch.zeros(0, 3, device="cuda"), torch.zeros(4, 513, device="cuda")):
        with pytest.raises(ValueError):
            m.evaluate.logit_audit_device(bad, bad)


def test_audit_multi_tile_walk():
    """n = 4096, D = 128: 64 row tiles, 16 ranges of 4 j tiles each - several tiles in both directions."""
    F, P, lab = _audit_case(4096, 128, 128, 3, 9)
    ref, counts, tol = E.audit_tolerance(F, P, lab, orders=("matmul",))
    got, c, _ = _device_audit(F, P, lab)
    assert c == counts
    for s in E.SUMS:
        print("audit 4096 x 128 %s: error %.3e tolerance %.3e" % (s, abs(got[s] - ref[s]), tol[s]))
        assert abs(got[s] - ref[s]) <= tol[s], (s, got[s], ref[s], tol[s])


# ------------------------------------------------------------------------------------------------ the record in the step
def _tuple(bt):
    B = bt["x_path"].shape[0]
    return ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], torch.zeros(B), torch.zeros(B),
            bt["grade"], bt["index"], bt["sample_idx"])


STEP_CASES = {
    "miccai2022": ("miccai2022", dict(nce_p=120, nce_k=200, nce_p2=20, nce_k2=128)),
    "miccai2022-fixed-weights": ("miccai2022", dict(nce_p=120, nce_k=200, nce_p2=20, nce_k2=128, assign_weights="False")),
    "miccai2022-kd": ("miccai2022", dict(nce_p=120, nce_k=200, nce_p2=20, nce_k2=128, distill="kd")),
    "mia2022": ("mia2022", dict(nce_k=64, grads_m=0.9, grads_thresh="False", thresh=0.1, niter_decay=10)),
    "mia2023": ("mia2023", dict(nce_k=64, nce_p=4, pos_extra="neighbors", neg_mode="all_others", start_reweight=0,
                                discrep_scale=1, max_discrep=2.0, use_grads_thresh="True", grads_thresh=0.1,
                                loss_weighting="GK_refine", batch_size=8)),
}


def _mk(variant, kw, n_data):
    """A seeded step of `variant` -> (step, labels or None)."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    opt = default_opt(**kw)
    labels, extra = None, {}
    if variant == "mia2023":
        labels = torch.arange(n_data) % 3
        extra = dict(train_class_idx=[np.nonzero((labels == c).numpy())[0] for c in range(3)])
    torch.manual_seed(7); np.random.seed(7)
    step = m.DistillStep(opt, n_data, device="cuda", variant=variant, **extra)
    step.model.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    step.ema_model.load_state_dict(W.make_state_dict(W.student_shapes(), 2))
    step.fix_model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    for crd in (step.criterion_kd, step.criterion_kd_path):          # (heads and banks: the seeded default initialisation)
        crd.contrast.verbose = False
    return step, labels


def _batches(variant, kw, n_data, labels, count, B=8, seed0=700):
    from oracle.step import synthetic_batch
    P, K = (kw["nce_p"], kw["nce_k"]) if variant == "miccai2022" else (1, kw["nce_k"])
    out = []
    for it in range(count):
        bt = synthetic_batch(B, 64, n_data=n_data, P=P, K=K, seed=seed0 + it)
        if labels is not None:
            bt["grade"] = labels[bt["index"]].long()
        out.append(bt)
    return out


KEYS = ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2", "logit_path", "pred_path", "path_feat",
        "fuse_feat", "fuse_logit", "scale", "w1", "w2", "rec_loss_div", "rec_loss_kd")


def _run_steps(case, with_record, n_steps=6, n_data=256):
    import multimodal_learning_amd as m
    variant, kw = STEP_CASES[case]
    m.set_precision("bf16")
    step, labels = _mk(variant, kw, n_data)
    rec = None
    if with_record:
        rec = step.record = m.EpochRecord(step)
        if variant == "mia2023":
            step.stores = m.FeatureStores(step, n_data)
    step.enable_graph()
    np.random.seed(3)                                                 # (the MICCAI bank's host rank draws)
    bts = _batches(variant, kw, n_data, labels, n_steps)
    outs = []
    if rec is not None:
        rec.reset()
    for it, bt in enumerate(bts):
        o = step.step(_tuple(bt), epoch=2)
        outs.append({k: o[k].detach().clone() for k in KEYS if k in o and o[k] is not None})
    torch.cuda.synchronize()
    assert step._slots and step._slots[0]["graph"] is not None, "the step was not replayed from a graph"
    return step, rec, bts, outs


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_record_in_step_equals_reference_accumulation(case):
    step, rec, bts, outs = _run_steps(case, True)
    _, _, _, plain = _run_steps(case, False)
    variant, kw = STEP_CASES[case]
    opt = step.opt
    # 1. the record changes nothing the step returns
    for a, b in zip(outs, plain):
        assert "rec_loss_div" in a and "rec_loss_div" not in b
        for k in b:
            assert torch.equal(a[k], b[k]), (case, k)
    # 2. read() == the reference's statements over the returned tensors (:305, :317-324, :339-340)
    got = rec.read()
    loss_epoch = loss_cls_epoch = loss_div_epoch = loss_kd_epoch = 0.0
    grad_path_epoch, q1, q2 = 0, 0.0, 0.0
    gk = opt.assign_weights == "True"
    loss_weights = None
    for o, bt in zip(outs, bts):
        loss_epoch += o["loss"].item()
        loss_cls_epoch += o["loss_cls"].item()
        loss_div, loss_kd = o["rec_loss_div"], o["rec_loss_kd"]
        if loss_div > 0.0:
            loss_div_epoch += loss_div.item()
        if loss_kd > 0.0:
            loss_kd_epoch += loss_kd.item()
        if gk:
            s = o["scale"].cpu().numpy().reshape(-1)
            loss_weights = np.zeros(s.shape[0]) if loss_weights is None else loss_weights
            loss_weights += s
        pred = np.argmax(o["pred_path"].cpu().numpy(), axis=1)        # (numpy: the first maximum)
        grad_path_epoch += int((pred == bt["grade"].numpy()).sum())
        if "w1" in o:
            q1 += math.fsum(o["w1"].double().reshape(-1).tolist()) / o["w1"].numel()
            q2 += math.fsum(o["w2"].double().reshape(-1).tolist()) / o["w2"].numel()
        # what the record took is what the step reports, by the plan's convention
        div_rep = (o["loss_div1"] + o["loss_div2"]).item() / (opt.alpha if step.plan.report == "scaled" else 1.0)
        kd_rep = (o["loss_kd1"] + o["loss_kd2"]).item() * (1.0 if step.plan.report in ("scaled", "baseline") else opt.beta)
        assert loss_div.item() == pytest.approx(div_rep, rel=1e-5, abs=1e-7)
        assert loss_kd.item() == pytest.approx(kd_rep, rel=1e-5, abs=1e-7)
    print("\n%s: record %s" % (case, {k: v for k, v in got.items() if k != "loss_weights"}))
    assert got["steps"] == len(outs) and got["rows"] == 8 * len(outs) and got["bad_labels"] == 0
    assert _same_floats([got["loss_epoch"], got["loss_cls_epoch"], got["loss_div_epoch"], got["loss_kd_epoch"]],
                        [loss_epoch, loss_cls_epoch, loss_div_epoch, loss_kd_epoch]), (got, loss_epoch, loss_div_epoch, loss_kd_epoch)
    assert got["grad_path_epoch"] == grad_path_epoch
    assert math.isfinite(loss_epoch) and loss_div_epoch > 0.0
    if gk:
        assert got["loss_weights"] is not None and _same_floats(got["loss_weights"].tolist(), loss_weights.tolist())
    else:
        assert got["loss_weights"] is None                            # --assign_weights False: :305 never runs
    if opt.distill == "kd":
        assert got["loss_kd_epoch"] == 0.0 and got["loss_kd_added"] == 0      # loss_kd = 0 never passes `> 0.0` (:323)
    else:
        assert got["loss_kd_added"] == len(outs) and loss_kd_epoch > 0.0
    if variant == "mia2023":
        assert got["teacher1_query_weight"] == q1 / len(outs) and got["teacher2_query_weight"] == q2 / len(outs)
        # 3. the four stores equal the scattered rows (:338-342)
        st = step.stores
        n_data = st.n_data
        want = {k: None for k in st.NAMES}
        rest = {}
        for o, bt in zip(outs, bts):
            idx = bt["index"].numpy()
            for name, key, sm in (("fuse_feat", "fuse_feat", False), ("path_feat", "path_feat", False),
                                  ("fuse_pred", "fuse_logit", True), ("path_pred", "logit_path", True)):
                rows = o[key].float().cpu().numpy()
                if want[name] is None:
                    want[name] = np.zeros((n_data, rows.shape[1]), dtype=np.float64 if sm else np.float32)
                    rest[name] = np.zeros((n_data, rows.shape[1]), dtype=np.float32)
                want[name][idx] = E.softmax_rows(rows, np.float64) if sm else rows
                if sm:
                    rest[name][idx] = E.softmax_rows(rows, np.float32)
        assert int(st.skipped.item()) == 0
        for name in ("fuse_feat", "path_feat"):
            assert np.array_equal(getattr(st, name).cpu().numpy(), want[name]), name
        for name in ("fuse_pred", "path_pred"):
            err = float(np.abs(getattr(st, name).cpu().numpy().astype(np.float64) - want[name]).max())
            assert err <= E.softmax_tolerance(want[name], rest[name]), (name, err)


def test_record_under_data_parallelism_raises():
    import multimodal_learning_amd as m
    from types import SimpleNamespace
    fake = SimpleNamespace(sync=object(), variant="miccai2022", plan=None, opt=None, device="cuda")
    with pytest.raises(NotImplementedError):
        m.EpochRecord(fake)
    with pytest.raises(NotImplementedError):
        m.FeatureStores(SimpleNamespace(sync=object(), variant="mia2023", device="cuda"), 16)


class _HostReadSpy(torch.utils._python_dispatch.TorchDispatchMode):
    """Every aten op that moves device data to the host: .item() (_local_scalar_dense), .cpu() / .to("cpu") (_to_copy), and a
    copy_ into a host tensor - counted the way tests/prof_copies_gpu.py counts copies."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.__name__.split(".")[0]
        src_gpu = any(torch.is_tensor(a) and a.is_cuda for a in args)
        if src_gpu and (name == "_local_scalar_dense" or (name == "_to_copy" and torch.is_tensor(out) and not out.is_cuda)
                        or (name == "copy_" and not args[0].is_cuda)):
            self.seen.append(name)
        return out


@pytest.mark.parametrize("case", ["miccai2022", "mia2023"])
def test_no_host_read_between_reset_and_read(case):
    """Replayed steps on device-resident batches with the record (and stores) attached issue no device-to-host copy and no
    synchronising call: torch's sync debug mode in "error" mode where this build honours it (an .item() raises under it; the
    run prints whether it did), and in every case a dispatch spy that lists the ops which move device data to the host."""
    import multimodal_learning_amd as m
    variant, kw = STEP_CASES[case]
    m.set_precision("bf16")
    step, labels = _mk(variant, kw, 256)
    rec = step.record = m.EpochRecord(step)
    if variant == "mia2023":
        step.stores = m.FeatureStores(step, 256)
    step.enable_graph()
    np.random.seed(3)
    bt = _batches(variant, kw, 256, labels, 1)[0]
    dev_bt = {k: v.cuda() for k, v in bt.items()}
    for _ in range(3):                                                # two eager steps, the capture
        step.step(_tuple(dev_bt), epoch=2)
    torch.cuda.synchronize()
    probe = torch.ones(1, device="cuda")
    spy = _HostReadSpy()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        rec.reset()
        with spy:
            for _ in range(4):
                step.step(_tuple(dev_bt), epoch=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("\n%s: sync debug mode honoured: %s; device-to-host ops seen by the dispatch spy: %s" % (case, honoured, spy.seen))
    assert spy.seen == [], spy.seen
    got = rec.read()
    assert got["steps"] == 4 and math.isfinite(got["loss_epoch"])
    with spy:                                                         # the spy does see a read
        probe.item()
    assert spy.seen


# ------------------------------------------------------------------------------------------------ train()
class _Loader(list):
    dataset = range(16)


def _train_setup(tmp_path, variant, **over):
    from oracle import weights as W
    from oracle.step import default_opt, synthetic_batch
    _, kw = STEP_CASES[variant]
    kw = dict(kw, batch_size=4, niter=0, niter_decay=3, epoch_count=1, measure=1, patience=-1.0, verbose=0,
              checkpoints_dir=str(tmp_path), exp_name="exp", fixed_model="pathomic_teacher", model_name="path_student")
    if variant == "mia2023":
        kw["nce_p"] = 2
    kw.update(over)
    opt = default_opt(**kw)
    n_data = 16
    labels = torch.arange(n_data) % 3
    os.makedirs(os.path.join(str(tmp_path), "exp", "pathomic_teacher"), exist_ok=True)
    torch.save({"model_state_dict": W.make_state_dict(W.teacher_shapes(320), 3)},
               os.path.join(str(tmp_path), "exp", "pathomic_teacher", "pathomic_teacher_1_best.pt"))
    P, K = (kw["nce_p"], kw["nce_k"]) if variant == "miccai2022" else (1, kw["nce_k"])
    train_loader, test_loader = _Loader(), _Loader()
    for it in range(4):
        bt = synthetic_batch(4, 64, n_data=n_data, P=P, K=K, seed=900 + it)
        bt["index"] = torch.arange(4 * it, 4 * it + 4)
        bt["sample_idx"][:, 0] = bt["index"]
        bt["grade"] = labels[bt["index"]].long()
        train_loader.append(_tuple(bt))
        z = torch.zeros(4)
        test_loader.append((bt["x_path"], z, bt["x_omic"], z, z, bt["grade"]))
    extra = dict(train_class_idx=[np.nonzero((labels == c).numpy())[0] for c in range(3)]) if variant == "mia2023" else {}
    return opt, n_data, train_loader, test_loader, extra


RECORD_KEYS = ("loss_epoch", "loss_cls_epoch", "loss_div_epoch", "loss_kd_epoch", "grad_path_epoch", "steps", "rows",
               "bad_labels", "loss_div_added", "loss_kd_added")


def _hand_loop(opt, n_data, train_loader, test_loader, variant, extra, epochs):
    """train()'s loop by hand over an identically seeded step: the same seeds, the same construction order."""
    import random
    import multimodal_learning_amd as m
    from multimodal_learning_amd import trainers
    torch.cuda.manual_seed_all(2019); torch.manual_seed(2019); random.seed(2019); np.random.seed(2019)
    sd = torch.load(trainers.teacher_checkpoint_path(opt, 1), map_location="cuda", weights_only=False)["model_state_dict"]
    step = m.DistillStep(opt, n_data, device="cuda", k=1, variant=variant, **extra)
    step.fix_model.load_state_dict(sd)
    rec = step.record = m.EpochRecord(step)
    if variant == "mia2023":
        step.stores = m.FeatureStores(step, n_data)
    step.enable_graph()
    out = []
    for epoch in epochs:
        rec.reset()
        for batch in train_loader:
            step.step(batch, epoch)
        step.scheduler.step()
        out.append(rec.read())
        if m.epoch_end_plan(opt, epoch, variant).measure:
            m.evaluate.test(opt, step.fix_model, step.model, test_loader, "cuda")
    return out


@pytest.mark.parametrize("variant", ["miccai2022", "mia2022", "mia2023"])
def test_train_returns_the_variants_tuple_and_the_hand_loops_epochs(tmp_path, variant):
    import multimodal_learning_amd as m
    from multimodal_learning_amd import trainers
    m.set_precision("bf16")
    opt, n_data, train_loader, test_loader, extra = _train_setup(tmp_path, variant)
    kw = dict(audit=True) if variant == "mia2023" else {}
    res = m.train(opt, train_loader, n_data, test_loader, test_loader, "cuda", 1, variant=variant, **extra, **kw)
    assert len(res) == trainers.ARITY[variant] == (4 if variant == "miccai2022" else 6)
    fix_model, model, optimizer, logger = res[:4]
    assert set(logger) == {"train", "test", "epochs"} and all(v == [] for v in logger["train"].values())
    assert set(logger["train"]) == set(logger["test"]) == {"loss", "pvalue", "cindex", "surv_acc", "grad_acc"}
    eps = logger["epochs"]
    assert [e["epoch"] for e in eps] == [1, 2, 3] and all(e["steps"] == 4 and e["rows"] == 16 for e in eps)
    hand = _hand_loop(opt, n_data, train_loader, test_loader, variant, extra, [1, 2, 3])
    for e, h in zip(eps, hand):
        for k in RECORD_KEYS:
            assert _same_floats([float(e[k])], [float(h[k])]), (variant, e["epoch"], k, e[k], h[k])
        assert _same_floats(np.asarray(e["loss_weights"]).tolist(), np.asarray(h["loss_weights"]).tolist())
        if variant == "mia2023":
            assert e["teacher1_query_weight"] == h["teacher1_query_weight"]
    # every epoch is measured (opt.measure) and lies inside every window (niter_decay = 3): the test pass ran, the best
    # checkpoint appeared at the first epoch whose mean metric beat 0, and only where the plan allows it
    for e in eps:
        plan = m.epoch_end_plan(opt, e["epoch"], variant)
        assert plan == (True, True, e["epoch"] > 0, True) and len(e["all_grad_metrics"]) == 4 and e["used_patches"]
        assert ("saved" in e) <= plan.may_save
        if variant == "mia2023":
            fa = e["feature_audit"]
            assert fa["intra_pairs"] + fa["inter_pairs"] == 256 and 0.0 <= e["logit_audit"] <= 2.0
            assert abs(fa["teacher_intra"]) <= 1.0 + 1e-6
    path = trainers.best_checkpoint_path(opt, 1)
    assert any("saved" in e for e in eps) and os.path.exists(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"split", "opt", "epoch", "model_state_dict", "optimizer_state_dict", "metrics"}
    assert ck["split"] == 1 and ck["epoch"] == 3 and set(ck["model_state_dict"]) == set(model.state_dict())
    if variant != "miccai2022":
        best_metrics, avg_metrics = res[4], res[5]
        assert len(best_metrics) == 4 and np.asarray(avg_metrics).shape == (4,)
        total = np.sum([e["all_grad_metrics"] for e in eps if e["epoch"] > 0], axis=0)
        assert np.array_equal(np.asarray(avg_metrics), total / 3.0)


def test_train_stops_early_and_saves_only_when_measured(tmp_path):
    import multimodal_learning_amd as m
    from multimodal_learning_amd import trainers
    m.set_precision("bf16")
    # a patience above the first epoch's loss SUM stops after that epoch, before the checkpoint test (:383-385)
    opt, n_data, train_loader, test_loader, extra = _train_setup(tmp_path, "miccai2022", patience=1e9)
    res = m.train(opt, train_loader, n_data, test_loader, test_loader, "cuda", 1)
    eps = res[3]["epochs"]
    assert len(eps) == 1 and eps[0]["early_stop"] and eps[0]["loss_epoch"] < 1e9
    assert not os.path.exists(trainers.best_checkpoint_path(opt, 1))
    # the MIA trainers return a name only a saved checkpoint binds: the reference's own exception
    opt, n_data, train_loader, test_loader, extra = _train_setup(tmp_path, "mia2022", patience=1e9)
    with pytest.raises(UnboundLocalError):
        m.train(opt, train_loader, n_data, test_loader, test_loader, "cuda", 1, variant="mia2022")
    # without opt.measure only epoch niter + niter_decay - 1 = 2 is measured: that is where the checkpoint appears
    opt, n_data, train_loader, test_loader, extra = _train_setup(tmp_path, "miccai2022", measure=0)
    res = m.train(opt, train_loader, n_data, test_loader, test_loader, "cuda", 1)
    eps = res[3]["epochs"]
    assert [("all_grad_metrics" in e, "saved" in e) for e in eps] == [(False, False), (True, True), (False, False)]
    assert os.path.exists(trainers.best_checkpoint_path(opt, 1))


def test_train_with_a_resident_loader(tmp_path):
    """16 rows resident on the device, B = 4: every epoch is n_data // batch_size = 4 replays of step.step(None, epoch)."""
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    opt, n_data, _, test_loader, _ = _train_setup(tmp_path, "miccai2022", nce_p=4, nce_p2=2, nce_k=8, nce_k2=4,
                                                  select_pos_mode="hard", n_data=16)
    opt.input_size_path, opt.pos_mode, opt.label_dim = 64, "multi_pos", 3
    g = torch.Generator().manual_seed(5)
    tiles = torch.randint(0, 256, (16, 128, 128, 3), dtype=torch.uint8, generator=g).cuda()
    labels = torch.arange(n_data) % 3
    ld = m.augment.ResidentTileLoader(opt, tiles, torch.randn(n_data, 320, generator=g), labels, seed=2)
    res = m.train(opt, ld, n_data, test_loader, test_loader, "cuda", 1)
    eps = res[3]["epochs"]
    assert [e["steps"] for e in eps] == [4, 4, 4] and all(e["rows"] == 16 and e["bad_labels"] == 0 for e in eps)
    assert all(math.isfinite(e["loss_epoch"]) and 0 <= e["grad_path_epoch"] <= 16 for e in eps)
    assert int(ld.batch_no.item()) == 12
    assert all(e["grad_acc_epoch"] == e["grad_path_epoch"] / 16 for e in eps)

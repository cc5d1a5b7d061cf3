"""The stage-1 record, its survival store and train_teacher() on the GPU (csrc/epochrec.hip, epoch.py,
trainers.py) against tests/epoch_stage1_emulation.py: sums bit for bit equal to Python's accumulation of the same float32
values, counts exact, the store between guard bands, two runs bitwise; the record inside TeacherStage1Step - eager and replayed
from both graph kinds - against a step without one and against the reference's accumulation statements; the epoch C-indices
against the all-pairs numpy value; no host synchronisation while stepping; train_teacher() against a hand loop.  Everything is
exact (bitwise or integer): no tolerance."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from tests import epoch_stage1_emulation as S
from tests.test_gpu_epoch import _HostReadSpy, _same_floats

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_process_as_found():
    """As tests/test_gpu_epoch.py: generator states, the arithmetic mode and the sync debug mode put back, steps and graphs
    collected and their cached blocks released."""
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


# ------------------------------------------------------------------------------------------------ the kernel alone
GUARD = 64


def _rec_dict(buf):
    w = buf.cpu().numpy()
    f = w.view(np.float64)
    assert not w[40:48].any(), "the spare words were written"
    return dict(sums=f[0:16].tolist(), added=w[16:32].tolist(), correct=w[32:35].tolist(), bad=int(w[35]), steps=int(w[36]),
                rows=int(w[37]), cursor=int(w[38]), overflow=int(w[39]))


def _run_kernel_case(calls, cap):
    """-> (record dict, raw words, whole store buffer with its guard bands or None)."""
    from multimodal_learning_amd import epoch
    buf = torch.zeros(epoch.S1_WORDS, device="cuda", dtype=torch.int64)
    whole = store = None
    if cap is not None:
        whole = torch.full((2 * GUARD + 5 * cap,), -7.0, device="cuda")
        store = whole[GUARD:GUARD + 5 * cap].view(5, cap)
    for c in calls:
        dev = [torch.tensor([v], dtype=torch.float32, device="cuda") for v in c["scalars"]]
        heads = [torch.tensor(h, device="cuda") for h in c.get("heads", ())]
        epoch.stage1_record_add(buf, dev, c["modes"], heads, torch.tensor(c["grade"], device="cuda") if heads else None,
                                [torch.tensor(x, device="cuda") for x in c["cols"]] if cap is not None else None, store)
    return _rec_dict(buf), buf.cpu().numpy(), None if whole is None else whole.cpu().numpy()


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_kernel_bitwise_against_the_emulation(B):
    for C in (1, 3, 16):
        for nh, ns in ((1, 0), (2, 1), (3, 16)):
            for cap in (None, B, 3 * B + 1):                          # no store | full after one call | fourth call partly dropped
                calls = S.kernel_case(B, C, nh, ns, np.random.default_rng(1000 * B + 10 * C + nh), cap)
                got, w1, whole1 = _run_kernel_case(calls, cap)
                _, w2, whole2 = _run_kernel_case(calls, cap)
                want = S.stage1_emulate(calls, cap or 0, None if cap is None else np.full((5, cap + 1), -7.0, np.float32))
                tag = (B, C, nh, ns, cap)
                assert _same_floats(got["sums"], want["sums"]), (tag, got["sums"], want["sums"])
                for k in ("added", "correct", "bad", "steps", "rows", "cursor", "overflow"):
                    assert got[k] == want[k], (tag, k, got[k], want[k])
                assert np.array_equal(w1, w2), "two runs differ"
                if cap is not None:
                    assert (whole1[:GUARD] == -7.0).all() and (whole1[GUARD + 5 * cap:] == -7.0).all(), "a write outside the store"
                    assert np.array_equal(whole1[GUARD:GUARD + 5 * cap].reshape(5, cap), want["store"][:, :cap]), tag
                    assert np.array_equal(whole1, whole2)
                    assert want["overflow"] == 5 * B - min(5 * B, cap) and want["cursor"] == min(5 * B, cap)
                    # the defects of tests/test_epoch_stage1_emulation_cpu.py are visible on these inputs
                    for d in ("cursor_advanced_first", "columns_swapped"):
                        bad = S.stage1_emulate(calls, cap, np.full((5, cap + 1), -7.0, np.float32), defect=d)
                        assert not np.array_equal(bad["store"], want["store"]), (tag, d)
                if ns and cap is None:
                    assert S.stage1_emulate(calls, defect="ge_zero")["added"] != want["added"]
                if C > 1:
                    assert S.stage1_emulate(calls, cap or 0, None if cap is None else np.full((5, cap + 1), -7.0, np.float32),
                                            defect="last_max")["correct"][0] < want["correct"][0]


def test_store_alone_and_a_corrupt_cursor_write_nothing_outside():
    """Survival rows without heads or scalars at B = 1; and a record that was never zeroed (a cursor of -5, of cap + 9 and of
    2^40): every row is dropped and counted, nothing is written."""
    from multimodal_learning_amd import epoch
    rng = np.random.default_rng(4)
    calls = S.kernel_case(1, 1, 0, 0, rng, cap=3)
    got, _, whole = _run_kernel_case(calls, 3)
    want = S.stage1_emulate(calls, 3, np.full((5, 4), -7.0, np.float32))
    assert (got["cursor"], got["overflow"], got["rows"], got["steps"]) == (3, 2, 5, 5) == (want["cursor"], want["overflow"], 5, 5)
    assert np.array_equal(whole[GUARD:GUARD + 15].reshape(5, 3), want["store"][:, :3])
    assert (whole[:GUARD] == -7.0).all() and (whole[GUARD + 15:] == -7.0).all()
    for cursor in (-5, 16 + 9, 1 << 40):
        buf = torch.zeros(epoch.S1_WORDS, device="cuda", dtype=torch.int64)
        buf[38] = cursor
        whole = torch.full((2 * GUARD + 5 * 16,), -7.0, device="cuda")
        cols = [torch.ones(8, device="cuda") for _ in range(5)]
        epoch.stage1_record_add(buf, cols=cols, store=whole[GUARD:GUARD + 80].view(5, 16))
        w = buf.cpu().numpy()
        assert int(w[39]) == 8 and int(w[38]) == cursor and bool((whole == -7.0).all().item()), cursor


def test_upper_edges_of_every_range():
    """B = 65536, C = 16, three heads, 16 scalars, cap = 1048576 with the cursor 5 rows short of room for the call: head 0 is
    right on every row (the largest count one 20-bit field of the shared tree word must carry), the last columns of the store are
    written, the 5 rows beyond are dropped, the guard bands stay."""
    from multimodal_learning_amd import epoch
    B, C, cap = 65536, 16, 1 << 20
    rng = np.random.default_rng(65536)
    heads = [rng.standard_normal((B, C)).astype(np.float32) for _ in range(3)]
    grade = heads[0].argmax(axis=1).astype(np.int64)
    cols = [(k + rng.random(B)).astype(np.float32) for k in range(5)]
    vals = rng.standard_normal(16).astype(np.float32)
    buf = torch.zeros(epoch.S1_WORDS, device="cuda", dtype=torch.int64)
    buf[38] = cap - B + 5
    whole = torch.full((2 * GUARD + 5 * cap,), -7.0, device="cuda")
    epoch.stage1_record_add(buf, [torch.tensor([v], device="cuda") for v in vals], [0] * 16,
                            [torch.tensor(h, device="cuda") for h in heads], torch.tensor(grade, device="cuda"),
                            [torch.tensor(x, device="cuda") for x in cols], whole[GUARD:GUARD + 5 * cap].view(5, cap))
    got = _rec_dict(buf)
    assert got["correct"] == [B] + [int((h.argmax(axis=1) == grade).sum()) for h in heads[1:]] and got["bad"] == 0
    assert (got["cursor"], got["overflow"], got["rows"], got["steps"]) == (cap, 5, B, 1)
    assert _same_floats(got["sums"], [float(v) for v in vals]) and got["added"] == [1] * 16
    w = whole.cpu().numpy()
    st = w[GUARD:GUARD + 5 * cap].reshape(5, cap)
    lo = cap - B + 5
    assert (w[:GUARD] == -7.0).all() and (w[GUARD + 5 * cap:] == -7.0).all() and (st[:, :lo] == -7.0).all()
    for k in range(5):
        assert np.array_equal(st[k, lo:], cols[k][:B - 5]), k


def test_refusals_write_nothing():
    from multimodal_learning_amd import epoch
    buf = torch.zeros(epoch.S1_WORDS, device="cuda", dtype=torch.int64)
    one = torch.ones(1, device="cuda")
    g = torch.zeros(4, device="cuda", dtype=torch.int64)
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf)                                  # nothing to add
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, [one], [2])                      # an unknown mode
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, heads=[torch.zeros(4, 17, device="cuda")], grade=g)
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, heads=[torch.zeros(4, 3, device="cuda")] * 4, grade=g)
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, cols=[torch.zeros(4, device="cuda")] * 5)
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ------------------------------------------------------------------------------------------------ the record in the step
B_STEP, N_DATA, K_CRD = 8, 256, 48
STEP_CASES = {
    "grad": dict(),
    "grad-crd": dict(crd=True),
    "grad-tsvd": dict(tsvd=True),
    "surv": dict(surv=True),
    "surv-crd": dict(surv=True, crd=True),
}


def _stage1_opt(surv=False, crd=False, tsvd=False, batch_size=B_STEP, n_data=N_DATA, **more):
    import multimodal_learning_amd as m
    kw = dict(task="surv", act_type="Sigmoid", label_dim=1) if surv else {}
    opt = m.stage2_opt(dropout_rate=0.0, batch_size=batch_size, cut_fuse_grad=False, num_teachers=2, nce_k=K_CRD, n_data=n_data,
                       **kw)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss = 1, 1.0, int(crd), 0, "False"
    opt.tSVD_loss = "True" if tsvd else "False"
    if tsvd:
        opt.tSVD_mode, opt.n_views, opt.aux_iter = "pathomic", 4, 2
        opt.mu, opt.pho, opt.max_mu, opt.Lambda_global = 0.01, 1.5, 1.0, 0.05
    for k, v in more.items():
        setattr(opt, k, v)
    return opt


def _surv_cols(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, generator=g) > 0.3).float(), torch.randint(1, 6, (B,), generator=g).float()      # censor, survtime (ties)


def _stage1_batches(count, surv, B=B_STEP, n_data=N_DATA, seed0=800, device=None):
    from oracle.step import synthetic_batch
    out = []
    for it in range(count):
        bt = synthetic_batch(B, 64, n_data=n_data, P=1, K=K_CRD, seed=seed0 + it)
        censor, survtime = _surv_cols(B, seed0 + it) if surv else (torch.zeros(B), torch.zeros(B))
        t = ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], censor, survtime, bt["grade"], bt["index"],
             bt["sample_idx"])
        if device is not None:
            t = (tuple(v.to(device) for v in t[0]),) + tuple(v.to(device) for v in t[1:])
        out.append(t)
    return out


def _mk_step(case):
    import multimodal_learning_amd as m
    from oracle import weights as W
    opt = _stage1_opt(**STEP_CASES[case])
    torch.manual_seed(7); np.random.seed(7)
    model, ema = m.define_net(opt, 1), m.define_net(opt, 1)
    sd = W.make_state_dict(W.teacher_shapes(320), 3)
    if not STEP_CASES[case].get("surv"):
        model.load_state_dict(sd); ema.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 4))
    else:
        ema.load_state_dict(model.state_dict())
    return m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()))


OUT_KEYS = ("loss", "loss_nll", "loss_pred_KD", "loss_CRD", "loss_tsvd", "loss_pred_KD_masking", "pred", "pred_path", "pred_omic",
            "loss_nll_fuse", "loss_nll_path", "loss_nll_omic", "loss_cox_fuse", "loss_cox_path", "loss_cox_omic")


def _tensors_of(obj, out):
    if torch.is_tensor(obj):
        out.append(obj.detach().clone())
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            _tensors_of(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors_of(v, out)
    return out


def _run_steps(case, with_record, graph, n_steps=6):
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    step = _mk_step(case)
    rec = None
    if with_record:
        rec = step.record = m.Stage1Record(step, n_steps * B_STEP)
        rec.reset()
    if graph:
        step.enable_graph()
    step.start_epoch()
    bts = _stage1_batches(n_steps, step.surv)
    outs, tnns = [], []
    for bt in bts:
        aux = step.tsvd_on and step._batch_idx % step.opt.aux_iter == 0
        o = step.step(bt, epoch=2)
        outs.append({k: o[k].detach().clone() for k in OUT_KEYS if k in o})
        tnns.append((step.path_TNN.detach().clone(), step.omic_TNN.detach().clone()) if aux else None)
    torch.cuda.synchronize()
    if graph:
        kinds = sorted(len(q["graphs"]) for q in step._g_sets)
        assert kinds and kinds[-1] == (2 if step.tsvd_on else 1), "the step was not replayed from its graph(s): %s" % kinds
    state = [p.detach().clone() for p in step.model.parameters()] + [p.detach().clone() for p in step.ema_model.parameters()]
    state += _tensors_of(step.optimizer.state_dict(), [])
    return step, rec, bts, outs, tnns, state


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_record_in_step_equals_reference_accumulation(case, graph):
    step, rec, bts, outs, _, state = _run_steps(case, True, graph)
    _, _, _, plain, tnns, plain_state = _run_steps(case, False, graph)
    task = "surv" if step.surv else "grad"
    # 1. the record changes nothing: outputs, parameters, EMA parameters, optimiser state
    for a, b in zip(outs, plain):
        assert set(a) == set(b)
        for k in b:
            assert torch.equal(a[k], b[k]), (case, k)
    assert len(state) == len(plain_state) and all(torch.equal(a, b) for a, b in zip(state, plain_state))
    # 2. read() == the reference's statements ("MIA 2022/train_test_tSVD.py":455-491) over the record-free step's outputs
    got = rec.read()
    br = "cox" if step.surv else "nll"
    host = []
    for o, bt in zip(plain, bts):
        f = lambda k: o[k].cpu().numpy().reshape(())[()]      # noqa: E731   (a numpy float32 scalar)
        host.append(dict(loss=f("loss"), loss_fuse=f("loss_%s_fuse" % br), loss_path=f("loss_%s_path" % br),
                         loss_omic=f("loss_%s_omic" % br), loss_tsvd=f("loss_tsvd"), loss_CRD=f("loss_CRD"),
                         loss_pred_KD=f("loss_pred_KD"), pred_KD_masking_loss=f("loss_pred_KD_masking"),
                         pred=o["pred"].cpu().numpy(), pred_path=o["pred_path"].cpu().numpy(),
                         pred_omic=o["pred_omic"].cpu().numpy(), grade=bt[5].numpy(), censor=bt[3].numpy(),
                         survtime=bt[4].numpy()))
    ref = S.reference_accumulation(host, task)
    avg_path_TNN, avg_omic_TNN, n_aux = 0, 0, 0
    for t in tnns:                                                    # :392, :409 on the steps that ran the update
        if t is not None:
            avg_path_TNN += t[0].item()
            avg_omic_TNN += t[1].item()
            n_aux += 1
    names = rec.SCALARS
    sums = [got[n + "_epoch" if n.startswith("loss") else n] for n in names]
    print("\n%s %s: record %s" % (case, "graph" if graph else "eager", got))
    assert _same_floats(sums, [float(v) for v in ref["sums"]] + [float(avg_path_TNN), float(avg_omic_TNN)]), (sums, ref["sums"])
    n = len(outs)
    assert got["steps"] == n and got["rows"] == n * B_STEP and got["bad_labels"] == 0 and got["overflow"] == 0
    assert [got[k + "_added"] for k in names[:4]] == [n] * 4 and math.isfinite(got["loss_epoch"])
    assert got["loss_KD_added"] == n and got["loss_KD_epoch"] > 0.0
    assert got["loss_CRD_added"] == (n if step.crd_on else 0) and got["loss_pred_KD_masking_added"] == 0
    assert got["loss_tsvd_added"] == (n if step.tsvd_on else 0)
    assert got["avg_path_TNN_added"] == got["avg_omic_TNN_added"] == n_aux == (n // 2 if step.tsvd_on else 0)
    if step.tsvd_on:
        assert got["avg_path_TNN"] > 0.0 and got["avg_omic_TNN"] > 0.0
    if task == "grad":
        assert [got["grad_acc_epoch"], got["grad_path_epoch"], got["grad_omic_epoch"]] == ref["correct"] and got["stored"] == 0
        with pytest.raises(ValueError):
            rec.cindex()
    else:
        # 3. the store holds the concatenated columns; the three C-indices equal the all-pairs numpy value exactly
        assert got["stored"] == n * B_STEP == rec.rows_host
        st = rec.store.cpu().numpy()
        for k in range(5):
            assert np.array_equal(st[k].astype(np.float64), ref["cols"][k]), S.COLUMNS[k]
        want = tuple(S.cindex_all_pairs(ref["cols"][k], ref["cols"][3], ref["cols"][4]) for k in range(3))
        assert rec.cindex() == want, (rec.cindex(), want)
        assert all(0.0 <= c <= 1.0 for c in want)


def test_read_raises_on_overflow_and_reset_rewinds():
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    step = _mk_step("surv")
    rec = step.record = m.Stage1Record(step, B_STEP + 3)              # the second step does not fit
    bts = _stage1_batches(2, True)
    rec.reset()
    step.step(bts[0], epoch=2)
    assert rec.read()["stored"] == B_STEP
    step.step(bts[1], epoch=2)
    with pytest.raises(RuntimeError, match="did not fit"):
        rec.read()
    rec.reset()                                                       # the memset rewinds the cursor
    step.step(bts[1], epoch=2)
    d = rec.read()
    assert d["stored"] == B_STEP and d["overflow"] == 0 and d["steps"] == 1 and rec.rows_host == B_STEP
    assert np.array_equal(rec.store[4, :B_STEP].cpu().numpy(), bts[1][4].numpy())


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_no_host_read_between_reset_and_read(case):
    """Replayed steps on device-resident batches with the record attached issue no device-to-host copy and no synchronising
    call: torch's sync debug mode in "error" mode (an .item() raises under it; the run prints whether it did) and the dispatch
    spy of tests/test_gpu_epoch.py."""
    import multimodal_learning_amd as m
    m.set_precision("bf16")
    step = _mk_step(case)
    rec = step.record = m.Stage1Record(step, 8 * B_STEP)
    step.enable_graph()
    bt = _stage1_batches(1, step.surv, device="cuda")[0]
    step.start_epoch()
    for _ in range(4):                                                # two eager steps, both captures
        step.step(bt, epoch=2)
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
        step.start_epoch()
        with spy:
            for _ in range(4):
                step.step(bt, epoch=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("\n%s: sync debug mode honoured: %s; device-to-host ops seen by the dispatch spy: %s" % (case, honoured, spy.seen))
    assert spy.seen == [], spy.seen
    got = rec.read()
    assert got["steps"] == 4 and math.isfinite(got["loss_epoch"]) and got["rows"] == 4 * B_STEP
    if step.surv:
        assert got["stored"] == 4 * B_STEP and len(rec.cindex()) == 3


# ------------------------------------------------------------------------------------------------ train_teacher()
class _Loader(list):
    dataset = range(16)


TRAIN_CASES = {
    "miccai2022-grad": ("miccai2022", dict()),
    "mia2022-grad-tsvd": ("mia2022", dict(tsvd=True)),
    "miccai2022-surv": ("miccai2022", dict(surv=True)),
}
EPOCHS = (16, 17, 18)        # the best-checkpoint test runs from epoch 16 on (`epoch > 15`)


def _train_setup(tmp_path, case):
    variant, kw = TRAIN_CASES[case]
    opt = _stage1_opt(batch_size=4, n_data=16, niter=0, niter_decay=EPOCHS[-1], epoch_count=EPOCHS[0], measure=1, verbose=0,
                      checkpoints_dir=str(tmp_path), exp_name="exp", model_name="pathomic_teacher",
                      fixed_model="pathomic_teacher", **kw)
    surv = bool(kw.get("surv"))
    train_loader, test_loader = _Loader(), _Loader()
    labels = torch.arange(16) % 3
    for it, bt in enumerate(_stage1_batches(4, surv, B=4, n_data=16, seed0=900)):
        bt = list(bt)
        bt[6] = torch.arange(4 * it, 4 * it + 4)
        bt[5] = labels[bt[6]].long()
        train_loader.append(tuple(bt))
        test_loader.append((bt[0][0], bt[1], bt[2], bt[3], bt[4], bt[5]))
    return variant, opt, train_loader, test_loader


def _hand_loop(opt, train_loader, test_loader, variant):
    """train_teacher()'s loop by hand over an identically seeded step WITHOUT a record: the reference's statements with their
    host reads after every step, then evaluate.test_teacher."""
    import random
    import multimodal_learning_amd as m
    torch.cuda.manual_seed_all(2019); torch.manual_seed(2019); random.seed(2019)
    step = m.TeacherStage1Step(opt, device="cuda", k=1)
    step.enable_graph()
    surv = opt.task == "surv"
    br = "cox" if surv else "nll"
    eps, best_acc, saved = [], 0.0, []
    for epoch in range(opt.epoch_count, opt.niter + opt.niter_decay + 1):
        step.start_epoch()
        host, tn = [], [0, 0]
        for batch_idx, bt in enumerate(train_loader):
            o = step.step(bt, epoch)
            f = lambda k: o[k].cpu().numpy().reshape(())[()]      # noqa: E731
            host.append(dict(loss=f("loss"), loss_fuse=f("loss_%s_fuse" % br), loss_path=f("loss_%s_path" % br),
                             loss_omic=f("loss_%s_omic" % br), loss_tsvd=f("loss_tsvd"), loss_CRD=f("loss_CRD"),
                             loss_pred_KD=f("loss_pred_KD"), pred_KD_masking_loss=f("loss_pred_KD_masking"),
                             pred=o["pred"].cpu().numpy(), pred_path=o["pred_path"].cpu().numpy(),
                             pred_omic=o["pred_omic"].cpu().numpy(), grade=bt[5].cpu().numpy(), censor=bt[3].cpu().numpy(),
                             survtime=bt[4].cpu().numpy()))
            if step.tsvd_on and batch_idx % opt.aux_iter == 0:
                tn[0] += step.path_TNN.item()
                tn[1] += step.omic_TNN.item()
            if opt.lr_policy == "onecycle":
                step.scheduler.step()
        if opt.lr_policy != "onecycle":
            step.scheduler.step()
        ref = S.reference_accumulation(host, opt.task)
        sums = [float(v) for v in ref["sums"]] + [float(tn[0]), float(tn[1])]
        ep = dict(epoch=epoch, sums=sums, means=[v / len(train_loader) for v in sums])
        if surv:
            ep["cindex"] = tuple(S.cindex_all_pairs(ref["cols"][k], ref["cols"][3], ref["cols"][4]) for k in range(3))
        else:
            ep["acc"] = [c / len(train_loader.dataset) for c in ref["correct"]]
        plan = m.teacher_epoch_end_plan(opt, epoch, variant)
        res = m.evaluate.test_teacher(opt, step.model, test_loader, "cuda")
        ep["test"] = res[:12]
        acc = res[4] if surv else res[9]
        ep["saved"] = bool(plan.may_save and acc > best_acc)
        if ep["saved"]:
            best_acc = acc
            saved.append([p.detach().clone() for p in step.model.parameters()])
        eps.append(ep)
    return step, eps, saved


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_train_teacher_equals_the_hand_loop(tmp_path, case):
    import multimodal_learning_amd as m
    from multimodal_learning_amd import epoch as EP
    from multimodal_learning_amd import trainers
    m.set_precision("bf16")
    variant, opt, train_loader, test_loader = _train_setup(tmp_path, case)
    res = m.train_teacher(copy.copy(opt), train_loader, 16, test_loader, test_loader, "cuda", 1, variant=variant)
    assert len(res) == 5
    module_list, model, ema_model, optimizer, logger = res
    assert module_list[0] is model and set(logger) == {"train", "test", "epochs"}
    assert set(logger["train"]) == set(logger["test"]) == {"loss", "pvalue", "cindex", "surv_acc", "grad_acc"}
    assert all(v == [] for v in logger["train"].values())
    eps = logger["epochs"]
    assert [e["epoch"] for e in eps] == list(EPOCHS) and all(e["steps"] == 4 and e["rows"] == 16 for e in eps)
    step, hand, saved = _hand_loop(copy.copy(opt), train_loader, test_loader, variant)
    names = EP.Stage1Record.SCALARS
    test_names = ("loss_test", "loss_test_fuse", "loss_test_path", "loss_test_omic", "cindex_test", "cindex_test_path",
                  "cindex_test_omic", "pvalue_test", "surv_acc_test", "grad_acc_test", "grad_path_test", "grad_omic_test")
    for e, h in zip(eps, hand):
        sums = [e[n + "_epoch" if n.startswith("loss") else n] for n in names]
        assert _same_floats(sums, h["sums"]), (case, e["epoch"], sums, h["sums"])
        assert _same_floats([e[n + "_mean"] for n in names], h["means"])
        if opt.task == "surv":
            assert (e["cindex_epoch"], e["cindex_path"], e["cindex_omic"]) == h["cindex"]
        else:
            assert [e["grad_acc_train"], e["grad_path_train"], e["grad_omic_train"]] == h["acc"]
        for n, v in zip(test_names, h["test"]):
            assert (e[n] is None and v is None) or _same_floats([float(e[n])], [float(v)]), (case, e["epoch"], n, e[n], v)
        assert ("saved" in e) == h["saved"] and e["used_patches"], (case, e["epoch"])
    if "tsvd" in case:
        assert all(e["avg_path_TNN_added"] == 2 and e["avg_path_TNN"] > 0.0 for e in eps)
    for a, b in zip(list(model.parameters()) + list(ema_model.parameters()),
                    list(step.model.parameters()) + list(step.ema_model.parameters())):
        assert torch.equal(a, b)
    # the best checkpoint: the reference's dict, the parameters of the LAST epoch that beat best_acc, and a file the stage-2
    # trainer's own teacher-loading lines accept
    path = trainers.best_checkpoint_path(opt, 1)
    assert any(h["saved"] for h in hand) and os.path.exists(path) and path == trainers.teacher_checkpoint_path(opt, 1)
    ck = torch.load(path, map_location="cuda", weights_only=False)
    keys = {"split", "opt", "epoch", "model_state_dict", "optimizer_state_dict", "metrics"}
    assert set(ck) == (keys | {"ema_model_state_dict"} if variant == "mia2022" else keys)
    assert ck["split"] == 1 and ck["epoch"] == EPOCHS[-1]
    probe = m.define_net(opt, 1).cuda()
    probe.load_state_dict(ck["model_state_dict"])
    for a, b in zip(probe.parameters(), saved[-1]):
        assert torch.equal(a, b)
    if opt.task == "grad":
        from oracle.step import default_opt
        opt2 = default_opt(nce_p=4, nce_k=8, nce_p2=2, nce_k2=4, select_pos_mode="hard", n_data=16, batch_size=4, checkpoints_dir=str(tmp_path), exp_name="exp",
                           fixed_model="pathomic_teacher", model_name="path_student")
        sd = torch.load(trainers.teacher_checkpoint_path(opt2, 1), map_location="cuda", weights_only=False)["model_state_dict"]
        if hasattr(sd, "_metadata"):
            del sd._metadata
        d2 = m.DistillStep(opt2, 16, device="cuda", k=1, variant="miccai2022")
        d2.fix_model.load_state_dict(sd)
        for a, b in zip(d2.fix_model.parameters(), saved[-1]):
            assert torch.equal(a, b)


def test_train_teacher_mia2023_across_start_epoch(tmp_path):
    """The MIA-2023 trainer at the size of tests/test_gpu_sp_loader.py's masking step (B = 4, 64 x 64 crops of 96 x 96 tiles, the
    6-view tuple of the resident superpixel loader): epoch 16 = start_epoch runs without the masking terms (replayed from the
    graph), epoch 17 with them (eager) - the record is their last launch too.  Against the hand loop; no file is written."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import epoch as EP
    from multimodal_learning_amd import trainers
    from tests.test_gpu_sp_loader import _src
    m.set_precision("bf16x6")
    B, S, SH, n = 4, 64, 96, 24
    opt = _stage1_opt(batch_size=B, n_data=n, niter=0, niter_decay=17, epoch_count=16, measure=1, verbose=0,
                      checkpoints_dir=str(tmp_path), exp_name="exp", model_name="pathomic_teacher", fixed_model="pathomic_teacher",
                      masking=1, start_epoch=16, Path_K=1, Omic_K=5, input_size_path=S, nce_p=4, nce_k=10, pos_mode="multi_pos",
                      num_superpixels=30)
    g = torch.Generator().manual_seed(1)
    ld = m.augment.ResidentSuperpixelLoader(opt, _src(n, SH, SH, 8).cuda(), torch.randn(n, 320, generator=g), torch.arange(n) % 3,
                                            seed=2)
    train_loader, test_loader = _Loader(), _Loader()
    for _ in range(3):
        bt = ld.next(batch_size=B)
        assert len(bt[0]) == 6
        bt = (tuple(v.clone() for v in bt[0]),) + tuple(v.clone() if torch.is_tensor(v) else v for v in bt[1:])
        train_loader.append(bt)
        z = torch.zeros(B)
        test_loader.append((bt[0][0], z, bt[2], z, z, bt[5]))
    res = m.train_teacher(copy.copy(opt), train_loader, n, test_loader, test_loader, "cuda", 1, variant="mia2023")
    eps = res[4]["epochs"]
    step, hand, saved = _hand_loop(copy.copy(opt), train_loader, test_loader, "mia2023")
    names = EP.Stage1Record.SCALARS
    assert [e["epoch"] for e in eps] == [16, 17] and all(e["steps"] == 3 and e["rows"] == 3 * B for e in eps)
    for e, h in zip(eps, hand):
        sums = [e[n_ + "_epoch" if n_.startswith("loss") else n_] for n_ in names]
        assert _same_floats(sums, h["sums"]), (e["epoch"], sums, h["sums"])
        assert [e["grad_acc_train"], e["grad_path_train"], e["grad_omic_train"]] == h["acc"]
        assert _same_floats([float(e["loss_test"]), float(e["grad_acc_test"])], [float(h["test"][0]), float(h["test"][9])])
        assert ("saved" in e) == h["saved"]
    assert eps[0]["loss_pred_KD_masking_added"] == 0 and eps[1]["loss_pred_KD_masking_added"] == 3
    assert eps[1]["loss_pred_KD_masking_epoch"] > 0.0
    for a, b in zip(list(res[1].parameters()) + list(res[2].parameters()),
                    list(step.model.parameters()) + list(step.ema_model.parameters())):
        assert torch.equal(a, b)
    # the reference's save is commented out (:389-397): the path is recorded, nothing is written
    assert any("saved" in e for e in eps) and not os.path.exists(trainers.best_checkpoint_path(opt, 1))


def test_train_teacher_refuses_what_the_variant_lacks(tmp_path):
    import multimodal_learning_amd as m
    _, opt, train_loader, test_loader = _train_setup(tmp_path, "mia2022-grad-tsvd")
    with pytest.raises(ValueError):
        m.train_teacher(opt, train_loader, 16, test_loader, test_loader, "cuda", 1, variant="miccai2022")
    with pytest.raises(ValueError):
        m.train_teacher(opt, train_loader, 16, test_loader, test_loader, "cuda", 1, variant="stage2")

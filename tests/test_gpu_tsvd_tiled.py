"""The tiled t-SVD prox (csrc/tsvd.hip, 128 < B <= 512 rows: block one-sided Jacobi across workgroups, one launch per
round-robin step) through both C-ABI entry points, tsvd.update_aux and the stage-1 step, against the float64 oracle
(oracle/variants.py:update_aux).

Tolerances.  tests/tsvd_emulation.py restates the device's algorithm in numpy float32; its error against the oracle at
every shape of tsvd_emulation.SHAPES is recorded in tests/golden/tsvd_tiled_restatement.json.  The device is held to
    aux:  4 x the restatement's max |error| at that shape + FLOOR["aux"] x max(max |ref|, 1)
    TNN:  4 x the restatement's relative error at that shape + FLOOR["tnn"]
where FLOOR is 4 x the largest excess of the device's error over the first term that an MI355X run of this file printed
(`excess[...]` lines below).  An aux floor above 2e-5 - the bound of the single-workgroup kernels - would be a finding.
Measured on the MI355X: at all seven shapes the device's error is below the restatement's own (aux 4.6e-7 .. 1.4e-6 against
1.3e-6 .. 6.6e-6, TNN 2.9e-8 .. 1.5e-6 relative against 1.9e-5 .. 1.8e-4), the largest excess is 0 and both floors are 0
(tsvd_emulation.FLOOR).
"""
import copy
import functools
import threading

import numpy as np
import pytest
import torch

from tests import tsvd_emulation as E
from tests.gpu_util import Guarded, Report

pytestmark = pytest.mark.gpu

PH_EINVAL = -22
EXCESS = {"aux": 0.0, "tnn": 0.0}


@functools.lru_cache(maxsize=None)
def _case(B, V, D, tau):
    from oracle import variants as OV
    adj = E.make_stack(B, V, D)
    ref, tnn_ref = OV.update_aux(adj, tau)
    return adj, ref, tnn_ref


def _call(adj, tau, dev_tau=False):
    """adj [B, B, V] cpu -> (aux [B, B, V] float32 numpy, tnn, tail [16], raw aux tensor) through the C-ABI, every output
    between guard bands and the workspace exactly ph_tsvd_workspace_bytes long."""
    from multimodal_learning_amd._lib import lib, ptr, stream, check
    L = lib()
    B, _, V = adj.shape
    a = adj.float().cuda().permute(2, 0, 1).contiguous()
    aux = Guarded((V, B, B), torch.float32)
    tnn = Guarded((1,), torch.float32)
    ws = Guarded((L.ph_tsvd_workspace_bytes(V, B),), torch.uint8, fill=0xFF)      # (NaN patterns: nothing may be read unwritten)
    if dev_tau:
        t = torch.tensor([tau], dtype=torch.float32, device="cuda")
        check(L.ph_tsvd_update_aux_dev(ptr(a), ptr(aux.t), ptr(tnn.t), V, B, ptr(t), ptr(ws.t), stream()), "ph_tsvd_update_aux_dev")
    else:
        check(L.ph_tsvd_update_aux(ptr(a), ptr(aux.t), ptr(tnn.t), V, B, float(tau), ptr(ws.t), stream()), "ph_tsvd_update_aux")
    torch.cuda.synchronize()
    assert aux.guards_intact() and tnn.guards_intact() and ws.guards_intact(), "a guard band was written"
    assert not torch.isnan(aux.t).any(), "aux elements left unwritten"
    tail = ws.t[-64:].view(torch.float32).cpu().numpy()
    return aux.t.permute(1, 2, 0).cpu().numpy(), float(tnn.t[0]), tail, aux.t.clone()


def _judge(R, what, aux, tnn, ref, tnn_ref, rec):
    """Adds the aux / TNN rows of one result to the report and keeps the excess over the restatement's share."""
    tol_a, tol_t = E.tolerances(rec)
    ea, et = E.errors(aux, tnn, ref, tnn_ref)
    scale = max(float(np.abs(ref).max()), 1.0)
    xa = max(ea - E.MARGIN * rec["aux_err"], 0.0) / scale
    xt = max(et - E.MARGIN * rec["tnn_rel"], 0.0)
    EXCESS["aux"], EXCESS["tnn"] = max(EXCESS["aux"], xa), max(EXCESS["tnn"], xt)
    print(f"   {what}: aux err {ea:.3e} (restatement {rec['aux_err']:.3e})  TNN rel {et:.3e} (restatement {rec['tnn_rel']:.3e})")
    print(f"   excess[aux] = {xa:.3e} of max(max |ref|, 1) (floor {E.FLOOR['aux']:.1e});  excess[tnn] = {xt:.3e} (floor {E.FLOOR['tnn']:.1e});"
          f"  largest so far {EXCESS['aux']:.3e} / {EXCESS['tnn']:.3e}")
    R.add(what + " aux", ea, float(np.abs(ref).max()), tol_a)
    R.add(what + " TNN (relative)", et, abs(tnn_ref), tol_t)


def _restated(adj, tau, ref, tnn_ref):
    """A record like the golden file's for a stack that is not in it (the restatement run on the spot)."""
    aux, tnn, sweeps = E.restate(adj.numpy(), tau)
    ea, et = E.errors(aux, tnn, ref, tnn_ref)
    return dict(aux_err=ea, tnn_rel=et, max_ref=float(np.abs(ref).max()), sweeps=sweeps)


@pytest.mark.parametrize("B,V,D,tau", E.SHAPES)
def test_tiled_update_aux_vs_oracle(B, V, D, tau):
    """Both entry points at every shape: accuracy, guard bands, every element written, bitwise agreement of the two
    entries and of a second call, sweep counters under the cap."""
    adj, ref, tnn_ref = _case(B, V, D, tau)
    rec = E.record()[E.key(B, V, D, tau)]
    R = Report(f"tiled t-SVD prox B={B} V={V} D={D} tau={tau} vs float64 oracle")
    aux, tnn, tail, raw = _call(adj, tau)
    aux_d, tnn_d, tail_d, raw_d = _call(adj, tau, dev_tau=True)
    aux_2, tnn_2, tail_2, raw_2 = _call(adj, tau)
    _judge(R, "host tau", aux, tnn, ref, tnn_ref, rec)
    _judge(R, "device tau", aux_d, tnn_d, ref, tnn_ref, rec)
    assert torch.equal(raw, raw_d) and tnn == tnn_d, "the two entry points differ"
    S = V // 2 + 1                              # (the tail's other slots are never written)
    assert torch.equal(raw, raw_2) and tnn == tnn_2 and np.array_equal(tail[:S], tail_2[:S]) and np.array_equal(tail[8:8 + S], tail_2[8:8 + S]), \
        "a second call differs"
    sweeps = tail[8:8 + S]
    print(f"   sweeps per slice {sweeps.tolist()} (restatement {rec['sweeps']})")
    assert (sweeps >= 1).all() and (sweeps < E.TB_MAX_SWEEPS).all(), sweeps
    R.finish()


@pytest.mark.parametrize("B,V,D,tau", E.SHAPES)
def test_tiled_update_aux_exact_cases(B, V, D, tau):
    """tau = 0 reproduces the input; a threshold above every singular value gives exact zeros and TNN == 0."""
    adj, _, _ = _case(B, V, D, tau)
    rec = E.record()[E.key(B, V, D, tau)]
    aux0, _, _, _ = _call(adj, 0.0)
    err = float(np.abs(aux0.astype(np.float64) - adj.numpy()).max())
    tol = E.MARGIN * rec["aux_err"] + E.FLOOR["aux"] * max(float(adj.abs().max()), 1.0)
    xa = max(err - E.MARGIN * rec["aux_err"], 0.0) / max(float(adj.abs().max()), 1.0)
    EXCESS["aux"] = max(EXCESS["aux"], xa)
    print(f"\n   tau = 0: max |aux - adj| {err:.3e}  tol {tol:.3e}   excess[aux] = {xa:.3e} (largest so far {EXCESS['aux']:.3e})")
    assert err <= tol, (err, tol)
    auxz, tnnz, _, _ = _call(adj, 1e4, dev_tau=True)
    assert not auxz.any() and tnnz == 0.0


def test_tiled_update_aux_degenerate_stacks():
    """B = 160: all zeros stays exactly zero; four identical views and a rank-1 stack are finite and the oracle's."""
    from oracle import variants as OV
    B, V, tau = 160, 4, 0.3
    auxz, tnnz, _, _ = _call(torch.zeros(B, B, V), tau)
    assert not auxz.any() and tnnz == 0.0
    adj, _, _ = _case(160, 4, 32, 0.3)
    same = adj[:, :, :1].repeat(1, 1, V).contiguous()
    g = torch.Generator().manual_seed(160)
    u, w, s = torch.rand(B, generator=g) + 0.1, torch.rand(B, generator=g) + 0.1, torch.rand(V, generator=g) + 0.5
    rank1 = (torch.outer(u, w) / B)[:, :, None] * s
    R = Report("tiled t-SVD prox, degenerate stacks at B = 160")
    for name, x, t in (("identical views", same, tau), ("rank-1 stack", rank1, 0.05)):
        ref, tnn_ref = OV.update_aux(x, t)
        rec = _restated(x, t, ref, tnn_ref)
        aux, tnn, _, _ = _call(x, t)
        assert np.isfinite(aux).all() and np.isfinite(tnn)
        _judge(R, name, aux, tnn, ref, tnn_ref, rec)
    R.finish()


def _stage1_opt(m, bs, aux_iter=1):
    opt = m.stage2_opt(dropout_rate=0.0, batch_size=bs, cut_fuse_grad=True, num_teachers=2)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss = 1, 1.0, 0, 0, "False"
    opt.tSVD_loss, opt.tSVD_mode, opt.n_views, opt.aux_iter = "True", "pathomic", 4, aux_iter
    opt.mu, opt.pho, opt.max_mu, opt.Lambda_global = 0.01, 1.5, 1.0, 0.05
    return opt


def _stage1(m, opt, sync=None):
    from oracle import weights as W
    model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
    model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3)); ema.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 4))
    return m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()), sync=sync)


def test_limits():
    """Above TSVD_MAX_ROWS rows: PH_EINVAL from the C-ABI, ValueError from tsvd.update_aux and from the stage-1 step's
    constructor (its own batch, or its batch times the world size)."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd._lib import lib, ptr, stream
    from tests.test_gpu_replicas import LocalGroup, LocalSync
    assert m.tsvd.TSVD_MAX_ROWS == E.TSVD_MAX_ROWS == 512
    L = lib()
    a = torch.zeros(16, device="cuda")
    assert L.ph_tsvd_update_aux(ptr(a), ptr(a), ptr(a), 4, 513, 0.1, ptr(a), stream()) == PH_EINVAL
    assert L.ph_tsvd_update_aux_dev(ptr(a), ptr(a), ptr(a), 4, 513, ptr(a), ptr(a), stream()) == PH_EINVAL
    with pytest.raises(ValueError, match="TSVD_MAX_ROWS"):
        m.tsvd.update_aux(torch.zeros(513, 513, 4, device="cuda"), 0.1)
    with pytest.raises(ValueError, match="TSVD_MAX_ROWS"):
        _stage1(m, _stage1_opt(m, 520))
    with pytest.raises(ValueError, match="TSVD_MAX_ROWS"):
        _stage1(m, _stage1_opt(m, 300), sync=LocalSync(LocalGroup(2), 0, expect_slice=False))


def test_workspace_bytes_unchanged_up_to_128_rows_and_grows_above():
    from multimodal_learning_amd._lib import lib
    L = lib()
    for V in (2, 4, 6, 8):
        for B in (1, 8, 64, 65, 127, 128):
            assert L.ph_tsvd_workspace_bytes(V, B) == ((V // 2 + 1) * 4 * B * B + 16) * 4
        for B in (129, 256, 512):
            assert L.ph_tsvd_workspace_bytes(V, B) > ((V // 2 + 1) * 4 * B * B + 16) * 4


def test_stage1_step_at_160_rows():
    """The stage-1 step at a batch of 160 (64 x 64 tiles): finite, and the auxiliary tensors and TNN it leaves are the
    oracle's prox of the adjacency tensors it computed."""
    import multimodal_learning_amd as m
    from oracle import variants as OV
    from oracle.step import synthetic_batch
    B = 160
    opt = _stage1_opt(m, B)
    st = _stage1(m, opt)
    bt = synthetic_batch(B, 64, seed=5)
    z = torch.zeros(B)
    out = st.step(((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"]))
    assert torch.isfinite(out["loss"]).all() and torch.isfinite(out["loss_tsvd"]).all()
    R = Report("stage-1 step at B = 160: aux tensors / TNN vs the oracle's prox of the step's adjacency tensors")
    tau = opt.Lambda_global / opt.mu
    for name, adj, aux, tnn in (("path", st.adj_tensor1, st.aux_tensor1, st.path_TNN), ("omic", st.adj_tensor2, st.aux_tensor2, st.omic_TNN)):
        stack = torch.stack([a.detach().cpu() for a in adj], dim=2)
        ref, tnn_ref = OV.update_aux(stack, tau)
        rec = _restated(stack, tau, ref, tnn_ref)
        got = torch.stack([a.cpu() for a in aux], dim=2).numpy()
        _judge(R, name, got, float(tnn), ref, tnn_ref, rec)
    R.finish()


def test_stage1_step_graph_replay_equals_eager_at_136_rows():
    """The stage-1 step at 136 rows, aux_iter = 2, replayed from captured graphs (the fixed launch count and the device-side
    flags keep the tiled prox capturable) against the same steps launched eagerly."""
    import multimodal_learning_amd as m
    from oracle.step import synthetic_batch
    B, aux_iter = 136, 2
    opt = _stage1_opt(m, B, aux_iter)
    opt.cut_fuse_grad = False
    opt.mu, opt.pho, opt.max_mu, opt.Lambda_global = 1e-3, 1.3, 10.0, 0.05
    bts = []
    for i in range(2):
        bt = synthetic_batch(B, 64, seed=90 + i)
        z = torch.zeros(B).cuda()
        bts.append(((bt["x_path"].cuda(), bt["ema_x_path"].cuda()), z, bt["x_omic"].cuda(), z, z, bt["grade"].cuda(), bt["index"].cuda(),
                    bt["sample_idx"].cuda()))
    res = {}
    for graph in (False, True):
        st = _stage1(m, copy.copy(opt))
        if graph:
            st.enable_graph()
        st.start_epoch()
        losses = []
        for it in range(8):
            out = st.step(bts[(it // 2) % 2])      # (both kinds of step on both input sets)
            losses.append({k: float(out[k]) for k in ("loss", "loss_nll", "loss_tsvd", "loss_pred_KD")})
        if graph:
            assert st._g_sets and len(st._g_sets) == 2 and all(len(q["graphs"]) == 2 for q in st._g_sets), \
                "steps 2.. must have been replayed from graphs (two input sets)"
        res[graph] = dict(losses=losses, w=st.model.state_dict()["path_net.fc_new2.weight"].clone() if "path_net.fc_new2.weight" in st.model.state_dict()
                          else next(iter(st.model.parameters())).detach().clone(), mu=st.mu, aux=st.aux_tensor1[2].clone())
    for it in range(8):
        for k, v in res[False]["losses"][it].items():
            g = res[True]["losses"][it][k]
            assert abs(g - v) <= 2e-3 * max(1.0, abs(v)), (it, k, g, v)
    assert res[True]["mu"] == res[False]["mu"]
    assert (res[True]["aux"] - res[False]["aux"]).abs().max().item() <= 2e-3 * max(1.0, res[False]["aux"].abs().max().item())
    assert (res[True]["w"] - res[False]["w"]).abs().max().item() <= 5e-3 * max(1e-3, res[False]["w"].abs().max().item())


def test_two_stage1_replicas_of_72_rows_equal_one_process_of_144():
    """The case the tiled prox exists for: under data parallelism the adjacency / auxiliary tensors span the global batch
    (2 x 72 = 144 rows > 128).  Two in-process replicas against one process on the whole batch."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd.dist import shard_batch
    from oracle.step import synthetic_batch
    from tests.test_gpu_replicas import LocalGroup, LocalSync
    B, H = 144, 64
    heads = ("classifier.0.weight", "path_net.fc_new2.weight", "omic_net.classifier.0.weight")
    m.set_precision("bf16x6")
    try:
        bt = synthetic_batch(B, H, seed=950)
        for k in ("x_path", "ema_x_path", "x_omic"):
            bt[k][B // 2:] = bt[k][:B // 2]
        z = torch.zeros(B)
        batch = ((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"])
        single = _stage1(m, _stage1_opt(m, B))
        names = dict(single.model.named_parameters())
        assert all(h in names for h in heads)
        o1 = single.step(batch)
        g1 = {h: names[h].grad.clone() for h in heads}
        group = LocalGroup(2)
        reps = [_stage1(m, _stage1_opt(m, B // 2), sync=LocalSync(group, r, expect_slice=False)) for r in range(2)]
        outs, errs = [None, None], []

        def run(r):
            try:
                outs[r] = reps[r].step(shard_batch(batch, r, 2))
                torch.cuda.synchronize()
            except BaseException as e:      # noqa: BLE001
                errs.append(e)
                group.barrier.abort()
        ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(300)
        if errs:
            raise errs[0]
        f0, f1 = reps[0].optimizer.flat, reps[1].optimizer.flat
        assert torch.equal(f0.grad, f1.grad) and torch.equal(f0.flat, f1.flat)
        assert reps[0].aux_tensor1[0].shape == (B, B)
        assert torch.equal(outs[0]["loss_tsvd"], outs[1]["loss_tsvd"])      # a function of the global batch
        assert abs(float(outs[0]["loss_tsvd"]) - float(o1["loss_tsvd"])) <= 2e-4 * max(abs(float(o1["loss_tsvd"])), 1e-3), \
            (float(outs[0]["loss_tsvd"]), float(o1["loss_tsvd"]))
        for k in ("loss_nll", "loss_pred_KD"):                              # partial sums over the replica's rows
            tot = sum(float(o[k]) for o in outs)
            assert abs(tot - float(o1[k])) <= 2e-4 * max(abs(float(o1[k])), 1e-3), (k, tot, float(o1[k]))
        for v in range(4):
            assert float((reps[0].aux_tensor1[v] - single.aux_tensor1[v]).abs().max()) <= 2e-5
            assert float((reps[0].adj_tensor2[v] - single.adj_tensor2[v]).abs().max()) <= 2e-5
            assert torch.equal(reps[0].aux_tensor2[v], reps[1].aux_tensor2[v])
        n0 = dict(reps[0].model.named_parameters())
        for h in heads:
            err = float((n0[h].grad - g1[h]).abs().max())
            assert err <= 1e-3 * float(g1[h].abs().max()) + 1e-7, (h, err)
    finally:
        m.set_precision("bf16")

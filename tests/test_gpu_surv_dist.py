"""The survival (Cox) task of the stage-1 teacher under data parallelism: the risk sets span the
global batch, as under the reference's nn.DataParallel (train_test_MT.py:63-64).  Pinned here:

  * the gathered loss kernel (ph_surv_pack_rows + ph_surv_stage1_loss_grad_gathered) is bitwise the single-process kernel
    on the concatenated batch, for every rank;
  * two replicas emulated on one GPU (threads exchanging through `LocalSync`, a copy of tests/test_gpu_replicas.py's
    stand-in with `all_gather_into`) equal one process on the whole batch, and a per-shard Cox loss would not;
  * one RCCL rank in a child process: the gathered step is captured in the step graph and replays like the eager twin."""
import copy
import os
import subprocess
import sys
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SURV_KEYS = ("loss_cox", "loss_cox_fuse", "loss_cox_path", "loss_cox_omic", "loss_kd_fuse", "loss_kd_path", "loss_kd_omic")


def _surv_opt(**kw):
    import multimodal_learning_amd as m
    base = dict(task="surv", act_type="Sigmoid", label_dim=1, dropout_rate=0.0, batch_size=8, cut_fuse_grad=False,
                num_teachers=2, reg_type="none")
    base.update(kw)
    opt = m.stage2_opt(**base)
    opt.pred_distill = 1
    return opt


# ------------------------------------------------------------------------------------------------ the kernel
def _surv_rows(B, seed):
    g = torch.Generator().manual_seed(seed)
    p = [torch.randn(B, generator=g) * 0.7 + 0.2 * k for k in range(3)]
    q = [x + 0.3 * torch.randn(B, generator=g) for x in p]
    t = torch.randint(1, max(2, B // 3), (B,), generator=g).float()          # many ties
    c = (torch.rand(B, generator=g) > 0.3).float()                            # about 30 % censored
    return [x.cuda() for x in p], [x.cuda() for x in q], t.cuda(), c.cuda()


@pytest.mark.parametrize("world,n", [(w, n) for w in (1, 2, 3, 8) for n in (1, 5, 64, 512) if w * n <= 4096])
def test_gathered_surv_kernel_is_bitwise_the_concatenated_one(world, n):
    from multimodal_learning_amd._lib import lib, ptr, stream
    B = world * n
    p, q, t, c = _surv_rows(B, 1000 * world + n)
    lam, kw = 0.7, 1.3
    for nt in range(4):
        qp = [ptr(x) for x in q] if nt else [None] * 3
        ref_terms = torch.empty(9, device="cuda")
        ref_d = torch.empty(3, B, device="cuda")
        assert lib().ph_surv_stage1_loss_grad(ptr(p[0]), ptr(p[1]), ptr(p[2]), *qp, ptr(t), ptr(c), B, nt, lam, kw,
                                              ptr(ref_terms), ptr(ref_d), stream()) == 0
        ref_fwd = torch.empty(9, device="cuda")
        assert lib().ph_surv_stage1_loss_grad(ptr(p[0]), ptr(p[1]), ptr(p[2]), *qp, ptr(t), ptr(c), B, nt, lam, kw,
                                              ptr(ref_fwd), None, stream()) == 0
        # each rank packs its rows into its block of the gathered buffer, where the all-gather would land them
        gathered = torch.full((world, 8, n), float("nan"), device="cuda")
        for r in range(world):
            s = slice(r * n, (r + 1) * n)
            qr = [ptr(x[s]) for x in q] if nt else [None] * 3
            assert lib().ph_surv_pack_rows(ptr(p[0][s]), ptr(p[1][s]), ptr(p[2][s]), *qr, ptr(t[s]), ptr(c[s]), n, nt,
                                           ptr(gathered[r]), stream()) == 0
        qs = q if nt else [torch.zeros_like(t)] * 3          # num_teachers 0: the teacher rows are packed as zeros
        assert torch.equal(gathered, torch.stack([x.reshape(world, n) for x in p + qs + [t, c]], 1)), nt
        ds = []
        for r in range(world):
            terms = torch.empty(9, device="cuda")
            d = torch.empty(3, n, device="cuda")
            assert lib().ph_surv_stage1_loss_grad_gathered(ptr(gathered), world, n, r, nt, lam, kw, ptr(terms), ptr(d),
                                                           stream()) == 0
            fwd = torch.empty(9, device="cuda")
            assert lib().ph_surv_stage1_loss_grad_gathered(ptr(gathered), world, n, r, nt, lam, kw, ptr(fwd), None,
                                                           stream()) == 0
            assert torch.equal(terms, ref_terms), (nt, r, terms, ref_terms)
            assert torch.equal(fwd, ref_fwd), (nt, r)
            ds.append(d)
        assert torch.equal(torch.cat(ds, 1), ref_d), (nt, (torch.cat(ds, 1) - ref_d).abs().max().item())


# ------------------------------------------------------------------------------------------------ two replicas
class LocalGroup:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world


class LocalSync:
    """tests/test_gpu_replicas.py's in-process stand-in of dist.ReplicaSync (the stage-1 step announces no gradient slice),
    with all_gather_into."""

    def __init__(self, group, rank):
        self.g, self.rank, self.world_size = group, rank, group.world

    def _exchange(self, t):
        self.g.slots[self.rank] = t
        self.g.barrier.wait()
        parts = list(self.g.slots)
        self.g.barrier.wait()
        return parts

    def _sum(self, t):
        parts = self._exchange(t.clone())
        tot = parts[0].clone()
        for p in parts[1:]:
            tot += p                       # rank order on every replica: bitwise identical results
        t.copy_(tot)
        return t

    def all_reduce_grads(self, flat):
        g = flat if torch.is_tensor(flat) else flat.grad
        return self._sum(g)

    def all_reduce_sum(self, t):
        return self._sum(t)

    def all_reduce_z(self, sums, count):
        self._sum(sums)
        return count * self.world_size

    def all_gather_rows(self, y, v1, v2):
        ys, a, b = self._exchange(y.clone()), self._exchange(v1.clone()), self._exchange(v2.clone())
        return torch.cat(ys, 0), torch.cat(a, 0), torch.cat(b, 0)

    def all_gather_cat(self, t):
        return torch.cat(self._exchange(t.clone()), 0)

    def all_gather_into(self, out, inp):
        for r, part in enumerate(self._exchange(inp.clone())):
            out[r].copy_(part)
        return out

    def attach_parts(self, crds, flats, modules):
        for crd in crds:
            crd.contrast.sync = self


def _replica_batch(B, seed):
    """Second half's images and omic vectors equal to the first half's (per-replica BatchNorm then sees the whole batch's
    statistics); survival times interleaved over the two halves, with a tie, so the risk sets cross the shard boundary."""
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, 64, seed=seed, P=1, K=16)
    for k in ("x_path", "ema_x_path", "x_omic"):
        bt[k][B // 2:] = bt[k][:B // 2]
    t = torch.tensor([2.0, 7.0, 1.0, 5.0, 4.0, 2.0, 8.0, 3.0])
    c = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0])
    return ((bt["x_path"], bt["ema_x_path"]), torch.zeros(B), bt["x_omic"], c, t, bt["grade"], bt["index"],
            bt["sample_idx"])


@pytest.mark.parametrize("nt", [1, 3])
def test_two_surv_replicas_equal_one_process_on_the_global_batch(nt):
    import multimodal_learning_amd as m
    from multimodal_learning_amd import ops
    from multimodal_learning_amd.dist import shard_batch
    from oracle import weights as W
    B = 8
    sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
    esd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 4)

    def build(bs, sync):
        opt = _surv_opt(batch_size=bs, num_teachers=nt)
        model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
        model.load_state_dict(sd); ema.load_state_dict(esd)
        return m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda()), sync=sync)

    heads = ("classifier.0.weight", "path_net.fc_new2.weight", "omic_net.classifier.0.weight")
    m.set_precision("bf16x6")
    try:
        batch = _replica_batch(B, 951)
        single = build(B, None)
        names = dict(single.model.named_parameters())
        assert all(h in names for h in heads), [n for n in names if "classifier" in n or "fc_new2" in n]
        o1 = single.step(batch)
        g1 = {h: names[h].grad.clone() for h in heads}
        group = LocalGroup(2)
        reps = [build(B // 2, LocalSync(group, r)) for r in range(2)]
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
        tol = 2e-4
        for k in SURV_KEYS:            # functions of the global batch: the same value on every replica
            assert torch.equal(outs[0][k], outs[1][k]), k
            ref = float(o1[k])
            assert abs(float(outs[0][k]) - ref) <= tol * max(abs(ref), 1e-3), (k, float(outs[0][k]), ref)
        n0 = dict(reps[0].model.named_parameters())
        for h in heads:
            err = float((n0[h].grad - g1[h]).abs().max())
            assert err <= 1e-3 * float(g1[h].abs().max()) + 1e-7, (h, err)
        # negative control: the Cox loss of one replica's rows alone (the per-replica objective) is far from the global one
        _, _, _, c, t, _, _, _ = shard_batch(batch, 0, 2)
        local = ops.surv_loss_terms(outs[0]["pred"], outs[0]["pred_path"], outs[0]["pred_omic"], t.cuda(), c.cuda())
        ref = float(o1["loss_cox"])
        assert abs(float(local.sum()) - ref) > 10 * tol * max(abs(ref), 1e-3), (float(local.sum()), ref)
    finally:
        m.set_precision("bf16")


# ------------------------------------------------------------------------------------------------ one RCCL rank, graphs
def _graph_pair_inputs(B, seed):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, 64, seed=seed, P=1, K=16)
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 6, (B,), generator=gen).float()
    c = (torch.rand(B, generator=gen) > 0.4).float()
    return bt, t, c


def _rank_child(store_path, out_path):
    """Run in a child process: one RCCL rank (world size 1, FileStore rendezvous), a TeacherStage1Step(surv) with a
    ReplicaSync and enable_graph() next to a sync=None twin launched eagerly, 7 steps each (odd steps device-resident
    inputs filled in place, even steps host tensors, as tests/test_gpu_survival.py's replay test)."""
    import warnings
    import torch.distributed as dist
    import multimodal_learning_amd as m
    from multimodal_learning_amd.dist import ReplicaSync
    from oracle import weights as W
    torch.cuda.set_device(0)
    # collectives inside captured graphs: the watchdog's asynchronous error handling must not touch the streams (as bench.py)
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
    dist.init_process_group("nccl", store=dist.FileStore(store_path, 1), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        B = 8
        opt = _surv_opt(num_teachers=3)
        sd = W.make_state_dict(W.teacher_shapes(320, label_dim=1), 3)
        res = {}
        for mode in ("eager", "graph"):
            model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
            model.load_state_dict(sd); ema.load_state_dict(sd)
            sync = ReplicaSync() if mode == "graph" else None
            st = m.TeacherStage1Step(copy.deepcopy(opt), device="cuda", models=(model.cuda(), ema.cuda()), sync=sync)
            if mode == "graph":
                st.enable_graph()
            steps, resident = [], None
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for it in range(7):
                    bt, t, c = _graph_pair_inputs(B, 40 + min(it, 5))
                    host = [bt["x_path"], bt["ema_x_path"], bt["x_omic"], c, t, bt["grade"], bt["index"], bt["sample_idx"]]
                    if it % 2 == 1:
                        if resident is None:
                            resident = [x.cuda().contiguous() for x in host]
                        for r, x in zip(resident, host):
                            r.copy_(x)
                        ins = resident
                    else:
                        ins = host
                    out = st.step(((ins[0], ins[1]), torch.zeros(B), ins[2], ins[3], ins[4], ins[5], ins[6], ins[7]))
                    rec = {k: v.detach().cpu().clone() for k, v in out.items() if k.startswith("loss")}
                    rec["w"] = st.model.classifier[0].weight.detach().cpu().clone()
                    rec["w_omic"] = st.model.omic_net.encoder[0][0].weight.detach().cpu().clone()
                    steps.append(rec)
                torch.cuda.synchronize()
            res[mode] = steps
            if mode == "graph":
                res["warnings"] = [str(w.message) for w in caught]
                res["want_graph"] = bool(getattr(st, "_want_graph", False))
                res["sets"] = sorted((q["adopted"], len(q["graphs"]), "_surv_gather" in q) for q in st._g_sets)
        torch.save(res, out_path)
    finally:
        dist.destroy_process_group()


def test_surv_step_with_one_rccl_rank_is_captured_and_replays_like_eager(tmp_path):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_surv_dist as T; T._rank_child(%r, %r)"
            % (ROOT, HERE, str(tmp_path / "store"), str(tmp_path / "res.pt")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    res = torch.load(str(tmp_path / "res.pt"))
    assert not [w for w in res["warnings"] if "capture" in w], res["warnings"]
    assert res["want_graph"], "the gathered survival step fell back to eager launches"
    assert res["sets"] == [(False, 1, True), (True, 1, True)], res["sets"]
    e, g = res["eager"], res["graph"]
    for k in SURV_KEYS:                # step 1, eager in both: the gathered kernel is bitwise the single-process one
        assert torch.equal(g[0][k], e[0][k]), (k, g[0][k], e[0][k])
    for it in range(2, 7):
        for k in ("loss", "loss_cox", "loss_cox_fuse", "loss_cox_path", "loss_cox_omic", "loss_pred_KD"):
            assert abs(g[it][k].item() - e[it][k].item()) <= 2e-3 * max(abs(e[it][k].item()), 1e-3), \
                (it, k, g[it][k].item(), e[it][k].item())
        for k in ("w", "w_omic"):
            assert (g[it][k] - e[it][k]).abs().max().item() <= 5e-3 * max(e[it][k].abs().max().item(), 1e-3), (it, k)

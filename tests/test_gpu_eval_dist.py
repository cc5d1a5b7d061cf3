"""The test pass sharded over replicas (evaluate.test_patches / test_teacher_patches with sync=).

Replicas are threads on one GPU exchanging through `LocalSync` (tests/test_gpu_surv_dist.py's stand-in with
`broadcast_from0` and a gather counter).  5 ROIs of 96 x 96, S = 64, grid 3: 45 rows; batches of 8 (six, the last one of 5
rows) over W = 2 and 4 replicas, and batches of 16 over W = 4 (three batches: one replica runs none).  Every replica has
its own copy of the networks; the copies of ranks != 0 have their BatchNorm running statistics perturbed beforehand.
Pinned: every replica's result is the single-process result of rank 0's networks bit for bit; the perturbed copies end
with rank 0's buffers; a perturbed copy evaluated alone gives other rows; exactly one gather per pass.
One real RCCL rank (world size 1, FileStore) in a child process equals sync=None."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests.gpu_util import assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_ROI, SH, S = 5, 96, 64
PATIENTS = ["TCGA-a", "TCGA-a", "TCGA-b", "TCGA-c", "TCGA-c"]
GRADES = [2, 2, 0, 1, 1]
CENSOR = [1.0, 1.0, 0.0, 1.0, 1.0]
SURVTIME = [5.0, 5.0, 9.0, 2.0, 2.0]


def _opt(batch_size=8, **kw):
    from oracle.step import default_opt
    return default_opt(dropout_rate=0.25, input_size_path=S, batch_size=batch_size, **kw)


def _store():
    g = torch.Generator().manual_seed(23)
    tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8)
    return tiles.cuda(), torch.randn(N_ROI, 320, generator=g), torch.tensor(GRADES)


def _loader(store, opt, surv=False):
    import multimodal_learning_amd as m
    tiles, omic, grade = store
    kw = dict(censor=CENSOR, survtime=SURVTIME) if surv else {}
    return m.augment.ResidentPatchLoader(opt, tiles, omic, grade, patient=PATIENTS, **kw)


def _nets(opt, perturb=0.0):
    """A copy of the (student, teacher) pair - the same weights every time; perturb != 0 moves every BatchNorm running
    statistic, as a replica's own training batches would have."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    surv = opt.task == "surv"
    student = None
    if not surv:
        student = m.define_net(opt, 1, path_only=True)
        student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
        student = student.cuda()
    teacher = m.define_net(opt, 1)
    teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320, label_dim=1) if surv else W.teacher_shapes(320), 3))
    teacher = teacher.cuda()
    if perturb:
        with torch.no_grad():
            for net in (student, teacher):
                if net is None:
                    continue
                for name, b in net.named_buffers():
                    if name.endswith("running_mean"):
                        b.add_(perturb)
                    elif name.endswith("running_var"):
                        b.mul_(1.0 + perturb)
                    elif name.endswith("num_batches_tracked"):
                        b.add_(7)
    return student, teacher


class LocalGroup:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=120)
        self.slots = [None] * world
        self.gathers = [0] * world
        self.broadcasts = [0] * world


class LocalSync:
    """tests/test_gpu_surv_dist.py's in-process stand-in of dist.ReplicaSync, reduced to what the test pass uses, with
    broadcast_from0; it counts the gathers and broadcasts of every rank."""

    def __init__(self, group, rank):
        self.g, self.rank, self.world_size = group, rank, group.world

    def _exchange(self, t):
        self.g.slots[self.rank] = t
        self.g.barrier.wait()
        parts = list(self.g.slots)
        self.g.barrier.wait()
        return parts

    def all_gather_cat(self, t):
        self.g.gathers[self.rank] += 1
        torch.cuda.synchronize()            # (the replicas are threads with one stream each: the parts must be complete)
        return torch.cat(self._exchange(t.clone()), 0)

    def broadcast_from0(self, tensors):
        self.g.broadcasts[self.rank] += 1
        torch.cuda.synchronize()
        src = self._exchange([t.detach().clone() for t in tensors])[0]
        for t, s in zip(tensors, src):
            t.detach().copy_(s)
        torch.cuda.synchronize()
        self.g.barrier.wait()
        return tensors


def _run_replicas(W, fn):
    """fn(rank, sync) on W threads; returns the per-rank results and the group."""
    group = LocalGroup(W)
    outs, errs = [None] * W, []

    def run(r):
        try:
            outs[r] = fn(r, LocalSync(group, r))
            torch.cuda.synchronize()
        except BaseException as e:      # noqa: BLE001
            errs.append(e)
            group.barrier.abort()
    ts = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    if errs:
        raise errs[0]
    return outs, group


@pytest.fixture(scope="module")
def store():
    return _store()


@pytest.mark.parametrize("batch,W", [(8, 2), (8, 4), (16, 4)])
def test_grading_replicas_equal_the_single_process_pass_of_rank_0(store, batch, W):
    import multimodal_learning_amd as m
    opt = _opt(batch)
    ld = _loader(store, opt)
    assert ld.n_rows == 45 and len(ld) == -(-45 // batch)
    s0, t0 = _nets(opt)
    single_p = m.evaluate.test_patches(opt, t0, s0, ld, "cuda", agg="median")
    single_t = m.evaluate.test_teacher_patches(opt, t0, ld, "cuda", agg=("quantile", 0.009))
    # negative control: a perturbed copy alone computes other rows
    sp, tp = _nets(opt, 0.05)
    alone = m.evaluate.test_patches(opt, tp, sp, ld, "cuda", agg="median")
    assert not np.array_equal(alone[0][6][6], single_p[0][6][6]) and not np.array_equal(alone[0][6][5], single_p[0][6][5])
    nets = [(s0, t0)] + [_nets(opt, 0.05 * r) for r in range(1, W)]
    ref_buffers = [[b.clone() for b in net.buffers()] for net in (s0, t0)]
    counts = {}

    def fn(r, sync):
        s, t = nets[r]
        a = m.evaluate.test_patches(opt, t, s, ld, "cuda", agg="median", sync=sync)
        counts[(r, 0)] = (sync.g.gathers[r], sync.g.broadcasts[r])
        b = m.evaluate.test_teacher_patches(opt, t, ld, "cuda", agg=("quantile", 0.009), sync=sync)
        counts[(r, 1)] = (sync.g.gathers[r], sync.g.broadcasts[r])
        return a, b
    outs, group = _run_replicas(W, fn)
    for r in range(W):
        assert_same(outs[r][0], single_p, "rank%d.test_patches" % r)
        assert_same(outs[r][1], single_t, "rank%d.test_teacher_patches" % r)
        assert counts[(r, 0)] == (1, 1) and counts[(r, 1)] == (2, 2), (r, counts)       # one gather per pass
        for net, ref in zip(nets[r], ref_buffers):
            for b, want in zip(net.buffers(), ref):
                assert torch.equal(b, want), r


def test_survival_replicas_equal_the_single_process_pass_of_rank_0(store):
    import multimodal_learning_amd as m
    W = 2
    opt = _opt(8, task="surv", act_type="Sigmoid", label_dim=1)
    ld = _loader(store, opt, surv=True)
    _, t0 = _nets(opt)
    single = m.evaluate.test_teacher_patches(opt, t0, ld, "cuda", agg="median")
    alone = m.evaluate.test_teacher_patches(opt, _nets(opt, 0.05)[1], ld, "cuda", agg="median")
    assert not np.array_equal(alone[0][13][0], single[0][13][0])
    nets = [t0, _nets(opt, 0.05)[1]]
    outs, group = _run_replicas(W, lambda r, sync: m.evaluate.test_teacher_patches(opt, nets[r], ld, "cuda", agg="median", sync=sync))
    for r in range(W):
        assert_same(outs[r], single, "rank%d" % r)
    assert group.gathers == [1, 1]
    for b, want in zip(nets[1].buffers(), t0.buffers()):
        assert torch.equal(b, want)


# ------------------------------------------------------------------------------------------------ one RCCL rank
def _rank_child(store_path, out_path):
    """Run in a child process: one RCCL rank (world size 1, FileStore rendezvous); both passes with a dist.ReplicaSync
    against sync=None, compared here; writes "ok" when every entry is equal."""
    import torch.distributed as dist
    import multimodal_learning_amd as m
    from multimodal_learning_amd.dist import ReplicaSync
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", store=dist.FileStore(store_path, 1), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        store = _store()
        opt = _opt(8)
        ld = _loader(store, opt)
        s0, t0 = _nets(opt)
        sync = ReplicaSync()
        assert sync.world_size == 1 and sync.rank == 0
        before = [b.clone() for b in t0.buffers()]
        assert_same(m.evaluate.test_patches(opt, t0, s0, ld, "cuda", agg="median", sync=sync),
                    m.evaluate.test_patches(opt, t0, s0, ld, "cuda", agg="median"), "test_patches")
        assert_same(m.evaluate.test_teacher_patches(opt, t0, ld, "cuda", sync=sync),
                    m.evaluate.test_teacher_patches(opt, t0, ld, "cuda"), "test_teacher_patches")
        sopt = _opt(8, task="surv", act_type="Sigmoid", label_dim=1)
        sld = _loader(store, sopt, surv=True)
        _, st = _nets(sopt)
        assert_same(m.evaluate.test_teacher_patches(sopt, st, sld, "cuda", sync=sync),
                    m.evaluate.test_teacher_patches(sopt, st, sld, "cuda"), "test_teacher_patches(surv)")
        assert all(torch.equal(a, b) for a, b in zip(before, t0.buffers()))
        torch.cuda.synchronize()
        with open(out_path, "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


def test_one_rccl_rank_equals_no_sync(tmp_path):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_eval_dist as T; T._rank_child(%r, %r)"
            % (ROOT, HERE, str(tmp_path / "store"), str(tmp_path / "res.txt")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert open(str(tmp_path / "res.txt")).read() == "ok"

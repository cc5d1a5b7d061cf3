"""CPU side of the data-parallel survival teacher: the persistent rank-ordered all-gather of
dist.ReplicaSync under gloo, the argument checks of the two survival entry points for the gathered batch (they return
before any HIP call, so they run without a GPU) and the construction-time checks of TeacherStage1Step under a sync."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

EINVAL = -22


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, fn, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = fn(rank, world)
    finally:
        dist.destroy_process_group()


def _run(fn, world=2):
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, fn, ret)) for r in range(world)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(120)
        assert p.exitcode == 0, "worker failed"
    return [ret[r] for r in range(world)]


def _gather_twice(rank, world):
    from multimodal_learning_amd.dist import ReplicaSync
    sync = ReplicaSync()
    out = torch.full((world, 8, 5), -1.0)
    ptr0 = out.data_ptr()
    res = []
    for call in range(2):
        inp = torch.arange(40, dtype=torch.float32).reshape(8, 5) + 1000.0 * rank + 100.0 * call
        got = sync.all_gather_into(out, inp)
        assert got is out
        res.append(out.clone())
    bad = None
    try:
        sync.all_gather_into(torch.empty(world + 1, 8, 5), torch.zeros(8, 5))
    except ValueError as e:
        bad = str(e)
    return res, ptr0 == out.data_ptr(), bad


def test_all_gather_into_is_rank_ordered_into_one_persistent_buffer():
    world = 2
    for res, same_ptr, bad in _run(_gather_twice, world):
        assert same_ptr
        assert bad is not None and "all_gather_into" in bad
        for call in range(2):
            for r in range(world):
                want = torch.arange(40, dtype=torch.float32).reshape(8, 5) + 1000.0 * r + 100.0 * call
                assert torch.equal(res[call][r], want), (call, r)


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_surv_pack_rows_rejects_bad_arguments_before_any_hip_call():
    L = _lib()
    buf = (C.c_float * 16)()
    d = C.cast(buf, C.c_void_p)          # a dummy non-NULL host pointer: only rejected calls are made with it

    def pack(p=d, pp=d, po=d, q=d, qp=d, qo=d, t=d, c=d, n=4, nt=1, rows=d):
        return L.ph_surv_pack_rows(p, pp, po, q, qp, qo, t, c, n, nt, rows, None)
    assert pack(n=0) == EINVAL
    assert pack(n=-3) == EINVAL
    assert pack(n=4097) == EINVAL
    assert pack(nt=-1) == EINVAL
    assert pack(nt=4) == EINVAL
    for k in ("p", "pp", "po", "t", "c", "rows"):
        assert pack(**{k: None}) == EINVAL, k
    for k in ("q", "qp", "qo"):          # the teacher rows are required when num_teachers > 0
        assert pack(**{k: None}) == EINVAL, k


def test_surv_gathered_loss_rejects_bad_arguments_before_any_hip_call():
    L = _lib()
    buf = (C.c_float * 16)()
    d = C.cast(buf, C.c_void_p)

    def gathered(rows=d, world=2, n=4, rank=0, nt=1, terms=d, dgrad=d):
        return L.ph_surv_stage1_loss_grad_gathered(rows, world, n, rank, nt, 1.0, 1.0, terms, dgrad, None)
    assert gathered(world=2, n=2049) == EINVAL          # global batch 4098 > 4096
    assert gathered(world=1, n=4097) == EINVAL
    assert gathered(world=8, n=513) == EINVAL
    assert gathered(world=65536, n=65536) == EINVAL      # the product overflows a 32-bit int
    assert gathered(world=2, rank=2) == EINVAL
    assert gathered(world=2, rank=-1) == EINVAL
    assert gathered(world=0, rank=0) == EINVAL
    assert gathered(n=0) == EINVAL
    assert gathered(nt=-1) == EINVAL
    assert gathered(nt=4) == EINVAL
    assert gathered(rows=None) == EINVAL
    assert gathered(terms=None) == EINVAL
    assert gathered(rows=None, dgrad=None) == EINVAL


def _surv_opt(**kw):
    import multimodal_learning_amd as m
    base = dict(task="surv", act_type="Sigmoid", label_dim=1, dropout_rate=0.0, batch_size=8, cut_fuse_grad=False,
                num_teachers=2, reg_type="none")
    base.update(kw)
    opt = m.stage2_opt(**base)
    opt.pred_distill = 1
    return opt


def test_surv_step_under_sync_checks_at_construction():
    """Both checks come before any model is built or any other use of the sync object (they run on the CPU)."""
    import multimodal_learning_amd as m

    class _Bare:
        world_size, rank = 2, 0

    class _Gathering(_Bare):
        def all_gather_into(self, out, inp):
            raise AssertionError("not called at construction")

        def attach_parts(self, *a):
            raise AssertionError("not reached")
    with pytest.raises(NotImplementedError, match="all_gather_into"):
        m.TeacherStage1Step(_surv_opt(), device="cpu", sync=_Bare())
    with pytest.raises(ValueError, match="4096"):
        m.TeacherStage1Step(_surv_opt(batch_size=2049), device="cpu", sync=_Gathering())
    # the other survival combinations still raise with a capable sync object
    for bad in (dict(tSVD_loss="True", n_views=2, tSVD_mode="path", mu=1.0), dict(masking=1)):
        opt = _surv_opt()
        for k, v in bad.items():
            setattr(opt, k, v)
        with pytest.raises(NotImplementedError):
            m.TeacherStage1Step(opt, device="cpu", sync=_Gathering())

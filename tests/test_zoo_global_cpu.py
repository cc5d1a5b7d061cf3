"""CPU side of the relational distillation losses over the global batch: the argument checks of
ph_rkd_loss_grad_part (they return before any HIP call, so they run without a GPU), its workspace size, and - under gloo
with two processes - the two autograd forms the data-parallel criteria use: the row all-gather with the local backward
(pkt, similarity) and the anchor-partitioned RKD wrapper, whose kernel call is replaced here by `rkd_part_torch`, the
torch statement of the kernel's contract (tests/zoo_emulation.py)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.zoo_emulation import rkd_part_torch      # the contract of a part, stated once

EINVAL = -22


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_rkd_part_rejects_bad_arguments_before_any_hip_call():
    L = _lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)          # a dummy non-NULL host pointer: only rejected calls are made with it

    def call(f_s=p, f_t=p, Bg=8, D=16, lo=0, na=8, loss=p, dx=p, ws=p):
        return L.ph_rkd_loss_grad_part(f_s, f_t, Bg, D, lo, na, 25.0, 50.0, loss, dx, ws, None)
    for kw in (dict(f_s=None), dict(f_t=None), dict(loss=None), dict(dx=None), dict(ws=None),
               dict(Bg=1, na=1), dict(Bg=0, na=1), dict(Bg=1025, na=1025), dict(Bg=1025, na=1), dict(D=0), dict(D=513),
               dict(D=-4), dict(lo=-1), dict(lo=-1, na=9), dict(na=0), dict(na=-3), dict(lo=1, na=8), dict(lo=8, na=1),
               dict(lo=7, na=2), dict(na=9), dict(lo=2 ** 31 - 1, na=2 ** 31 - 1)):
        assert call(**kw) == EINVAL, kw


def test_rkd_part_workspace_is_monotone():
    L = _lib()
    w = L.ph_rkd_part_workspace_bytes
    assert w(2, 1, 1) > 0
    # room for the two Bg x Bg norm matrices and a slab of dv rows at least
    assert w(512, 128, 64) >= 4 * (2 * 512 * 512 + 64 * 512 * 128)
    for Bg in (2, 15, 64, 192, 512, 1024):
        for D in (1, 32, 128, 512):
            prev = 0
            for na in sorted({1, 2, min(Bg, 63), min(Bg, 64), min(Bg, 65), Bg}):
                cur = w(Bg, D, na)
                assert cur >= prev > -1, (Bg, D, na)
                prev = cur
            assert w(Bg + 1, D, 1) >= w(Bg, D, 1) and w(Bg, D + 1, 1) >= w(Bg, D, 1)
    assert w(1024, 512, 1024) < 1 << 29            # the largest problem stays below half a GiB


def test_rkd_part_restatement_adds_up_to_the_reference(golden_dir):
    """`rkd_part_torch` over a three-way partition of the 192-row reference golden: the parts add up to RKD.py's loss and
    gradient (this pins the restatement the gloo test below and the GPU tests' partition property rest on)."""
    g = np.load(os.path.join(golden_dir, "zoo_global_b192_d128.npz"))
    f_s, f_t = torch.as_tensor(g["f_s"]).float(), torch.as_tensor(g["f_t"]).float()
    loss, dx = 0.0, torch.zeros_like(f_s)
    for r in range(3):
        l, d = rkd_part_torch(f_s, f_t, 64 * r, 64, 25.0, 50.0)
        loss, dx = loss + float(l), dx + d
    ref_l, ref_g = float(g["rkd"]), torch.as_tensor(g["rkd_g"])
    assert abs(loss - ref_l) <= 1e-7 + 1e-4 * abs(ref_l), (loss, ref_l)
    assert float((dx - ref_g).abs().max()) <= 1e-8 + 2e-3 * float(ref_g.abs().max())


# ------------------------------------------------------------------------------------------------ gloo, two processes
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
        p.join(180)
        assert p.exitcode == 0, "worker failed"
    return [ret[r] for r in range(world)]


N, D = 5, 12


def _rows(world):
    g = torch.Generator().manual_seed(41)
    return (torch.randn(world * N, D, generator=g).relu_(), torch.randn(world * N, D, generator=g).relu_(),
            torch.randn(world * N, D, generator=g))


def _gather_rows(rank, world):
    from multimodal_learning_amd.dist import ReplicaSync
    from multimodal_learning_amd.train_step import _GatherRowsFn
    sync = ReplicaSync()
    f_s, _, wt = _rows(world)
    x = f_s[rank * N:(rank + 1) * N].clone().requires_grad_(True)
    y = _GatherRowsFn.apply(x, sync)
    (y * wt).sum().backward()
    return y.detach(), x.grad


def test_gathered_rows_come_rank_ordered_and_the_backward_keeps_the_local_rows():
    world = 2
    f_s, _, wt = _rows(world)
    for r, (y, gx) in enumerate(_run(_gather_rows, world)):
        assert torch.equal(y, f_s)
        assert torch.equal(gx, wt[r * N:(r + 1) * N])


def _rkd_wrapped(rank, world):
    import multimodal_learning_amd.distiller_zoo as Z
    from multimodal_learning_amd.dist import ReplicaSync
    sync = ReplicaSync()
    Z.rkd_part = rkd_part_torch                   # the kernel call, replaced by the restatement of its contract
    f_s, f_t, _ = _rows(world)
    x = f_s[rank * N:(rank + 1) * N].clone().requires_grad_(True)
    loss = Z.RKDLoss(sync=sync)(x, f_t[rank * N:(rank + 1) * N])
    (3.0 * loss).backward()
    return loss.detach(), x.grad


def test_partitioned_rkd_wrapper_sums_to_the_one_process_gradient():
    world = 2
    f_s, f_t, _ = _rows(world)
    ref_l, ref_g = rkd_part_torch(f_s, f_t, 0, world * N, 25.0, 50.0)
    res = _run(_rkd_wrapped, world)
    tot = sum(float(l) for l, _ in res)
    assert abs(tot - float(ref_l)) <= 1e-5 * abs(float(ref_l)), (tot, float(ref_l))
    # each replica's part is a part, not the whole (the parts differ from the total)
    assert all(abs(float(l) - float(ref_l)) > 1e-3 * abs(float(ref_l)) for l, _ in res)
    got = torch.cat([g for _, g in res], 0)
    assert float((got - 3.0 * ref_g).abs().max()) <= 1e-5 * float(ref_g.abs().max()) * 3.0

"""The relational distillation losses (rkd, pkt, similarity) over the global batch:
  * ph_rkd_loss_grad_part - the anchor-partitioned, tiled RKD kernels of csrc/zoo_rkd.hip - against the reference's own
    RKD.py at 192, 256 and 512 rows (tests/golden/make_golden_zoo_global.py), its partition property, its determinism,
    its agreement with the one-workgroup-per-anchor kernels at 128 rows, coinciding rows across a range boundary;
  * PKT and Similarity at those row counts through the existing entries;
  * DistillStep(variant="mia2022", --distill rkd | pkt | similarity) under data parallelism: two emulated replicas
    against one process on the whole batch, and one real RCCL rank in a child process."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = ((192, 128), (256, 64), (512, 128))
W_D, W_A = 25.0, 50.0
# tests/test_gpu_losses.py (RKD / PKT / SP against the reference golden): loss (atol, rtol), gradient (atol, rtol), max-norm
RKD_TOL = ((1e-7, 1e-4), (1e-8, 2e-3))


def _golden(golden_dir, Bg, D):
    g = np.load(os.path.join(golden_dir, "zoo_global_b%d_d%d.npz" % (Bg, D)))
    return g, torch.as_tensor(g["f_s"]).float().cuda(), torch.as_tensor(g["f_t"]).float().cuda()


def _part(f_s, f_t, lo, n):
    from multimodal_learning_amd.distiller_zoo import rkd_part
    loss, dx = rkd_part(f_s.contiguous(), f_t.contiguous(), lo, n, W_D, W_A)
    return loss.clone(), dx.clone()


def _sum_parts(f_s, f_t, ranges):
    loss, dx = None, None
    for lo, n in ranges:                          # rank order
        l, d = _part(f_s, f_t, lo, n)
        loss, dx = (l, d) if loss is None else (loss + l, dx + d)
    return loss, dx


def test_rkd_pkt_sp_above_128_rows_vs_reference_golden(golden_dir):
    """Full anchor range (what RKDLoss runs on one GPU above 128 rows) against RKD.py; PKT and Similarity at the same
    row counts through their existing entries.  The gradient atols of PKT (1e-10, pinned at 128 rows) and SP (1e-9,
    pinned at 64 rows) shrink with the gradients, which scale as 1 / B^2."""
    from multimodal_learning_amd.distiller_zoo import RKDLoss, PKT, Similarity
    from tests.gpu_util import Report
    R = Report("RKD / PKT / SP above 128 rows vs REFERENCE golden")
    for Bg, D in SHAPES:
        g, f_s, f_t = _golden(golden_dir, Bg, D)
        f_s.requires_grad_(True)
        l = RKDLoss()(f_s, f_t)
        gr, = torch.autograd.grad(3.0 * l, f_s)
        R.close(np.asarray(g["rkd"]).reshape(()), l.reshape(()), *RKD_TOL[0], f"RKD loss Bg={Bg} D={D}")
        R.close(3.0 * g["rkd_g"], gr, *RKD_TOL[1], f"RKD grad Bg={Bg} D={D}")
        l = PKT()(f_s, f_t)
        gr, = torch.autograd.grad(l, f_s)
        R.close(np.asarray(g["pkt"]).reshape(()), l.reshape(()), 1e-9, 2e-3, f"PKT loss Bg={Bg}")
        R.close(g["pkt_g"], gr, 1e-10 * (128.0 / Bg) ** 2, 5e-3, f"PKT grad Bg={Bg}")
        l = Similarity()(f_s, f_t)
        gr, = torch.autograd.grad(l.sum(), f_s)
        R.close(np.asarray(g["sp"]).reshape(()), l.reshape(()), 1e-8, 1e-4, f"SP loss Bg={Bg}")
        R.close(g["sp_g"], gr, 1e-9 * (64.0 / Bg) ** 2, 2e-3, f"SP grad Bg={Bg}")
    R.finish()


def test_rkd_parts_add_up_and_repeat_bitwise(golden_dir):
    """Any partition of [0, Bg) into contiguous anchor ranges: the parts, summed in rank order, equal the full-range call
    (loss and gradient, the golden tolerances); two identical calls give the same bits."""
    from tests.gpu_util import Report
    R = Report("RKD parts vs the full anchor range")
    g = torch.Generator().manual_seed(3)
    ragged = (torch.randn(15, 40, generator=g).relu_().cuda(), torch.randn(15, 40, generator=g).relu_().cuda())
    cases = [((512, 128), [[(r * (512 // w), 512 // w) for r in range(w)] for w in (1, 2, 8)]),
             ((192, 128), [[(0, 64), (64, 64), (128, 64)]]),
             (None, [[(0, 7), (7, 8)]])]
    for shape, partitions in cases:
        if shape is None:
            f_s, f_t = ragged
        else:
            _, f_s, f_t = _golden(golden_dir, *shape)
        full_l, full_g = _part(f_s, f_t, 0, f_s.shape[0])
        again_l, again_g = _part(f_s, f_t, 0, f_s.shape[0])
        assert torch.equal(full_l, again_l) and torch.equal(full_g, again_g), "two identical calls differ"
        for ranges in partitions:
            l, d = _sum_parts(f_s, f_t, ranges)
            tag = "Bg=%d x %d" % (f_s.shape[0], len(ranges))
            R.close(full_l, l, *RKD_TOL[0], "loss " + tag)
            R.close(full_g, d, *RKD_TOL[1], "grad " + tag)
        lo, n = partitions[-1][-1]
        a, b = _part(f_s, f_t, lo, n), _part(f_s, f_t, lo, n)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two identical part calls differ"
    R.finish()


def test_rkd_part_at_128_rows_matches_the_golden_and_the_one_workgroup_kernels(golden_dir):
    """B = 128 (`rkd128` of zoo_sp_featskl.npz): the tiled kernels over the full range meet the tolerances the
    one-workgroup-per-anchor kernels are held to, and agree with those kernels' output within them."""
    from multimodal_learning_amd.distiller_zoo import RKDLoss
    from tests.gpu_util import Report
    g = np.load(os.path.join(golden_dir, "zoo_sp_featskl.npz"))
    R = Report("RKD, tiled kernels at B = 128")
    f_s = torch.as_tensor(g["r_f_s128"]).cuda().requires_grad_(True)
    f_t = torch.as_tensor(g["r_f_t128"]).cuda()
    old_l = RKDLoss(W_D, W_A)(f_s, f_t)
    old_g, = torch.autograd.grad(old_l, f_s)
    new_l, new_g = _part(f_s.detach(), f_t, 0, 128)
    R.close(np.asarray(g["rkd128"]).reshape(()), new_l.reshape(()), *RKD_TOL[0], "tiled loss vs golden")
    R.close(g["rkd_g128"], new_g, *RKD_TOL[1], "tiled grad vs golden")
    R.close(old_l.detach().reshape(()), new_l.reshape(()), *RKD_TOL[0], "tiled loss vs one-workgroup kernels")
    R.close(old_g, new_g, *RKD_TOL[1], "tiled grad vs one-workgroup kernels")
    R.finish()


def test_rkd_parts_with_coinciding_rows_across_a_range_boundary_are_finite():
    """Rows 0 and n equal (zero distance, zero difference vector, on both sides of the boundary between two ranges) and
    one all-zero row: finite loss and gradient from every part, and the parts still add up."""
    g = torch.Generator().manual_seed(9)
    n, D = 24, 48
    f_s, f_t = torch.randn(2 * n, D, generator=g).relu_(), torch.randn(2 * n, D, generator=g).relu_()
    f_s[n], f_t[n] = f_s[0], f_t[0]
    f_s[5] = 0.0
    f_s, f_t = f_s.cuda(), f_t.cuda()
    full_l, full_g = _part(f_s, f_t, 0, 2 * n)
    assert torch.isfinite(full_l).all() and torch.isfinite(full_g).all()
    tot_l, tot_g = 0.0, torch.zeros_like(f_s)
    for lo in (0, n):
        l, d = _part(f_s, f_t, lo, n)
        assert torch.isfinite(l).all() and torch.isfinite(d).all(), lo
        tot_l, tot_g = tot_l + l, tot_g + d
    assert float((tot_l - full_l).abs()) <= RKD_TOL[0][0] + RKD_TOL[0][1] * float(full_l.abs())
    assert float((tot_g - full_g).abs().max()) <= RKD_TOL[1][0] + RKD_TOL[1][1] * float(full_g.abs().max())
    # student rows that coincide while the teacher's do not: still finite (no gradient through a zero vector)
    f_t2 = f_t.clone(); f_t2[n] = f_t2[1]
    l, d = _part(f_s, f_t2, n, n)
    assert torch.isfinite(l).all() and torch.isfinite(d).all()


# ------------------------------------------------------------------------------------------------ two replicas
class LocalGroup:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world


class LocalSync:
    """tests/test_gpu_replicas.py's in-process stand-in of dist.ReplicaSync, with all_gather_into."""

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

    def begin_grad_slice(self, flat, lo):
        g = flat if torch.is_tensor(flat) else flat.grad
        self.pending = (lo, g[lo:].clone())

    def all_reduce_grads(self, flat):
        g = flat if torch.is_tensor(flat) else flat.grad
        pend, self.pending = getattr(self, "pending", None), None
        if pend is None:
            return self._sum(g)
        lo, snap = pend
        assert torch.equal(snap, g[lo:]), "gradients behind the announced offset changed after the announcement"
        self._sum(g[lo:])
        return self._sum(g[:lo])

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
        out.copy_(torch.stack(self._exchange(inp.clone()), 0))
        return out

    def attach(self, step):
        for crd in (step.criterion_kd, step.criterion_kd_path):
            crd.contrast.sync = self

    def attach_parts(self, crds, flats, modules):
        for crd in crds:
            crd.contrast.sync = self


def _build(distill, sync, B, n_data, **over):
    """tests/test_gpu_replicas.py's `_build` for variant "mia2022" with a feature-level baseline criterion."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import default_opt
    opt = default_opt(nce_k=512, grads_m=0.9, grads_thresh="False", thresh=0.1, batch_size=B, distill=distill,
                      num_teachers=2, which_teacher="fuse", assign_weights="False", alpha=1.0, beta=0.5,
                      **over)
    step = m.DistillStep(opt, n_data, device="cuda", sync=sync, variant="mia2022")
    step.model.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
    step.ema_model.load_state_dict(W.make_state_dict(W.student_shapes(), 2))
    step.fix_model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
    return step, opt


def _batch(B, H, n_data, seed=900):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, H, n_data=n_data, P=1, K=512, seed=seed)
    h = B // 2
    for k in ("x_path", "ema_x_path", "x_omic"):
        bt[k][h:] = bt[k][:h]              # per-shard BatchNorm statistics == whole-batch statistics
    z = torch.zeros(B)
    return ((bt["x_path"], bt["ema_x_path"]), z, bt["x_omic"], z, z, bt["grade"], bt["index"], bt["sample_idx"])


# gradients that are plain sums over the batch rows of quantities downstream of the student feature: the grading head and
# the affine parameters of the BatchNorm1d that produces the feature (through which the feature criterion's gradient flows)
HEAD = ("fc_new2.weight", "fc_new2.bias", "fc_new1.1.weight", "fc_new1.1.bias")


def _head_grads(step):
    ps = dict(step.model.named_parameters())
    return {name: ps[name].grad.detach().clone() for name in HEAD}


LOSS_KEYS = ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2")


def _loss_ok(tot, ref):
    return abs(tot - ref) <= 2e-4 * max(abs(ref), 1e-2)


@pytest.mark.parametrize("distill", ["rkd", "pkt", "similarity"])
def test_two_replicas_equal_one_process_on_the_global_batch(distill):
    """Two replicas of 4 rows against one process on the 8 rows.  The second half of the batch repeats the first (so
    that per-shard BatchNorm statistics equal the whole batch's): feature rows r and r + 4 coincide, on both sides of
    the rank boundary.  Negative control: the criterion evaluated per shard - summed or averaged over the shards, the two
    natural per-replica forms - misses the same bounds in loss and in the gradient with respect to the feature."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import distiller_zoo as Z
    from multimodal_learning_amd.dist import shard_batch
    B, H, n_data = 8, 64, 1024
    m.set_precision("bf16x6")
    try:
        batch = _batch(B, H, n_data)
        single, opt = _build(distill, None, B, n_data)
        o1 = single.step(batch, epoch=3)
        torch.cuda.synchronize()
        g1 = _head_grads(single)
        group = LocalGroup(2)
        reps = [_build(distill, LocalSync(group, r), B // 2, n_data)[0] for r in range(2)]
        outs, errs = [None, None], []

        def run(r):
            try:
                torch.cuda.set_device(0)
                outs[r] = reps[r].step(shard_batch(batch, r, 2), epoch=3)
                torch.cuda.synchronize()
            except BaseException as e:      # noqa: BLE001 - re-raised in the main thread
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
        assert torch.equal(reps[0].ema_flat.flat, reps[1].ema_flat.flat)
        assert torch.isfinite(f0.grad).all()
        for k in LOSS_KEYS:
            tot, ref = sum(float(o[k]) for o in outs), float(o1[k])
            print("%s %-10s replicas %.9g  one process %.9g" % (distill, k, tot, ref))
            assert _loss_ok(tot, ref), (k, tot, ref)
        assert float(o1["loss_kd1"]) > 0.0
        g2 = _head_grads(reps[0])
        gmax = max(float(v.abs().max()) for v in g1.values())
        for k, v in g1.items():
            err = float((g2[k] - v).abs().max())
            print("%s grad %-18s err %.3e  max|ref| %.3e" % (distill, k, err, float(v.abs().max())))
            assert err <= 1e-3 * float(v.abs().max()) + 1e-6 * gmax, (k, err, float(v.abs().max()))
        # ---- negative control on the step's own features
        crit = {"rkd": Z.RKDLoss, "pkt": Z.PKT, "similarity": Z.Similarity}[distill]()
        f_s = o1["path_feat"].detach().clone().requires_grad_(True)
        f_t = o1["fuse_feat"].detach()
        glob = crit(f_s, f_t).reshape(())
        g_glob, = torch.autograd.grad(glob, f_s)
        assert _loss_ok(opt.beta * float(glob.detach()), float(o1["loss_kd1"]))
        h = B // 2
        shard = [crit(f_s[r * h:(r + 1) * h], f_t[r * h:(r + 1) * h]).reshape(()) for r in range(2)]
        g_shard, = torch.autograd.grad(shard[0] + shard[1], f_s)
        for wgt in (1.0, 0.5):
            per = wgt * float(shard[0] + shard[1])
            gerr = float((wgt * g_shard - g_glob).abs().max())
            print("%s per-shard x %.1f: loss %.6g vs global %.6g, grad err %.3e of %.3e"
                  % (distill, wgt, per, float(glob), gerr, float(g_glob.abs().max())))
            assert not _loss_ok(opt.beta * per, opt.beta * float(glob)), (wgt, per, float(glob))
            assert gerr > 1e-3 * float(g_glob.abs().max()), (wgt, gerr)
    finally:
        m.set_precision("bf16")


def test_rkd_global_batch_above_1024_rows_is_refused_at_construction():
    import multimodal_learning_amd as m
    from oracle.step import default_opt

    class _Sync:
        rank = 0

        def __init__(self, world):
            self.world_size = world

        def all_gather_cat(self, t):
            return t

        def all_reduce_sum(self, t):
            return t

    for bs, world in ((205, 5), (129, 8), (1025, 1)):
        opt = default_opt(nce_k=64, batch_size=bs, distill="rkd", num_teachers=2, assign_weights="False")
        with pytest.raises(ValueError, match="1024"):
            m.DistillStep(opt, 256, device="cuda", sync=_Sync(world), variant="mia2022")

    class _NoReduce:
        rank, world_size = 0, 2

        def all_gather_cat(self, t):
            return t

    opt = default_opt(nce_k=64, batch_size=4, distill="rkd", num_teachers=2, assign_weights="False")
    with pytest.raises(NotImplementedError, match="all_reduce_sum"):
        m.DistillStep(opt, 256, device="cuda", sync=_NoReduce(), variant="mia2022")


# ------------------------------------------------------------------------------------------------ one RCCL rank
def _rank_child(store_path, out_path):
    """Run in a child process: one RCCL rank (world size 1, FileStore rendezvous).  A `--distill rkd` step with a
    ReplicaSync next to a sync=None twin (same weights, same batches): three eager steps each, then the sync step
    replays its captured graph for three more while the twin stays eager.

    Batch 136: above 128 rows the twin without sync runs the tiled kernels over the full anchor range too, so the two
    sides differ ONLY in what this test is about - the all-gather, the all-reduce of the gradient parts, the row slicing of
    the wrapper, the capture.  At B <= 128 the twin runs the one-workgroup kernels, whose fp32 rounding differs from the
    tiled kernels' by ~2e-7 relative (within tolerance in test_rkd_part_at_128_rows_... and, at step level, in the
    two-replica test above), and Adam's first steps from zero moments amplify such a difference 50-fold per step
    (measured at B = 8: loss_kd1 2e-7 apart at step 0, loss_cls 1.3e-5 at step 1, loss_div1 7.8e-4 at step 2), which would
    measure the optimiser's sensitivity, not the sync path.  The first step at B = 8 (kernel against kernel under the real
    collectives, before any update) is compared as well."""
    import warnings
    import torch.distributed as dist
    import multimodal_learning_amd as m
    from multimodal_learning_amd.dist import ReplicaSync
    torch.cuda.set_device(0)
    # collectives inside captured graphs: the watchdog's asynchronous error handling must not touch the streams (as bench.py)
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
    dist.init_process_group("nccl", store=dist.FileStore(store_path, 1), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        H, n_data = 64, 1024
        m.set_precision("bf16x6")
        res = {}
        for mode in ("plain", "sync"):
            small, _ = _build("rkd", ReplicaSync() if mode == "sync" else None, 8, n_data)
            out = small.step(_batch(8, H, n_data), epoch=3)
            res[mode + "_b8"] = {k: out[k].detach().cpu().clone() for k in LOSS_KEYS}
            del small
            B = 136
            step, _ = _build("rkd", ReplicaSync() if mode == "sync" else None, B, n_data)
            steps = []
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for it in range(6):
                    if it == 3 and mode == "sync":
                        step.enable_graph()
                    out = step.step(_batch(B, H, n_data, seed=900 + it), epoch=3)
                    steps.append({k: out[k].detach().cpu().clone() for k in LOSS_KEYS})
                torch.cuda.synchronize()
            res[mode] = steps
            if mode == "sync":
                res["warnings"] = [str(w.message) for w in caught]
                res["want_graph"] = bool(getattr(step, "_want_graph", False))
        torch.save(res, out_path)
    finally:
        dist.destroy_process_group()


def test_rkd_step_with_one_rccl_rank_equals_the_step_without_sync(tmp_path):
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_zoo_global as T; T._rank_child(%r, %r)"
            % (ROOT, HERE, str(tmp_path / "store"), str(tmp_path / "res.pt")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    res = torch.load(str(tmp_path / "res.pt"))
    assert not [w for w in res["warnings"] if "capture" in w], res["warnings"]
    assert res["want_graph"], "the rkd step under a sync fell back to eager launches"
    for k in LOSS_KEYS:
        a, b = float(res["sync_b8"][k]), float(res["plain_b8"][k])
        print("B = 8 step 0 %-10s sync %.9g  plain %.9g" % (k, a, b))
        assert np.isfinite(a) and _loss_ok(a, b), (k, a, b)
    for it in range(6):                 # steps 0-2 eager on both sides, 3-5 replayed under the sync
        for k in LOSS_KEYS:
            a, b = float(res["sync"][it][k]), float(res["plain"][it][k])
            print("step %d %-10s sync %.9g  plain %.9g" % (it, k, a, b))
            assert np.isfinite(a), (it, k)
            assert _loss_ok(a, b), (it, k, a, b)
        assert float(res["plain"][it]["loss_kd1"]) > 0.0

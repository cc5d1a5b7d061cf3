"""Cost of the order-statistic aggregation and of the sharded test pass (not a test):
python tests/bench_eval_dist_gpu.py

  1. ph_group_quantile by device events at 4500 rows / 250 patients / C = 3 (the wave form) and at one group of 4096 rows
     (the workgroup form), next to ph_group_agg(max) at the same sizes in the same process.
  2. The 576-row pass of section 23 (64 ROIs of 1024 x 1024, S = 512, batches of 64, student + teacher, bf16) with
     sync=None against a world-size-1 dist.ReplicaSync in the same process: the cost of the broadcast and the gather.
  3. Where the box has more than one GPU: the same pass at W = 2 / 4 / 8 against W = 1, one fresh child process per GPU
     (at most 8).  The expectation to compare against: the forward part divided by W, plus one gather."""
import contextlib
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimodal_learning_amd as m  # noqa: E402

N_ROI, SH, S, B, REPS = 64, 1024, 512, 64, 5


def build_pass(device):
    m.set_precision("bf16")
    torch.manual_seed(0)
    opt = m.stage2_opt(dropout_rate=0.25, batch_size=B, input_size_path=S)
    g = torch.Generator().manual_seed(0)
    tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8).to(device)
    grade = torch.arange(N_ROI) // 2 % 3
    patient = ["p%02d" % (i // 2) for i in range(N_ROI)]
    loader = m.augment.ResidentPatchLoader(opt, tiles, torch.randn(N_ROI, 320, generator=g), grade, patient=patient, device=device)
    student = m.define_net(opt, 1, path_only=True).to(device)
    teacher = m.define_net(opt, 1).to(device)
    return opt, loader, student, teacher


def timed_pass(opt, loader, student, teacher, device, sync, reps=REPS):
    def one():
        with contextlib.redirect_stdout(io.StringIO()):
            return m.evaluate.test_patches(opt, teacher, student, loader, device, sync=sync)
    one(); one()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, n):
    fn(); fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n


def kernels():
    rs = torch.Generator().manual_seed(1)
    for N, ids, what in ((4500, np.repeat(np.arange(250), 18), "250 patients of 18 rows (wave form)"),
                         (4096, np.zeros(4096, dtype=np.int64), "one group of 4096 rows (workgroup form)")):
        pred = torch.log_softmax(torch.randn(N, 3, generator=rs) * 2, 1).cuda()
        G = int(ids.max()) + 1
        off, order = m.ops.group_csr(ids, G)
        do, dr = torch.from_numpy(off).cuda(), torch.from_numpy(order).cuda()
        n = 20
        a = event_ms(lambda: m.ops.group_agg(pred, do, dr, off, "max"), n)
        print(f"N={N} C=3, {what}: ph_group_agg max {a:.4f} ms per call", end="")
        for q in (0.5, 0.009):
            t = event_ms(lambda: m.ops.group_quantile(pred, do, dr, off, q), n)
            print(f" | ph_group_quantile q={q} {t:.4f} ms", end="")
        print(f"  (device events, {n} calls each, allocation of the output included)")


def child(rank, world, store_path, out_path):
    import torch.distributed as dist
    from multimodal_learning_amd.dist import ReplicaSync
    dev = "cuda:%d" % rank
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", store=dist.FileStore(store_path, world), rank=rank, world_size=world,
                            device_id=torch.device("cuda", rank))
    try:
        opt, loader, student, teacher = build_pass(dev)
        med, lo, hi = timed_pass(opt, loader, student, teacher, dev, ReplicaSync())
        if rank == 0:
            with open(out_path, "w") as f:
                f.write("%.3f %.3f %.3f" % (med, lo, hi))
    finally:
        dist.destroy_process_group()


def main():
    import torch.distributed as dist
    from multimodal_learning_amd.dist import ReplicaSync
    print("device:", torch.cuda.get_device_name(0), "x", torch.cuda.device_count(), "| torch", torch.__version__)
    kernels()
    opt, loader, student, teacher = build_pass("cuda:0")
    base = timed_pass(opt, loader, student, teacher, "cuda:0", None)
    print(f"test_patches, {loader.n_rows} rows in {len(loader)} batches of {B}, sync=None: median {base[0]:.1f} ms "
          f"(min {base[1]:.1f}, max {base[2]:.1f}; {REPS} passes)")
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("nccl", store=dist.FileStore(os.path.join(tmp, "s1"), 1), rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
        try:
            one = timed_pass(opt, loader, student, teacher, "cuda:0", ReplicaSync())
        finally:
            dist.destroy_process_group()
        print(f"the same with a world-size-1 ReplicaSync (two broadcasts, one gather): median {one[0]:.1f} ms "
              f"(min {one[1]:.1f}, max {one[2]:.1f}) - {one[0] - base[0]:+.1f} ms")
        del opt, loader, student, teacher
        torch.cuda.empty_cache()
        ngpu = torch.cuda.device_count()
        if ngpu < 2:
            print("one GPU visible: the W = 2 / 4 / 8 passes are not measured")
            return
        res = {}
        for W in (1, 2, 4, 8):
            if W > ngpu:
                break
            store, out = os.path.join(tmp, "s_w%d" % W), os.path.join(tmp, "o_w%d" % W)
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(r), str(W), store, out],
                                      stdout=subprocess.DEVNULL) for r in range(W)]
            rcs = [p.wait(timeout=900) for p in procs]
            if any(rcs):
                print(f"W={W}: a child failed {rcs}")
                break
            res[W] = [float(v) for v in open(out).read().split()]
            print(f"W={W} (one process per GPU): median {res[W][0]:.1f} ms (min {res[W][1]:.1f}, max {res[W][2]:.1f})"
                  + (f" - {res[1][0] / res[W][0]:.2f}x of W=1" if W > 1 else ""))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
    else:
        main()

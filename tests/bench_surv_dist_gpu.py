"""Cost of the data-parallel survival path (not a test): python tests/bench_surv_dist_gpu.py

1. The stage-1 teacher step under --task surv at B = 64, 512 x 512, bf16, replayed from captured HIP graphs: with a
   world-size-1 ReplicaSync (one RCCL rank, FileStore rendezvous: the survival rows go through ph_surv_pack_rows, one
   all-gather and ph_surv_stage1_loss_grad_gathered; the gradient all-reduce runs as well) against sync=None, the two
   alternating on one device (rounds of R steps each) so that clock / thermal drift hits both alike.
2. The survival loss alone, back to back (device events): pack + gathered kernel against ph_surv_stage1_loss_grad.
Kernel durations: run it under `rocprofv3 --kernel-trace --stats` with PH_SURV_DIST_ROUNDS=1."""
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m
from multimodal_learning_amd._lib import lib, ptr, stream
from bench import make_batch

B, H, R = 64, 512, 10
ROUNDS = int(os.environ.get("PH_SURV_DIST_ROUNDS", "5"))
m.set_precision("bf16")
torch.cuda.set_device(0)
os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")      # collectives inside captured graphs (as bench.py)
store = os.path.join(tempfile.mkdtemp(), "store")
dist.init_process_group("nccl", store=dist.FileStore(store, 1), rank=0, world_size=1, device_id=torch.device("cuda", 0))


def make_step(sync):
    opt = m.stage2_opt(dropout_rate=0.1, batch_size=B, cut_fuse_grad=True, num_teachers=2, task="surv", act_type="Sigmoid",
                       label_dim=1)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 1, 1.0, 0, 0, "False", "False"
    st = m.TeacherStage1Step(opt, device="cuda", sync=sync)
    bt = list(make_batch(B, H, 1024, opt, "cuda", 0))
    g = torch.Generator().manual_seed(7)
    bt[3] = (torch.rand(B, generator=g) > 0.3).float().cuda()              # censor
    bt[4] = torch.randint(1, 100, (B,), generator=g).float().cuda()        # survtime (ties)
    return st, tuple(bt)


try:
    steps = {"sync=None": make_step(None), "ReplicaSync world 1": make_step(m.dist.ReplicaSync())}
    for st, bt in steps.values():
        for _ in range(2):
            st.step(bt)
        st.enable_graph()
        for _ in range(3):
            st.step(bt)
    torch.cuda.synchronize()
    for name, (st, _) in steps.items():
        assert st._want_graph, name + ": the step fell back to eager launches"
    times = {k: [] for k in steps}
    for _ in range(ROUNDS):
        for k, (st, bt) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(R):
                st.step(bt)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / R * 1e3)
    for k, v in times.items():
        print(f"stage-1 surv step, {k}: median {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f}; "
              f"{ROUNDS} rounds x {R} graph-replayed steps, B={B}, {H}x{H}, bf16)")

    # the loss launches alone at the same batch (no collective: the gathered buffer is the packed block at world size 1)
    gen = torch.Generator().manual_seed(3)
    p = [torch.randn(B, generator=gen).cuda() for _ in range(6)]
    t = torch.randint(1, 100, (B,), generator=gen).float().cuda()
    c = (torch.rand(B, generator=gen) > 0.3).float().cuda()
    rows, terms, d = torch.empty(8, B, device="cuda"), torch.empty(9, device="cuda"), torch.empty(3, B, device="cuda")

    def single():
        lib().ph_surv_stage1_loss_grad(*[ptr(x) for x in p], ptr(t), ptr(c), B, 2, 1.0, 1.0, ptr(terms), ptr(d), stream())

    def gathered():
        lib().ph_surv_pack_rows(*[ptr(x) for x in p], ptr(t), ptr(c), B, 2, ptr(rows), stream())
        lib().ph_surv_stage1_loss_grad_gathered(ptr(rows), 1, B, 0, 2, 1.0, 1.0, ptr(terms), ptr(d), stream())
    for name, fn in (("ph_surv_stage1_loss_grad", single), ("ph_surv_pack_rows + ph_surv_stage1_loss_grad_gathered", gathered)):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name}: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call back to back (B={B})")
finally:
    dist.destroy_process_group()

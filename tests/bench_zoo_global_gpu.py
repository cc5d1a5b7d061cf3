"""Cost of the relational distillation losses over the global batch (not a test):
    python tests/bench_zoo_global_gpu.py [--baseline-only]

(a) ph_rkd_loss_grad_part alone, back to back (device events): Bg = 512, D = 128 with 64 anchors (one replica of eight)
    and Bg = 256, D = 128 over the full range (one GPU), as time and as a share of the exact-fp32 matrix peak.  The
    operation count is the angle term's three products per (anchor, j, k) tile pair - A_s = E_j E_k^T, A_t alike,
    dE_j += G E_k - each n_anchors * Bg^2 * D multiply-adds.
(b) the `--distill rkd` step of DistillStep(variant="mia2022") at B = 64, 512 x 512, bf16, replayed from its captured
    HIP graph: with a world-size-1 ReplicaSync (one RCCL rank: all-gather, partitioned kernels, all-reduce of the
    gradient parts, gradient all-reduce) against sync=None, alternating on one device in rounds of R steps.
(c) ph_rkd_loss_grad (the one-workgroup-per-anchor kernels) at B = 64 and 128, D = 128.
--baseline-only runs what a tree without the partitioned kernels can run - (b) without sync and (c) - so that the same
tool measures the parent commit.  Kernel durations: run under `rocprofv3 --kernel-trace --stats` with PH_ZOO_ROUNDS=1."""
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

BASELINE_ONLY = "--baseline-only" in sys.argv
B, H, R = 64, 512, 10
ROUNDS = int(os.environ.get("PH_ZOO_ROUNDS", "5"))
PEAK_F32_MATRIX = 157.3e12          # MI355X, exact-fp32 MFMA, FLOP/s
m.set_precision("bf16")
torch.cuda.set_device(0)
os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")      # collectives inside captured graphs (as bench.py)
store = os.path.join(tempfile.mkdtemp(), "store")
dist.init_process_group("nccl", store=dist.FileStore(store, 1), rank=0, world_size=1, device_id=torch.device("cuda", 0))


def make_step(sync):
    opt = m.stage2_opt(batch_size=B, distill="rkd", assign_weights="False", num_teachers=2, beta=0.5)
    st = m.DistillStep(opt, 1024, device="cuda", sync=sync, variant="mia2022")
    return st, make_batch(B, H, 1024, opt, "cuda", 0)


def timed(fn, n=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per call


def rows(Bg, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bg, D, generator=g).relu_().cuda(), torch.randn(Bg, D, generator=g).relu_().cuda()


try:
    # ---- (c) the one-workgroup-per-anchor kernels
    for Bo in (64, 128):
        f_s, f_t = rows(Bo, 128, Bo)
        loss, dx = torch.empty(1, device="cuda"), torch.empty_like(f_s)
        ws = torch.empty(lib().ph_rkd_workspace_bytes(Bo, 128), device="cuda", dtype=torch.uint8)
        ts = [timed(lambda: lib().ph_rkd_loss_grad(ptr(f_s), ptr(f_t), ptr(loss), ptr(dx), Bo, 128, 25.0, 50.0, ptr(ws),
                                                   stream())) for _ in range(ROUNDS)]
        print(f"(c) ph_rkd_loss_grad B={Bo} D=128: median {statistics.median(ts):.1f} us  (min {min(ts):.1f}, max {max(ts):.1f}; "
              f"{ROUNDS} rounds x 200 calls)")

    # ---- (a) the partitioned kernels
    if not BASELINE_ONLY:
        for Bg, D, lo, na in ((512, 128, 128, 64), (256, 128, 0, 256), (512, 128, 0, 512)):
            f_s, f_t = rows(Bg, D, Bg + na)
            loss, dx = torch.empty(1, device="cuda"), torch.empty_like(f_s)
            ws = torch.empty(lib().ph_rkd_part_workspace_bytes(Bg, D, na), device="cuda", dtype=torch.uint8)
            ts = [timed(lambda: lib().ph_rkd_loss_grad_part(ptr(f_s), ptr(f_t), Bg, D, lo, na, 25.0, 50.0, ptr(loss), ptr(dx),
                                                            ptr(ws), stream()), n=50) for _ in range(ROUNDS)]
            flop = 3 * 2.0 * na * Bg * Bg * D
            med = statistics.median(ts)
            print(f"(a) ph_rkd_loss_grad_part Bg={Bg} D={D} anchors [{lo}, {lo + na}): median {med:.1f} us  (min {min(ts):.1f}, "
                  f"max {max(ts):.1f}; {ROUNDS} rounds x 50 calls, all launches of the entry);  {flop / 1e9:.2f} GFLOP in the "
                  f"three angle products -> {flop / (med * 1e-6) / 1e12:.1f} TFLOP/s = "
                  f"{100 * flop / (med * 1e-6) / PEAK_F32_MATRIX:.1f} % of the exact-fp32 matrix peak "
                  f"(floor at peak {flop / PEAK_F32_MATRIX * 1e6:.0f} us)")

    # ---- (b) the step
    steps = {"sync=None": make_step(None)}
    if not BASELINE_ONLY:
        steps["ReplicaSync world 1"] = make_step(m.dist.ReplicaSync())
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
        print(f"(b) --distill rkd step, {k}: median {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f}; "
              f"{ROUNDS} rounds x {R} graph-replayed steps, B={B}, {H}x{H}, bf16)")
finally:
    dist.destroy_process_group()

"""Cost of the survival task in the stage-1 mean-teacher step (not a test): python tests/bench_surv_gpu.py

1. The step at B = 64, 512 x 512, bf16, replayed from captured HIP graphs: --task surv against --task grad, the two
   alternating on one device (rounds of R steps each) so that clock / thermal drift hits both alike.
2. The kernels launched by one eager step of each task (torch profiler), and their difference.
3. ph_cindex_counts at N = 4096 and N = 65536 (three risk vectors, one launch)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m
from bench import make_batch

B, H, ROUNDS, R = 64, 512, 5, 10
m.set_precision("bf16")


def make_step(task):
    kw = dict(task="surv", act_type="Sigmoid", label_dim=1) if task == "surv" else {}
    opt = m.stage2_opt(dropout_rate=0.1, batch_size=B, cut_fuse_grad=True, num_teachers=2, **kw)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 1, 1.0, 0, 0, "False", "False"
    st = m.TeacherStage1Step(opt, device="cuda")
    bt = list(make_batch(B, H, 1024, opt, "cuda", 0))
    g = torch.Generator().manual_seed(7)
    bt[3] = (torch.rand(B, generator=g) > 0.3).float().cuda()              # censor
    bt[4] = torch.randint(1, 100, (B,), generator=g).float().cuda()        # survtime (ties)
    return st, tuple(bt)


def kernels_per_step(st, bt):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.step(bt)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return names


steps = {t: make_step(t) for t in ("grad", "surv")}
launches = {}
for t, (st, bt) in steps.items():
    for _ in range(2):
        st.step(bt)
    launches[t] = kernels_per_step(st, bt)
    st.enable_graph()
    for _ in range(3):
        st.step(bt)
torch.cuda.synchronize()
times = {"grad": [], "surv": []}
for _ in range(ROUNDS):
    for t, (st, bt) in steps.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(R):
            st.step(bt)
        torch.cuda.synchronize()
        times[t].append((time.perf_counter() - t0) / R * 1e3)
for t in ("grad", "surv"):
    v = times[t]
    print(f"stage-1 step {t}: median {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f}; {ROUNDS} rounds x {R} "
          f"graph-replayed steps, B={B}, {H}x{H}, bf16)")
print(f"device operations per eager step: grad {len(launches['grad'])}, surv {len(launches['surv'])}")
only = lambda a, b: sorted(set(a) - set(b))      # noqa: E731
print("  only in grad:", only(launches["grad"], launches["surv"]))
print("  only in surv:", only(launches["surv"], launches["grad"]))

rs = torch.Generator().manual_seed(3)
for N in (4096, 65536):
    t = torch.randint(1, 1000, (N,), generator=rs).float().cuda()
    e = (torch.rand(N, generator=rs) > 0.4).float().cuda()
    hs = [torch.randn(N, generator=rs).cuda() for _ in range(3)]
    for _ in range(3):
        m.ops.cindex_counts(t, e, hs)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20 if N <= 4096 else 5
    ev0.record()
    for _ in range(n):
        m.ops.cindex_counts(t, e, hs)
    ev1.record()
    torch.cuda.synchronize()
    print(f"ph_cindex_counts N={N}, 3 risk vectors: {ev0.elapsed_time(ev1) / n:.3f} ms per call")

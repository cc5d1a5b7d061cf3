"""Trunk forward + backward of ResNet-18 against ResNet-34 (not a test):   python tests/bench_resnet34_gpu.py
Perf mode (bf16), B = 64 at 512 x 512 by default (B / H in the environment override).  The two networks alternate in one process -
round r times ResNet-18, then ResNet-34 - after a warm-up of both, each timed with device events around `REPS` forward + backward pairs
through the C-ABI (ph_resnet_forward in train mode, ph_resnet_backward).  Prints the per-round and median times, their ratio, and the
FLOP ratio computed from ph_resnet_unit_shape and the units' output maps (forward + dgrad + wgrad per unit, no dgrad for the stem)."""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trunk_flops(L, plan):
    """Multiply-add FLOPs of one forward + backward of the plan's convolutions."""
    out4, dims, off = (C.c_int * 4)(), (C.c_int * 4)(), C.c_size_t(0)
    total = 0
    for u in range(L.ph_resnet_num_units(plan)):
        assert L.ph_resnet_unit_shape(plan, u, out4) == 0 and L.ph_resnet_tensor_info(plan, 0, u, C.byref(off), dims) == 0
        cout, cin, ks = out4[0], out4[1], out4[2]
        fwd = 2 * dims[0] * dims[1] * dims[2] * cout * cin * ks * ks
        total += fwd * (2 if u == 0 else 3)
    return total


class Trunk:
    def __init__(self, name, net, B, H):
        from multimodal_learning_amd import ops
        self.name, self.net = name, net.cuda().train()
        self.plan = net._get_plan(B, H, H)
        self.packed, self.table = net._get_packed(self.plan), net._param_table()
        self.ws = torch.empty(self.plan.ws_bytes, device="cuda", dtype=torch.uint8)
        self.f3, self.f4 = torch.empty(B, 256, device="cuda"), torch.empty(B, 512, device="cuda")
        self.g3, self.g4 = torch.randn(B, 256, device="cuda"), torch.randn(B, 512, device="cuda")
        self.grads = [torch.empty_like(p) for p in net._trunk_params()]
        self.gptrs = ops.void_array([g.data_ptr() for g in self.grads])

    def fwd_bwd(self, x):
        from multimodal_learning_amd._lib import lib, check, ptr, stream
        check(lib().ph_resnet_forward(self.plan.h, self.table, ptr(self.packed), ptr(x), ptr(self.ws), ptr(self.f3), ptr(self.f4), 1,
                                      stream()), "ph_resnet_forward")
        check(lib().ph_resnet_backward(self.plan.h, self.table, ptr(self.packed), ptr(self.ws), ptr(self.g3), ptr(self.g4), self.gptrs,
                                       stream()), "ph_resnet_backward")

    def time_ms(self, x, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            self.fwd_bwd(x)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps


def main():
    import multimodal_learning_amd as m
    assert torch.cuda.is_available(), "needs a GPU"
    B, H = int(os.environ.get("B", 64)), int(os.environ.get("H", 512))
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 10))
    m.set_precision("bf16")
    torch.manual_seed(0)
    x = torch.rand(B, 3, H, H, device="cuda") * 2 - 1
    trunks = [Trunk("resnet18", m.ResNet18(pretrained=False, path_dim=128, num_classes=3), B, H),
              Trunk("resnet34", m.ResNet34(pretrained=False, path_dim=128, num_classes=3), B, H)]
    L = m.lib()
    flops = {t.name: trunk_flops(L, t.plan.h) for t in trunks}
    for t in trunks:
        for _ in range(3):
            t.fwd_bwd(x)
    torch.cuda.synchronize()
    times = {t.name: [] for t in trunks}
    for r in range(rounds):
        for t in trunks:
            times[t.name].append(t.time_ms(x, reps))
        print("round %d: resnet18 %.3f ms, resnet34 %.3f ms" % (r, times["resnet18"][-1], times["resnet34"][-1]), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    for t in trunks:
        assert all(torch.isfinite(g).all() for g in t.grads), t.name
        print("%s: B %d, %d x %d, bf16: forward + backward median %.3f ms (min %.3f, max %.3f), %d units, %.1f GFLOP, %.1f TFLOP/s"
              % (t.name, B, H, H, med[t.name], min(times[t.name]), max(times[t.name]), L.ph_resnet_num_units(t.plan.h),
                 flops[t.name] / 1e9, flops[t.name] / med[t.name] / 1e9))
    print("time ratio resnet34 / resnet18: %.3f   FLOP ratio: %.3f" % (med["resnet34"] / med["resnet18"], flops["resnet34"] / flops["resnet18"]))


if __name__ == "__main__":
    main()

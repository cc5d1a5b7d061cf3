"""Time of one ph_crd_kmeans_centers call (not a test, not part of bench.py):

    python tests/bench_kmeans_gpu.py [--iters 16] [--classes 3] [--json PATH]

(n_data 1536, k 2), (n_data 1536, k 4) and (n_data 65 536, k 4): both banks, uniform rows as ContrastMemory initialises them,
classes of equal size.  Device events around the whole call (k + 2 * iters launches), warmed up, repeated until a second is
filled - eager, and replayed from a captured graph, which is how the step runs it.  The bytes the call must read are computed
from the shapes: every assignment reads each member row of both banks once (512 B), and so does every pick of the
initialisation but the last; partial sums and centres are noise next to it.  The share is that byte count over the whole-call
time over the 6.29 TB/s a copy kernel reaches on the MI355X - a whole-call figure, not a kernel's.  Nothing is asserted."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m  # noqa: E402,F401
from multimodal_learning_amd._lib import lib, ptr, stream, check  # noqa: E402

HBM_COPY = 6.29e12          # B/s
D = 128


def timed(fn, min_seconds=1.0, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1); reps += 10
    return total / reps * 1e3, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    L, C, T = lib(), a.classes, a.iters
    res = dict(iters=T, classes=C, cases=[])
    for n, k in ((1536, 2), (1536, 4), (65536, 4)):
        g = torch.Generator(device="cuda").manual_seed(n + k)
        stdv = (3.0 / D) ** 0.5
        banks = [torch.zeros(n + C * k, D, device="cuda") for _ in range(2)]
        for b in banks:
            b[:n] = (torch.rand(n, D, generator=g, device="cuda") * 2 - 1) * stdv
        labels = torch.arange(n, device="cuda") % C
        lists = [torch.nonzero(labels == c).flatten().int() for c in range(C)]
        members = torch.cat(lists).contiguous()
        offsets = torch.tensor([0] + [len(x) for x in lists], device="cuda").cumsum(0).int()
        max_rows = max(len(x) for x in lists)
        ws = torch.empty(L.ph_crd_kmeans_centers_workspace_bytes(C, max_rows, k), dtype=torch.uint8, device="cuda")

        def call():
            check(L.ph_crd_kmeans_centers(ptr(banks[0]), ptr(banks[1]), ptr(members), ptr(offsets), C, max_rows, n, D, k, T, None,
                                          None, ptr(ws), stream()), "ph_crd_kmeans_centers")
        us, reps = timed(call)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        us_g, reps_g = timed(graph.replay)
        per_iter = 2 * n * D * 4
        total = (T + k - 1) * per_iter
        row = dict(n_data=n, k=k, launches=k + 2 * T, us_eager=us, us_graph=us_g, bytes_per_iteration=per_iter, bytes_call=total,
                   share_eager=total / (us * 1e-6) / HBM_COPY, share_graph=total / (us_g * 1e-6) / HBM_COPY)
        res["cases"].append(row)
        print(f"n_data {n:6d} k {k}: {k + 2 * T} launches, {us:8.1f} us eager ({reps} calls), {us_g:8.1f} us from a graph ({reps_g} replays); "
              f"{per_iter / 1e6:.2f} MB per iteration, {total / 1e6:.1f} MB per call -> whole-call share of {HBM_COPY / 1e12:.2f} TB/s: "
              f"{100 * row['share_eager']:.2f} % eager, {100 * row['share_graph']:.2f} % from a graph")
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()

"""Cost of the averaged grading metrics and the ROC curves (not a test): python tests/bench_evalavg_gpu.py

Rows of log-probabilities at the two row counts of a test split: 300 patients x 3 grades (the patient level) and 4500 patches
x 3 (the patch level of a 500-ROI fold).  Reported per size: the macro tail (evaluate.grading_metrics_device(avg="macro"): two
count kernels and one host read) and the C + 1 curves (evaluate.roc_curve_device per grade and micro: one host read each) on the
host clock around calls that end in their host read, next to sklearn on the copied rows (the copy included); and the two
kernels alone (ph_rank_counts_classes, ph_roc_points micro and one class) by device events."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m

C = 3


def sync_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out), r


def event_ms(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n


def curves_device(pred, gd):
    return [m.evaluate.roc_curve_device(pred, gd, c) for c in list(range(C)) + ["micro"]]


def macro_host(pred, gd):
    probs, gt = pred.cpu().numpy(), gd.cpu().numpy()
    return m.evaluate.grading_metrics(np.eye(C, dtype=np.float32)[gt], probs, avg="macro")


def curves_host(pred, gd):
    from sklearn import metrics as skm
    probs, gt = pred.cpu().numpy(), gd.cpu().numpy()
    onehot = np.eye(C, dtype=np.int64)[gt]
    return [skm.roc_curve(onehot[:, c], probs[:, c]) for c in range(C)] + [skm.roc_curve(onehot.reshape(-1), probs.reshape(-1))]


print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
rs = torch.Generator().manual_seed(1)
for what, N in (("patient level", 300), ("patch level", 4500)):
    pred = torch.log_softmax(torch.randn(N, C, generator=rs) * 2, 1).cuda()
    gd = torch.randint(0, C, (N,), generator=rs).cuda()
    macro_host(pred, gd); curves_host(pred, gd); curves_device(pred, gd)
    m.evaluate.grading_metrics_device(pred, gd, "macro")
    dv = sync_ms(lambda: m.evaluate.grading_metrics_device(pred, gd, "macro"), 20)
    sk = sync_ms(lambda: macro_host(pred, gd), 20)
    print(f"{what}, N={N} C={C}: macro tail on the device median {dv[0]:.3f} ms (min {dv[1]:.3f}, max {dv[2]:.3f}), "
          f"sklearn on copied rows median {sk[0]:.3f} ms (min {sk[1]:.3f}, max {sk[2]:.3f}); 20 runs, host clock")
    print("   largest |device - sklearn| over the four numbers: %.3g" % max(abs(a - float(b)) for a, b in zip(dv[3], sk[3])))
    dv = sync_ms(lambda: curves_device(pred, gd), 20)
    sk = sync_ms(lambda: curves_host(pred, gd), 20)
    same = all(np.array_equal(a, b) for x, y in zip(dv[3], sk[3]) for a, b in zip(x, y))
    print(f"{what}, N={N} C={C}: {C + 1} ROC curves on the device median {dv[0]:.3f} ms (min {dv[1]:.3f}, max {dv[2]:.3f}), "
          f"sklearn on copied rows median {sk[0]:.3f} ms (min {sk[1]:.3f}, max {sk[2]:.3f}); 20 runs, host clock; "
          f"curves equal: {same}")
    print(f"   ph_rank_counts_classes N={N} C={C}: {event_ms(lambda: m.ops.rank_counts_classes(pred, gd), 20):.3f} ms per call; "
          f"ph_roc_points micro (M={N * C}): {event_ms(lambda: m.ops.roc_points(pred, gd, -1), 20):.3f} ms; "
          f"one class (M={N}): {event_ms(lambda: m.ops.roc_points(pred, gd, 1), 20):.3f} ms (device events, 20 calls)")

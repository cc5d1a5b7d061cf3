"""Cost of the patch-level test pass (not a test): python tests/bench_eval_gpu.py

A resident store of 64 ROIs of 1024 x 1024, S = 512, grid 3: 576 patch rows in batches of 64, student and frozen teacher,
bf16.  Reported: the forward part of the pass (loader + both networks), the metric tail on the device (patch metrics of both
branches, per-patient max aggregation, patient metrics of both branches - host clock around calls that end in their host
read), the same tail through sklearn and pandas after copying the rows, the host reads of one evaluate.test_patches call,
and the two count kernels alone at the size of a 500-ROI fold (4500 rows, M = 13 500 pairs) and at the limit M = 1 048 575."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m

N_ROI, SH, S, B, REPS = 64, 1024, 512, 64, 5
m.set_precision("bf16")
torch.manual_seed(0)
opt = m.stage2_opt(dropout_rate=0.25, batch_size=B, input_size_path=S)
g = torch.Generator().manual_seed(0)
tiles = torch.randint(0, 256, (N_ROI, SH, SH, 3), generator=g, dtype=torch.uint8).cuda()
grade = torch.arange(N_ROI) // 2 % 3                                # two ROIs per patient, one grade per patient
patient = ["p%02d" % (i // 2) for i in range(N_ROI)]
loader = m.augment.ResidentPatchLoader(opt, tiles, torch.randn(N_ROI, 320, generator=g), grade, patient=patient)
student = m.define_net(opt, 1, path_only=True).cuda()
teacher = m.define_net(opt, 1).cuda()
student.eval(); teacher.eval()


def sync_ms(fn, reps=REPS):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out), r


def forward():
    pp, pf, gr = [], [], []
    with torch.no_grad():
        for x_path, x_grph, x_omic, _, _, gd in loader:
            _, _, _, pred_path, _ = student(x_path=x_path, x_grph=x_grph, x_omic=x_omic)
            pred = teacher(x_path=x_path, x_grph=x_grph, x_omic=x_omic)[5]
            pp.append(pred_path); pf.append(pred); gr.append(gd)
    return torch.cat(pp).float().contiguous(), torch.cat(pf).float().contiguous(), torch.cat(gr)


def tail_device(d_path, d_fuse, d_grade, ld):
    E = m.evaluate
    res = [E.grading_metrics_device(d_fuse, d_grade), E.grading_metrics_device(d_path, d_grade)]
    for d in (d_path, d_fuse):
        res.append(E.grading_metrics_device(E.aggregate_by_patient(ld, d, "max"), ld.patient_grade))
    return res


def tail_host(d_path, d_fuse, d_grade, ids, C=3):
    import pandas as pd
    probs_path, probs_all, gt = d_path.cpu().numpy(), d_fuse.cpu().numpy(), d_grade.cpu().numpy()
    onehot = np.eye(C, dtype=np.float32)[gt]
    res = [m.evaluate.grading_metrics(onehot, probs_all), m.evaluate.grading_metrics(onehot, probs_path)]
    pg = pd.Series(gt).groupby(ids).agg("max").to_numpy()
    for p in (probs_path, probs_all):
        agg = pd.DataFrame(p).groupby(ids).agg("max").to_numpy()
        res.append(m.evaluate.grading_metrics(np.eye(C, dtype=np.float32)[pg], agg))
    return res


print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
forward(); forward()                                                 # warm every shape (plans, code objects)
med, lo, hi, (d_path, d_fuse, d_grade) = sync_ms(forward)
print(f"forward part, {len(loader.dataset)} rows in {len(loader)} batches of {B}, {S}x{S}, student + teacher, bf16: "
      f"median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}; {REPS} passes)")
ids = np.repeat(np.asarray(patient), 9)
tail_device(d_path, d_fuse, d_grade, loader); tail_host(d_path, d_fuse, d_grade, ids)
med, lo, hi, rd = sync_ms(lambda: tail_device(d_path, d_fuse, d_grade, loader), 20)
print(f"metric tail on the device ({d_path.shape[0]} rows, {loader.num_patients} patients): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; 20 runs)")
med, lo, hi, rh = sync_ms(lambda: tail_host(d_path, d_fuse, d_grade, ids), 20)
print(f"the same tail through sklearn / pandas on copied rows: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; 20 runs)")
print("largest |device - sklearn| over the 16 numbers: %.3g" % max(abs(a - float(b)) for x, y in zip(rd, rh) for a, b in zip(x, y)))

# a 500-ROI fold: 4500 rows of log-probabilities, 250 patients
rs = torch.Generator().manual_seed(1)
for N in (4500, 349525):
    pred = torch.log_softmax(torch.randn(N, 3, generator=rs) * 2, 1).cuda()
    gd = torch.randint(0, 3, (N,), generator=rs).cuda()
    for name, fn in (("ph_rank_counts", m.ops.rank_counts), ("ph_confusion_counts", m.ops.confusion_counts)):
        for _ in range(2):
            fn(pred, gd)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20 if N <= 4500 else 3
        ev0.record()
        for _ in range(n):
            fn(pred, gd)
        ev1.record()
        torch.cuda.synchronize()
        print(f"{name} N={N} C=3 (M={3 * N}): {ev0.elapsed_time(ev1) / n:.3f} ms per call (device events, {n} calls)")
    if N == 4500:
        ids5 = np.repeat(np.arange(250), 18)
        off, order = m.ops.group_csr(ids5, 250)
        do, dr = torch.from_numpy(off).cuda(), torch.from_numpy(order).cuda()
        for fun in ("max", "mean"):
            m.ops.group_agg(pred, do, dr, off, fun)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(20):
                m.ops.group_agg(pred, do, dr, off, fun)
            ev1.record()
            torch.cuda.synchronize()
            print(f"ph_group_agg {fun} N=4500 G=250 C=3: {ev0.elapsed_time(ev1) / 20:.3f} ms per call (device events, 20 calls)")
        sk = sync_ms(lambda: m.evaluate.grading_metrics(np.eye(3, dtype=np.float32)[gd.cpu().numpy()], pred.cpu().numpy()), 10)
        dv = sync_ms(lambda: m.evaluate.grading_metrics_device(pred, gd), 10)
        print(f"four metrics at N=4500: device {dv[0]:.3f} ms, sklearn on copied rows {sk[0]:.3f} ms (medians of 10, host clock)")

# host reads of one whole call
calls = {"n": 0}
for name in ("cpu", "item", "tolist", "numpy"):
    orig = getattr(torch.Tensor, name)

    def counted(self, *a, _orig=orig, **k):
        calls["n"] += 1
        return _orig(self, *a, **k)
    setattr(torch.Tensor, name, counted)
m.evaluate.test_patches(opt, teacher, student, loader, "cuda")
print(f"host reads (Tensor.cpu / item / tolist / numpy) of one evaluate.test_patches call over {len(loader)} batches: {calls['n']}")

#!/usr/bin/env python3
"""Timing of the DSCD criterion of the MIA-2022 tree (not a pytest file), one process on one device:

    python tests/bench_dscd_gpu.py [--repeats N] [--skip-step]

  (a) ph_crd_select_dscd, with and without the negative weights, alternated with ph_crd_select on the same arrays at the same
      ranking work (select_pos = 1, select_neg = 0, K2 = K), at B = 64, P = 300, P2 = 20, K = 1024.  A repeat is CALLS
      back-to-back calls between two device events; at least 20 timed repeats per entry after warm-up, the three entries taken in
      turn inside every round.  Printed: the median of each entry and ph_crd_select's own max - min spread over its repeats.
      The tool fails (exit status 1) if a new entry's median exceeds ph_crd_select's median by more than that spread.
  (b) the replayed DistillStep(variant="mia2022") at 512 x 512, B = 64, D = 128, n_data = 1024 with crd_criterion "v3" (the
      K + 1 = 1025 columns of its index tensor) and "dscd" (nce_p + nce_k = 1324 columns: more bank rows per sample and bank):
      the back-to-back step time and the head phase (streams joined -> gradient of the student feature) from the ph_prof_stamp
      markers.  No threshold."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

B, D, P, P2, K, N_DATA = 64, 128, 300, 20, 1024, 1024
CALLS = 200


def select_timings(repeats):
    from multimodal_learning_amd._lib import lib, ptr, stream
    L, st = lib(), stream()
    g = torch.Generator().manual_seed(3)
    PK, S2 = P + K, P2 + K
    diff = (torch.rand(B, PK, generator=g) - 0.5).cuda()
    out1, out2 = torch.rand(B, PK, generator=g).cuda(), torch.rand(B, PK, generator=g).cuda()
    sel = torch.empty(B, S2, dtype=torch.int32, device="cuda")
    xs, xt = torch.empty(B, S2, device="cuda"), torch.empty(B, S2, device="cuda")
    a = (ptr(diff), ptr(out1), ptr(out2), None, ptr(sel), ptr(xs), ptr(xt))
    entries = {
        "ph_crd_select (parent entry)": lambda: L.ph_crd_select(*a, B, P, K, P2, K, 0, 1, st),
        "ph_crd_select_dscd": lambda: L.ph_crd_select_dscd(*a, B, P, K, P2, 1, 0, st),
        "ph_crd_select_dscd, weighted": lambda: L.ph_crd_select_dscd(*a, B, P, K, P2, 1, 1, st),
    }
    for call in entries.values():      # warm-up: code objects, clocks
        for _ in range(3 * CALLS):
            assert call() == 0
    torch.cuda.synchronize()
    us = {k: [] for k in entries}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for name, call in entries.items():
            e0.record()
            for _ in range(CALLS):
                call()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    return us


def step_timings(crit):
    import bench
    import multimodal_learning_amd as m
    dev = torch.device("cuda:0")
    kw = dict(nce_k=K, grads_m=0.9, grads_thresh="False", thresh=0.1, dropout_rate=0.1, batch_size=B)
    if crit != "v3":
        kw.update(crd_criterion=crit, nce_p=P, nce_p2=P2, nce_k2=K, neg_reweight="True", select_pos_mode="hard")
    opt = m.stage2_opt(**kw)
    step = m.DistillStep(opt, N_DATA, device=dev, variant="mia2022")
    step._stamps = torch.zeros(16, dtype=torch.int64, device=dev)
    width = P + K if crit != "v3" else K + 1
    bts = []
    for i in range(2):
        bt = list(bench.make_batch(B, 512, N_DATA, opt, dev, seed=31 + i))
        gi = torch.Generator().manual_seed(50 + i)
        sidx = torch.randint(0, N_DATA, (B, width), generator=gi).to(dev)
        sidx[:, 0] = bt[6].to(dev)
        bt[7] = sidx
        bts.append(tuple(bt))
    for c in (step.criterion_kd, step.criterion_kd_path):
        c.contrast.verbose = False
    for i in range(3):
        step.step(bts[i % 2], epoch=5)
    step.enable_graph()
    rows = []
    for i in range(24):
        step.step(bts[i % 2], epoch=5)
        torch.cuda.synchronize()
        if i >= 4:
            rows.append(step._stamps.cpu().numpy().astype(np.int64).copy())
    assert step._static is not None and step._static["graph"] is not None, "graph path was not taken"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(30):
        step.step(bts[i % 2], epoch=5)
    torch.cuda.synchronize()
    per_step_us = (time.perf_counter() - t0) / 30 * 1e6
    t = np.stack(rows)
    rel = (t - t[:, :1]) * 0.01      # us since marker 0
    return per_step_us, float(np.median(rel[:, 4] - rel[:, 2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert a.repeats >= 20, "at least 20 timed repeats per entry"
    print("device:", torch.cuda.get_device_name(0))
    us = select_timings(a.repeats)
    parent = us["ph_crd_select (parent entry)"]
    med_p, spread = float(np.median(parent)), float(max(parent) - min(parent))
    print("(a) selection at B = %d, P = %d, P2 = %d, K = %d; %d repeats of %d calls" % (B, P, P2, K, a.repeats, CALLS))
    ok = True
    for name, v in us.items():
        med = float(np.median(v))
        print("    %-32s median %7.2f us   min %7.2f   max %7.2f" % (name, med, min(v), max(v)))
        if name != "ph_crd_select (parent entry)" and med > med_p + spread:
            ok = False
            print("    ^ exceeds the parent entry's median %.2f us by more than its spread %.2f us" % (med_p, spread))
    print("    parent entry: median %.2f us, max - min spread %.2f us -> %s" % (med_p, spread, "within" if ok else "EXCEEDED"))
    if not a.skip_step:
        print("(b) replayed mia2022 step at 512 x 512, B = %d" % B)
        for crit in ("v3", "dscd"):
            per_step, head = step_timings(crit)
            print("    crd_criterion %-5s step %9.1f us   head phase (join -> feature gradient) %8.1f us" % (crit, per_step, head), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

"""Cost of the survival strata chain (not a test): python tests/bench_survstrata_gpu.py [N ...]

N = 1000, 10 000, 100 000 and 1 048 576 patients, K = 2 (percentile (33, 66)), two kinds of survival times: every patient its
own time (as many table slots as patients: the worst case of the all-pairs passes) and times on a grid of 1 / 64 (a few
thousand slots, as months or days give).  Reported per size, after one warm-up call each:
  - evaluate.survival_strata_device on the host clock around the call, which ends in its one device-to-host copy (medians);
  - the chain alone (ops.surv_strata, surv_table, surv_logrank_km: seven kernel launches and four memsets, into preallocated
    outputs; the wrappers' workspace allocations from torch's cache are inside) by device events around EACH chain (medians);
  - the host path the parent offers for the same answer, on the same box in the same run: the numpy restatement
    (tests/survstrata_emulation.chain_ref: sort-based) and utils.cox_log_rank (the median split's host loop over the distinct
    event times; quadratic, so it is run up to 100 000 patients and once there).
The integers of the device result are compared with the restatement at every size."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m
from multimodal_learning_amd import utils as U
from tests import survstrata_emulation as E

Q = (33, 66)
REPS = {1000: 20, 10000: 20, 100000: 5, 1 << 20: 3}


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out), r


def event_ms(fn, n):
    """Median over n chains, each between its own pair of device events."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1))
    return statistics.median(out)


def launches_only(dh, dt, de):
    N, K, G = dh.shape[0], len(Q), len(Q) + 1
    dev = dh.device
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)      # noqa: E731
    cuts, stat, surv = (torch.empty(n, device=dev, dtype=torch.float64) for n in (K, 2 * K, N * G))
    group, sizes, bad, npts, times = i32(N), i32(K + 1), i32(1), i32(2), torch.empty(N, device=dev, dtype=torch.float32)
    tabs = [i32(N * G) for _ in range(3)]

    def run():
        m.ops.surv_strata(dh, Q, cuts, group, sizes, bad)
        m.ops.surv_table(dt, de, group, G, times, tabs[0], tabs[1], tabs[2], npts)
        m.ops.surv_logrank_km(tabs[0], tabs[1], npts, G, [(0, 1), (1, 2)], stat, surv)
    return run


def main():
    sizes = [int(a) for a in sys.argv[1:]] or sorted(REPS)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| K = 2, percentile", Q)
    for N in sizes:
        reps = REPS.get(N, 5)
        for kind in ("distinct times", "times on a 1/64 grid"):
            hazard, survtime, event = E.case("continuous", N, seed=N % 1000)
            if kind != "distinct times":
                survtime = np.round(survtime * np.float32(64.0)) / np.float32(64.0)
            dh, dt, de = (torch.from_numpy(a).cuda() for a in (hazard, survtime, event))
            m.evaluate.survival_strata_device(dh, dt, de, Q)
            dv = host_ms(lambda: m.evaluate.survival_strata_device(dh, dt, de, Q), reps)
            ev = event_ms(launches_only(dh, dt, de), reps)
            E.chain_ref(hazard, survtime, event, Q)
            t0 = [time.perf_counter()]
            em = []
            for _ in range(min(reps, 5)):
                ref = E.chain_ref(hazard, survtime, event, Q)
                em.append((time.perf_counter() - t0[0]) * 1e3)
                t0[0] = time.perf_counter()
            same = all(np.array_equal(dv[3][k], ref[k]) for k in ("group", "sizes", "times", "at_risk", "observed", "censored"))
            same = same and np.array_equal(dv[3]["cuts"].view(np.int64), ref["cuts"].view(np.int64))
            line = (f"N={N} ({kind}, {ref['times'].shape[0]} slots): survival_strata_device median {dv[0]:.3f} ms (min {dv[1]:.3f}, "
                    f"max {dv[2]:.3f}; {reps} calls, host clock, copy included); the chain alone median {ev:.3f} ms (device "
                    f"events around each of {reps} chains); numpy restatement median {statistics.median(em):.3f} ms ({len(em)} runs)")
            if N <= 100000:
                h64 = hazard.astype(np.float64)
                cr = []
                for _ in range(3 if N <= 10000 else 1):
                    t1 = time.perf_counter()
                    U.cox_log_rank(h64, event, survtime)
                    cr.append((time.perf_counter() - t1) * 1e3)
                line += f"; utils.cox_log_rank (median split only) median {statistics.median(cr):.3f} ms ({len(cr)} runs)"
            else:
                line += "; utils.cox_log_rank not measured at this size (quadratic host loop)"
            print(line + f"; integers and cuts equal to the restatement: {same}", flush=True)


if __name__ == "__main__":
    main()

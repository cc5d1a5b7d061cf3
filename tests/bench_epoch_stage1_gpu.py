"""Cost of the stage-1 epoch record (not a test):
    python tests/bench_epoch_stage1_gpu.py [--batch 64] [--size 512] [--steps 20] [--rounds 5] [--tasks grad,surv]

The replayed TeacherStage1Step at the benchmark shape (bench.py: B = 64, 512 x 512, resident inputs), three arms ALTERNATING
in one process on one box, `rounds` blocks of `steps` steps each, host clock around a block with a device synchronisation at
its end:
  plain      the step as the parent commit runs it (no record attached);
  record     a second, identically built step with a Stage1Record attached;
  host reads the plain step followed by the reference's own per-step reads - the four .item() of the loss sums, the three
             `> 0.0` tests with their .item() ("MIA 2022/train_test_tSVD.py":455-467) and, under grading, the three
             .eq().sum().item() (:486-491), under survival the five .cpu().numpy() copies (:479-483).
Reported: the median over the blocks of ms per step, per arm, every block's figure, and the run-to-run spread of the plain arm
(max - min of its blocks), against which the record arm's distance from the plain arm is to be read."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m      # noqa: E402
import bench                              # noqa: E402


def build(task, B, H, dev, with_record, steps):
    kw = dict(task="surv", act_type="Sigmoid", label_dim=1) if task == "surv" else {}
    opt = m.stage2_opt(dropout_rate=0.1, batch_size=B, cut_fuse_grad=True, num_teachers=2, **kw)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 1, 1.0, 0, 0, "False", "False"
    step = m.TeacherStage1Step(opt, device=dev)
    bts = []
    for i in range(2):
        bt = list(bench.make_batch(B, H, 1024, opt, dev, seed=i))
        if task == "surv":
            g = torch.Generator().manual_seed(7 + i)
            bt[3] = (torch.rand(B, generator=g) > 0.3).float().to(dev)              # censor
            bt[4] = torch.randint(1, 100, (B,), generator=g).float().to(dev)        # survtime (ties)
        bts.append(tuple(bt))
    if with_record:
        step.record = m.Stage1Record(step, steps * B)
    step.enable_graph()
    for i in range(4):                                # two eager steps, the capture, one replay
        step.step(bts[i % 2], epoch=1)
    torch.cuda.synchronize()
    return step, bts


def reference_reads(out, bt, acc, surv):
    """The reference's per-step host reads over the step's returned tensors."""
    br = "cox" if surv else "nll"
    acc["loss"] = acc.get("loss", 0) + out["loss"].data.item()
    for k in ("fuse", "path", "omic"):
        acc[k] = acc.get(k, 0) + (0 + out["loss_%s_%s" % (br, k)]).item()
    for k in ("loss_tsvd", "loss_CRD", "loss_pred_KD"):
        if out[k] > 0.0:
            acc[k] = acc.get(k, 0) + out[k].item()
    if surv:
        for k, t in (("r0", out["pred"]), ("r1", out["pred_path"]), ("r2", out["pred_omic"]), ("c", bt[3]), ("t", bt[4])):
            acc[k] = np.concatenate((acc.get(k, np.array([])), t.detach().cpu().numpy().reshape(-1)))
    else:
        grade = bt[5]
        for k in ("pred", "pred_path", "pred_omic"):
            pred = out[k].argmax(dim=1, keepdim=True)
            acc["ok_" + k] = acc.get("ok_" + k, 0) + pred.eq(grade.view_as(pred)).sum().item()


def block(step, bts, steps, reads, surv):
    acc = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step.step(bts[i % 2], epoch=1)
        if reads:
            reference_reads(out, bts[i % 2], acc, surv)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def step_part(task, B, H, steps, rounds, dev):
    surv = task == "surv"
    plain, bts = build(task, B, H, dev, False, steps)
    rec, bts_r = build(task, B, H, dev, True, steps)
    arms = {"plain": [], "record": [], "host reads": []}
    for _ in range(rounds):
        rec.record.reset()
        arms["plain"].append(block(plain, bts, steps, False, surv))
        arms["record"].append(block(rec, bts_r, steps, False, surv))
        arms["host reads"].append(block(plain, bts, steps, True, surv))
    got = rec.record.read()
    med = {k: statistics.median(v) for k, v in arms.items()}
    spread = max(arms["plain"]) - min(arms["plain"])
    diff = med["record"] - med["plain"]
    line = (f"stage-1 {task} B={B} {H}x{H}, {rounds} alternating blocks of {steps} replayed steps, ms per step (median of the "
            f"blocks): " + "; ".join(f"{k} {med[k]:.3f} [{', '.join('%.3f' % x for x in arms[k])}]" for k in arms)
            + f"; record - plain = {diff:+.3f} ms against a run-to-run spread of the plain arm of {spread:.3f} ms"
            + (" (beyond the spread)" if abs(diff) > spread else " (within the spread)")
            + f"; record <= host reads: {med['record'] <= med['host reads']}"
            + f"; the last epoch's record: steps {got['steps']}, loss sum {got['loss_epoch']:.4f}")
    if surv:
        line += ", C-indices %s" % (tuple(round(c, 4) for c in rec.record.cindex()),)
    print(line, flush=True)
    del plain, rec
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tasks", default="grad,surv")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    m.set_precision("bf16")
    for t in [x for x in a.tasks.split(",") if x]:
        step_part(t, a.batch, a.size, a.steps, a.rounds, dev)


if __name__ == "__main__":
    main()

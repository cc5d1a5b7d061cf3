"""Cost of the epoch record, the MIA-2023 stores and the similarity audit (not a test):
    python tests/bench_epoch_gpu.py [--batch 64] [--size 512] [--steps 20] [--rounds 3] [--variants miccai2022,mia2023]
                                    [--audit 1024,8192,65536]

1. The replayed step at the benchmark shape (bench.py: B = 64, 512 x 512, resident inputs), three arms ALTERNATING in one
   process on one box, `rounds` blocks of `steps` steps each, host clock around a block with a device synchronisation at its end:
     plain      the step as the parent commit runs it (no record attached);
     record     a second, identically built step with an EpochRecord (and, for mia2023, FeatureStores) attached;
     host reads the plain step followed by the reference's own per-step reads - scale.cpu(), loss.item(), loss_cls.item(),
                the two `> 0.0` tests with their .item(), the arg-max count's .item() (MICCAI-2022
                train_test_path_multi_distill.py:305, :317-324, :340) and, for mia2023, the four .cpu() copies and the two
                .cpu().mean() of "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":338-342, :380-383.
   Reported: the median over the blocks of ms per step, per arm, and every block's figure.
2. The audit (evaluate.feature_audit_device, its one host read included) at n = 1024, 8192, 65536 rows of D = 128, median
   of the calls after a warm-up; for n <= 8192 beside it the host route: the stores copied to the host and sklearn's
   cosine_similarity with the reference's three formulas."""
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


def build(variant, B, H, dev, with_record):
    if variant == "miccai2022":
        opt = m.stage2_opt(dropout_rate=0.1, batch_size=B)
        n_data = 1024
        step = m.DistillStep(opt, n_data, device=dev)
        for c in (step.criterion_kd, step.criterion_kd_path):
            c.contrast.verbose = False
        bts = [bench.make_batch(B, H, n_data, opt, dev, seed=i) for i in range(2)]
    else:
        step, bts, _ = bench.variant_setup(variant, B, H, dev)
        n_data = step.criterion_kd.contrast.memory_v1.shape[0]
    if with_record:
        step.record = m.EpochRecord(step)
        if variant == "mia2023":
            step.stores = m.FeatureStores(step, n_data)
    step.enable_graph()
    for i in range(4):                                # two eager steps, the capture, one replay
        step.step(bts[i % 2], epoch=1)
    torch.cuda.synchronize()
    return step, bts


def reference_reads(out, grade, acc):
    """The reference's per-step host reads over the step's returned tensors."""
    if out["scale"] is not None:
        acc["w"] = acc.get("w", 0.0) + out["scale"].detach().cpu().numpy()
    acc["loss"] = acc.get("loss", 0.0) + out["loss"].item()
    acc["cls"] = acc.get("cls", 0.0) + out["loss_cls"].item()
    loss_div = out["loss_div1"] + out["loss_div2"]
    if loss_div > 0.0:
        acc["div"] = acc.get("div", 0.0) + loss_div.item()
    loss_kd = out["loss_kd1"] + out["loss_kd2"]
    if loss_kd > 0.0:
        acc["kd"] = acc.get("kd", 0.0) + loss_kd.item()
    pred = out["pred_path"].argmax(dim=1, keepdim=True)
    acc["ok"] = acc.get("ok", 0) + pred.eq(grade.view_as(pred)).sum().item()
    if "w1" in out:
        for k in ("fuse_feat", "path_feat"):
            out[k].cpu().detach().numpy()
        torch.softmax(out["fuse_logit"], 1).cpu().detach().numpy()
        torch.softmax(out["logit_path"], 1).cpu().detach().numpy()
        out["w1"].cpu().mean(); out["w2"].cpu().mean()


def block(step, bts, steps, reads):
    acc = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step.step(bts[i % 2], epoch=1)
        if reads:
            reference_reads(out, bts[i % 2][5], acc)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def step_part(variant, B, H, steps, rounds, dev):
    plain, bts = build(variant, B, H, dev, False)
    rec, bts_r = build(variant, B, H, dev, True)
    arms = {"plain": [], "record": [], "host reads": []}
    for _ in range(rounds):
        rec.record.reset()
        arms["plain"].append(block(plain, bts, steps, False))
        arms["record"].append(block(rec, bts_r, steps, False))
        arms["host reads"].append(block(plain, bts, steps, True))
    got = rec.record.read()
    med = {k: statistics.median(v) for k, v in arms.items()}
    print(f"{variant} B={B} {H}x{H}, {rounds} alternating blocks of {steps} replayed steps, ms per step (median of the blocks): "
          + "; ".join(f"{k} {med[k]:.3f} [{', '.join('%.3f' % x for x in arms[k])}]" for k in arms)
          + f"; record / plain = {med['record'] / med['plain']:.4f}, host reads / plain = {med['host reads'] / med['plain']:.4f}"
          + f"; the last epoch's record: steps {got['steps']}, loss sum {got['loss_epoch']:.4f}", flush=True)
    del plain, rec
    torch.cuda.empty_cache()


def audit_part(sizes, D, dev):
    from sklearn.metrics.pairwise import cosine_similarity
    for n in sizes:
        g = torch.Generator().manual_seed(n)
        F = torch.randn(n, D, generator=g)
        P = 0.5 * F + torch.randn(n, D, generator=g)
        lab = torch.arange(n) % 3
        dF, dP, dl = F.to(dev), P.to(dev), lab.to(dev)
        d = m.evaluate.feature_audit_device(dF, dP, dl)
        reps = 10 if n <= 8192 else 3
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = m.evaluate.feature_audit_device(dF, dP, dl)
            ts.append((time.perf_counter() - t0) * 1e3)
        line = (f"audit n={n} D={D}: feature_audit_device median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, {reps} calls, "
                f"host clock, its one read included); teacher intra / inter {d['teacher_intra']:.6f} / {d['teacher_inter']:.6f}, "
                f"similarity_diff {d['similarity_diff']:.6f}")
        if n <= 8192:
            t0 = time.perf_counter()
            Fh, Ph, lh = dF.cpu().numpy(), dP.cpu().numpy(), dl.cpu().numpy()
            Sf, Sp = cosine_similarity(Fh), cosine_similarity(Ph)
            ind = 1.0 * np.equal(np.tile(lh.reshape(-1, 1), (1, n)), np.tile(lh.reshape(1, -1), (n, 1)))
            host = (Sf[ind == 1].mean(), Sf[ind == 0].mean(), Sp[ind == 1].mean(), Sp[ind == 0].mean(), np.mean(np.abs(Sf - Sp)))
            ms = (time.perf_counter() - t0) * 1e3
            line += (f"; host route (copies, sklearn, the three formulas) {ms:.1f} ms (one run), teacher intra {host[0]:.6f}, "
                     f"similarity_diff {host[4]:.6f}")
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", default="miccai2022,mia2023")
    ap.add_argument("--audit", default="1024,8192,65536")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    m.set_precision("bf16")
    for v in [x for x in a.variants.split(",") if x]:
        step_part(v, a.batch, a.size, a.steps, a.rounds, dev)
    audit_part([int(x) for x in a.audit.split(",") if x], 128, dev)


if __name__ == "__main__":
    main()

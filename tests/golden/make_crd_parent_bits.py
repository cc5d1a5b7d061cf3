#!/usr/bin/env python
"""The bits of every CRD entry point, as one commit computes them on the MI355X: tests/golden/crd_parent_bits.npz.

Run on the GPU by the commit BEFORE the bank refactor; tests/test_gpu_crd_parent_bits.py recomputes
the same quantities through `RUNS` / `record` below and compares bit for bit.  Only the criteria's public entry points are
used, so the file runs unchanged on either side of the refactor.

    python tests/golden/make_crd_parent_bits.py [OUT.npz]

Every run is a criterion built under a fixed torch seed (so the constructor's own bank draw is inside), Embed weights from
oracle.weights.make_state_dict, and two calls on inputs of a seeded CPU generator: the first sets Z, the second scores
against the momentum-updated bank.  Recorded per call: the loss, the per-sample losses where the entry point has them, the
gradients of f_s and of the first weight of both Embed heads, `params`, the updated rows of both banks.  The projection
heads read 16-wide features: the recorded weight gradients stay small."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S_DIM = 16
LABELS = 3


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _load_embeds(crd, seed):
    from oracle import weights as W
    for k, head in enumerate((crd.embed_s, crd.embed_t)):
        head.load_state_dict(W.make_state_dict({n: tuple(v.shape) for n, v in head.state_dict().items()}, seed + k))


class Run:
    """One criterion object and its two calls.  `kind`: dcd (CRD_loss.CRDLoss), mem3 (ContrastMemory_v3.forward), v3
    (CRD_criterion_v3.CRDLoss), mt (CRD_criterion.CRDLoss), v10 (CRD_criterion_v10.CRDLoss)."""

    def __init__(self, kind, seed, B, n_data, D=128, P=1, K=16, P2=1, K2=16, select_neg="False", mode="hard", ranks=None,
                 sample_KD="False", pos_extra="neighbors", centers_kmeans="sklearn", scan=None):
        import multimodal_learning_amd as m
        from multimodal_learning_amd.CL_utils import CRD_criterion, CRD_criterion_v3, CRD_criterion_v10, memory_new
        self.kind, self.B, self.n, self.D, self.P, self.K, self.mode, self.ranks = kind, B, n_data, D, P, K, mode, ranks
        self.gen = torch.Generator().manual_seed(1000 + seed)
        self.labels = torch.arange(n_data) % LABELS
        torch.manual_seed(seed)
        opt = m.stage2_opt(feat_dim=D, s_dim=S_DIM, t_dim=S_DIM, nce_p=P, nce_k=K, nce_p2=P2, nce_k2=K2, n_data=n_data,
                           select_neg_pairs=select_neg, select_pos_mode=mode, sample_KD=sample_KD, pos_extra=pos_extra,
                           centers_kmeans=centers_kmeans)
        if kind == "mem3":
            self.mem = memory_new.ContrastMemory_v3(D, n_data, P, K, opt.nce_t, opt.nce_m, True, P2, select_neg, K2)
            self.crd = None
        else:
            if kind == "dcd":
                self.crd = m.CRDLoss(opt, n_data)
            elif kind == "v3":
                self.crd = CRD_criterion_v3.CRDLoss(opt, n_data)
            elif kind == "mt":
                self.crd = CRD_criterion.CRDLoss(opt)
            else:
                class_idx = [np.nonzero((self.labels == c).numpy())[0] for c in range(LABELS)]
                saved = os.environ.get("PH_CRD_SCAN")
                if scan is not None:
                    os.environ["PH_CRD_SCAN"] = scan
                try:
                    self.crd = CRD_criterion_v10.CRDLoss(opt, n_data, class_idx)      # (reads PH_CRD_SCAN here, once)
                finally:
                    if scan is not None:
                        if saved is None:
                            del os.environ["PH_CRD_SCAN"]
                        else:
                            os.environ["PH_CRD_SCAN"] = saved
            _load_embeds(self.crd, 40 + 2 * seed)
            self.mem = self.crd.contrast
        self.mod = (self.crd if self.crd is not None else self.mem).cuda()
        self.mem.verbose = False

    def call(self):
        """-> {name: array} of one call."""
        g, B, n, kind = self.gen, self.B, self.n, self.kind
        index = torch.randperm(n, generator=g)[:B]
        width = {"dcd": self.P + self.K, "mem3": self.P + self.K}.get(kind, self.K + 1)
        sidx = torch.randint(0, n, (B, width), generator=g); sidx[:, 0] = index
        w = torch.rand(B, generator=g) + 0.5
        out = {}
        if kind == "mem3":
            v1 = torch.nn.functional.normalize(torch.randn(B, self.D, generator=g)).cuda().requires_grad_(True)
            v2 = torch.nn.functional.normalize(torch.randn(B, self.D, generator=g)).cuda().requires_grad_(True)
            o1, o2 = self.mem(0.1, v1, v2, index.cuda(), sidx.cuda(), select_pos_mode=self.mode, ranks=self.ranks)
            w1 = torch.rand(o1.shape, generator=g).cuda(); w2 = torch.rand(o2.shape, generator=g).cuda()
            gv1, gv2 = torch.autograd.grad((o1 * w1).sum() + (o2 * w2).sum(), [v1, v2])
            out.update(out_v1=_np(o1), out_v2=_np(o2), d_v1=_np(gv1), d_v2=_np(gv2))
        else:
            crd = self.crd
            f_s = torch.randn(B, S_DIM, generator=g).cuda().requires_grad_(True)
            f_t = torch.randn(B, S_DIM, generator=g).cuda()
            ix = index.cuda()
            if kind == "dcd":
                loss = crd(0.1, f_s, f_t, ix, sidx.cuda(), ranks=self.ranks)
            elif kind == "v3":
                loss = crd(w.cuda(), f_s, f_t, ix, None)           # the device draw of the columns and its step counter
            elif kind == "mt":
                loss = crd(f_s, f_t, ix, None)
            else:
                loss, rows = crd(w.cuda(), f_s, f_t, self.labels[index].cuda(), ix, sidx.cuda())
                out["sample_loss"] = _np(rows)
            scalar = loss if loss.numel() == 1 else (loss * w.cuda()).sum()      # (sample_KD: the [B] per-sample losses)
            heads = [next(iter(crd.embed_s.parameters())), next(iter(crd.embed_t.parameters()))]
            gs = torch.autograd.grad(scalar.sum(), [f_s] + heads)
            out.update(loss=_np(loss), d_f_s=_np(gs[0]), d_w_embed_s=_np(gs[1]), d_w_embed_t=_np(gs[2]))
        ixc = index.cuda()
        out.update(params=_np(self.mem.params), bank_v1_rows=_np(self.mem.memory_v1[ixc]), bank_v2_rows=_np(self.mem.memory_v2[ixc]))
        return out


# tag -> Run arguments.  The widths and sizes are the smallest at which each path of crd_core is taken: a bank that is no
# multiple of the 32-row tile of the KNN scan (70), the workspace branch of ph_crd_loss_grad (P2 + K2 >= 1024), both
# split rules of the bank-scan form (n_data 70: nsplit 1, 1030: nsplit 32), every feature width
RUNS = {
    "c1_dcd_hard":        dict(kind="dcd", seed=1, B=5, n_data=70, P=4, K=16, P2=2, K2=8, select_neg="True", mode="hard"),
    "c2_dcd_ranks_kd":    dict(kind="dcd", seed=2, B=5, n_data=70, P=4, K=16, P2=2, K2=8, select_neg="False", mode="mid",
                               ranks=[3, 1], sample_KD="True"),
    "c3_mem3_forward":    dict(kind="mem3", seed=3, B=5, n_data=70, D=64, P=4, K=16, P2=2, K2=8, select_neg="True", mode="hard"),
    "c4_dcd_long":        dict(kind="dcd", seed=4, B=3, n_data=1100, P=4, K=1030, P2=2, K2=8, select_neg="False", mode="hard"),
    "c5_v3_draw":         dict(kind="v3", seed=5, B=5, n_data=70, K=16),
    "c5_mt_draw":         dict(kind="mt", seed=6, B=5, n_data=70, K=16),
    "c6_v10_knn_d128":    dict(kind="v10", seed=7, B=5, n_data=70, D=128, P=3, K=16, scan="0"),
    "c6_v10_knn_d256":    dict(kind="v10", seed=8, B=5, n_data=70, D=256, P=3, K=16, scan="0"),
    "c7_v10_scan_n70":    dict(kind="v10", seed=9, B=5, n_data=70, P=3, K=70, scan="1"),
    "c7_v10_scan_n1030":  dict(kind="v10", seed=10, B=5, n_data=1030, P=3, K=1030, scan="1"),
    "c8_v10_means":       dict(kind="v10", seed=11, B=5, n_data=70, P=2, K=16, pos_extra="centers"),
    "c8_v10_kmeans":      dict(kind="v10", seed=12, B=5, n_data=70, P=3, K=16, pos_extra="centers", centers_kmeans="device"),
}
STEP_VARIANTS = ("miccai2022", "mia2022", "mia2023")
STEP_KEYS = ("loss", "loss_cls", "loss_div1", "loss_div2", "loss_kd1", "loss_kd2", "scale")


def record(tag):
    """Both calls of one stand-alone run -> {"<tag>.<call>.<name>": array}."""
    run = Run(**RUNS[tag])
    return {"%s.%d.%s" % (tag, it, k): v for it in range(2) for k, v in run.call().items()}


def record_step(variant):
    """One eager DistillStep iteration with the fused loss head, at the smallest configuration tests/test_gpu_step.py uses for
    the variant (its own builders): the loss dictionary and the updated bank rows of both criteria."""
    import multimodal_learning_amd as m
    from oracle.step import default_opt, synthetic_batch
    from tests.test_gpu_step import _mk_step, _mk_variant_step, _tuple
    m.set_precision("bf16x6")
    try:
        if variant == "miccai2022":
            opt = default_opt()
            opt.fused_loss_head = True
            step = _mk_step(opt, 1024, seed=0)
            ranks = [np.random.RandomState(i).choice(np.arange(30, 100), 20, replace=False) for i in range(2)]
            bt = synthetic_batch(8, 64, seed=21)
            out = step.step(_tuple(bt), ranks=ranks)
        elif variant == "mia2022":
            opt = default_opt(nce_k=64, grads_m=0.9, grads_thresh="False", thresh=0.1, niter_decay=10)
            opt.fused_loss_head = True
            step, n_data, _ = _mk_variant_step("mia2022", opt)
            bt = synthetic_batch(8, 64, n_data=n_data, P=1, K=64, seed=400)
            out = step.step(_tuple(bt), epoch=3)
        else:
            opt = default_opt(nce_k=64, nce_p=4, pos_extra="neighbors", neg_mode="all_others", start_reweight=0, discrep_scale=1,
                              max_discrep=2.0, use_grads_thresh="True", grads_thresh=0.1, loss_weighting="GK_refine", batch_size=8)
            opt.fused_loss_head = True
            step, n_data, labels = _mk_variant_step("mia2023", opt)
            bt = synthetic_batch(8, 64, n_data=n_data, P=1, K=64, seed=500)
            bt["grade"] = labels[bt["index"]].long()
            out = step.step(_tuple(bt), epoch=2)
        assert step._fused_head_ok()
        rec = {"step_%s.%s" % (variant, k): _np(out[k]) for k in STEP_KEYS}
        ix = bt["index"].cuda()
        for i, crd in enumerate((step.criterion_kd, step.criterion_kd_path)):
            rec["step_%s.crd%d.params" % (variant, i)] = _np(crd.contrast.params)
            rec["step_%s.crd%d.bank_v1_rows" % (variant, i)] = _np(crd.contrast.memory_v1[ix])
            rec["step_%s.crd%d.bank_v2_rows" % (variant, i)] = _np(crd.contrast.memory_v2[ix])
        return rec
    finally:
        m.set_precision("bf16")


def main(out):
    bits = {}
    for tag in RUNS:
        bits.update(record(tag))
    for variant in STEP_VARIANTS:
        bits.update(record_step(variant))
    torch.cuda.synchronize()
    np.savez(out, **bits)
    print("wrote %s: %d arrays, %d bytes" % (out, len(bits), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "crd_parent_bits.npz"))

#!/usr/bin/env python3
"""Golden vectors for the clustered class-centre positives of the MIA-2023 CRD bank (`--pos_extra centers --nce_p 3` and `4`,
"MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py":81-101,117-137 with ContrastLoss :241-277), produced by running
the reference's CRDLoss for two calls per nce_p.  Build container only.  Writes tests/golden/mia2023_crd_v10_kmeans.npz.

The reference fits sklearn KMeans from a random initialisation; the product runs a deterministic k-means of its own
(DESIGN.md section 16).  The two meet on a PLANTED bank (tests/kmeans_emulation.planted_bank: every class is exactly nce_p - 1
tight blobs), where any k-means finds the planted partition, and the loss and its gradients are symmetric in the centres of a
class.  Nothing here assumes that: the KMeans name in the reference module is wrapped by a subclass that records labels_, and the
script fails unless every fit reproduced the planted partition.  nce_m = 0.99 keeps the rows updated by the first call inside
their blobs.  The recipe's seed is stored, not the banks."""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference/MIA 2023/stage2_unimodal_student"


def main():
    from make_golden import install_shims, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    from oracle import weights as W
    from tests import kmeans_emulation as E
    with contextlib.redirect_stdout(io.StringIO()):
        v10 = importlib.import_module("CL_utils.CRD_criterion_v10")
    fits = []

    class RecordingKMeans(v10.KMeans):
        def fit(self, X, *a, **k):
            r = super().fit(X, *a, **k)
            fits.append(np.asarray(self.labels_).copy())
            return r
    v10.KMeans = RecordingKMeans

    n_data, K, B, seed = E.GOLDEN["n_data"], 64, 8, E.GOLDEN["seed"]
    rec = dict(n_data=n_data, K=K, B=B, bank_seed=seed, nce_m=0.99, nce_p=np.asarray(E.GOLDEN["nce_p"]))
    for NP in E.GOLDEN["nce_p"]:
        k = NP - 1
        b1, b2, labels, blobs = E.planted_bank(seed, n_data, k)
        labels = torch.as_tensor(labels)
        class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
        opt = types.SimpleNamespace(s_dim=128, t_dim=128, feat_dim=128, nce_k=K, nce_t=0.07, nce_m=0.99, nce_p=NP,
                                    pos_extra="centers")
        torch.manual_seed(4)
        np.random.seed(17 + NP)                      # sklearn's KMeans(random_state=None) draws from numpy's global state
        with contextlib.redirect_stdout(io.StringIO()):
            crd = v10.CRDLoss(opt, n_data, class_idx)
        crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 52))
        crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 53))
        crd.contrast.memory_v1.copy_(torch.as_tensor(b1)); crd.contrast.memory_v2.copy_(torch.as_tensor(b2))
        g = torch.Generator().manual_seed(13 + NP)
        pre = f"p{NP}."
        for it in range(2):
            f_s = torch.randn(B, 128, generator=g).relu_().requires_grad_(True)
            f_t = torch.randn(B, 128, generator=g).relu_()
            index = torch.randperm(n_data, generator=g)[:B]
            sidx = torch.randint(0, n_data, (B, K + 1), generator=g); sidx[:, 0] = index
            grade = labels[index]
            w = (1 + torch.rand(B, generator=g)).view(-1, 1)
            del fits[:]
            with contextlib.redirect_stdout(io.StringIO()):
                loss, sample_loss = crd(w, f_s, f_t, grade, index, sidx)
            # fits: the three classes of bank 1 (:85-92), then the three classes of bank 2 (:121-128)
            assert len(fits) == 6, len(fits)
            for i, lab in enumerate(fits):
                bank, c = i // 3, i % 3
                pairs = set(zip(lab.tolist(), blobs[bank, class_idx[c]].tolist()))
                assert len(pairs) == k and len({p[0] for p in pairs}) == k and len({p[1] for p in pairs}) == k, \
                    f"nce_p {NP} call {it}: KMeans did not reproduce the planted partition of bank {bank + 1} class {c}: {pairs}"
            gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight], retain_graph=True)
            rec.update({pre + f"f_s{it}": f_s, pre + f"f_t{it}": f_t, pre + f"index{it}": index, pre + f"sidx{it}": sidx,
                        pre + f"grade{it}": grade, pre + f"w{it}": w, pre + f"loss{it}": loss,
                        pre + f"sample_loss{it}": sample_loss, pre + f"g_fs{it}": gs[0], pre + f"g_ws{it}": gs[1],
                        pre + f"g_wt{it}": gs[2], pre + f"params{it}": crd.contrast.params.clone(),
                        pre + f"bank_v1_rows{it}": crd.contrast.memory_v1[index].clone(),
                        pre + f"bank_v2_rows{it}": crd.contrast.memory_v2[index].clone()})
        print(f"nce_p {NP}: every fit reproduced the planted partition; losses", float(rec[pre + "loss0"]), float(rec[pre + "loss1"]))
    np.savez_compressed(os.path.join(HERE, "mia2023_crd_v10_kmeans.npz"), **npz(rec))
    print("written mia2023_crd_v10_kmeans.npz")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the MIA-2023 CRD criterion with more than eight KNN positives (`--pos_extra neighbors`, nce_p 16 and
24), produced by running the reference's "MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py" for two calls each at
B = 8 over a bank of 384 rows.  Build container only.  Writes tests/golden/mia2023_crd_v10_np.npz; the keys of nce_p = P carry
the prefix "pP_".

The reference orders the similarities with an unstable torch.sort; this project's KNN is the stable sort.  The two agree as
long as the sort never has to order equal values, i.e. as long as the masked zeros stay out of the first nce_p: the script
fails unless every query has at least nce_p same-class rows of positive similarity in both banks, at both calls."""
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
N_DATA, K, B = 384, 128, 8
NUM_POS = (16, 24)


def positive_rows(bank, labels, index):
    """Per query: the number of same-class bank rows whose float64 cosine with the query's own row is positive, and the
    class-masked similarities in descending order (two equal ones among the first would be a tie for the unstable sort to break)."""
    m = bank.double().numpy()
    mn = m / np.linalg.norm(m, axis=1, keepdims=True)
    sim = mn[index.numpy()] @ mn.T
    sim = np.where(labels.numpy()[None, :] == labels.numpy()[index.numpy()][:, None], sim, 0.0)
    return (sim > 0).sum(1), -np.sort(-sim, axis=1)


def main():
    from make_golden import install_shims, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    from oracle import weights as W
    from oracle.variants import CRDv10State
    with contextlib.redirect_stdout(io.StringIO()):
        v10 = importlib.import_module("CL_utils.CRD_criterion_v10")
    g = torch.Generator().manual_seed(31)
    labels = torch.randint(0, 3, (N_DATA,), generator=g)
    class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
    rec = dict(n_data=N_DATA, K=K, num_pos=np.asarray(NUM_POS), bank_seed=62, labels=labels)
    for NP in NUM_POS:
        opt = types.SimpleNamespace(s_dim=128, t_dim=128, feat_dim=128, nce_k=K, nce_t=0.07, nce_m=0.5, nce_p=NP,
                                    pos_extra="neighbors")
        torch.manual_seed(4)
        with contextlib.redirect_stdout(io.StringIO()):
            crd = v10.CRDLoss(opt, N_DATA, class_idx)
        crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 50))
        crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 51))
        st = CRDv10State(N_DATA, labels, K=K, seed=62)
        crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
        for it in range(2):
            f_s = torch.randn(B, 128, generator=g).relu_().requires_grad_(True)
            f_t = torch.randn(B, 128, generator=g).relu_()
            index = torch.randperm(N_DATA, generator=g)[:B]
            sidx = torch.randint(0, N_DATA, (B, K + 1), generator=g); sidx[:, 0] = index
            grade = labels[index]
            w = (1 + torch.rand(B, generator=g)).view(-1, 1)
            for bank in (crd.contrast.memory_v1, crd.contrast.memory_v2):
                npos, top = positive_rows(bank, labels, index)
                if npos.min() < NP:
                    raise SystemExit(f"nce_p {NP} call {it}: a query has only {npos.min()} same-class rows of positive similarity; "
                                     "the reference's unstable sort would order the masked zeros")
                gap = -np.diff(top[:, :NP + 1], axis=1)
                if gap.min() <= 1e-6:
                    raise SystemExit(f"nce_p {NP} call {it}: two of the first {NP + 1} similarities are {gap.min():.1e} apart")
            with contextlib.redirect_stdout(io.StringIO()):
                loss, sample_loss = crd(w, f_s, f_t, grade, index, sidx)
            gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight], retain_graph=True)
            p = f"p{NP}_"
            rec.update({f"{p}f_s{it}": f_s, f"{p}f_t{it}": f_t, f"{p}index{it}": index, f"{p}sidx{it}": sidx, f"{p}grade{it}": grade,
                        f"{p}w{it}": w, f"{p}loss{it}": loss, f"{p}sample_loss{it}": sample_loss, f"{p}g_fs{it}": gs[0],
                        f"{p}g_ws{it}": gs[1], f"{p}g_wt{it}": gs[2], f"{p}params{it}": crd.contrast.params.clone(),
                        f"{p}bank_v1_rows{it}": crd.contrast.memory_v1[index].clone()})
    np.savez_compressed(os.path.join(HERE, "mia2023_crd_v10_np.npz"), **npz(rec))
    print("written mia2023_crd_v10_np.npz")


if __name__ == "__main__":
    main()

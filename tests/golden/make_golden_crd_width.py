#!/usr/bin/env python3
"""Golden vectors of the reference's CRD classes at feat_dim 64 and 256 (every other golden here is at 128), produced by importing
and running the reference classes on the CPU (build container only; shims of make_golden.py):

  v3mem   MICCAI-2022 CL_utils/memory_new.ContrastMemory_v3 standalone, select_pos_mode "hard", two calls
  crd     MICCAI-2022 CL_utils/CRD_loss.CRDLoss ("hard"), two calls
  s1      MICCAI-2022 CL_utils/CRD_criterion.CRDLoss (the stage-1 vanilla bank, two-layer heads), two calls
  v3      "MIA 2022" CL_utils/CRD_criterion_v3.CRDLoss, two calls
  v10     "MIA 2023" CL_utils/CRD_criterion_v10.CRDLoss, pos_extra "neighbors", two calls

n_data = 256, B = 4, s_dim = t_dim = 64, column lists of tens.  Banks and head weights are seed recipes (`bank`, `head`), repeated
in tests/test_gpu_crd_width_modules.py: the file holds inputs, outputs, gradients (d f_s of both calls, the weight gradients of the second), params and the updated bank
rows only.

Usage:  python tests/golden/make_golden_crd_width.py        # writes tests/golden/crd_width.npz
"""
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
REFS = {"miccai": "/root/reference/MICCAI-2022", "mia2022": "/root/reference/MIA 2022",
        "mia2023": "/root/reference/MIA 2023/stage2_unimodal_student"}
N_DATA, B, SDIM = 256, 4, 64


def bank(D, seed):
    """[n_data, D] uniform in +-1/sqrt(D/3), the reference's initialisation (memory_new.py:246-247) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    stdv = 1.0 / (D / 3) ** 0.5
    return torch.rand(N_DATA, D, generator=g).mul_(2 * stdv).add_(-stdv)


def head(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(*s, generator=g) * (0.1 if len(s) == 2 else 0.02) for k, s in shapes.items()}


def head1(D):
    return {"linear.weight": (D, SDIM), "linear.bias": (D,)}


def head2(D):
    return {"linear.0.weight": (D, SDIM), "linear.0.bias": (D,), "linear.2.weight": (D, D), "linear.2.bias": (D,)}


def _use(ref):
    """Switch to another reference tree: its CL_utils package replaces the one imported before."""
    for name in [n for n in sys.modules if n == "CL_utils" or n.startswith("CL_utils.")]:
        del sys.modules[name]
    for r in REFS.values():
        while r in sys.path:
            sys.path.remove(r)
    sys.path.insert(0, REFS[ref])
    os.chdir(REFS[ref])


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


def _load(crd, D, seeds, two_layer=False):
    shapes = head2(D) if two_layer else head1(D)
    crd.embed_s.load_state_dict(head(shapes, seeds[0])); crd.embed_t.load_state_dict(head(shapes, seeds[1]))
    crd.contrast.memory_v1.copy_(bank(D, seeds[2])); crd.contrast.memory_v2.copy_(bank(D, seeds[3]))


def _batch(g, width):
    f_s = torch.randn(B, SDIM, generator=g).relu_().requires_grad_(True)
    f_t = torch.randn(B, SDIM, generator=g).relu_()
    index = torch.randperm(N_DATA, generator=g)[:B]
    sidx = torch.randint(0, N_DATA, (B, width), generator=g); sidx[:, 0] = index
    return f_s, f_t, index, sidx


def main():
    from make_golden import install_shims, npz
    install_shims()
    rec = dict(n_data=N_DATA, B=B, s_dim=SDIM, P=30, K=60, P2=10, K2=40, K1=48, num_pos=3)
    P, K, P2, K2, K1, NP = 30, 60, 10, 40, 48, 3
    labels = torch.randint(0, 3, (N_DATA,), generator=torch.Generator().manual_seed(11))
    rec["labels"] = labels
    class_idx = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
    for D in (64, 256):
        # ---- MICCAI-2022: ContrastMemory_v3 standalone, CRD_loss.CRDLoss, CRD_criterion.CRDLoss
        _use("miccai")
        with _quiet():
            mn = importlib.import_module("CL_utils.memory_new")
            cl = importlib.import_module("CL_utils.CRD_loss")
            c1 = importlib.import_module("CL_utils.CRD_criterion")
        mem = mn.ContrastMemory_v3(D, N_DATA, P, K, 0.07, 0.5, True, P2, "True", K2)
        mem.memory_v1.copy_(bank(D, 21)); mem.memory_v2.copy_(bank(D, 22))
        g = torch.Generator().manual_seed(77 + D)
        for it in range(2):
            v1 = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).requires_grad_(True)
            v2 = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).requires_grad_(True)
            y = torch.randperm(N_DATA, generator=g)[:B]
            idx = torch.randint(0, N_DATA, (B, P + K), generator=g); idx[:, 0] = y
            w1 = torch.randn(B, P2 + K2, 1, generator=g); w2 = torch.randn(B, P2 + K2, 1, generator=g)
            with _quiet():
                o1, o2 = mem(0.1, v1, v2, y, idx, select_pos_mode="hard")
            gv1, gv2 = torch.autograd.grad((o1 * w1).sum() + (o2 * w2).sum(), [v1, v2])
            t = f"v3mem{D}_{it}"
            rec.update({f"{t}_v1": v1, f"{t}_v2": v2, f"{t}_y": y, f"{t}_idx": idx, f"{t}_w1": w1, f"{t}_w2": w2, f"{t}_out1": o1,
                        f"{t}_out2": o2, f"{t}_gv1": gv1, f"{t}_gv2": gv2, f"{t}_params": mem.params.clone(),
                        f"{t}_rows1": mem.memory_v1[y].clone(), f"{t}_rows2": mem.memory_v2[y].clone()})
        opt = types.SimpleNamespace(s_dim=SDIM, t_dim=SDIM, feat_dim=D, nce_p=P, nce_k=K, nce_p2=P2, nce_k2=K2, nce_t=0.07, nce_m=0.5,
                                    select_pos_pairs=True, select_neg_pairs="True", sample_KD="False", select_pos_mode="hard",
                                    n_data=N_DATA)
        with _quiet():
            crd = cl.CRDLoss(opt, N_DATA)
        _load(crd, D, (10, 11, 21, 22))
        g = torch.Generator().manual_seed(78 + D)
        for it in range(2):
            f_s, f_t, index, sidx = _batch(g, P + K)
            with _quiet():
                loss = crd(0.1, f_s, f_t, index, sidx)
            gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
            t = f"crd{D}_{it}"
            rec.update({f"{t}_f_s": f_s, f"{t}_f_t": f_t, f"{t}_index": index, f"{t}_sidx": sidx, f"{t}_loss": loss, f"{t}_g_fs": gs[0],
                        f"{t}_g_ws": gs[1], f"{t}_g_wt": gs[2], f"{t}_params": crd.contrast.params.clone(),
                        f"{t}_rows1": crd.contrast.memory_v1[index].clone(), f"{t}_rows2": crd.contrast.memory_v2[index].clone()})
        opt1 = types.SimpleNamespace(s_dim=SDIM, t_dim=SDIM, feat_dim=D, nce_k=K1, nce_t=0.07, nce_m=0.5, n_data=N_DATA)
        with _quiet():
            crd = c1.CRDLoss(opt1)
        _load(crd, D, (70, 71, 81, 82), two_layer=True)
        g = torch.Generator().manual_seed(79 + D)
        for it in range(2):
            f_s, f_t, index, sidx = _batch(g, K1 + 1)
            with _quiet():
                loss = crd(f_s, f_t, index, sidx)
            gs = torch.autograd.grad(loss.sum(), [f_s, crd.embed_s.linear[0].weight, crd.embed_t.linear[2].bias])
            t = f"s1{D}_{it}"
            rec.update({f"{t}_f_s": f_s, f"{t}_f_t": f_t, f"{t}_index": index, f"{t}_sidx": sidx, f"{t}_loss": loss, f"{t}_g_fs": gs[0],
                        f"{t}_g_w0": gs[1], f"{t}_g_tb2": gs[2], f"{t}_params": crd.contrast.params.clone(),
                        f"{t}_rows1": crd.contrast.memory_v1[index].clone(), f"{t}_rows2": crd.contrast.memory_v2[index].clone()})
        # ---- MIA 2022: CRD_criterion_v3.CRDLoss
        _use("mia2022")
        with _quiet():
            v3 = importlib.import_module("CL_utils.CRD_criterion_v3")
            crd = v3.CRDLoss(opt1, N_DATA)
        _load(crd, D, (30, 31, 41, 42))
        g = torch.Generator().manual_seed(80 + D)
        for it in range(2):
            f_s, f_t, index, sidx = _batch(g, K1 + 1)
            w = 0.3 + 0.1 * it
            with _quiet():
                loss = crd(w, f_s, f_t, index, sidx)
            gs = torch.autograd.grad(loss.sum(), [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight])
            t = f"v3{D}_{it}"
            rec.update({f"{t}_f_s": f_s, f"{t}_f_t": f_t, f"{t}_index": index, f"{t}_sidx": sidx, f"{t}_w": w, f"{t}_loss": loss,
                        f"{t}_g_fs": gs[0], f"{t}_g_ws": gs[1], f"{t}_g_wt": gs[2], f"{t}_params": crd.contrast.params.clone(),
                        f"{t}_rows1": crd.contrast.memory_v1[index].clone()})
        # ---- MIA 2023: CRD_criterion_v10.CRDLoss, neighbors
        _use("mia2023")
        opt10 = types.SimpleNamespace(s_dim=SDIM, t_dim=SDIM, feat_dim=D, nce_k=K1, nce_t=0.07, nce_m=0.5, nce_p=NP, pos_extra="neighbors")
        with _quiet():
            v10 = importlib.import_module("CL_utils.CRD_criterion_v10")
            crd = v10.CRDLoss(opt10, N_DATA, class_idx)
        _load(crd, D, (50, 51, 61, 62))
        g = torch.Generator().manual_seed(81 + D)
        for it in range(2):
            f_s, f_t, index, sidx = _batch(g, K1 + 1)
            grade = labels[index]
            w = (1 + torch.rand(B, generator=g)).view(-1, 1)
            with _quiet():
                loss, sample_loss = crd(w, f_s, f_t, grade, index, sidx)
            gs = torch.autograd.grad(loss, [f_s, crd.embed_s.linear.weight, crd.embed_t.linear.weight], retain_graph=True)
            t = f"v10{D}_{it}"
            rec.update({f"{t}_f_s": f_s, f"{t}_f_t": f_t, f"{t}_index": index, f"{t}_sidx": sidx, f"{t}_grade": grade, f"{t}_w": w,
                        f"{t}_loss": loss, f"{t}_sample_loss": sample_loss, f"{t}_g_fs": gs[0], f"{t}_g_ws": gs[1], f"{t}_g_wt": gs[2],
                        f"{t}_params": crd.contrast.params.clone(), f"{t}_rows1": crd.contrast.memory_v1[index].clone()})
    for k in [k for k in rec if k.endswith(("_0_g_ws", "_0_g_wt", "_0_g_w0"))]:      # full weight gradients: of the second call only
        del rec[k]
    np.savez_compressed(os.path.join(HERE, "crd_width.npz"), **npz(rec))
    print("wrote crd_width.npz")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the relational distiller-zoo losses over a GLOBAL batch (more rows than one replica holds): the
reference's own RKDLoss, PKT and Similarity ("MIA 2022/distiller_zoo/RKD.py", "PKT.py", "SP.py", loaded from their files
as make_golden_zoo.py does) on randn.relu features of (Bg, D) = (192, 128), (256, 64), (512, 128).  Build container only.
Writes tests/golden/zoo_global_b<Bg>_d<D>.npz: the inputs, the three losses and their gradients with respect to f_s.

The inputs are rounded to fp16-representable values and stored as float16 (the reference runs on their exact float32
images), which keeps every file under 1 MiB; losses and gradients are the reference's float32 results."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
SHAPES = ((192, 128), (256, 64), (512, 128))


def main():
    from make_golden import npz
    from make_golden_zoo import load
    rkd, pkt, sp = load("RKD").RKDLoss(), load("PKT").PKT(), load("SP").Similarity()
    g = torch.Generator().manual_seed(29)
    for Bg, D in SHAPES:
        f_s16 = torch.randn(Bg, D, generator=g).relu_().half()
        f_t16 = torch.randn(Bg, D, generator=g).relu_().half()
        f_s, f_t = f_s16.float().requires_grad_(True), f_t16.float()
        rec = {"f_s": f_s16, "f_t": f_t16}
        for name, crit in (("rkd", rkd), ("pkt", pkt), ("sp", sp)):
            l = crit(f_s, f_t)
            gr, = torch.autograd.grad(l.sum(), f_s)
            rec[name] = l.detach().reshape(-1)[0]
            rec[name + "_g"] = gr
        path = os.path.join(HERE, "zoo_global_b%d_d%d.npz" % (Bg, D))
        np.savez_compressed(path, **npz(rec))
        print("wrote", os.path.basename(path), os.path.getsize(path), {k: float(rec[k]) for k in ("rkd", "pkt", "sp")})


if __name__ == "__main__":
    main()

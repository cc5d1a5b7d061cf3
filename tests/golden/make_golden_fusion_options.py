#!/usr/bin/env python3
"""Golden vectors for the fusion heads over their option set (skip, use_bilinear, gate1, gate2, scale_dim1, scale_dim2),
produced by importing and RUNNING the reference's own classes on the CPU: BilinearFusion of MICCAI-2022/fusion.py and
PolynomialFusion of "MIA 2023/stage2_unimodal_student/fusion.py".  Nothing is transcribed.  dropout_rate 0, train mode,
B = 4, weights from the seed recipe of oracle.weights.make_state_dict over the module's own state_dict shapes.

Per case: the output, loss = sum(out * r) for a fixed random r, both input gradients, every parameter gradient, the names
of the parameters whose .grad stays None, the state_dict key -> shape list, and the reference's own float32-vs-float64
distance of every recorded quantity (the same module in double on the same weights).  A committed file may hold 1 MiB, so
a gradient above 4096 elements is stored as a 1024-element strided sample plus its float64 l2 norm.  The shapes the
reference itself cannot run are recorded with the exception type it raised.
Build container only.  Writes tests/golden/fusion_options.npz."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF_BF = "/root/reference/MICCAI-2022"
REF_PF = "/root/reference/MIA 2023/stage2_unimodal_student"

OPTS = ("skip", "use_bilinear", "gate1", "gate2", "scale_dim1", "scale_dim2")
BF_CASES = [(1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (0, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 0, 0, 0, 1, 1),
            (1, 1, 1, 1, 2, 4), (0, 0, 1, 1, 2, 4)]
PF_CASES = BF_CASES[:5] + [(0, 1, 1, 1, 1, 1)]
# (kind, options, width): the last one reaches the vector tails (Kronecker row 33 x 17 = 561 columns, skip row 114)
CASES = [("bf", c, 128) for c in BF_CASES] + [("pf", c, 128) for c in PF_CASES] + [("bf", (1, 1, 1, 1, 2, 4), 64)]
REFUSED = [("bf", (1, 1, 0, 1, 2, 1), 128),      # a gate off with that side's scale != 1
           ("pf", (1, 1, 1, 1, 2, 4), 128)]      # (dim1 + 1)(dim2 + 1) != (mmhid + 1)^2
SAMPLE_ABOVE, SAMPLE_N = 4096, 1024
WEIGHT_SEED, INPUT_SEED = 11, 12


def case_tag(kind, c, width):
    return "%s_%d%d%d%d_%dx%d_w%d" % ((kind,) + tuple(c) + (width,))


def sample(g):
    """A strided sample of SAMPLE_N elements of a flat tensor (the tests take the same one)."""
    stride = g.numel() // SAMPLE_N
    return g[::stride][:SAMPLE_N]


def load_class(ref_dir, name):
    """The class `name` of ref_dir/fusion.py, imported from where it lies (its `from utils import ..` resolves there)."""
    for m in ("utils", "fusion"):
        sys.modules.pop(m, None)
    sys.path.insert(0, ref_dir)
    try:
        spec = importlib.util.spec_from_file_location("fusion", os.path.join(ref_dir, "fusion.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ref_dir)
    return getattr(mod, name)


def inputs(width):
    g = torch.Generator().manual_seed(INPUT_SEED + width)
    return (torch.randn(4, width, generator=g), torch.randn(4, width, generator=g), torch.randn(4, width, generator=g))


def run(cls, c, width, dtype):
    from oracle import weights as W
    net = cls(dim1=width, dim2=width, mmhid=width, dropout_rate=0, **dict(zip(OPTS, c)))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(W.make_state_dict(shapes, WEIGHT_SEED))
    net = net.to(dtype).train()
    v1, v2, r = (t.to(dtype) for t in inputs(width))
    v1.requires_grad_(True); v2.requires_grad_(True)
    out = net(v1, v2)
    loss = (out * r).sum()
    loss.backward()
    q = dict(out=out.detach(), loss=loss.detach(), dv1=v1.grad, dv2=v2.grad)
    none = []
    for k, p in net.named_parameters():
        if p.grad is None:
            none.append(k)
            continue
        g = p.grad.reshape(-1)
        if g.numel() > SAMPLE_ABOVE:
            q["gs_" + k] = sample(g).clone()
            q["gn_" + k] = g.double().norm()
        else:
            q["g_" + k] = p.grad
    return q, none, shapes


def main():
    from make_golden import install_shims, npz
    install_shims()
    os.chdir(REF_BF)
    classes = dict(bf=load_class(REF_BF, "BilinearFusion"), pf=load_class(REF_PF, "PolynomialFusion"))
    rec, meta = {}, dict(cases=[], refused=[], sample_above=SAMPLE_ABOVE, sample_n=SAMPLE_N, weight_seed=WEIGHT_SEED)
    for width in sorted({w for _, _, w in CASES}):
        v1, v2, r = inputs(width)
        rec["in_w%d_v1" % width], rec["in_w%d_v2" % width], rec["in_w%d_r" % width] = v1, v2, r
    for kind, c, width in CASES:
        tag = case_tag(kind, c, width)
        q32, none, shapes = run(classes[kind], c, width, torch.float32)
        q64, none64, _ = run(classes[kind], c, width, torch.float64)
        assert none == none64
        dist = {}
        for k, v in q32.items():
            rec[tag + "|" + k] = v
            # the reference's own float32-vs-float64 distance: largest absolute difference (the gradient of a Linear bias in
            # front of a BatchNorm is exactly zero in exact arithmetic, so a relative figure would mean nothing there)
            dist[k] = float((v.double() - q64[k]).abs().max())
        meta["cases"].append(dict(tag=tag, kind=kind, width=width, opts=dict(zip(OPTS, c)), none_grads=none,
                                  shapes=[[k, list(s)] for k, s in shapes.items()], ref_f32_vs_f64=dist))
        print(tag, "loss %.6f" % float(q32["loss"]), "none:", none, "max f32-f64 %.2e" % max(dist.values()))
    for kind, c, width in REFUSED:
        try:
            run(classes[kind], c, width, torch.float32)
            raise AssertionError("the reference ran %s" % case_tag(kind, c, width))
        except Exception as e:      # noqa: BLE001 - the type is what is recorded
            if isinstance(e, AssertionError):
                raise
            meta["refused"].append(dict(kind=kind, width=width, opts=dict(zip(OPTS, c)), exc_type=type(e).__name__,
                                        message=str(e)))
            print("refused", case_tag(kind, c, width), type(e).__name__, str(e)[:80])
    rec["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "fusion_options.npz")
    np.savez_compressed(path, **npz(rec))
    print("wrote fusion_options.npz with", len(rec), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of a ResNet-34 trunk (BasicBlock, [3, 4, 6, 3]) by importing and RUNNING the reference's ``resnets.ResNet``
on the CPU, once in float32 and once as the same module in float64.

Runs only in the build container (needs /root/reference); the GPU box gets the committed ``tests/golden/resnet34_*.npz``.
Nothing from the reference is copied: its module is imported from where it lies (with the shims of make_golden.py), fed
weights from ``oracle.weights.make_state_dict`` over the module's own ``{key: shape}`` - no weights are stored, only the
ordered key list and the shapes - executed, and only input recipes + outputs are saved.

Two cases: B = 4 at 64 x 64 (the smallest square map: layer 4 is 2 x 2) and B = 3 at 96 x 160 (layer 4 is 3 x 5).
``oracle.step.synthetic_batch`` draws square images: the non-square case takes the top-left 96 x 160 window of its
160 x 160 batch (`crop_batch`, which the tests repeat).

Per case: the train-mode forward (f3, features, hazard, pred), the gradients of the loss of tests/test_gpu_resnet.py
(test_student_forward_backward_parity_mode) that test stores for ResNet-18 plus one middle identity block per layer, the f3 source
and the last convolution; the running statistics of bn1 and the last BatchNorm after that step; then an eval-mode forward
and the eval-mode gradient of the NLL with respect to the image.  Weight gradients above 40 000 elements go in as sum and
abs-sum.  The float64 run stores arrays up to 10 000 elements in full under ``<key>__f64``; of a larger array it stores what
the tests need from it - ``<key>__f64err`` = max |float32 run - float64 run| and ``<key>__f64absmax`` - so that each file stays
in the size class of modules_b4_h64.npz.

Usage:  python tests/golden/make_golden_resnet34.py      # writes tests/golden/resnet34_b4_h64.npz, resnet34_b3_96x160.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/MICCAI-2022"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

LAYERS = [3, 4, 6, 3]
WEIGHT_SEED = 41
CASES = (("resnet34_b4_h64.npz", 4, 64, 64, 7), ("resnet34_b3_96x160.npz", 3, 96, 160, 8))      # file, B, H, W, batch seed
BIG_GRAD = 40000      # weight gradients above this many elements: sum and abs-sum
FULL_F64 = 10000      # float64 arrays up to this many elements are stored in full

# state_dict key -> golden key: the ResNet-18 test's set at the matching places, then the ResNet-34 additions
GRADS = (("fc_new2.weight", "g_fc2_w"), ("fc_new1.0.weight", "g_fc1_w"), ("layer4.2.bn2.weight", "g_l4_2_bn2_w"),
         ("layer3.1.conv2.weight", "g_l3_1_conv2"), ("layer2.0.downsample.0.weight", "g_l2_0_ds"),
         ("layer1.0.conv1.weight", "g_l1_0_conv1"), ("bn1.weight", "g_bn1_w"), ("conv1.weight", "g_conv1"),
         ("layer1.2.conv1.weight", "g_l1_2_conv1"), ("layer2.3.bn2.weight", "g_l2_3_bn2_w"),
         ("layer3.4.conv1.weight", "g_l3_4_conv1"), ("layer3.5.bn2.weight", "g_l3_5_bn2_w"),
         ("layer3.5.bn2.bias", "g_l3_5_bn2_b"), ("layer4.2.conv2.weight", "g_l4_2_conv2"))
ABS_ONLY = ("g_l4_2_conv2",)      # stored as sums whatever its size


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp (numpy stamps the members with the current time): the same arrays
    give the same bytes, so the committed files regenerate bit-identically."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def crop_batch(B, H, W, seed):
    from oracle.step import synthetic_batch
    bt = synthetic_batch(B, max(H, W), seed=seed)
    return bt["x_path"][:, :, :H, :W].contiguous(), bt["grade"]


def run(net, x, grade, dtype):
    """One train step's forward / backward, then the eval-mode forward and image gradient; everything as `dtype`."""
    out = {}
    net.train()
    f3, feat, hazard, pred, _ = net(x_path=x)
    loss = (feat * torch.linspace(0.5, 1.5, 128, dtype=dtype)).sum() + (hazard * torch.tensor([1.0, -2.0, 0.5], dtype=dtype)).sum() \
        + 0.1 * f3.sum()
    loss.backward()
    out.update(f3=f3, feat=feat, hazard=hazard, pred=pred)
    P = dict(net.named_parameters())
    for key, name in GRADS:
        g = P[key].grad
        if name in ABS_ONLY or g.numel() > BIG_GRAD:
            out[name + "_sum"], out[name + "_abs"] = g.sum(), g.abs().sum()
        else:
            out[name] = g
    sd = net.state_dict()
    out.update(rm_bn1=sd["bn1.running_mean"].clone(), rv_bn1=sd["bn1.running_var"].clone(),
               rm_l4=sd["layer4.2.bn2.running_mean"].clone(), rv_l4=sd["layer4.2.bn2.running_var"].clone())
    net.eval()
    xg = x.clone().requires_grad_(True)
    e = net(x_path=xg)
    nll = torch.nn.functional.nll_loss(e[3], grade)
    dx, = torch.autograd.grad(nll, xg)
    out.update(eval_f3=e[0], eval_feat=e[1], eval_hazard=e[2], eval_pred=e[3], eval_nll=nll, eval_dx=dx)
    return {k: v.detach() for k, v in out.items()}


def main():
    from make_golden import install_shims
    install_shims()
    sys.path.insert(0, REF)
    import resnets as R
    from oracle import weights as W

    def build():
        torch.manual_seed(0)
        return R.ResNet(R.BasicBlock, LAYERS, path_dim=128, act=torch.nn.LogSoftmax(dim=1), num_classes=3)

    shapes = {k: tuple(v.shape) for k, v in build().state_dict().items()}
    keys = list(shapes)
    assert "layer3.5.bn2.weight" in shapes and "layer4.2.conv2.weight" in shapes and "layer1.3.conv1.weight" not in shapes
    for fname, B, H, Wd, bseed in CASES:
        x, grade = crop_batch(B, H, Wd, bseed)
        rec = dict(B=B, H=H, W=Wd, batch_seed=bseed, weight_seed=WEIGHT_SEED, layers=np.asarray(LAYERS),
                   keys=np.asarray(keys), shapes=np.asarray([",".join(str(d) for d in shapes[k]) for k in keys]))
        res = {}
        for dtype in (torch.float32, torch.float64):
            net = build()
            net.load_state_dict(W.make_state_dict(shapes, WEIGHT_SEED))
            if dtype == torch.float64:
                net = net.double()
            res[dtype] = run(net, x.to(dtype), grade, dtype)
        for k, v in res[torch.float32].items():
            rec[k] = v.numpy()
            v64 = res[torch.float64][k]
            if v64.numel() <= FULL_F64:
                rec[k + "__f64"] = v64.numpy()
            else:
                rec[k + "__f64err"] = (v.double() - v64).abs().max().numpy()
                rec[k + "__f64absmax"] = v64.abs().max().numpy()
        path = os.path.join(HERE, fname)
        save_npz(path, rec)
        print(fname, os.path.getsize(path), "bytes;", "f3 f32-f64 %.2e" % np.abs(rec["f3"] - rec["f3__f64"]).max(),
              "hazard %.2e" % np.abs(rec["hazard"] - rec["hazard__f64"]).max())


if __name__ == "__main__":
    main()

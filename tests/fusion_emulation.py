"""A restatement of the two fusion heads (BilinearFusion, PolynomialFusion) over their whole option set, forward and
backward, written from the formulas and independent of the package: plain torch tensor algebra on the CPU, float64 by
default.  The float32 form follows the kernels' grouping where it matters: a Linear over 4096 or more columns is summed
in the split-K order of ops.linear_fwd / ph_sgemm_splitk (slabs of K, four interleaved running sums over the slabs,
(p0 + p1) + (p2 + p3), then the bias), and the linear maps over a concatenation are sums over column blocks.

TEST INFRASTRUCTURE: the reference values of tests/test_fusion_options_cpu.py and tests/test_gpu_fusion_options.py.
`defect` injects one deliberate mistake, for the tests that check that the comparison can fail."""
import torch

OPTS = ("skip", "use_bilinear", "gate1", "gate2", "scale_dim1", "scale_dim2")
DEFECTS = ("skip_order", "no_one", "gate_off_gated", "z_v1_only", "kron2_no_one")
GK = 32      # K step of the split-K kernel: a slab is a multiple of it


def _linear(x, w, b, splitk):
    """x @ w^T + b; in the kernels' split-K grouping when `splitk` and the shape takes that path."""
    Bn, K = x.shape
    N = w.shape[0]
    if not (splitk and K >= 4096 and Bn * N <= 256 * 256):
        return x @ w.t() + b
    nsplit = 128 if K >= 8192 else 32
    kchunk = -(-(-(-K // nsplit)) // GK) * GK
    nsplit = -(-K // kchunk)
    part = [x[:, s * kchunk:(s + 1) * kchunk] @ w[:, s * kchunk:(s + 1) * kchunk].t() for s in range(nsplit)]
    p = []
    for q in range(4):
        acc = torch.zeros_like(part[0])
        for s in range(q, nsplit, 4):
            acc = acc + part[s]
        p.append(acc)
    return b + ((p[0] + p[1]) + (p[2] + p[3]))


def _cat_linear(blocks, w, b):
    """(x_0 | x_1 | ..) @ w^T + b as the sum over column blocks of w, the first block carrying the bias."""
    y, off = None, 0
    for x in blocks:
        t = x @ w[:, off:off + x.shape[1]].t()
        y = t + b if y is None else y + t
        off += x.shape[1]
    assert off == w.shape[1], (off, w.shape)
    return y


def _bn_relu(x, g, b, eps=1e-5):
    """BatchNorm1d with the batch's statistics (biased variance), then ReLU"""
    m = x.mean(0, keepdim=True)
    v = ((x - m) ** 2).mean(0, keepdim=True)
    return torch.relu((x - m) / torch.sqrt(v + eps) * g + b)


def _kron(a, b):
    return (a.unsqueeze(2) * b.unsqueeze(1)).flatten(1)


def forward(kind, opts, P, vec1, vec2, splitk=False, defect=None):
    """kind 'bf' | 'pf'; opts: dict over OPTS; P: name -> tensor (the state_dict's parameter names); train mode, dropout 0."""
    skip, ub, g1, g2 = opts["skip"], opts["use_bilinear"], opts["gate1"], opts["gate2"]
    v1, v2 = torch.relu(vec1), torch.relu(vec2)
    one = torch.ones(v1.shape[0], 1, dtype=v1.dtype)

    def unit(k, gate, v):
        if gate or defect == "gate_off_gated":
            h = torch.relu(v @ P["linear_h%d.0.weight" % k].t() + P["linear_h%d.0.bias" % k])
            if ub:
                wz = P["linear_z%d.weight" % k]
                z = _linear(_kron(v1, v2), wz.reshape(wz.shape[0], -1), P["linear_z%d.bias" % k], splitk)
            else:
                zin = [v1, torch.zeros_like(v2)] if defect == "z_v1_only" else [v1, v2]
                z = _cat_linear(zin, P["linear_z%d.0.weight" % k], P["linear_z%d.0.bias" % k])
            v = torch.sigmoid(z) * h
        return torch.relu(v @ P["linear_o%d.0.weight" % k].t() + P["linear_o%d.0.bias" % k])

    def encode(name, x):
        w, b = P[name + ".0.weight"], P[name + ".0.bias"]
        y = _cat_linear(x, w, b) if isinstance(x, list) else _linear(x, w, b, splitk)
        return _bn_relu(y, P[name + ".1.weight"], P[name + ".1.bias"])

    o1, o2 = unit(1, g1, v1), unit(2, g2, v2)
    e1 = torch.cat((o1, one if defect != "no_one" else 0 * one), 1)
    e2 = torch.cat((o2, one), 1)
    tail = ([e2, e1] if defect == "skip_order" else [e1, e2]) if skip else None
    out = encode("encoder1", _kron(e1, e2))
    last = "encoder2"
    if kind == "pf":
        e12 = torch.cat((out, one if defect != "kron2_no_one" else 0 * one), 1)
        out = encode("encoder2", _kron(e12, e12))
        last = "encoder3"
    return encode(last, [out] + tail if skip else out)


def run_case(kind, opts, state_dict, vec1, vec2, r, dtype=torch.float64, splitk=False, defect=None):
    """Forward and backward of loss = sum(out * r).  Returns dict(out, loss, dv1, dv2, grads: name -> tensor or None)."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state_dict.items()
         if v.is_floating_point() and "running_" not in k}
    v1 = vec1.detach().to(dtype).clone().requires_grad_(True)
    v2 = vec2.detach().to(dtype).clone().requires_grad_(True)
    out = forward(kind, opts, P, v1, v2, splitk=splitk, defect=defect)
    loss = (out * r.to(dtype)).sum()
    loss.backward()
    return dict(out=out.detach(), loss=loss.detach(), dv1=v1.grad, dv2=v2.grad, grads={k: p.grad for k, p in P.items()})


def sample(g, n):
    """The strided n-element sample of a flat tensor that the golden generator stores for the large gradients."""
    g = g.reshape(-1)
    return g[::g.numel() // n][:n]


def quantities(res, sample_above, sample_n):
    """The recorded quantities of a result, under the fixture's names: out, loss, dv1, dv2, g_<name> for a gradient of at
    most `sample_above` elements, gs_<name> (sample) and gn_<name> (float64 l2 norm) above."""
    q = dict(out=res["out"], loss=res["loss"], dv1=res["dv1"], dv2=res["dv2"])
    for k, g in res["grads"].items():
        if g is None:
            continue
        if g.numel() > sample_above:
            q["gs_" + k] = sample(g, sample_n)
            q["gn_" + k] = g.double().norm()
        else:
            q["g_" + k] = g
    return q

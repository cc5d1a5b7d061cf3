"""Drop-ins for the reference's fusion heads: BilinearFusion (MICCAI-2022/fusion.py:6-63) and PolynomialFusion
("MIA 2023/stage2_unimodal_student/fusion.py":6-74).  Same constructors, parameter names and
forward(vec1, vec2) -> [B, mmhid] for the whole option set (skip, use_bilinear, gate1, gate2, scale_dim1, scale_dim2); the
arithmetic runs through the C-ABI dense kernels.  The Kronecker product o1 (x) o2 is formed by ``ph_outer`` and contracted
by a split-K SGEMM; the concatenations of the skip connection and of the linear gate are never formed (ops.cat_linear: a
sum of GEMMs over column blocks of the weight).

The frozen stage-2 teacher (train_test_path_multi_distill.py:170-173) runs the fused forward-only calls; when a gradient
is required (stage-1 teacher training, row f-1) the same arithmetic runs taped through ops.*Fn.  Both forms walk ONE
description of the data flow (`_gated_pair`, `_encode`), so they share the dropout call sites and offsets.
"""
import torch
import torch.nn as nn

from . import ops
from .utils import init_max_weights


class _FwdOnly:
    """The fused forward-only calls."""
    relu = staticmethod(lambda x: ops.eltwise(x, None, ops.EW_RELU))
    outer = staticmethod(ops.outer)
    linear = staticmethod(ops.linear_fwd)
    linear_relu = staticmethod(lambda x, w, b: ops.linear_fwd(x, w, b, ops.ACT_RELU))
    gate = staticmethod(lambda z, h: ops.eltwise(z, h, ops.EW_GATE))
    cat_linear = staticmethod(ops.cat_linear_fwd)


class _Taped:
    """The same operators with a backward."""
    relu = staticmethod(lambda x: ops.ReluFn.apply(ops._f32(x)))
    outer = staticmethod(ops.OuterFn.apply)
    linear = staticmethod(ops.LinearFn.apply)
    linear_relu = staticmethod(lambda x, w, b: ops.LinearActFn.apply(x, w, b, ops.ACT_RELU))
    gate = staticmethod(ops.GateFn.apply)
    cat_linear = staticmethod(ops.cat_linear)


class _GatedFusion(nn.Module):
    """What both heads share: the two gated multimodal units, dropout bookkeeping, BatchNorm + ReLU."""

    def _build_units(self, skip, use_bilinear, gate1, gate2, dim1, dim2, scale_dim1, scale_dim2, dropout_rate):
        self.skip, self.use_bilinear, self.gate1, self.gate2 = skip, use_bilinear, gate1, gate2
        self.relu = nn.ReLU(inplace=False)
        dim1_og, dim2_og, dim1, dim2 = dim1, dim2, dim1 // scale_dim1, dim2 // scale_dim2
        # a gate that is off applies linear_o_k = Linear(dim_k, dim_k) to the dim_k_og-wide input (fusion.py:46,53): the
        # reference fails at its first forward with a RuntimeError (shapes cannot be multiplied); here at construction
        for k, gate, d, d_og in ((1, gate1, dim1, dim1_og), (2, gate2, dim2, dim2_og)):
            if not gate and d != d_og:
                raise RuntimeError("gate%d = 0 with scale_dim%d != 1: linear_o%d is Linear(%d, %d) and would be applied to "
                                   "the %d-wide input (mat1 and mat2 shapes cannot be multiplied)" % (k, k, k, d, d, d_og))
        self.linear_h1 = nn.Sequential(nn.Linear(dim1_og, dim1), nn.ReLU())
        self.linear_z1 = nn.Bilinear(dim1_og, dim2_og, dim1) if use_bilinear else nn.Sequential(nn.Linear(dim1_og + dim2_og, dim1))
        self.linear_o1 = nn.Sequential(nn.Linear(dim1, dim1), nn.ReLU(), nn.Dropout(p=dropout_rate))
        self.linear_h2 = nn.Sequential(nn.Linear(dim2_og, dim2), nn.ReLU())
        self.linear_z2 = nn.Bilinear(dim1_og, dim2_og, dim2) if use_bilinear else nn.Sequential(nn.Linear(dim1_og + dim2_og, dim2))
        self.linear_o2 = nn.Sequential(nn.Linear(dim2, dim2), nn.ReLU(), nn.Dropout(p=dropout_rate))
        self.post_fusion_dropout = nn.Dropout(p=dropout_rate)
        return dim1, dim2

    def _finish_init(self, dropout_rate):
        self.dropout_rate = dropout_rate
        self._rng_offset = 0
        self.rng_seed = 0x5EED
        self.register_buffer("rng_step", torch.zeros(1, dtype=torch.int64), persistent=False)
        init_max_weights(self)

    def unused_parameters(self):
        """The parameters no forward reads: linear_h_k and linear_z_k of a gate that is off.  They stay in the state_dict
        and in the optimiser's list as in the reference, where their .grad stays None."""
        mods = ([self.linear_h1, self.linear_z1] if not self.gate1 else []) + \
               ([self.linear_h2, self.linear_z2] if not self.gate2 else [])
        return [p for m_ in mods for p in m_.parameters()]

    def _drop(self, x):
        if self.training and self.dropout_rate > 0:
            ops.dropout_(x, self.dropout_rate, self.rng_seed, self._rng_offset, self.rng_step, alpha=False)
            self._rng_offset += x.numel()
        return x

    # ---- taped form of the same dropout (same call sites and offsets, so both paths draw the same masks)
    def _drop_ag(self, x):
        if self.training and self.dropout_rate > 0:
            x = ops.DropoutFn.apply(x, self.dropout_rate, self.rng_seed, self._rng_offset, self.rng_step, False)
            self._rng_offset += x.numel()
        return x

    def _bn_relu(self, x, bn):
        if not self.training:
            if torch.is_grad_enabled() and x.requires_grad:
                return ops.BN1dEvalFn.apply(x, bn, True)      # a gradient flows through the eval-mode net to its inputs
            return ops.bn1d_eval(x, bn, relu=True)
        return ops.BN1dFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                True, True)

    def _unit(self, F, drop, k, v, v1, v2, v12):
        """o_k: the gated unit of modality k (fusion.py:41-53), or Linear-ReLU-Dropout of its input when the gate is off."""
        if (self.gate1, self.gate2)[k - 1]:
            lin_h, lin_z = getattr(self, "linear_h%d" % k)[0], getattr(self, "linear_z%d" % k)
            h = F.linear_relu(v, lin_h.weight, lin_h.bias)
            if self.use_bilinear:
                z = F.linear(v12, lin_z.weight.view(lin_z.weight.shape[0], -1), lin_z.bias)
            else:
                z = F.cat_linear([(v1, False), (v2, False)], lin_z[0].weight, lin_z[0].bias)
            v = F.gate(z, h)
        lin_o = getattr(self, "linear_o%d" % k)[0]
        return drop(F.linear_relu(v, lin_o.weight, lin_o.bias))

    def _gated_pair(self, F, drop, vec1, vec2):
        v1 = F.relu(vec1)                                                           # fusion.py:38-39
        v2 = F.relu(vec2)
        # the nn.Bilinear operand, only when a bilinear gate reads it
        v12 = F.outer(v1, v2, 0) if self.use_bilinear and (self.gate1 or self.gate2) else None
        o1 = self._unit(F, drop, 1, v1, v1, v2, v12)
        o2 = self._unit(F, drop, 2, v2, v1, v2, v12)
        return o1, o2

    def _encode(self, F, drop, enc, x):
        """Linear - BatchNorm1d - ReLU - Dropout over x; a list x = [(block, one_follows), ..] stands for the concatenation."""
        if isinstance(x, list):
            out = F.cat_linear(x, enc[0].weight, enc[0].bias)
        else:
            out = F.linear(x, enc[0].weight, enc[0].bias)
        return drop(self._bn_relu(out, enc[1]))

    def _skip_blocks(self, out, o1, o2):
        """cat(out, o1e, o2e) of fusion.py:61: o1e / o2e are the rows with the appended 1 that ph_outer(.., 1) consumes."""
        return [(out, False), (o1, True), (o2, True)] if self.skip else out

    def forward(self, vec1, vec2):
        if torch.is_grad_enabled() and (vec1.requires_grad or vec2.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            return self._forward_autograd(vec1, vec2)     # stage-1 teacher training (row f-1)
        return self._run(_FwdOnly, self._drop, vec1, vec2)

    def _forward_autograd(self, vec1, vec2):
        return self._run(_Taped, self._drop_ag, vec1, vec2)

    def _run(self, F, drop, vec1, vec2):
        self._rng_offset = 0     # per-call-site offsets are static; the device step counter makes steps differ
        out = self._fuse(F, drop, vec1, vec2)
        if self.training and self.dropout_rate > 0:
            ops.counter_inc(self.rng_step)
        return out


class BilinearFusion(_GatedFusion):
    def __init__(self, skip=1, use_bilinear=1, gate1=1, gate2=1, dim1=32, dim2=32, scale_dim1=1, scale_dim2=1,
                 mmhid=64, dropout_rate=0.25):
        super().__init__()
        dim1, dim2 = self._build_units(skip, use_bilinear, gate1, gate2, dim1, dim2, scale_dim1, scale_dim2, dropout_rate)
        skip_dim = dim1 + dim2 + 2 if skip else 0
        self.encoder1 = nn.Sequential(nn.Linear((dim1 + 1) * (dim2 + 1), mmhid), nn.BatchNorm1d(mmhid), nn.ReLU(),
                                      nn.Dropout(p=dropout_rate))
        self.encoder2 = nn.Sequential(nn.Linear(mmhid + skip_dim, mmhid), nn.BatchNorm1d(mmhid), nn.ReLU(),
                                      nn.Dropout(p=dropout_rate))
        self._finish_init(dropout_rate)

    def _fuse(self, F, drop, vec1, vec2):
        o1, o2 = self._gated_pair(F, drop, vec1, vec2)
        o12 = drop(F.outer(o1, o2, 1))                                              # fusion.py:56-59
        out = self._encode(F, drop, self.encoder1, o12)
        return self._encode(F, drop, self.encoder2, self._skip_blocks(out, o1, o2))


class PolynomialFusion(_GatedFusion):
    """The fourth-order head of the MIA-2023 tree: out12 = encoder1(o1e (x) o2e), then out12e (x) out12e into encoder2, and
    an encoder3 that takes the skip connection."""

    def __init__(self, skip=1, use_bilinear=1, gate1=1, gate2=1, dim1=32, dim2=32, scale_dim1=1, scale_dim2=1,
                 mmhid=64, dropout_rate=0.25):
        super().__init__()
        dim1, dim2 = self._build_units(skip, use_bilinear, gate1, gate2, dim1, dim2, scale_dim1, scale_dim2, dropout_rate)
        # encoder2 is declared over (dim1 + 1)(dim2 + 1) columns and fed (mmhid + 1)^2 (fusion.py:31,66-68): where the two
        # differ the reference fails at its first forward with a RuntimeError; here at construction
        if (dim1 + 1) * (dim2 + 1) != (mmhid + 1) ** 2:
            raise RuntimeError("PolynomialFusion: encoder2 is Linear((dim1 + 1)(dim2 + 1) = %d, mmhid) and is fed the "
                               "(mmhid + 1)^2 = %d columns of out12 (x) out12 (mat1 and mat2 shapes cannot be multiplied)"
                               % ((dim1 + 1) * (dim2 + 1), (mmhid + 1) ** 2))
        skip_dim = dim1 + dim2 + 2 if skip else 0
        self.encoder1 = nn.Sequential(nn.Linear((dim1 + 1) * (dim2 + 1), mmhid), nn.BatchNorm1d(mmhid), nn.ReLU(),
                                      nn.Dropout(p=dropout_rate))
        self.encoder2 = nn.Sequential(nn.Linear((dim1 + 1) * (dim2 + 1), mmhid), nn.BatchNorm1d(mmhid), nn.ReLU(),
                                      nn.Dropout(p=dropout_rate))
        self.encoder3 = nn.Sequential(nn.Linear(mmhid + skip_dim, mmhid), nn.BatchNorm1d(mmhid), nn.ReLU(),
                                      nn.Dropout(p=dropout_rate))
        self._finish_init(dropout_rate)

    def _fuse(self, F, drop, vec1, vec2):
        o1, o2 = self._gated_pair(F, drop, vec1, vec2)
        o12 = drop(F.outer(o1, o2, 1))                                              # fusion.py:61-62
        out12 = self._encode(F, drop, self.encoder1, o12)
        # the second Kronecker step (:65-67); taped, both operand gradients of ph_outer_bwd add up in out12
        o1212 = drop(F.outer(out12, out12, 1))
        out = self._encode(F, drop, self.encoder2, o1212)
        return self._encode(F, drop, self.encoder3, self._skip_blocks(out, o1, o2))

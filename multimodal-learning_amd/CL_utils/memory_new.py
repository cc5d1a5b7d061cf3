"""Drop-in for the reference's CL_utils/memory_new.py ContrastMemory_v3 (:225-397): same buffers
(`params` [K,T,Z_v1,Z_v2,momentum,P], `memory_v1`, `memory_v2`), same forward semantics
(score with the PRE-update bank, discrepancy-driven positive/negative selection, first-call Z,
momentum update).  The forward returns (out_v1, out_v2) like the reference when called directly; inside
CRDLoss the fused loss+gradient kernel is used instead (nothing [B,P+K,128]-sized is materialised).

Also the home of what every CRD criterion of the package shares: `ContrastBank`, the base of the
memory modules; `CrdCall`, what one call consists of; `crd_core`, the fused step over a bank and a call.
`ContrastMemory_v4` and `ContrastMemory_mono` at the end of the file are the banks of the MIA-2022 tree's DSCD criteria
("MIA 2022/CL_utils/memory_new.py":398-561 and :565-698; CL_utils/CRD_loss_v2.py)."""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .._lib import lib, check, ptr, stream, require_cuda


FEAT_DIMS = (64, 128, 256)      # the row widths the bank kernels are built for (csrc/crd.hip)


def check_feat_dim(feat_dim, what="feat_dim"):
    """The criteria call this at construction: a width the kernels refuse (PH_EINVAL) fails here, by name."""
    if feat_dim not in FEAT_DIMS:
        raise ValueError("%s %r: the CRD bank kernels are built for the widths %s" % (what, feat_dim, list(FEAT_DIMS)))
    return int(feat_dim)


class CrdCall:
    """What one CRD call consists of, beside the bank and the two embeddings (plain container; crd_core has no other input).
    `P` positive + `K` negative columns per sample, of which `P2` + `K2` enter the loss (`select_pos` / `select_neg`: by their
    rank in the score discrepancy, positives at `ranks` [P2] int32 or, None, the hardest; off: the first P2 / K2);
    `idx` [B, P + K] int64: the columns as rows of bank 1, and of bank 2 unless `idx_bank2` (same shape) names other rows;
    `posw_s` / `posw_t` [B, P] float32: weights of the positives in the student's / the teacher's term (None: 1 / P2 each);
    `scan`: None, or dict(idx [B, >= col0 + K] int64, col0, K) - the bank-scan form, the K negatives are columns
    col0 .. col0 + K of that tensor and `idx` / `idx_bank2` hold the P positives alone; `per_sample`: the [B] losses, not
    their sum.
    The DSCD criteria of the MIA-2022 tree: `rank_ascending` None = the selection above; True / False =
    ph_crd_select_dscd - the P positives ranked by the discrepancy ascending (ContrastMemory_v4) or descending
    (ContrastMemory_mono), every one of the K negatives kept (K2 == K); `neg_reweight`: their scores times 1 + discrepancy;
    `one_direction`: only out_v2 / Z_v2 / d loss / d v2 exist (ContrastMemory_mono)."""
    __slots__ = ("P", "K", "P2", "K2", "select_pos", "select_neg", "idx", "idx_bank2", "posw_s", "posw_t", "scan", "ranks",
                 "per_sample", "rank_ascending", "neg_reweight", "one_direction")

    def __init__(self, P, K, P2, K2, idx, select_pos=False, select_neg=False, idx_bank2=None, posw_s=None, posw_t=None,
                 scan=None, ranks=None, per_sample=False, rank_ascending=None, neg_reweight=False, one_direction=False):
        self.P, self.K, self.P2, self.K2 = int(P), int(K), int(P2), int(K2)
        self.rank_ascending = None if rank_ascending is None else bool(rank_ascending)
        self.neg_reweight, self.one_direction = bool(neg_reweight), bool(one_direction)
        if self.rank_ascending is None and (self.neg_reweight or self.one_direction):
            raise ValueError("CrdCall: neg_reweight / one_direction belong to the DSCD selection (rank_ascending True or False)")
        if self.rank_ascending is not None and (self.K2 != self.K or scan is not None or idx_bank2 is not None):
            raise ValueError("CrdCall: the DSCD selection keeps every negative (K2 == K) of one gathered index list")
        self.select_pos, self.select_neg = bool(select_pos), bool(select_neg)
        self.idx, self.idx_bank2, self.posw_s, self.posw_t = idx, idx_bank2, posw_s, posw_t
        self.scan, self.ranks, self.per_sample = scan, ranks, bool(per_sample)
        width = self.P if scan is not None else self.P + self.K
        if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[1] != width:
            raise ValueError("CrdCall.idx must be int64 [B, %d] (%s), got %s" % (
                width, "P: the positives of the bank-scan form" if scan is not None else "P + K",
                tuple(idx.shape) if torch.is_tensor(idx) else type(idx).__name__))
        B = idx.shape[0]
        if idx_bank2 is not None and (idx_bank2.dtype != torch.int64 or idx_bank2.shape != idx.shape):
            raise ValueError("CrdCall.idx_bank2 must be int64 %s like idx, got %s" % (tuple(idx.shape), tuple(idx_bank2.shape)))
        for name, w in (("posw_s", posw_s), ("posw_t", posw_t)):
            if w is not None and (w.dtype != torch.float32 or tuple(w.shape) != (B, self.P)):
                raise ValueError("CrdCall.%s must be float32 [B, P] = %s, got %s" % (name, (B, self.P), tuple(w.shape)))
        if scan is not None:
            neg, col0 = scan["idx"], int(scan["col0"])
            if int(scan["K"]) != self.K:
                raise ValueError("CrdCall.scan: K %d of the sampled negatives against K %d of the call" % (int(scan["K"]), self.K))
            if neg.dtype != torch.int64 or neg.dim() != 2 or neg.shape[0] != B or neg.shape[1] < col0 + self.K or neg.stride(1) != 1:
                raise ValueError("CrdCall.scan: the sampled negatives must be int64 [B, >= %d] with unit column stride"
                                 % (col0 + self.K))
            if self.select_pos or self.select_neg:
                raise NotImplementedError("bank-scan form with a ranked pair selection (it needs the per-column score list)")


def _checked(call, y, B):
    """The call's columns and the batch's bank rows as the kernels read them: on the device, contiguous, one row per sample."""
    idx = require_cuda(call.idx).contiguous()
    y = require_cuda(y).contiguous()
    if y.dtype != torch.int64 or idx.shape[0] != B:
        raise RuntimeError("contrast_idx must be int64 [B, nce_p+nce_k] and idx int64 [B]")
    return idx, y


def _set_z_once(mem, sums, count):
    """The first call of a bank: Z_v1, Z_v2 from the score sums `sums` over `count` scores (memory_new.py:368-379), summed
    over the replicas under data parallelism."""
    if mem.sync is not None:
        count = mem.sync.all_reduce_z(sums, count)
    check(lib().ph_crd_setz(ptr(mem.params), ptr(sums), count, float(mem.nLem), stream()), "ph_crd_setz")
    mem._z_set = True
    if mem.verbose:   # the reference prints Z once (memory_new.py:371,375); costs one host sync
        z = mem.params[2:4].tolist()
        if not mem.one_direction:      # (ContrastMemory_mono has Z_v2 alone, "MIA 2022/CL_utils/memory_new.py":674-677)
            print("normalization constant Z_v1 is set to {:.1f}".format(z[0]))
        print("normalization constant Z_v2 is set to {:.1f}".format(z[1]))


def _loss_divisor(mem, B):
    """What the rows' losses are divided by: the (global) batch size, or nothing in ContrastLoss_v2's per-sample branch
    (CRD_loss.py:246-250)."""
    return 1.0 if mem.sample_KD else float(mem.batch_norm_size or B)


def _finish_loss(lossp, per_sample, loss_out):
    """The [B] per-sample losses (each already divided by the batch normaliser), or their sum into `loss_out` (or a new 0-d)."""
    if per_sample:
        return lossp
    loss = loss_out if loss_out is not None else torch.empty((), device=lossp.device, dtype=torch.float32)
    check(lib().ph_sum(ptr(lossp), ptr(loss), lossp.shape[0], 1.0, stream()), "ph_sum")
    return loss


def crd_core(v1, v2, mem, y, call, loss_out=None, outputs_only=False):
    """The fused CRD step on normalised embeddings: scores against the PRE-update banks, pair selection, first-call Z,
    NCE loss, analytic gradients, bank momentum update.  `mem`: the bank (a ContrastBank), `y` [B] its rows of this batch,
    `call`: the CrdCall - everything else this call does; it is kept in `mem.last["call"]` until the next one.  Returns
    (loss, dv1, dv2) with dv = d loss / d v for a unit upstream gradient (call.per_sample: row b of dv belongs to loss[b]).
    `loss_out`: optional 0-d destination of the summed loss.  No autograd here: _CRDCoreFn wraps it, the fused loss head of
    DistillStep calls it directly.
    `outputs_only`: the standalone ContrastMemory_v3.forward - instead of the loss, return (out_v1, out_v2, rows1, rows2):
    the selected scores / Z [B, P2+K2] and the gathered pre-update bank rows its backward needs."""
    v1, v2 = ops._f32(v1), ops._f32(v2)
    if call.scan is not None:
        if outputs_only:
            raise NotImplementedError("the bank-scan form of the negatives has no [B, P+K] score tensor to return")
        return _crd_core_scan(v1, v2, mem, y, call, loss_out)
    B, D = v1.shape
    P, K, P2, K2 = call.P, call.K, call.P2, call.K2
    PK, S2 = P + K, P2 + K2
    dev = v1.device
    idx, y = _checked(call, y, B)
    out1 = torch.empty(B, PK, device=dev, dtype=torch.float32)
    out2 = torch.empty_like(out1)
    diff = torch.empty_like(out1)
    L = lib()
    st = stream()
    idx2 = call.idx_bank2                            # MIA-2023 v10: bank-specific positive rows
    check(L.ph_crd_score(ptr(v1), ptr(v2), ptr(idx), ptr(idx2), ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(out1),
                         ptr(out2), ptr(diff), B, PK, D, mem.T, st), "ph_crd_score")
    sel = torch.empty(B, S2, device=dev, dtype=torch.int32)
    xs = torch.empty(B, S2, device=dev, dtype=torch.float32)
    xt = torch.empty_like(xs)
    if call.rank_ascending is None:
        check(L.ph_crd_select(ptr(diff), ptr(out1), ptr(out2), ptr(call.ranks), ptr(sel), ptr(xs), ptr(xt), B, P, K, P2, K2,
                              int(call.select_neg), int(call.select_pos), st), "ph_crd_select")
    else:
        check(L.ph_crd_select_dscd(ptr(diff), ptr(out1), ptr(out2), ptr(call.ranks), ptr(sel), ptr(xs), ptr(xt), B, P, K, P2,
                                   int(call.rank_ascending), int(call.neg_reweight), st), "ph_crd_select_dscd")
    if not mem._z_set:
        sums = torch.empty(2, device=dev, dtype=torch.float32)
        check(L.ph_crd_zsum(ptr(xs), ptr(xt), ptr(sums), B * S2, st), "ph_crd_zsum")
        _set_z_once(mem, sums, float(B * S2))
    if outputs_only:
        o1 = torch.empty(B, S2, device=dev, dtype=torch.float32)
        o2 = torch.empty_like(o1)
        rows1 = torch.empty(B, S2, D, device=dev, dtype=torch.float32)
        rows2 = torch.empty_like(rows1)
        check(L.ph_crd_outputs(ptr(xs), ptr(xt), ptr(sel), ptr(idx), ptr(idx2), ptr(mem.memory_v1), ptr(mem.memory_v2),
                               ptr(mem.params), ptr(o1), ptr(o2), ptr(rows1), ptr(rows2), B, PK, S2, D, st), "ph_crd_outputs")
        result = (o1, o2, rows1, rows2)
    else:
        lossp = torch.empty(B, device=dev, dtype=torch.float32)
        dv2 = torch.empty(B, D, device=dev, dtype=torch.float32)
        dv1 = None if call.one_direction else torch.empty_like(dv2)
        # long column lists (nce_k = 4096 of the MIA trainers) are dealt to several workgroups per sample through a workspace
        lg_ws = (torch.empty(L.ph_crd_loss_grad_workspace_bytes_w(B, D), device=dev, dtype=torch.uint8) if P2 + K2 >= 1024 else None)
        if call.one_direction:      # ContrastMemory_mono: v2 is the student, memory_v1 the teacher bank, T where that buffer keeps it
            check(L.ph_crd_loss_grad_one(ptr(xt), ptr(sel), ptr(idx), ptr(call.posw_t), ptr(mem.memory_v1), ptr(mem.params),
                                         float(mem.T), ptr(lossp), ptr(dv2), B, PK, P2, K2, D, float(mem.nLem),
                                         1.0 / _loss_divisor(mem, B), ptr(lg_ws), st), "ph_crd_loss_grad_one")
        else:
            check(L.ph_crd_loss_grad(ptr(xs), ptr(xt), ptr(sel), ptr(idx), ptr(idx2), ptr(call.posw_s), ptr(call.posw_t),
                                     ptr(mem.memory_v1), ptr(mem.memory_v2),
                                     ptr(mem.params), ptr(lossp), ptr(dv1), ptr(dv2), B, PK, P2, K2, D, float(mem.nLem),
                                     1.0 / _loss_divisor(mem, B), ptr(lg_ws), st), "ph_crd_loss_grad")
        result = (_finish_loss(lossp, call.per_sample, loss_out), dv1, dv2)
    _crd_update(mem, y, v1, v2, D)
    mem.last = dict(sel=sel, xs=xs, xt=xt, diff=diff, call=call)
    return result


def _crd_core_scan(v1, v2, mem, y, call, loss_out):
    """crd_core with the negatives in bank-scan form (`call.scan`, built by CRD_criterion_v10.CRDLoss.neighbor_columns when
    nce_k reaches the number of bank rows - BASELINE configs[4] read as 65 536 negatives per query, SURVEY 8-e assumption
    (i)).  Same sums as the gathered kernels (reference CRD_criterion_v10.py:106-153, :300-306), taken over every bank row
    weighted by its multiplicity among the query's negatives: one read of each bank per GEMM instead of B x K gathered rows."""
    B, D = v1.shape
    P, K, n = call.P, call.K, mem.nLem
    col0 = int(call.scan["col0"])
    neg = require_cuda(call.scan["idx"])
    dev = v1.device
    idx, y = _checked(call, y, B)
    L, st = lib(), stream()
    idx2 = call.idx_bank2
    xs = torch.empty(B, P, device=dev, dtype=torch.float32); xt = torch.empty_like(xs); diff = torch.empty_like(xs)
    check(L.ph_crd_score(ptr(v1), ptr(v2), ptr(idx), ptr(idx2), ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(xs), ptr(xt),
                         ptr(diff), B, P, D, mem.T, st), "ph_crd_score")
    sel = torch.arange(P, device=dev, dtype=torch.int32).repeat(B, 1).contiguous()
    mult = torch.empty(B, n, device=dev, dtype=torch.int32)
    check(L.ph_crd_neg_hist(ptr(neg), neg.stride(0), col0, K, B, n, ptr(mult), st), "ph_crd_neg_hist")
    S1 = torch.empty(B, n, device=dev, dtype=torch.float32); S2 = torch.empty_like(S1)
    ops.sgemm(v1, mem.memory_v2, None, S1, B, n, D, D, 1, 1, D)      # S1[b][r] = v1[b] . bank2[r]  (out_v1, Z_v1, feeds dv1)
    ops.sgemm(v2, mem.memory_v1, None, S2, B, n, D, D, 1, 1, D)
    ws = torch.empty(L.ph_crd_scan_neg_workspace_bytes(B, n), device=dev, dtype=torch.uint8)
    if not mem._z_set:
        sums = torch.empty(2, device=dev, dtype=torch.float32)
        check(L.ph_crd_zsum(ptr(xs), ptr(xt), ptr(sums), B * P, st), "ph_crd_zsum")
        check(L.ph_crd_scan_neg(ptr(S1), ptr(S2), ptr(mult), ptr(mem.params), ptr(ws), None, ptr(sums), B, n, K, 1.0, 1, st),
              "ph_crd_scan_neg (Z)")
        _set_z_once(mem, sums, float(B * (P + K)))
    bnorm = _loss_divisor(mem, B)
    lossn = torch.empty(B, device=dev, dtype=torch.float32)
    check(L.ph_crd_scan_neg(ptr(S1), ptr(S2), ptr(mult), ptr(mem.params), ptr(ws), ptr(lossn), None, B, n, K, 1.0 / bnorm, 0, st),
          "ph_crd_scan_neg")
    lossp = torch.empty(B, device=dev, dtype=torch.float32)
    dv1 = torch.empty(B, D, device=dev, dtype=torch.float32); dv2 = torch.empty_like(dv1)
    check(L.ph_crd_loss_grad_pos(ptr(xs), ptr(xt), ptr(sel), ptr(idx), ptr(idx2), ptr(call.posw_s), ptr(call.posw_t),
                                 ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(mem.params), ptr(lossp), ptr(dv1), ptr(dv2), B, P, K, D,
                                 float(n), 1.0 / bnorm, st), "ph_crd_loss_grad_pos")
    # dv1 += coef1 [B, n] x bank2 [n, D] (split over the rows: fixed-order partial sums), likewise dv2
    nsplit = 128 if n >= 8192 else (32 if n >= 1024 else 1)
    part = torch.empty(nsplit * B * D, device=dev, dtype=torch.float32)
    for coef, bank, dv in ((S1, mem.memory_v2, dv1), (S2, mem.memory_v1, dv2)):
        dn = torch.empty(B, D, device=dev, dtype=torch.float32)
        if nsplit > 1:
            check(L.ph_sgemm_splitk(ptr(coef), ptr(bank), None, ptr(dn), ptr(part), nsplit, B, D, n, n, 1, D, 1, D, ops.ACT_NONE, st),
                  "ph_sgemm_splitk")
        else:
            ops.sgemm(coef, bank, None, dn, B, D, n, n, 1, D, 1)
        dv.add_(dn)
    lossp.add_(lossn)
    loss = _finish_loss(lossp, call.per_sample, loss_out)
    _crd_update(mem, y, v1, v2, D)
    mem.last = dict(sel=sel, xs=xs, xt=xt, diff=diff, mult=mult, call=call)
    return loss, dv1, dv2


def _crd_update(mem, y, v1, v2, D):
    """Momentum update AFTER scoring (memory_new.py:382-395); under data parallelism every replica applies the update of
    the whole global batch."""
    if mem.sync is not None:
        yy, vv1, vv2 = mem.sync.all_gather_rows(y, v1.detach(), v2.detach())
    else:
        yy, vv1, vv2 = y, v1.detach(), v2.detach()
    check(lib().ph_crd_update(ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(vv1), ptr(vv2), ptr(yy), ptr(mem.params),
                              yy.shape[0], D, stream()), "ph_crd_update")


class _CRDCoreFn(torch.autograd.Function):
    """(v1, v2) -> NCE loss (s_loss + t_loss of CRD_loss.py:172-174) with analytic gradients."""

    @staticmethod
    def forward(ctx, v1, v2, mem, y, call):
        loss, dv1, dv2 = crd_core(v1, v2, mem, y, call)
        ctx.save_for_backward(dv1, dv2)      # (dv1 None under call.one_direction)
        ctx.per_sample = call.per_sample
        return loss

    @staticmethod
    def backward(ctx, g):
        dv1, dv2 = ctx.saved_tensors
        if ctx.per_sample:
            g = g.reshape(-1, 1)      # d loss_b / d v_b is row b of dv
        return (None if dv1 is None else dv1 * g), dv2 * g, None, None, None      # (no dv1: the one-directional criterion)


class _CRDOutputsFn(torch.autograd.Function):
    """(v1, v2) -> (out_v1, out_v2) of ContrastMemory_v3.forward (memory_new.py:249-397), each [B, P2+K2, 1]:
    out_v1 = exp(memory_v2[sel] . v1 / T) / Z_v1 depends on v1 only, out_v2 on v2 only (Z are constants, :368-379)."""

    @staticmethod
    def forward(ctx, v1, v2, mem, y, call):
        o1, o2, rows1, rows2 = crd_core(v1, v2, mem, y, call, outputs_only=True)
        ctx.save_for_backward(o1, o2, rows1, rows2)
        ctx.T = float(mem.T)
        return o1.unsqueeze(-1), o2.unsqueeze(-1)

    @staticmethod
    def backward(ctx, g1, g2):
        o1, o2, rows1, rows2 = ctx.saved_tensors
        B, S2 = o1.shape
        D = rows1.shape[2]
        g1 = None if g1 is None else ops._f32(g1).reshape(B, S2).contiguous()
        g2 = None if g2 is None else ops._f32(g2).reshape(B, S2).contiguous()
        dv1 = torch.empty(B, D, device=o1.device, dtype=torch.float32)
        dv2 = torch.empty_like(dv1)
        check(lib().ph_crd_outputs_bwd(ptr(g1), ptr(g2), ptr(o1), ptr(o2), ptr(rows1), ptr(rows2), ctx.T, ptr(dv1), ptr(dv2),
                                       B, S2, D, stream()), "ph_crd_outputs_bwd")
        return dv1, dv2, None, None, None


class _CRDOutputsMonoFn(torch.autograd.Function):
    """(v1, v2) -> out_v2 [B, P2+K, 1] of ContrastMemory_mono.forward ("MIA 2022/CL_utils/memory_new.py":590-698):
    out_v2 = exp(memory_v1[sel] . v2 / T) / Z_v2; v1 (the teacher's feature) only ranks the positives and updates its bank."""

    @staticmethod
    def forward(ctx, v1, v2, mem, y, call):
        _, o2, rows1, _ = crd_core(v1, v2, mem, y, call, outputs_only=True)
        ctx.save_for_backward(o2, rows1)
        ctx.T = float(mem.T)
        return o2.unsqueeze(-1)

    @staticmethod
    def backward(ctx, g2):
        o2, rows1 = ctx.saved_tensors
        B, S2 = o2.shape
        D = rows1.shape[2]
        g2 = ops._f32(g2).reshape(B, S2).contiguous()
        dv1 = torch.empty(B, D, device=o2.device, dtype=torch.float32)      # (zeros: the NULL gradient of direction 1)
        dv2 = torch.empty_like(dv1)
        check(lib().ph_crd_outputs_bwd(None, ptr(g2), ptr(o2), ptr(o2), ptr(rows1), ptr(rows1), ctx.T, ptr(dv1), ptr(dv2),
                                       B, S2, D, stream()), "ph_crd_outputs_bwd")
        return None, dv2, None, None, None


def draw_uniform_indices(mem, y, width):
    """`contrast_idx is None` in every ContrastMemory of the reference (memory_new.py:265-267, CRD_criterion.py:37-39,
    CRD_criterion_v3.py:37-39): `width` bank rows per sample drawn from the AliasMethod table over uniform unigrams
    (:229-231, :401-458) - with all-ones unigrams every table entry keeps probability 1, so the draw IS the uniform integer
    draw - and column 0 overwritten with y.  One launch (ph_alias_uniform_draw: counter-based, keyed by (seed, step, element));
    the device-side step counter makes captured replays draw afresh.  Distributional parity: the reference's stream is torch's
    CUDA generator.  Under data parallelism (`mem.sync`) the rank is mixed into the seed, so that W replicas draw W times as
    many distinct negatives as one (the reference's one DataParallel process draws one global batch of independent rows).  The
    step counter `mem._draw_step` is not part of the module's state_dict (its keys are the reference's); DistillStep.state_dict
    saves it (`crd_draw_steps`) so that a resumed run continues the stream."""
    y = require_cuda(y).contiguous()
    B = y.shape[0]
    if mem._draw_step is None or mem._draw_step.device != y.device:
        mem._draw_step = torch.zeros(1, device=y.device, dtype=torch.int64)
    if mem._draw_seed is None:
        seed = int(torch.initial_seed())
        sync = mem.sync
        if sync is not None and getattr(sync, "rank", 0):
            seed ^= (int(sync.rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        mem._draw_seed = seed & 0x7FFFFFFFFFFFFFFF
    out = torch.empty(B, width, device=y.device, dtype=torch.int64)
    check(lib().ph_alias_uniform_draw(ptr(y), ptr(out), int(mem.nLem), B, width, mem._draw_seed, ptr(mem._draw_step), stream()),
          "ph_alias_uniform_draw")
    mem._draw_step += 1
    return out


class ContrastBank(nn.Module):
    """What the memory modules of all four criteria are: `params` = [K, T, Z_v1, Z_v2, momentum(, P)] and the two banks
    [n_data, D], uniform in +-1 / sqrt(D / 3) (memory_new.py:232-237), the first-call state of Z, the hooks of data
    parallelism, the state of the `contrast_idx is None` draw.  `P` / `P2` / `K2` and the selection switches: the list widths
    of a bank whose calls all look alike (`plan`); None where the criterion builds every call itself (CRD_criterion_v10)."""

    def __init__(self, inputSize, outputSize, K, T, momentum, P=None, P2=None, K2=None, select_pos_pairs=False,
                 select_neg_pairs="False", params_P=False, params=None):
        super().__init__()
        self.nLem, self.K, self.T = outputSize, K, T
        self.P, self.P2, self.K2 = P, P2, K2
        self.select_pos_pairs, self.select_neg_pairs = select_pos_pairs, select_neg_pairs
        self.one_direction = False     # ContrastMemory_mono: Z_v2 and d loss / d v2 alone
        # `params`: a bank with a layout of its own (ContrastMemory_mono) - Z_v2 and the momentum stay at indices 3 and 4
        self.register_buffer("params", torch.tensor(params if params is not None else
                                                    [K, T, -1, -1, momentum] + ([P] if params_P else []), dtype=torch.float32))
        stdv = 1.0 / math.sqrt(inputSize / 3)
        self.register_buffer("memory_v1", torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))
        self.register_buffer("memory_v2", torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))
        self._z_set = False
        self.sync = None               # set by dist.attach() under data parallelism
        self.batch_norm_size = None    # global batch under data parallelism
        self.sample_KD = False         # CRD_loss.CRDLoss under --sample_KD True: the rows' losses are not divided by the batch
        self.verbose = True
        self.last = None               # what the last call made: sel / xs / xt / diff (mult, the KNN tensors) and its CrdCall
        self._draw_step = self._draw_seed = None      # draw_uniform_indices

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._z_set = bool((self.params[2:4] > 0).all().item())

    def plan(self, idx, ranks=None, per_sample=False):
        """The call of a bank with constant list widths over the columns `idx` [B, P + K]."""
        return CrdCall(self.P, self.K, self.P2, self.K2, idx, select_pos=self.select_pos_pairs is True,
                       select_neg=self.select_neg_pairs == "True", ranks=ranks, per_sample=per_sample)


class ContrastMemory_v3(ContrastBank):
    def __init__(self, inputSize, outputSize, P, K, T=0.07, momentum=0.5, select_pos_pairs=True, P2=10,
                 select_neg_pairs=True, K2=512):
        if select_pos_pairs is not True or select_neg_pairs not in ("True", "False", True, False):
            raise NotImplementedError("select_pos_pairs is always on in the reference (options.py:44-45)")
        if select_neg_pairs in (True, False):
            select_neg_pairs = "True" if select_neg_pairs else "False"
        super().__init__(inputSize, outputSize, K, T, momentum, P, P2, K if select_neg_pairs == "False" else K2,
                         select_pos_pairs, select_neg_pairs, params_P=True)

    def draw_ranks(self, epoch, select_pos_mode):
        """The host-RNG draw of memory_new.py:311-322 (numpy global RNG, like the reference)."""
        if select_pos_mode == "hard":
            return None
        if select_pos_mode == "mid":
            r = np.random.choice(np.arange(30, 100, 1), self.P2, replace=False)
        elif select_pos_mode == "random":
            r = np.random.randint(0, self.P, self.P2)
        elif select_pos_mode == "curriculum":
            interval = 4 - np.ceil(3 * epoch)
            r = np.random.randint(50 * (interval - 1), 50 * interval, self.P2)
        else:
            raise NotImplementedError(select_pos_mode)
        if r.max() >= self.P:
            raise RuntimeError("select_pos_mode '%s' needs nce_p > %d" % (select_pos_mode, int(r.max())))
        return torch.as_tensor(np.asarray(r), dtype=torch.int32)

    def draw_indices(self, y):
        """idx == None (memory_new.py:265-267): B * (K + P) rows drawn from the AliasMethod table, column 0 := y."""
        return draw_uniform_indices(self, y, self.P + self.K)

    def _plan(self, epoch, dev, y, idx, select_pos_mode, ranks, per_sample=False):
        if idx is None:
            idx = self.draw_indices(y)
        if ranks is None:
            ranks = self.draw_ranks(epoch, select_pos_mode)
        if ranks is not None and not (torch.is_tensor(ranks) and ranks.is_cuda and ranks.dtype == torch.int32):
            ranks = torch.as_tensor(np.asarray(ranks), dtype=torch.int32).to(dev, non_blocking=True)
        return self.plan(idx, ranks, per_sample)

    def loss(self, epoch, v1, v2, y, idx, select_pos_mode="mid", ranks=None):
        """s_loss + t_loss of CRDLoss.forward (CRD_loss.py:167-174) in one fused pass (what CRDLoss calls)."""
        return _CRDCoreFn.apply(v1, v2, self, y, self._plan(epoch, v1.device, y, idx, select_pos_mode, ranks, self.sample_KD))

    def forward(self, epoch, v1, v2, y, idx=None, select_pos_mode="mid", ranks=None):
        """memory_new.py:249-397 as written: returns (out_v1, out_v2), each [B, P2+K2, 1] (selected positives first),
        differentiable w.r.t. v1 / v2; sets Z on the first call, momentum-updates the rows `y` of both banks.  The rank
        list of the `mid` / `random` / `curriculum` modes comes from numpy's global RNG exactly as in the reference
        (:311-322) unless `ranks` is given."""
        return _CRDOutputsFn.apply(v1, v2, self, y, self._plan(epoch, v1.device, y, idx, select_pos_mode, ranks))


def _draw_ranks(P, P2, epoch, select_pos_mode, mid):
    """The host-RNG rank draws of the DSCD banks ("MIA 2022/CL_utils/memory_new.py":480-495 and :646-658; numpy's global RNG, like
    the reference); `mid`: that bank's own draw.  A rank at or above P fails as ContrastMemory_v3.draw_ranks does."""
    if select_pos_mode == "hard":
        return None
    if select_pos_mode == "mid":
        r = mid()
    elif select_pos_mode == "random":
        r = np.random.randint(0, P, P2)
    elif select_pos_mode == "curriculum":
        interval = 4 - np.ceil(3 * epoch)
        r = np.random.randint(50 * (interval - 1), 50 * interval, P2)
    else:
        raise NotImplementedError(select_pos_mode)
    if r.max() >= P or r.min() < 0:
        raise RuntimeError("select_pos_mode '%s' needs nce_p > %d" % (select_pos_mode, int(r.max())))
    return torch.as_tensor(np.asarray(r), dtype=torch.int32)


class _DscdBank(ContrastBank):
    """What ContrastMemory_v4 and ContrastMemory_mono share: the reference's constructor arguments and attributes, the plan of a
    call (the P positives ranked by ph_crd_select_dscd, all K negatives kept: select_neg_pairs and K2 are stored and never read,
    as there), the rank draws, the `idx is None` draw."""
    rank_ascending = None      # the subclass's direction of the positive ranking

    def _init_dscd(self, P2, K2, select_neg_pairs, neg_reweight):
        self.P2, self.K2 = P2, K2
        self.select_neg_pairs, self.neg_reweight = select_neg_pairs, neg_reweight

    def draw_indices(self, y):
        return draw_uniform_indices(self, y, self.P + self.K)

    def plan(self, idx, ranks=None, per_sample=False):
        """The call over the columns `idx` [B, P + K] (what the fused loss head of DistillStep asks a bank for)."""
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[1] != self.P + self.K:
            raise RuntimeError("contrast_idx must be [B, nce_p + nce_k] = [B, %d + %d], got %s"
                               % (self.P, self.K, tuple(idx.shape) if torch.is_tensor(idx) else type(idx).__name__))
        return CrdCall(self.P, self.K, self.P2, self.K, idx, ranks=ranks, per_sample=per_sample,
                       rank_ascending=self.rank_ascending, neg_reweight=self.neg_reweight == "True" and not self.one_direction,
                       one_direction=self.one_direction)

    def _plan(self, epoch, dev, y, idx, select_pos_mode, ranks, per_sample=False):
        if idx is None:
            idx = self.draw_indices(y)
        if ranks is None:
            ranks = self.draw_ranks(epoch, select_pos_mode)
        if ranks is not None:
            if not torch.is_tensor(ranks):
                ranks = torch.as_tensor(np.asarray(ranks), dtype=torch.int32)
            if not ranks.is_cuda:      # (a device tensor is a graph input: checked where it was drawn)
                if ranks.numel() != self.P2 or int(ranks.max()) >= self.P or int(ranks.min()) < 0:
                    raise RuntimeError("ranks must be %d values below nce_p = %d" % (self.P2, self.P))
                ranks = ranks.to(torch.int32).to(dev, non_blocking=True)
        return self.plan(idx, ranks, per_sample)

    def loss(self, epoch, v1, v2, y, idx, select_pos_mode="hard", ranks=None):
        """The criterion's loss in one fused pass (what CRD_loss_v2.CRDLoss / CRDLoss_v2 call)."""
        return _CRDCoreFn.apply(v1, v2, self, y, self._plan(epoch, v1.device, y, idx, select_pos_mode, ranks, self.sample_KD))


class ContrastMemory_v4(_DscdBank):
    """"MIA 2022/CL_utils/memory_new.py":398-561.  params = [K, T, Z_v1, Z_v2, momentum, P]; called as (epoch, student, teacher, y,
    idx, mode), so memory_v1 is the student bank.  Positives by t_relation - s_relation descending (:473-476) = the discrepancy
    of ph_crd_score ASCENDING; all K negatives, under neg_reweight == "True" weighted by 1 + discrepancy in both directions
    (:510-517).  Where the reference fails at its first call (UnboundLocalError: out_v2_pos for select_pos_pairs other than True,
    out_v2_neg for a neg_reweight outside "True" / "False"), this fails at construction."""
    rank_ascending = True

    def __init__(self, inputSize, outputSize, P, K, T=0.07, momentum=0.5, select_pos_pairs=True, P2=10,
                 select_neg_pairs=False, neg_reweight=True, K2=512):
        if not (select_pos_pairs == True):      # noqa: E712  (the reference's own comparison, :471)
            raise UnboundLocalError("local variable 'out_v2_pos' referenced before assignment")
        if neg_reweight not in ("True", "False"):
            raise UnboundLocalError("local variable 'out_v2_neg' referenced before assignment")
        super().__init__(inputSize, outputSize, K, T, momentum, P, P2, K, select_pos_pairs, select_neg_pairs, params_P=True)
        self._init_dscd(P2, K2, select_neg_pairs, neg_reweight)

    def draw_ranks(self, epoch, select_pos_mode):
        return _draw_ranks(self.P, self.P2, epoch, select_pos_mode,
                           lambda: np.random.choice(np.arange(30, 100, 1), self.P2, replace=False))      # :484

    def forward(self, epoch, v1, v2, y, idx=None, select_pos_mode="mid", ranks=None):
        """:422-561 as written: (out_v1, out_v2), each [B, P2+K, 1], differentiable w.r.t. v1 / v2."""
        return _CRDOutputsFn.apply(v1, v2, self, y, self._plan(epoch, v1.device, y, idx, select_pos_mode, ranks))


class ContrastMemory_mono(_DscdBank):
    """"MIA 2022/CL_utils/memory_new.py":565-698, the one-directional bank.  params = [P, K, T, Z_v2, momentum] (:584: its own
    order; Z_v2 and the momentum sit where the kernels read them, T is passed).  Called as (epoch, teacher, student, y, idx,
    mode): memory_v1 is the TEACHER bank, only out_v2 = exp(memory_v1[idx] . v2 / T) exists.  Positives by the discrepancy
    descending (:632-642), `mid` draws randint(50, 100) (:649); all K negatives, unweighted - neg_reweight is stored and unused.
    forward returns (out_v2, memory_v1) (:698)."""
    rank_ascending = False

    def __init__(self, inputSize, outputSize, P, K, T=0.07, momentum=0.5, select_pos_pairs=True, P2=10,
                 select_neg_pairs=False, neg_reweight=True, K2=512):
        if not (select_pos_pairs == True):      # noqa: E712  (:630: without it the reference keeps all P + K columns as positives-first)
            raise NotImplementedError("ContrastMemory_mono without select_pos_pairs (options.py:44-45: always on)")
        super().__init__(inputSize, outputSize, K, T, momentum, P, P2, K, select_pos_pairs, select_neg_pairs,
                         params=[P, K, T, -1, momentum])
        self._init_dscd(P2, K2, select_neg_pairs, neg_reweight)
        self.one_direction = True

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._z_set = bool((self.params[3] > 0).item())

    def draw_ranks(self, epoch, select_pos_mode):
        return _draw_ranks(self.P, self.P2, epoch, select_pos_mode, lambda: np.random.randint(50, 100, self.P2))      # :649

    def forward(self, epoch, v1, v2, y, idx=None, select_pos_mode="hard", ranks=None):
        out_v2 = _CRDOutputsMonoFn.apply(v1, v2, self, y, self._plan(epoch, v1.device, y, idx, select_pos_mode, ranks))
        return out_v2, self.memory_v1

"""Feature-distillation baselines of the reference's distiller zoo that the trainers can select with `--distill`
(part): `Similarity` ("MIA 2022/distiller_zoo/SP.py": similarity-preserving KD; also
`opt.distill == "sp"` in the MIA-2023 stage-2 trainer, train_test_path_multi_distill.py:369-370) and `feats_KL`
("MIA 2022/distiller_zoo/feats_KL.py": KL divergence between softmaxed feature vectors).  Both are compositions of
kernels of the hot path (fp32 GEMM, row L2 normalisation, squared-difference reduction, the KL kernels); the teacher
side is treated as a constant (the trainers pass it detached).  `RKDLoss` ("MIA 2022/distiller_zoo/RKD.py") and `PKT`
("MIA 2022/distiller_zoo/PKT.py"), the `--distill rkd|pkt` choices of train_test_path_multi_distill_v2.py:339-342, are
closed-form loss + gradient kernels of their own (csrc/zoo.hip; where a batch does not fit the one-workgroup form's LDS -
above 128 rows, or fewer at feature widths above 128 - and under data parallelism RKD runs the anchor-partitioned kernels
of csrc/zoo_rkd.hip).  The other zoo members are not built.

`Similarity`, `PKT` and `RKDLoss` relate every row of a batch to every other row.  Given a `sync` object (dist.ReplicaSync:
one process per GPU, each holding `n` rows) they evaluate the loss of the GLOBAL batch of `world_size * n` rows, as the
reference's nn.DataParallel trainer does on the gathered outputs (train_test_path_multi_distill_v2.py:286, 307-308):
  * `Similarity`, `PKT`: the rows are all-gathered (train_step._GatherRowsFn) and every replica evaluates the same
    criterion on them; the value is the global loss on every replica, the backward hands back this replica's rows.
  * `RKDLoss`: the B^3 * D angle term is split - replica r takes the anchors [r n, (r + 1) n) through
    ph_rkd_loss_grad_part, ONE all-reduce sums the [Bg, D] gradient parts; the value is THIS replica's part of the loss
    (the parts add up to the global loss), the backward returns this replica's rows of the summed gradient, without a
    collective.
In both forms the replicas' parameter gradients add up to the single-process gradient of the global loss."""
import torch
import torch.nn as nn

from . import ops
from ._lib import lib, check, ptr, stream
from .tsvd import _SqDiffFn


RKD_MAX_ROWS = 1024       # ph_rkd_loss_grad_part: rows of the (global) batch


def _gather_pair(f_s, f_t, sync):
    """(student rows with the local backward, teacher rows) of every replica, rank-ordered."""
    from .train_step import _GatherRowsFn
    return _GatherRowsFn.apply(f_s, sync), sync.all_gather_cat(f_t.detach().contiguous())


class Similarity(nn.Module):
    """SP.py:9-30: G = rownormalize(f f^T) for student and teacher, loss = ||G_t - G_s||_F^2 / B^2 (shape [1]).
    `sync`: the loss of the global batch (identical on every replica), see the module docstring."""

    def __init__(self, sync=None):
        super().__init__()
        self.sync = sync

    def forward(self, f_s, f_t):
        bsz = f_s.shape[0]
        f_s = ops._f32(f_s).reshape(bsz, -1)
        f_t = ops._f32(f_t.detach()).reshape(bsz, -1)
        if self.sync is not None:
            f_s, f_t = _gather_pair(f_s, f_t, self.sync)
            bsz = f_s.shape[0]
        g_s = ops.L2NormFn.apply(ops.LinearFn.apply(f_s, f_s, None))
        with torch.no_grad():
            g_t = ops.L2NormFn.apply(ops.LinearFn.apply(f_t, f_t, None))
        return _SqDiffFn.apply(g_s, g_t, 1.0 / (bsz * bsz)).reshape(1)


class feats_KL(nn.Module):
    """feats_KL.py:13-20: sum KL(softmax(f_t) || softmax(f_s)) / B."""

    def forward(self, f_s, f_t):
        return ops.KLFn.apply(f_s, f_t.detach(), 1.0, float(f_s.shape[0]))


class _LossGradFn(torch.autograd.Function):
    """loss(f_s; f_t) whose kernel returns the gradient with respect to f_s together with the value."""

    @staticmethod
    def forward(ctx, f_s, f_t, kind, w_d, w_a):
        f_s, f_t = ops._f32(f_s), ops._f32(f_t.detach())
        B, D = f_s.shape
        loss = torch.empty(1, device=f_s.device, dtype=torch.float32)
        dx = torch.empty_like(f_s)
        if kind == "pkt":
            ws = torch.empty(lib().ph_pkt_workspace_bytes(B, D), device=f_s.device, dtype=torch.uint8)
            check(lib().ph_pkt_loss_grad(ptr(f_s), ptr(f_t), ptr(loss), ptr(dx), B, D, ptr(ws), stream()), "ph_pkt_loss_grad")
        elif lib().ph_rkd_one_workgroup_fits(B, D):     # the anchor kernel keeps E [B][D] and A [B][B] in LDS
            ws = torch.empty(lib().ph_rkd_workspace_bytes(B, D), device=f_s.device, dtype=torch.uint8)
            check(lib().ph_rkd_loss_grad(ptr(f_s), ptr(f_t), ptr(loss), ptr(dx), B, D, float(w_d), float(w_a), ptr(ws),
                                         stream()), "ph_rkd_loss_grad")
        else:
            loss, dx = rkd_part(f_s.contiguous(), f_t.contiguous(), 0, B, w_d, w_a)
        ctx.save_for_backward(dx)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dx, = ctx.saved_tensors
        return dx * g, None, None, None, None


def rkd_part(g_s, g_t, anchor_lo, n_anchors, w_d, w_a):
    """ph_rkd_loss_grad_part on the contiguous fp32 rows g_s, g_t [Bg, D]: (loss_part [1], dx_part [Bg, D]) of the anchors
    [anchor_lo, anchor_lo + n_anchors); the parts of a partition of [0, Bg) add up to RKD.py's loss and gradient."""
    g_s, g_t = ops._f32(g_s), ops._f32(g_t)
    Bg, D = g_s.shape
    if not (2 <= Bg <= RKD_MAX_ROWS and 1 <= D <= 512):
        raise ValueError("rkd: %d rows of %d features (the partitioned kernel holds 2..%d rows of 1..512)" % (Bg, D, RKD_MAX_ROWS))
    loss = torch.empty(1, device=g_s.device, dtype=torch.float32)
    dx = torch.empty_like(g_s)
    ws = torch.empty(lib().ph_rkd_part_workspace_bytes(Bg, D, n_anchors), device=g_s.device, dtype=torch.uint8)
    check(lib().ph_rkd_loss_grad_part(ptr(g_s), ptr(g_t), Bg, D, int(anchor_lo), int(n_anchors), float(w_d), float(w_a),
                                      ptr(loss), ptr(dx), ptr(ws), stream()), "ph_rkd_loss_grad_part")
    return loss, dx


class _RkdGatheredFn(torch.autograd.Function):
    """RKD over the global batch of a data-parallel run (the ops.SurvStage1GatheredFn pattern).  Forward: ONE all-gather of
    this replica's (student, teacher) rows, ph_rkd_loss_grad_part on this replica's anchor range of the gathered rows, ONE
    all-reduce (sum) of the [Bg, D] gradient parts.  Returns THIS replica's part of the loss - the replicas' values add up
    to the global loss.  Backward: this replica's rows of the summed gradient times the incoming scalar, no collective;
    the gradient all-reduce of the step then adds the replicas' parameter gradients up to the single-process gradient."""

    @staticmethod
    def forward(ctx, f_s, f_t, w_d, w_a, sync):
        if f_s.dtype != torch.float32 or f_t.dtype != torch.float32 or f_s.dim() != 2 or f_s.shape != f_t.shape:
            raise RuntimeError("expected two float32 [n, D] tensors")
        f_t = f_t.detach()
        n, D = f_s.shape
        g = sync.all_gather_cat(torch.cat([f_s.detach(), f_t], dim=1))          # [Bg, 2 D], rank-ordered
        g_s, g_t = g[:, :D].contiguous(), g[:, D:].contiguous()
        lo = sync.rank * n
        loss, dx = rkd_part(g_s, g_t, lo, n, w_d, w_a)
        sync.all_reduce_sum(dx)
        ctx.save_for_backward(dx[lo:lo + n])
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        d, = ctx.saved_tensors
        return d * g, None, None, None, None


class PKT(nn.Module):
    """PKT.py:7-46: KL between the row-normalised cosine-similarity distributions of teacher and student (0-d).
    `sync`: the loss of the global batch (identical on every replica), see the module docstring."""

    def __init__(self, sync=None):
        super().__init__()
        self.sync = sync

    def forward(self, f_s, f_t):
        f_s, f_t = f_s.reshape(f_s.shape[0], -1), f_t.reshape(f_t.shape[0], -1)
        if self.sync is not None:
            f_s, f_t = _gather_pair(ops._f32(f_s), ops._f32(f_t), self.sync)
        return _LossGradFn.apply(f_s, f_t, "pkt", 0.0, 0.0)


class RKDLoss(nn.Module):
    """RKD.py:8-45: w_d * distance-wise + w_a * angle-wise relational losses (0-d).  Where ph_rkd_one_workgroup_fits(B, D)
    (at most 128 rows, and B (D + 1) + B (B + 1) + B floats within 150 KiB of LDS: 105 rows at D = 256, 66 at D = 512): the
    one-workgroup-per-anchor kernels of csrc/zoo.hip; otherwise, up to 1024 rows of up to 512 features: the tiled kernels of
    csrc/zoo_rkd.hip over the full anchor range.
    `sync`: this replica's anchor range of the global batch (world_size * B <= 1024); the value is this replica's PART of
    the global loss, see the module docstring."""

    def __init__(self, w_d=25, w_a=50, sync=None):
        super().__init__()
        self.w_d, self.w_a, self.sync = w_d, w_a, sync

    def forward(self, f_s, f_t):
        f_s, f_t = f_s.reshape(f_s.shape[0], -1), f_t.reshape(f_t.shape[0], -1)
        if self.sync is not None:
            return _RkdGatheredFn.apply(f_s, f_t, self.w_d, self.w_a, self.sync)
        return _LossGradFn.apply(f_s, f_t, "rkd", self.w_d, self.w_a)

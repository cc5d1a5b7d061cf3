"""Drop-in for the hot-loop functions of the reference's MICCAI-2022/train_test_path_multi_distill.py:
``update_ema_variables`` (:34-38), ``AEKD_loss`` (:41-70) and the batch body of ``train()`` (:242-330,
here ``DistillStep``), plus the fused optimiser behind ``define_optimizer`` (networks_new.py:80-90)."""
import collections
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import lib, check, ptr, stream
from .step_graph import StepGraphs


# ----------------------------------------------------------------------------------------- flat storage
class FlatParams:
    """Re-homes a list of tensors into ONE contiguous fp32 buffer (each tensor 16-B aligned) so that the
    optimiser / EMA / gradient all-reduce are single streaming kernels instead of ~70 small launches."""

    def __init__(self, tensors, with_grad=False):
        tensors = list(tensors)
        dev = tensors[0].device
        offs, off = [], 0
        for t in tensors:
            offs.append(off)
            off += (t.numel() + 3) // 4 * 4
        self.numel = off
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32) if with_grad else None
        self.offsets = offs
        self.tensors = tensors
        for t, o in zip(tensors, offs):
            n = t.numel()
            self.flat[o:o + n].copy_(t.detach().reshape(-1))
            t.data = self.flat[o:o + n].view(t.shape)
            if with_grad and t.requires_grad:
                t.grad = self.grad[o:o + n].view(t.shape)
        ops.register_flat(self)       # define_reg finds the flat layout of a parameter through its storage

    def segments(self, pred):
        """Maximal [start, end) runs of consecutive tensors for which pred(t) holds."""
        segs, cur = [], None
        for t, o in zip(self.tensors, self.offsets):
            e = o + (t.numel() + 3) // 4 * 4
            if pred(t):
                if cur is not None and cur[1] == o:
                    cur[1] = e
                else:
                    cur = [o, e]
                    segs.append(cur)
            else:
                cur = None
        return [tuple(s) for s in segs]


class PinnedRing:
    """Host staging for small per-step values that are uploaded with an asynchronous copy while the device still
    works on earlier steps: a ring of pinned rows, each guarded by an event recorded after its copy (a single pinned
    buffer would be overwritten by the host, which runs steps ahead of the device, before the copy has executed)."""

    def __init__(self, shape, dtype, depth=16):
        self.buf = torch.zeros((depth,) + tuple(shape), dtype=dtype).pin_memory()
        self.events = [None] * depth
        self.k = 0

    def upload(self, dst, values):
        i = self.k % len(self.events)
        self.k += 1
        if self.events[i] is not None:
            self.events[i].synchronize()
        row = self.buf[i]
        row.copy_(torch.as_tensor(values, dtype=row.dtype).reshape(row.shape))
        dst.copy_(row, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (L2-in-grad weight decay, bias correction, eps outside the sqrt) as one
    HIP kernel over flat parameter / gradient / state buffers (ph_adam_ema_step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise NotImplementedError("one parameter group (the reference passes model.parameters())")
        self._flat = None
        self._step = 0
        self.ema_flat = None      # optional FlatParams of the EMA model to update in the same kernel
        self.ema_alpha = None
        self.ema_range = None
        self._hyper = None        # device float[12] {lr, 1-beta1^t, sqrt(1-beta2^t), ema_alpha, 1-ema_alpha, 0, 0, 0, beta1, 1-beta1, beta2, 1-beta2}: graph-replayable
        self._hyper_host = None
        self._prepared = False
        self._inactive = None     # ids of the parameters that take no part in the objective (set_inactive)

    def _active(self, t):
        return t.requires_grad and (self._inactive is None or id(t) not in self._inactive)

    def _ensure_flat(self):
        if self._flat is None:
            ps = self.param_groups[0]["params"]
            if not ps[0].is_cuda:
                raise RuntimeError("FusedAdam needs parameters on the GPU (no CPU fallback)")
            self._flat = FlatParams(ps, with_grad=True)
            self._m = torch.zeros_like(self._flat.flat)
            self._v = torch.zeros_like(self._flat.flat)
            self._segs = self._flat.segments(self._active)
            self._hyper = torch.zeros(12, device=ps[0].device, dtype=torch.float32)
            self._hyper_host = PinnedRing((12,), torch.float32)
            ops.bump_weight_epoch()
        return self._flat

    def prepare_step(self):
        """Host side of a step: advance t, compute the bias corrections in double (as torch.optim.Adam's Python
        scalars) and enqueue their copy to device memory.  Split from step() so that the kernel launches can be
        captured in a HIP graph while these per-step scalars keep changing."""
        self._ensure_flat()
        g = self.param_groups[0]
        self._step += 1
        b1, b2 = g["betas"]
        a = self.ema_alpha if self.ema_alpha is not None else 0.0
        # [8..11] = beta1, 1 - beta1, beta2, 1 - beta2: read by the kernel in place of its launch arguments (a captured launch
        # would keep the betas of the capture; OneCycleLR cycles beta1 - networks_new.define_scheduler)
        self._hyper_host.upload(self._hyper, [g["lr"], 1.0 - b1 ** self._step, math.sqrt(1.0 - b2 ** self._step), a, 1.0 - a,
                                              0.0, 0.0, 0.0, b1, 1.0 - b1, b2, 1.0 - b2])
        self._prepared = True

    @property
    def flat(self):
        return self._ensure_flat()

    def set_inactive(self, params):
        """Parameters that take no part in the objective (an option branch leaves a module unused): the reference's
        torch.optim optimiser skips a parameter whose .grad is None - no weight decay, no moment update - whereas the flat
        gradient buffer would hand the kernel a zero gradient and decay the weights.  Their segments leave the update."""
        self._inactive = {id(p) for p in params}
        if self._flat is not None:
            self._segs = self._flat.segments(self._active)

    def zero_grad(self, set_to_none=False):
        """Gradients are views of one flat buffer: zeroing is a single memset and the views persist."""
        f = self._ensure_flat()
        f.grad.zero_()
        for t, o in zip(f.tensors, f.offsets):
            if t.requires_grad and (t.grad is None or t.grad.data_ptr() != f.grad.data_ptr() + 4 * o):
                t.grad = f.grad[o:o + t.numel()].view(t.shape)

    def _begin_step(self):
        """What every step starts with: a gradient tensor torch re-allocated (e.g. after zero_grad(set_to_none=True)) is
        copied back into the flat buffer, and the step scalars are uploaded unless prepare_step() already did."""
        f = self._ensure_flat()
        for t, o in zip(f.tensors, f.offsets):
            if t.requires_grad and t.grad is not None and t.grad.data_ptr() != f.grad.data_ptr() + 4 * o:
                f.grad[o:o + t.numel()].copy_(t.grad.reshape(-1))
                t.grad = f.grad[o:o + t.numel()].view(t.shape)
        if not self._prepared:
            self.prepare_step()
        self._prepared = False
        return f, self.param_groups[0]

    def _ema_segments(self):
        """(start, end, EMA slice or None) of the updated segments, split at the EMA boundary (student params | embed params)."""
        ema_on = self.ema_flat is not None and self.ema_range is not None
        for (s, e) in self._segs:
            cuts = [s, self.ema_range[1], e] if ema_on and s < self.ema_range[1] < e else [s, e]
            for a, b in zip(cuts[:-1], cuts[1:]):
                yield a, b, (self.ema_flat.flat[a:b] if ema_on and a >= self.ema_range[0] and b <= self.ema_range[1] else None)

    @torch.no_grad()
    def step(self, closure=None):
        f, g = self._begin_step()
        for s, e, ema in self._ema_segments():
            check(lib().ph_adam_ema_step_dev(ptr(f.flat[s:e]), ptr(f.grad[s:e]), ptr(self._m[s:e]), ptr(self._v[s:e]),
                                             ptr(ema), e - s, -1.0, g["betas"][1], g["eps"],      # (beta1 < 0: betas from hyper[8..11])
                                             g["weight_decay"], ptr(self._hyper), stream()), "ph_adam_ema_step_dev")
        ops.bump_weight_epoch()

    def state_dict(self):
        """torch.optim.Adam's layout (state[i] = {step, exp_avg, exp_avg_sq} per parameter index, so the reference's
        `optimizer.load_state_dict` - train_test_path_multi_distill.py:387-402 saves / restores exactly that - accepts
        it) plus the flat buffers under "fused" for an exact, copy-only restore."""
        sd = super().state_dict()
        if self._flat is not None and self._step > 0:
            f = self._flat
            sd["state"] = {i: dict(step=torch.tensor(float(self._step)),
                                   exp_avg=self._m[o:o + t.numel()].view(t.shape).clone(),
                                   exp_avg_sq=self._v[o:o + t.numel()].view(t.shape).clone())
                           for i, (t, o) in enumerate(zip(f.tensors, f.offsets))
                           if self._active(t)}
        sd["fused"] = dict(step=self._step, exp_avg=None if self._flat is None else self._m.clone(),
                           exp_avg_sq=None if self._flat is None else self._v.clone())
        return sd

    def load_state_dict(self, sd):
        """Accepts this class's own state_dict or a plain torch.optim.Adam one (a checkpoint written by the reference)."""
        sd = dict(sd)                      # the caller's checkpoint object stays intact (it may be loaded again)
        fused = sd.pop("fused", None)
        per_param = sd.get("state") or {}
        sd["state"] = {}                   # the moments live in the flat buffers, not in torch's per-parameter state
        super().load_state_dict(sd)
        has_fused = fused is not None and fused["exp_avg"] is not None
        if has_fused or per_param:
            self._ensure_flat()
            if not has_fused:
                self._m.zero_(); self._v.zero_()
            self._restore(fused, per_param, dict(exp_avg=self._m, exp_avg_sq=self._v))

    def _restore(self, fused, per_param, bufs):
        """The moments `bufs` (state name -> flat buffer) and the step count from the flat copies under "fused" if they are
        there, else from torch's per-parameter state."""
        first = next(iter(bufs))
        if fused is not None and fused.get(first) is not None:
            self._step = fused["step"]
            for k, b in bufs.items():
                b.copy_(fused[k])
        elif per_param:
            f, steps = self._flat, set()
            for i, st in per_param.items():
                t, o = f.tensors[int(i)], f.offsets[int(i)]
                if tuple(st[first].shape) != tuple(t.shape):
                    raise ValueError("optimizer state %d has shape %s, parameter %s" % (int(i), tuple(st[first].shape), tuple(t.shape)))
                for k, b in bufs.items():
                    b[o:o + t.numel()].copy_(st[k].reshape(-1))
                steps.add(int(float(st["step"])))
            if len(steps) != 1:
                raise NotImplementedError("per-parameter step counts differ (%s): the fused kernel keeps one" % sorted(steps))
            self._step = steps.pop()


class FusedAdagrad(FusedAdam):
    """torch.optim.Adagrad as the reference builds it (networks_new.py:86-87: lr, weight_decay, initial_accumulator_value = 0.1;
    lr_decay 0, eps 1e-10) over the same flat buffers as FusedAdam, EMA copy fused (ph_adagrad_ema_step_dev).  `_v` holds the
    accumulator `sum`; there is no first moment."""

    def __init__(self, params, lr=1e-2, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10):
        torch.optim.Optimizer.__init__(self, list(params), dict(lr=lr, lr_decay=0, eps=eps, weight_decay=weight_decay,
                                                                  initial_accumulator_value=initial_accumulator_value))
        if len(self.param_groups) != 1:
            raise NotImplementedError("one parameter group (the reference passes model.parameters())")
        self._flat = None
        self._step = 0
        self.ema_flat = self.ema_alpha = self.ema_range = None
        self._hyper = self._hyper_host = self._inactive = None
        self._prepared = False

    def _ensure_flat(self):
        if self._flat is None:
            super()._ensure_flat()
            self._m = None
            self._v.fill_(float(self.param_groups[0]["initial_accumulator_value"]))
        return self._flat

    def prepare_step(self):
        self._ensure_flat()
        self._step += 1
        a = self.ema_alpha if self.ema_alpha is not None else 0.0
        self._hyper_host.upload(self._hyper, [self.param_groups[0]["lr"], 1.0, 1.0, a, 1.0 - a, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        self._prepared = True

    @torch.no_grad()
    def step(self, closure=None):
        f, g = self._begin_step()
        for a, b, ema in self._ema_segments():
            check(lib().ph_adagrad_ema_step_dev(ptr(f.flat[a:b]), ptr(f.grad[a:b]), ptr(self._v[a:b]), ptr(ema), b - a,
                                                g["eps"], g["weight_decay"], ptr(self._hyper), stream()),
                  "ph_adagrad_ema_step_dev")
        ops.bump_weight_epoch()

    def state_dict(self):
        """torch.optim.Adagrad's layout (state[i] = {step, sum}; like torch, filled from construction on: step 0 and
        sum = initial_accumulator_value before the first step) plus the flat accumulator under "fused".
        One difference from torch.optim.Adagrad is documented rather than mirrored: a requires_grad parameter that received NO
        gradient in a step (torch: .grad is None -> skipped) sees a zero gradient here, i.e. weight decay and the accumulator
        still advance - unless the owner declares it unused (`set_inactive`, what DistillStep does for the option branches that
        leave a criterion idle)."""
        sd = torch.optim.Optimizer.state_dict(self)
        if self._flat is not None:
            f = self._flat
            sd["state"] = {i: dict(step=torch.tensor(float(self._step)), sum=self._v[o:o + t.numel()].view(t.shape).clone())
                           for i, (t, o) in enumerate(zip(f.tensors, f.offsets)) if self._active(t)}
        else:
            init = float(self.param_groups[0]["initial_accumulator_value"])
            sd["state"] = {i: dict(step=torch.tensor(0.0), sum=torch.full_like(t, init, dtype=torch.float32))
                           for i, t in enumerate(self.param_groups[0]["params"]) if self._active(t)}
        sd["fused"] = dict(step=self._step, sum=None if self._flat is None else self._v.clone())
        return sd

    def load_state_dict(self, sd):
        """Accepts this class's own state_dict or a plain torch.optim.Adagrad one (a checkpoint written by the reference)."""
        sd = dict(sd)
        fused = sd.pop("fused", None)
        per_param = sd.get("state") or {}
        sd["state"] = {}
        torch.optim.Optimizer.load_state_dict(self, sd)
        self._ensure_flat()
        if fused is not None and fused.get("sum") is not None and tuple(fused["sum"].shape) != tuple(self._v.shape):
            raise ValueError("fused accumulator has %d elements, the parameters %d" % (fused["sum"].numel(), self._v.numel()))
        self._restore(fused, per_param, dict(sum=self._v))


def update_ema_variables(model, ema_model, alpha, global_step):
    """train_test_path_multi_distill.py:34-38 - parameters only, BN buffers untouched."""
    alpha = min(1 - 1 / (global_step + 1), alpha)
    for mod in ema_model.modules():
        if hasattr(mod, "_get_packed"):
            mod._follow_epoch = True       # its weights change through raw pointers
    with torch.no_grad():
        for ema_param, param in zip(ema_model.parameters(), model.parameters()):
            check(lib().ph_ema_update(ptr(ema_param.data), ptr(param.data), param.numel(), alpha, stream()),
                  "ph_ema_update")
    ops.bump_weight_epoch()


def _gk_gram(opt, main_loss, feat_s, loss_t_list, sync=None):
    """The front end of every scalar GK-Refine form: d loss_i / d feat_s per loss (the CE gradient last when opt.CE_grads),
    stacked, their Gram matrix (ph_gram), summed over the replicas.  The reference obtains each gradient by a FULL backward
    pass (5 ResNet-18 backward passes thrown away except the hook value, train_test_path_multi_distill.py:49-56); the identical
    values are the VJPs stopped at feat_s, so this costs a few [B,128]-sized kernels.  Returns (gram[ng * ng], ng)."""
    losses = list(loss_t_list) + ([main_loss] if opt.CE_grads else [])
    grads = [torch.autograd.grad(l, feat_s, retain_graph=True)[0] for l in losses]
    ng = len(grads)
    G = torch.stack([g.reshape(-1) for g in grads]).contiguous()
    gram = torch.empty(ng * ng, device=G.device, dtype=torch.float32)
    check(lib().ph_gram(ptr(G), ptr(gram), ng, G.shape[1], stream()), "ph_gram")
    if sync is not None:
        sync.all_reduce_sum(gram)        # global-batch cosine under data parallelism
    return gram, ng


def AEKD_loss(opt, optimizer, main_loss, feat_s, loss_t_list, sync=None):
    """GK-Refine (train_test_path_multi_distill.py:41-70): weights = row sums of the (x len(loss_t_list))
    cosine Gram matrix of d loss_i / d feat_s (_gk_gram).  Returns (scale[5], total_KD_loss)."""
    gram, ng = _gk_gram(opt, main_loss, feat_s, loss_t_list, sync)
    scale = torch.empty(ng, device=gram.device, dtype=torch.float32)
    check(lib().ph_gk_scale(ptr(gram), None, ng, 0, float(len(loss_t_list)), ptr(scale), None, stream()), "ph_gk_scale")
    losses_div_tensor = torch.stack(list(loss_t_list))
    total_KD_loss = torch.dot(scale[:-1], losses_div_tensor)      # :68 (mirrors the slicing as written)
    return scale, total_KD_loss


def _gk_momentum_scale(opt, main_loss, feat_s, loss_t_list, state, init, sync=None):
    """The weights of the MIA-2022 trainer's GK-Refine ("MIA 2022/train_test_path_multi_distill_v2.py":89-132): the cosine
    Gram is NOT multiplied by len(loss_t_list) (:113), may be binarised with `opt.thresh` when opt.grads_thresh == "True"
    (:114-115), and the weights are an EMA over iterations with opt.grads_m (:121-124), updated in place in the caller's
    `state` (`init`: device int32 [1], 0 = no earlier iteration; both None: fresh ones).  Returns (state, init)."""
    gram, ng = _gk_gram(opt, main_loss, feat_s, loss_t_list, sync)
    if state is None:
        state = torch.zeros(ng, device=gram.device, dtype=torch.float32)
        init = torch.zeros(1, device=gram.device, dtype=torch.int32)
    check(lib().ph_gk_scale_momentum(ptr(gram), ng, 1 if opt.grads_thresh == "True" else 0, float(opt.thresh),
                                     float(opt.grads_m), ptr(state), ptr(init), stream()), "ph_gk_scale_momentum")
    return state, init


def momentum_AEKD_loss(opt, optimizer, main_loss, feat_s, loss_t_list, mo_scale, sync=None):
    """GK-Refine of the MIA-2022 trainer (_gk_momentum_scale) with the trainer's calling convention: `mo_scale` is None on
    the first call; returns (mo_scale, total_KD_loss)."""
    state = init = None
    if mo_scale is not None:
        state = mo_scale.detach().clone()
        init = torch.ones(1, device=state.device, dtype=torch.int32)
    state, _ = _gk_momentum_scale(opt, main_loss, feat_s, loss_t_list, state, init, sync)
    total_KD_loss = torch.dot(state[:-1], torch.stack(list(loss_t_list)))
    return state, total_KD_loss


def _validate_task(opt, who, surv_ok=False):
    """The task / head pairing.  Grading: the log-softmax head.  Survival (`surv_ok`, the stage-1 teacher only): exactly
    act_type Sigmoid with label_dim 1 - the reference crashes on surv with LSM (CoxLoss reshapes a [B, 3] prediction against
    B times), and its stage-2 trainers cannot run surv at all (`loss_cls.item()` on the int 0,
    train_test_path_multi_distill.py:318)."""
    task, act = getattr(opt, "task", "grad"), getattr(opt, "act_type", "LSM")
    if task == "surv" and surv_ok:
        if act != "Sigmoid" or getattr(opt, "label_dim", 1) != 1:
            raise NotImplementedError("%s: task 'surv' needs act_type 'Sigmoid' and label_dim 1 (got %r, %r)"
                                      % (who, act, getattr(opt, "label_dim", None)))
        return
    if task != "grad":
        raise NotImplementedError("%s: task %r - the survival (Cox) task is built for the stage-1 teacher only; "
                                  "this trainer runs the grading task" % (who, task))
    if act != "LSM":
        raise NotImplementedError("%s: act_type %r (the grading task uses the log-softmax head)" % (who, act))


def _validate_opt(opt, who, surv_ok=False):
    """A drop-in must fail loudly where it diverges: option values the reference's batch body would honour and this
    package does not implement raise here instead of silently training another objective."""
    _validate_task(opt, who, surv_ok)
    if getattr(opt, "reg_type", "none") not in ("none", "path", "mm", "all", "omic"):
        raise NotImplementedError("reg method [%s] is not implemented" % opt.reg_type)      # networks_new.py:106-107
    if getattr(opt, "mode", "pathomic") != "pathomic":
        raise NotImplementedError("%s: mode %r (the distillation trainers build the pathomic teacher and a path student)"
                                  % (who, opt.mode))
    if getattr(opt, "optimizer_type", "adam") not in ("adam", "adagrad"):
        raise NotImplementedError("%s: optimizer_type %r (adam and adagrad are built; adabound needs the absent `adabound` "
                                  "package, networks_new.py:82-83)" % (who, opt.optimizer_type))
    if getattr(opt, "fusion_type", "pofusion") not in ("pofusion", "polynomial_fusion"):
        raise NotImplementedError("%s: fusion_type %r (pofusion and polynomial_fusion are built)" % (who, opt.fusion_type))
    if getattr(opt, "return_grad", "False") != "False":
        raise NotImplementedError("%s: return_grad needs the reference's absent my_utils.compute_gradients" % who)
    if getattr(opt, "use_vgg_features", 0):
        raise NotImplementedError("%s: use_vgg_features (pre-extracted features bypass the ResNet trunk)" % who)
    if getattr(opt, "path_arch", "resnet18") not in ("resnet18", "resnet34"):
        raise NotImplementedError("%s: path_arch %r (the BasicBlock trunks resnet18 and resnet34 are built)" % (who, opt.path_arch))


# What DistillStep's generic loss path does for one option combination (distill_loss_plan):
#   kl          teachers that feed a KL term, in the trainers' order: a subset of ("fuse", "ema")
#   feat        the feature-level term: "crd2" (criterion_kd on the fused teacher + criterion_kd_path on the mean teacher),
#               "crd1" (one call, through criterion_kd whichever teacher is chosen), "zoo" (a distiller_zoo criterion on the
#               fused teacher's feature) or "none"
#   weighting   "gk" (the variant's GK-Refine) or "sum" (fixed weights alpha / beta)
#   rank_draws  host RNG rank draws per step (memory_new.py:311): one per CRD call of the MICCAI-2022 bank and of the DSCD banks
#               of the MIA-2022 tree (opt.crd_criterion "dscd" / "dscd_mono"), else 0
#   unused      names of the CRD criteria whose embedding heads sit in the optimiser without ever receiving a gradient
#   crd_heads   whether the CRD embedding heads are in the optimiser's parameter list at all
#   report      what the returned loss terms are: "scaled" (alpha * div, beta * kd), "unscaled_rows" (div, kd as computed, plus
#               the MIA-2023 per-sample extras rows_div1, rows_kd1, w1, w2) or "baseline" (div as computed, beta * kd)
#   kd_global   the zoo criterion returns the GLOBAL batch's loss on every replica: reported as 1 / world_size of it
LossPlan = collections.namedtuple("LossPlan", "kl feat weighting rank_draws unused crd_heads report kd_global")

ZOO_DISTILL = ("kd", "feats_KL", "rkd", "pkt", "similarity")      # `--distill` baselines of the MIA-2022 trainer (kd: no criterion)

# opt.crd_criterion of variant "mia2022": the three import lines of "MIA 2022/train_test_path_multi_distill_v2.py":24-26 -
# CRD_criterion_v3.CRDLoss (the one left uncommented there, the default), CRD_loss_v2.CRDLoss (DSCD over ContrastMemory_v4) and
# CRD_loss_v2.CRDLoss_v2 (its one-directional form; the trainer's set-up keeps it in comments at :333-337)
CRD_CRITERIA = ("v3", "dscd", "dscd_mono")


def crd_criterion_of(opt, variant):
    """The resolved opt.crd_criterion (absent: "v3"); anything else, or a DSCD criterion outside variant "mia2022", is a
    ValueError."""
    crit = getattr(opt, "crd_criterion", "v3")
    if crit not in CRD_CRITERIA:
        raise ValueError("crd_criterion %r: one of %s" % (crit, list(CRD_CRITERIA)))
    if crit != "v3" and variant != "mia2022":
        raise ValueError("crd_criterion %r belongs to variant 'mia2022' (the MIA-2022 tree's CRD_loss_v2.py)" % crit)
    return crit


def distill_loss_plan(opt, variant, sync=None):
    """The ONE place that reads num_teachers / which_teacher / distill / assign_weights: which terms the generic loss path of
    DistillStep computes, how it weights and reports them (LossPlan) - or, for a combination the reference's batch body cannot
    run or this package does not build, the exception (the reference's own type where it fails itself).  Pure: no device, no
    networks, no library."""
    nt, which, distill = opt.num_teachers, opt.which_teacher, opt.distill
    gk = opt.assign_weights == "True"
    kl = ("fuse", "ema") if nt == 2 else {"fuse": ("fuse",), "self_EMA": ("ema",)}.get(which, ()) if nt == 1 else ()
    if variant == "mia2022" and distill != "crd":
        # train_test_path_multi_distill_v2.py:316-342, 419-483: KL to one or two teachers plus one feature-level criterion
        # between the student feature and the fused teacher's, no embedding heads in the optimiser
        from .distiller_zoo import RKD_MAX_ROWS
        if distill not in ZOO_DISTILL:
            raise NotImplementedError("--distill %s (built: crd, kd, feats_KL, rkd, pkt, similarity)" % distill)
        spans_batch = sync is not None and distill in ("rkd", "pkt", "similarity")
        if spans_batch:
            # these relate every row of the batch to every other row: under data parallelism the criterion sees the
            # GLOBAL batch (the reference's nn.DataParallel gathers the outputs, :286, :307-308)
            need = ("all_gather_cat", "all_reduce_sum") if distill == "rkd" else ("all_gather_cat",)
            lack = [c for c in need if not callable(getattr(sync, c, None))]
            if lack:
                raise NotImplementedError("--distill %s with data parallelism spans the global batch: the sync object "
                                          "must provide %s" % (distill, ", ".join(lack)))
            if distill == "rkd" and opt.batch_size * sync.world_size > RKD_MAX_ROWS:
                raise ValueError("--distill rkd: global batch %d x %d exceeds the %d rows of the partitioned RKD kernel"
                                 % (opt.batch_size, sync.world_size, RKD_MAX_ROWS))
        if not kl:                                                                                          # :419-422
            raise NotImplementedError("num_teachers %r / which_teacher %r" % (nt, which))
        if gk and not (distill == "kd" and nt == 2):
            raise NotImplementedError("assign_weights with --distill %s: the trainer builds KD_loss_list only for crd and "
                                      "kd with two teachers (:463-468)" % distill)
        return LossPlan(kl, "none" if distill == "kd" else "zoo", "gk" if gk else "sum", 0, (), False, "baseline",
                        spans_batch and distill != "rkd")       # (rkd returns this replica's PART of the global loss)
    if not kl:
        # :263-271 define loss_div in three branches only; anything else reaches `loss_KD = opt.alpha * loss_div` unbound
        raise UnboundLocalError("local variable 'loss_div' referenced before assignment (num_teachers %r / which_teacher "
                                "%r: train_test_path_multi_distill.py:263-271)" % (nt, which))
    if distill not in ("crd", "kd"):
        raise NotImplementedError(distill)                                                                  # :289-290
    if gk and nt != 2:
        # :293-301 build KD_loss_list under `if opt.num_teachers == 2` only; :304 then reads it
        raise UnboundLocalError("local variable 'KD_loss_list' referenced before assignment (--assign_weights True needs "
                                "--num_teachers 2: train_test_path_multi_distill.py:293-304)")
    if gk and variant == "mia2023" and getattr(opt, "loss_weighting", "GK_refine") != "GK_refine":
        raise NotImplementedError("loss_weighting '%s' (the shipped command uses GK_refine)" % opt.loss_weighting)
    # `--distill kd`: no CRD call, both criteria idle; `--num_teachers 1`: ONE call through criterion_kd whichever teacher is
    # chosen (:282-285), criterion_kd_path idle
    feat, unused = (("none", ("criterion_kd", "criterion_kd_path")) if distill == "kd" else
                    ("crd2", ()) if nt == 2 else ("crd1", ("criterion_kd_path",)))
    calls = {"crd2": 2, "crd1": 1, "none": 0}[feat]
    # only the MIA-2023 body with both CRD calls reports its terms unscaled, with the per-sample values
    report = "unscaled_rows" if variant == "mia2023" and feat == "crd2" else "scaled"
    # host-drawn ranks: the MICCAI-2022 bank and the DSCD banks of the MIA-2022 tree (they enter a captured graph as inputs)
    ranked = variant == "miccai2022" or crd_criterion_of(opt, variant) != "v3"
    return LossPlan(kl, feat, "gk" if gk else "sum", calls if ranked else 0, unused, True, report, False)


EpochEndPlan = collections.namedtuple("EpochEndPlan", "measure use_patches add_to_average may_save")

# (patch window, checkpoint window) of the three trainers' epoch ends, and the divisor of the averaged metrics
EPOCH_END_WINDOWS = {"miccai2022": (10, 10), "mia2022": (20, 20), "mia2023": (20, 20)}
EPOCH_AVERAGE_OVER = 3.0                               # MICCAI :404, v2 :584, MIA-2023 :534


def epoch_end_plan(opt, epoch, variant):
    """What the three trainers' train() decides after the last batch of `epoch` from the options alone (EpochEndPlan) - pure,
    like distill_loss_plan.  Lines: MICCAI-2022/train_test_path_multi_distill.py | "MIA 2022/train_test_path_multi_distill_v2.py"
    | "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py".
      measure         `opt.measure or epoch == niter + niter_decay - 1` (:348 | :527 | :478): the test pass and everything below
                      run only then.  (The loop's last epoch is niter + niter_decay, :228: without opt.measure the ONE measured
                      epoch is the one before it.)
      use_patches     the nine-patch loader replaces the plain one: epoch > niter + niter_decay - 10 (:360) | - 20 (:539 | :489)
      add_to_average  epoch > niter_decay - 3 (:368 | :547 | :497); the sum is divided by 3.0 whatever the count (:404 | :584 | :534)
      may_save        the best-checkpoint test runs: epoch > niter_decay - 10 (:387) | - 20 (:566 | :516) - note niter_decay
                      alone, not niter + niter_decay.
    What depends on the epoch's numbers stays with the caller: the early stop (`task == "grad"` and the SUM loss_epoch <
    opt.patience, :383 | :562 | :512, tested BEFORE the checkpoint) and whether the mean metric beats best_acc."""
    if variant not in EPOCH_END_WINDOWS:
        raise ValueError("variant must be 'miccai2022', 'mia2022' or 'mia2023'")
    patch_w, save_w = EPOCH_END_WINDOWS[variant]
    total = opt.niter + opt.niter_decay
    measure = bool(opt.measure) or epoch == total - 1
    return EpochEndPlan(measure, measure and epoch > total - patch_w, measure and epoch > opt.niter_decay - 3,
                        measure and epoch > opt.niter_decay - save_w)


TeacherEpochEndPlan = collections.namedtuple("TeacherEpochEndPlan", "measure use_patches may_save")
TEACHER_PATCH_WINDOW, TEACHER_SAVE_AFTER = 15, 15


def teacher_epoch_end_plan(opt, epoch, variant):
    """What the three stage-1 trainers' train() decides after the last batch of `epoch` from the options alone - pure, like
    epoch_end_plan.  The three agree; lines: MICCAI-2022/train_test_MT.py | "MIA 2022/train_test_tSVD.py" |
    "MIA 2023/stage1_multi_modal_teacher/train_test_MT_SP_Masking.py".
      measure      `opt.measure or epoch == niter + niter_decay - 1` (:269 | :509 | :358): the test pass and everything below run
                   only then (the loop's last epoch is niter + niter_decay: without opt.measure the ONE measured epoch is the
                   one before it).
      use_patches  the nine-patch loader replaces the plain one: epoch > niter + niter_decay - 15 (:288 | :533 | :378).  The
                   reference rebinds `test_loader` for good; the window reaches the last epoch, so that changes nothing.
      may_save     the best-checkpoint test runs: epoch > 15 (:295 | :540 | :385) - the epoch itself, not a distance to the end.
    Both are False on an epoch that is not measured.  Whether the test metric beats best_acc stays with the caller."""
    if variant not in EPOCH_END_WINDOWS:
        raise ValueError("variant must be 'miccai2022', 'mia2022' or 'mia2023'")
    total = opt.niter + opt.niter_decay
    measure = bool(opt.measure) or epoch == total - 1
    return TeacherEpochEndPlan(measure, measure and epoch > total - TEACHER_PATCH_WINDOW, measure and epoch > TEACHER_SAVE_AFTER)


# ----------------------------------------------------------------------------------------- the hot loop
def _backward_and_update(step, loss):
    """The end of a step (train_test_path_multi_distill.py:326-329): backward, the replicas' gradient sum, fused update + EMA."""
    step.optimizer.zero_grad()
    loss.backward()
    if step.sync is not None:
        step.sync.all_reduce_grads(step.optimizer.flat)
    step.optimizer.step()


class DistillStep:
    """The batch body of train() (train_test_path_multi_distill.py:242-330) over the drop-in modules:
    student fwd, EMA fwd, teacher fwd, CE + 2xKL + 2xCRD, GK-Refine, backward, fused Adam + EMA.

    No host synchronisation inside `step` (the reference does >= 7 `.item()` syncs); losses are returned
    as device scalars."""

    def __init__(self, opt, n_data, device="cuda", k=1, sync=None, models=None, variant="miccai2022",
                 train_class_idx=None):
        """variant "miccai2022": MICCAI-2022/train_test_path_multi_distill.py:242-330 (DC-Distill CRD + GK-Refine);
        variant "mia2022": "MIA 2022/train_test_path_multi_distill_v2.py":388-500 (vanilla K+1 CRD bank of
        CRD_criterion_v3 with the epoch weight, momentum GK-Refine carried over the iterations, row a17; opt.crd_criterion
        "dscd" / "dscd_mono": that tree's CRD_loss_v2 criteria over a [B, nce_p + nce_k] index tensor);
        variant "mia2023": "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":307-448 (per-sample KL
        rows, confidence-discrepancy query weights, the class-aware KNN bank of CRD_criterion_v10 - needs
        `train_class_idx`, the per-class lists of bank rows - and the per-sample GK-Refine, row a18)."""
        from .networks_new import define_net, define_optimizer, define_scheduler
        from .kd_loss import DistillKL
        if variant not in ("miccai2022", "mia2022", "mia2023"):
            raise ValueError("variant must be 'miccai2022', 'mia2022' or 'mia2023'")
        self.crd_criterion = crd_criterion_of(opt, variant)
        if variant == "mia2022":
            if self.crd_criterion == "v3":
                from .CL_utils.CRD_criterion_v3 import CRDLoss
            elif self.crd_criterion == "dscd":
                from .CL_utils.CRD_loss_v2 import CRDLoss
            else:
                from .CL_utils.CRD_loss_v2 import CRDLoss_v2 as CRDLoss
        elif variant == "miccai2022":
            from .CL_utils import CRDLoss
        else:
            from .CL_utils.CRD_criterion_v10 import CRDLoss as _CRDv10
            from .mia2023 import DistillKL
            if train_class_idx is None:
                raise ValueError("variant 'mia2023' needs train_class_idx (CRD_criterion_v10.py:25)")
            CRDLoss = lambda o, n: _CRDv10(o, n, train_class_idx)    # noqa: E731
        self.variant = variant
        _validate_opt(opt, "DistillStep")
        if variant == "mia2023" and getattr(opt, "path_dim", 128) not in (64, 128, 256):
            # the per-sample GK-Refine (ph_gk_rows) runs on the student's feature rows, path_dim wide
            raise ValueError("DistillStep, variant 'mia2023': path_dim %r; the per-sample GK-Refine kernel is built for the "
                             "widths [64, 128, 256]" % opt.path_dim)
        self._mo_state = None     # momentum GK-Refine weights (mia2022), updated in place on the device
        self.sampler = None       # optional ContrastIndexSampler: draws sample_idx when the batch carries None
        self.loader = None        # optional augment.ResidentTileLoader: step(None) takes its batches from it
        self._loader_bt = self._sample_idx_buf = self._capture_pre = None
        self.record = None        # optional epoch.EpochRecord: every step ends with its launch (eager and captured alike)
        self.stores = None        # optional epoch.FeatureStores (mia2023): the per-sample stores, filled inside the step
        self._e_dev = None        # the epoch weight (mia2022) / re-weighting switch (mia2023) as a persistent device scalar
        self._mo_init = None
        self._lh_const = {}       # loss_head._const: small constant device vectors by value (not part of state_dict)
        self.opt = opt
        self.device = torch.device(device)
        self.sync = sync
        if models is None:
            self.fix_model = define_net(opt, k).to(self.device)
            self.model = define_net(opt, k, path_only=True).to(self.device)
            self.ema_model = define_net(opt, k, path_only=True).to(self.device)
        else:
            self.fix_model, self.model, self.ema_model = models
        for p in self.fix_model.parameters():
            p.detach_(); p.requires_grad = False                                   # :170-173
        for p in self.ema_model.parameters():
            p.detach_()                                                            # :178-180
        self.criterion_div = DistillKL(opt.kd_T)                                   # :197
        self.criterion_kd = CRDLoss(opt, n_data).to(self.device)                   # :202
        self.criterion_kd_path = CRDLoss(opt, n_data).to(self.device)              # :206
        if self.crd_criterion == "dscd_mono":      # CRDLoss_v2 has no embed_t (v2 trainer :336-337)
            self.module_list = nn.ModuleList([self.model, self.criterion_kd.embed_s, self.criterion_kd_path.embed_s])
        else:
            self.module_list = nn.ModuleList([self.model, self.criterion_kd.embed_s, self.criterion_kd.embed_t,
                                              self.criterion_kd_path.embed_s, self.criterion_kd_path.embed_t])
        # the option combination decides the loss path ONCE (or raises where the reference's body, or this package, cannot run it)
        self.plan = plan = distill_loss_plan(opt, variant, sync)
        self.zoo_kd = None        # the feature-level baseline criterion of the MIA-2022 trainer's other `--distill` choices
        if plan.feat == "zoo":
            from . import distiller_zoo as Z
            # (rkd / pkt / similarity relate the rows of the batch: with a sync object, those of the GLOBAL batch)
            self.zoo_kd = (Z.feats_KL() if opt.distill == "feats_KL" else
                           {"rkd": Z.RKDLoss, "pkt": Z.PKT, "similarity": Z.Similarity}[opt.distill](sync=sync))
        if not plan.crd_heads:
            self.module_list = nn.ModuleList([self.model])                         # v2 :316-342: no embedding heads in the optimiser
        self.optimizer = define_optimizer(opt, self.module_list)                   # :211
        self.scheduler = define_scheduler(opt, self.optimizer)                     # :212
        # a CRD criterion the option branch leaves unused: its embedding heads stay in the optimiser's parameter list as in
        # the reference, where their .grad stays None and the update skips them
        unused = [getattr(self, c) for c in plan.unused]
        if unused and hasattr(self.optimizer, "set_inactive"):
            self.optimizer.set_inactive([p for c in unused for m_ in (c.embed_s, getattr(c, "embed_t", None)) if m_ is not None
                                         for p in m_.parameters()])
        self.iter_num = opt.global_step
        self._want_graph = False
        self._static = None       # the input set of the last graph step
        self._slots = None        # the StepGraphs of the graph path, built on first need; None drops every captured graph
        self._side_stream = torch.cuda.Stream(device=self.device) if getattr(opt, "overlap_teachers", True) else None
        # the fused teacher on a third stream (opt.teacher_streams = 1: behind the mean teacher on the second)
        self._side_stream2 = (torch.cuda.Stream(device=self.device)
                              if self._side_stream is not None and getattr(opt, "teacher_streams", 2) == 2 else None)
        self._stamps = None      # int64 [16] device tensor: set BEFORE enable_graph() to have the body mark its phases
        # side stream of the fused loss head (loss_head.py: second CRD chain, head weight gradients); opt.overlap_head = False: off
        self._head_side = (torch.cuda.Stream(device=self.device)
                           if self.device.type == "cuda" and getattr(opt, "overlap_head", True) else None)
        self.module_list.train(); self.fix_model.train()                           # :231-232 (EMA stays in train mode)
        # flat EMA storage with the student's layout -> EMA is fused into the Adam kernel
        flat = self.optimizer.flat
        n_student = len(list(self.model.parameters()))
        self.ema_flat = FlatParams(list(self.ema_model.parameters()))
        self.model._direct_grad = True     # trunk gradients are written straight into the flat .grad views
        # `opt.lambda_reg * define_reg(opt, model)` (:312-313).  The stage-2 command passes --reg_type none; with `all`
        # the L1 gradient is added into the same flat buffer, so the trunk's gradients must ACCUMULATE (autograd's
        # AccumulateGrad) instead of overwriting.  `path` / `mm` / `omic` probe attributes the ResNet student does not
        # have: the reference fails with AttributeError on its first batch, here already at construction.
        self._reg_on = opt.reg_type != "none"
        if self._reg_on:
            from .networks_new import define_reg
            define_reg(opt, self.model)
            self.model._direct_grad = False
        for mod in self.ema_model.modules():
            if hasattr(mod, "_get_packed"):
                mod._follow_epoch = True   # updated by the fused Adam+EMA kernel through raw pointers
        end = flat.offsets[n_student] if n_student < len(flat.offsets) else flat.numel
        self.optimizer.ema_flat = self.ema_flat
        self.optimizer.ema_range = (0, end)
        if sync is not None:
            sync.attach(self)
            # with a regulariser the trunk gradients reach the flat buffer later, through AccumulateGrad (_direct_grad is
            # False): the layer-3/4 slice is NOT final when the trunk backward passes layer 3, so its all-reduce must not
            # start there (it would reduce a buffer that is still being accumulated into: ADVICE r02)
            if (hasattr(sync, "begin_grad_slice") and getattr(opt, "overlap_grad_allreduce", True)
                    and self.model._direct_grad):
                # everything from layer3.0.conv1.weight to the end of the flat buffer (layers 3-4, heads, CRD embeddings)
                # is final once the trunk backward has passed layer 3: its all-reduce starts there (dist.begin_grad_slice)
                first = self.model.layer3[0].conv1.weight
                lo = next(o for t, o in zip(flat.tensors, flat.offsets) if t is first)
                # (stamp 11: the moment the first phase starts - bench.py's `comm` reports the window it has to hide in)
                self.model._grad_ready_hook = lambda: (self._stamp(11), self.sync.begin_grad_slice(self.optimizer.flat, lo))[1]

    def _two_chains(self, f1, f2):
        """Two independent launch chains of ~10 short launches (the two CRD criteria: separate banks, separate heads), of the
        generic path and of the fused loss head alike: the second is issued first, on the head's side stream, the first on the
        current stream, then the join - before anything reads the second's result; autograd replays each backward on the
        stream its forward used.  One stream, f1 then f2, under data parallelism (the criteria's all-gathers must keep one
        issue order on every rank).  Every tensor f2 hands back (nested tuples included) was allocated in the side stream's
        pool and is used on this one from here on: each is recorded on it - after the join; recording before it is
        equivalent, the record only has to precede the tensor's release."""
        hs = self._head_side if self.sync is None else None
        if hs is None:
            return f1(), f2()
        main = torch.cuda.current_stream()
        hs.wait_stream(main)
        with torch.cuda.stream(hs):
            r2 = f2()
        r1 = f1()
        main.wait_stream(hs)
        todo = [r2]
        while todo:
            t = todo.pop()
            if torch.is_tensor(t):
                t.record_stream(main)
            elif isinstance(t, (tuple, list)):
                todo.extend(t)
        return r1, r2

    def _stamp(self, k):
        """Phase marker k (ph_prof_stamp: the device wall clock when the current stream gets here; also inside a graph)."""
        if self._stamps is not None:
            check(lib().ph_prof_stamp(self._stamps.data_ptr() + 8 * k, stream()), "ph_prof_stamp")

    # ------------------------------------------------------------------ one step
    def _device_body(self, x_path, ema_x_path, x_omic, grade, index, sample_idx, bnorm, e, r1, r2):
        """Everything of the step that runs on the device (capturable in one HIP graph)."""
        # The two teachers' forwards do not depend on the student's: they run on a second stream (a parallel branch
        # of the captured graph) so their small-kernel tails overlap the student's convolutions.
        main = torch.cuda.current_stream()
        side = self._side_stream
        # the student and the teacher read the same x_path (:249, :256): one packing pass into the trunk's input layout
        # serves both (before the streams fork, so both consumers are ordered after it)
        from .resnets import pack_shared_input
        self._stamp(0)
        pack_shared_input(x_path, (self.model, self.fix_model.path_net))
        side2 = self._side_stream2 if side is not None else None
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side), torch.no_grad():
                _, ema_path_feat, ema_logit_path, _, _ = self.ema_model(x_path=ema_x_path)                  # :254
                self._stamp(8)
            if side2 is not None:
                side2.wait_stream(main)
            with torch.cuda.stream(side2 if side2 is not None else side), torch.no_grad():
                fuse_feat, _, _, _, logits, pred, _, _, _, _, _ = self.fix_model(x_path=x_path, x_omic=x_omic)  # :256
                self._stamp(9)
            for t in (ema_path_feat, ema_logit_path, fuse_feat, logits[-1]):
                t.record_stream(main)
        _, path_feat, logit_path, pred_path, _ = self.model(x_path=x_path)                                   # :249
        self._stamp(1)
        if self._stamps is not None and path_feat.requires_grad:
            path_feat.register_hook(lambda g: (self._stamp(4), g)[1])
        if side is not None:
            main.wait_stream(side)
            if side2 is not None:
                main.wait_stream(side2)
        else:
            with torch.no_grad():
                _, ema_path_feat, ema_logit_path, _, _ = self.ema_model(x_path=ema_x_path)                  # :254
                fuse_feat, _, _, _, logits, pred, _, _, _, _, _ = self.fix_model(x_path=x_path, x_omic=x_omic)  # :256
        self._stamp(2)
        teachers = (ema_logit_path, logits[-1], fuse_feat, ema_path_feat)
        if self._fused_head_ok():
            # :262-313 as one function of the student feature (loss_head.py): same values, ~50 launches instead of ~125
            from .loss_head import FusedDistillLossFn, FusedMia2023LossFn, LossHeadCtx
            Hc = LossHeadCtx(self, grade, logits[-1].detach(), ema_logit_path.detach(), fuse_feat.detach(),
                             ema_path_feat.detach(), index, sample_idx, r1, r2, bnorm, variant=self.variant,
                             e_dev=e if self.variant != "miccai2022" else None)
            loss = (FusedMia2023LossFn if self.variant == "mia2023" else FusedDistillLossFn).apply(path_feat, Hc)
            loss = self._add_reg(loss)                                                                      # :312-313
            self.optimizer.zero_grad()                                                                      # :326
            self._stamp(3)
            loss.backward()                                                                                 # :327
            # the heads' weight gradients (loss_head._head_grads) - joined only where it forks that stream (`sync is None`):
            # under data parallelism it never joins the capture, and waiting on a stream outside a capture invalidates the
            # capture (hipErrorStreamCaptureIsolation)
            if self._head_side is not None and self.sync is None:
                torch.cuda.current_stream().wait_stream(self._head_side)
            self._stamp(5)
            if self.sync is not None:
                self.sync.all_reduce_grads(self.optimizer.flat)
                self._stamp(10)       # stamp 5 -> 10 = the part of the gradient all-reduce the backward did not hide
            self.optimizer.step()                                                                           # :328 (+ :329 fused)
            self._stamp(6)
            o = Hc.out
            extra = {k: o[k] for k in ("rows_div1", "rows_kd1", "w1", "w2") if k in o}       # (the MIA-2023 body's per-sample values)
            res = self._result(loss, o["loss_cls"], [o["loss_div1"], o["loss_div2"], o["loss_kd1"], o["loss_kd2"]], o["scale"],
                               (o["logit_path"], o["pred_path"], path_feat), teachers, extra)
            if self.record is None and self.stores is None:
                return res
            # the head's UNSCALED terms: `terms` [div1, div2, CE, kd1, kd2] of the MICCAI / MIA-2022 head (the CRD terms before
            # the MIA-2022 epoch weight), the reported ones of the MIA-2023 head
            if "terms" in o:
                t = o["terms"]
                kd1, kd2 = (t[3] * e, t[4] * e) if self.variant == "mia2022" else (t[3], t[4])
                return self._recorded(res, t[0], t[1], kd1, kd2, grade, index)
            return self._recorded(res, o["loss_div1"], o["loss_div2"], o["loss_kd1"], o["loss_kd2"], grade, index)
        return self._generic_loss(e, r1, r2, grade, index, sample_idx, bnorm, path_feat, logit_path, pred_path, teachers)

    def _recorded(self, res, div1, div2, kd1, kd2, grade, index):
        """The end of a step with `step.record` / `step.stores` attached: what the trainers accumulate per batch, taken from
        the terms as the body computed them - loss_div = div1 + div2 unscaled (train_test_path_multi_distill.py:266 / :268 /
        :270; a term the branch lacks is an exact zero), loss_kd = opt.beta * (kd1 + kd2) (:315) - handed to the record in
        one launch, and the MIA-2023 stores' four scatters.  The two values join the result as `rec_loss_div`, `rec_loss_kd`."""
        if self.record is not None:
            with torch.no_grad():
                res["rec_loss_div"] = (div1 + div2).detach().reshape(())
                res["rec_loss_kd"] = (self.opt.beta * (kd1 + kd2)).detach().reshape(())
            self.record.add(res, res["rec_loss_div"], res["rec_loss_kd"], grade)
        if self.stores is not None:
            self.stores.add(res, index)
        return res

    @staticmethod
    def _result(loss, loss_cls, terms, scale, student, teachers, extra=None):
        """What a step returns: the loss, its terms [div1, div2, kd1, kd2] (by the plan's reporting convention), the GK-Refine
        weights (None with fixed weights), the student's and the teachers' outputs - all detached device tensors."""
        d = [t.detach() for t in [loss, loss_cls, *terms, *student]]
        ema_logit, fuse_logit, fuse_feat, ema_feat = teachers
        return dict(loss=d[0], loss_cls=d[1], loss_div1=d[2], loss_div2=d[3], loss_kd1=d[4], loss_kd2=d[5], scale=scale,
                    logit_path=d[6], pred_path=d[7], path_feat=d[8], ema_logit=ema_logit, fuse_logit=fuse_logit,
                    fuse_feat=fuse_feat, ema_feat=ema_feat, **(extra or {}))

    def _generic_loss(self, e, r1, r2, grade, index, sample_idx, bnorm, path_feat, logit_path, pred_path, teachers):
        """Losses, backward and update of the three batch bodies on the generic autograd path, every option branch
        (MICCAI-2022 train_test_path_multi_distill.py:262-329, "MIA 2022/train_test_path_multi_distill_v2.py":419-486,
        "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":348-448), as `self.plan` lays it out: KL terms,
        feature terms, weighting, total, update, report.  Every value stays on the device.  `e`: the epoch fraction (MICCAI),
        the epoch weight of the CRD loss (MIA-2022) or the re-weighting switch (MIA-2023: 0 while epoch < opt.start_reweight -
        query weights all ones, :373-375 -, then 1) as a device scalar."""
        opt, v, plan = self.opt, self.variant, self.plan
        a, b = opt.alpha, opt.beta
        ema_logit_path, fuse_logit, fuse_feat, ema_path_feat = teachers
        rows = v == "mia2023"                   # (its DistillKL / CRDLoss also return the per-sample rows)
        z = torch.zeros((), device=self.device)                   # a term the branch does not have
        loss_cls = ops.NLLFn.apply(pred_path, grade, bnorm)                                                 # :262

        # ---- 1. KL terms (:263-271; v2 :419-422; MIA-2023 :349-350)
        div1 = div2 = kd1 = kd2 = z
        rows_div1 = rows_div2 = rows_kd1 = rows_kd2 = w1 = w2 = None
        if "fuse" in plan.kl:
            r = self.criterion_div(logit_path, fuse_logit.detach())                                         # :264
            div1, rows_div1 = r if rows else (r, None)
        if "ema" in plan.kl:
            r = self.criterion_div(logit_path, ema_logit_path.detach())                                     # :265
            div2, rows_div2 = r if rows else (r, None)

        # ---- 2. feature terms
        if rows and plan.feat in ("crd2", "crd1"):
            from .mia2023 import assign_sample_weights
            # :361-364 - log-probability margins: the softmax normaliser cancels, so the kernel reads the logits
            w1 = assign_sample_weights(logit_path, fuse_logit, grade, opt.discrep_scale, opt.max_discrep, from_logits=True)
            w2 = assign_sample_weights(logit_path, ema_logit_path, grade, opt.discrep_scale, opt.max_discrep, from_logits=True)
            w1 = (1.0 + e * w1).view(-1, 1); w2 = (1.0 + e * w2).view(-1, 1)                                # :373-382

        def crd(criterion, t_feat, w, ranks):
            """One CRD call -> (loss, per-sample rows or None)."""
            if v == "miccai2022":
                return criterion(e, path_feat, t_feat.detach(), index, sample_idx, ranks=ranks), None       # :278-279
            if v == "mia2022" and self.crd_criterion != "v3":
                # CRD_loss_v2: (epoch fraction, f_s, f_t, idx, contrast_idx) -> 0-d, no epoch weight on the term
                return criterion(self._epoch_frac, path_feat, t_feat.detach(), index, sample_idx, ranks=ranks), None
            if v == "mia2022":
                # v2 trainer :436-437: the first argument is the epoch weight of the per-sample CRD loss; result shape [1]
                return criterion(e, path_feat, t_feat.detach(), index, sample_idx).reshape(()), None
            return criterion(w, path_feat, t_feat.detach(), grade, index, sample_idx)                       # :386, :388
        if plan.feat == "crd2":
            # (the only place with two independent chains: the second runs on the head's side stream, one stream under sync)
            (kd1, rows_kd1), (kd2, rows_kd2) = self._two_chains(lambda: crd(self.criterion_kd, fuse_feat, w1, r1),
                                                                lambda: crd(self.criterion_kd_path, ema_path_feat, w2, r2))
        elif plan.feat == "crd1":
            # one teacher: the call goes through criterion_kd with that teacher's feature (MICCAI :282-285)
            kd1, rows_kd1 = crd(self.criterion_kd, *((fuse_feat, w1) if "fuse" in plan.kl else (ema_path_feat, w2)), r1)
        elif plan.feat == "zoo":
            kd1 = self.zoo_kd(path_feat, fuse_feat.detach()).reshape(())                                    # v2 :430-457

        # ---- 3. weighting
        scaled = [a * div1, a * div2, b * kd1, b * kd2]                                                     # :293-297
        scale = None
        if plan.weighting == "sum" and plan.feat == "crd2" and not rows:
            loss_KD = scaled[0] + scaled[1] + scaled[2] + scaled[3]                                         # :309 (two teachers)
        elif plan.weighting == "sum":
            # :309 as the one-teacher / kd branches reach it, v2 :482, MIA-2023 :427 (a missing term is an exact zero)
            loss_KD = a * (div1 + div2) + b * (kd1 + kd2)
        elif rows:
            from .mia2023 import GK_refine_thresh
            # MIA-2023 :407-414: per-sample rows; the CRD body's list is scaled, the `--distill kd` list is NOT (:414)
            gk_list = [a * rows_div1, a * rows_div2, b * rows_kd1, b * rows_kd2] if plan.feat == "crd2" else [rows_div1, rows_div2]
            scale, loss_KD = GK_refine_thresh(opt, self.optimizer, loss_cls, path_feat, gk_list,             # :422
                                              batch_norm_size=self.criterion_div.batch_norm_size, sync=self.sync)
        else:
            gk_list = scaled if plan.feat == "crd2" else scaled[:2]                                         # :293-300 (kd: the KL terms)
            if v == "miccai2022":
                scale, loss_KD = AEKD_loss(opt, self.optimizer, loss_cls, path_feat, gk_list, self.sync)    # :304
            else:
                # v2 trainer :474-477: momentum GK-Refine; the weight vector lives in ONE device buffer updated in place
                # (so that a captured HIP graph keeps reading / writing the same storage), x len(list) unless thresholded
                self._mo_state, self._mo_init = _gk_momentum_scale(opt, loss_cls, path_feat, gk_list, self._mo_state,
                                                                   self._mo_init, self.sync)
                self._mo_init.fill_(1)
                scale = self._mo_state.clone()       # a value snapshot for the caller; no graph through the weights
                loss_KD = torch.dot(scale[:-1], torch.stack([l.reshape(()) for l in gk_list]))
                if opt.grads_thresh == "False":
                    loss_KD = loss_KD * len(gk_list)

        # ---- 4. total, 5. update
        loss = self._add_reg(opt.lambda_nll * loss_cls + loss_KD)                                           # :312-313
        _backward_and_update(self, loss)                                                                    # :326-329

        # ---- 6. report (the plan's convention)
        student = (logit_path, pred_path, path_feat)
        rec = ((lambda res: res) if self.record is None and self.stores is None else
               (lambda res: self._recorded(res, div1, div2, kd1, kd2, grade, index)))
        if plan.report == "scaled":
            return rec(self._result(loss, loss_cls, scaled, scale, student, teachers))
        if plan.report == "unscaled_rows":
            return rec(self._result(loss, loss_cls, [div1, div2, kd1, kd2], scale, student, teachers,
                                    dict(rows_div1=rows_div1.detach(), rows_kd1=rows_kd1.detach(), w1=w1.detach(), w2=w2.detach())))
        # "baseline": the KL terms as computed, beta * criterion.  Under data parallelism rkd / pkt / similarity are losses of the
        # GLOBAL batch (distiller_zoo).  The value that entered backward() is what the criterion returns - this replica's part of
        # the global loss with the summed gradient behind it (rkd), or the global loss itself (pkt, similarity: every replica
        # evaluates it, the backward keeps its own rows) - so that the replicas' parameter gradients add up to the single-process
        # gradient.  The REPORTED `loss_kd1` and `loss` follow the step's convention that the replicas' values add up to the
        # single-process ones: this replica's part (rkd), the global value / world_size (pkt, similarity: plan.kd_global).
        loss, kd = loss.detach(), kd1.detach()
        if plan.kd_global:
            w = float(self.sync.world_size)
            loss = loss - b * (kd - kd / w)
            kd = kd / w
        return rec(self._result(loss, loss_cls, [div1, div2, b * kd, z], scale, student, teachers))

    def _add_reg(self, loss):
        """+ opt.lambda_reg * define_reg(opt, model) (train_test_path_multi_distill.py:312-313)."""
        if not self._reg_on:
            return loss
        from .networks_new import define_reg
        # replicas SUM their losses / gradients (global-batch normalisers): the batch-independent L1 term is split evenly
        # so that the sum carries it once, as the reference's one DataParallel process does
        w = self.sync.world_size if self.sync is not None else 1
        return loss + (self.opt.lambda_reg / w) * define_reg(self.opt, self.model)

    def _fused_head_ok(self):
        """The closed-form loss head covers the shipped MICCAI and MIA-2022 stage-2 commands: two teachers, CRD, GK-Refine
        (plain / momentum) with the CE gradient, a log-softmax grading head.  `opt.fused_loss_head = False` selects the
        generic autograd path."""
        opt, plan = self.opt, self.plan
        if getattr(opt, "sample_KD", "False") != "False":
            # per-sample CRD rows ([B]-shaped loss_kd): the reference's body then fails inside AEKD_loss's `loss_t.backward()`
            # ("grad can be implicitly created only for scalar outputs") - the generic path fails the same way, the closed
            # form would silently compute something else
            return False
        if self._reg_on:
            # the fused head WRITES fc_new2's gradients (accumulate=False) after L1RegFn.backward has added
            # lambda_reg * sgn(W) into the same flat buffer: the L1 term on fc_new2 would be lost
            return False
        if self.variant != "miccai2022" and not torch.is_tensor(self._e_dev):
            return False
        if self.variant == "mia2023" and getattr(opt, "pos_extra", "neighbors") != "neighbors":
            return False
        if self.crd_criterion == "dscd_mono":
            # one direction, no embed_t: the closed form's CRD chain and head-gradient tail are written for two heads per
            # criterion - the one-directional criterion stays on the generic path
            return False
        return (getattr(opt, "fused_loss_head", True) and plan.feat == "crd2" and plan.weighting == "gk"
                and bool(opt.CE_grads)
                and isinstance(getattr(self.model, "fc_new2", None), nn.Linear)
                and isinstance(getattr(self.model, "act", None), nn.LogSoftmax))

    def _draw_ranks(self, epoch, ranks):
        """Host-RNG rank draws of memory_new.py:311 for the two CRD calls (kd1 then kd2), as device int32."""
        e = epoch / self.opt.niter_decay
        out = []
        # the host RNG advances once per CRD CALL of the MICCAI-2022 bank (memory_new.py:311): two calls in the shipped command,
        # one with --num_teachers 1 (through criterion_kd), none with --distill kd; the vanilla / KNN banks of the other
        # variants have no rank-drawn pair selection
        for i, crd in enumerate((self.criterion_kd, self.criterion_kd_path)):
            if i >= self.plan.rank_draws:
                out.append(None)
                continue
            r = ranks[i] if ranks is not None else crd.contrast.draw_ranks(e, crd.select_pos_mode)
            out.append(None if r is None else torch.as_tensor(np.asarray(r), dtype=torch.int32))
        return e, out

    def enable_graph(self):
        """Replay the device part of the step from ONE captured HIP graph (the step is ~700 kernel launches;
        eager dispatch makes it host-bound).  Call after at least two eager steps (first-call CRD Z, lazy plans);
        shapes must stay fixed afterwards."""
        self._want_graph = True

    def step(self, batch, epoch=0, ranks=None):
        opt = self.opt
        # :231-232 re-asserted per call: the reference sets train mode at every epoch because its test() leaves the
        # networks in eval mode (evaluate.test does the same here); the EMA model is never put in eval mode there
        self.module_list.train(); self.fix_model.train()
        self._capture_pre = None
        if batch is None:
            # on-device input pipeline (augment.ResidentTileLoader, `step.loader = loader`): the batch is produced from the
            # resident tile store.  In graph mode the loader's launches are captured IN FRONT of the step's own, so a
            # replay is the whole iteration - shuffle indices, both augmented views, contrast indices, step - and the host
            # launches nothing in between (eager launches between replays cost 1-4 ms per step on this runtime).
            loader = self.loader
            if loader is None:
                raise ValueError("step(None) needs step.loader (augment.ResidentTileLoader)")
            in_graph = self._want_graph and self.iter_num - opt.global_step >= 2
            if self._loader_bt is None:
                self._loader_bt = loader.next(opt.batch_size)          # allocates the resident input set
            elif not in_graph:
                loader.next(into=self._loader_bt)
            batch = self._loader_bt
            if in_graph:
                self._capture_pre = lambda: loader.next(into=self._loader_bt)
        (x_path, ema_x_path), x_grph, x_omic, censor, survtime, grade, index, sample_idx = batch
        dev = self.device
        if sample_idx is None:
            # the loader's contrast-index draw (data_loaders_MT.py:229-249) on the device: set `step.sampler` to a
            # ContrastIndexSampler built from the training labels; one launch per step, outside the captured graph
            if self.sampler is None:
                raise ValueError("the batch carries no sample_idx and no step.sampler (ContrastIndexSampler) is set")
            buf = self._sample_idx_buf
            if buf is None or buf.shape[0] != index.shape[0]:
                buf = self._sample_idx_buf = torch.empty(index.shape[0], self.sampler.width, device=dev, dtype=torch.int64)
            sample_idx = self.sampler(index, grade, out=buf)
        bnorm = float(x_path.shape[0] * (self.sync.world_size if self.sync is not None else 1))
        self.criterion_div.batch_norm_size = bnorm
        self.criterion_kd.contrast.batch_norm_size = bnorm
        self.criterion_kd_path.contrast.batch_norm_size = bnorm
        e, rk = self._draw_ranks(epoch, ranks)
        self._epoch_frac = e
        if self.crd_criterion != "v3" and sample_idx.shape[1] != opt.nce_p + opt.nce_k:
            raise RuntimeError("crd_criterion %r: sample_idx must be [B, nce_p + nce_k] = [B, %d + %d], got width %d (the v3 "
                               "criterion's width is nce_k + 1 = %d)" % (self.crd_criterion, opt.nce_p, opt.nce_k,
                                                                          sample_idx.shape[1], opt.nce_k + 1))
        if self.variant != "miccai2022":
            # the epoch weight multiplies the CRD loss on the device (mia2022) / switches the re-weighting on (mia2023, :373):
            # one persistent scalar so a captured graph reads the current value instead of baking the capture-time epoch in
            if self._e_dev is None:
                self._e_dev = torch.zeros(1, device=dev, dtype=torch.float32)
            # (the DSCD criteria carry no epoch weight: the scalar ph_gk_finish_momentum multiplies in is 1)
            self._e_dev.fill_((float(e) if self.crd_criterion == "v3" else 1.0) if self.variant == "mia2022"
                              else 0.0 if epoch < opt.start_reweight else 1.0)
            e = self._e_dev
        self.optimizer.ema_alpha = min(1 - 1 / (self.iter_num + 1), opt.ema_decay)                          # :36
        use_graph = self._want_graph and self.iter_num - opt.global_step >= 2
        if not use_graph:
            x_path = x_path.to(dev, non_blocking=True)                             # ONE H2D copy (reference: three)
            ema_x_path = ema_x_path.to(dev, non_blocking=True)
            x_omic = x_omic.to(dev, non_blocking=True)
            grade = grade.to(dev, non_blocking=True)
            index = index.to(dev, non_blocking=True)
            sample_idx = sample_idx.to(dev, non_blocking=True)
            r1, r2 = [None if r is None else r.to(dev, non_blocking=True) for r in rk]
            self.optimizer.prepare_step()
            out = self._device_body(x_path, ema_x_path, x_omic, grade, index, sample_idx, bnorm, e, r1, r2)
            self.iter_num += 1
            return out
        # ---- graph path: per-step scalars in device memory, inputs at fixed addresses (step_graph.py: resident input sets
        # are adopted and replayed without a copy, anything else is staged into one private set: 2 x 76 us for two 201 MB views)
        given = dict(zip(self._IN_NAMES, (x_path, ema_x_path, x_omic, grade, index, sample_idx)))
        if self._slots is None:
            self._slots = StepGraphs(self.device, "distill", self._IN_NAMES, (self.model, self.ema_model, self.fix_model))
        st = self._slots.input_set(given)
        hit = self._graph(st, rk, bnorm, e)
        if hit is None:                      # capture failed: eager from now on
            self._static = None
            out = self._device_body(*[given[k].to(dev) for k in self._IN_NAMES], bnorm, e,
                                    *[None if r is None else r.to(dev) for r in rk])
            self.iter_num += 1
            return out
        self._static = st
        for j, (dst, src) in enumerate(zip(st["r"], rk)):
            if dst is not None:
                ring = st.setdefault("r_ring", {}).get(j)
                if ring is None:
                    ring = st["r_ring"][j] = PinnedRing(tuple(dst.shape), torch.int32)
                ring.upload(dst, src)
        self.optimizer.prepare_step()
        self.optimizer._prepared = False
        hit[0].replay()
        self.iter_num += 1
        return hit[1]

    _IN_NAMES = ("x_path", "ema_x_path", "x_omic", "grade", "index", "sample_idx")

    def _graph(self, st, r_like, bnorm, e):
        """(graph, outputs) of the step on the input set `st`, which owns the rank buffers `r` of the two CRD calls."""
        if "r" not in st:
            st["r"] = [None if r is None else torch.empty(tuple(r.shape), device=self.device, dtype=torch.int32) for r in r_like]
        # (_capture_pre: the on-device input pipeline fills this input set first)
        return self._slots.graph(self, st, "step", lambda: self._device_body(*[st[k] for k in self._IN_NAMES], bnorm, e, *st["r"]),
                                 first=self._capture_pre)

    def precapture(self, batch, epoch=0):
        """Capture the graph for another resident input set without running a step (e.g. the second buffer of a
        loader's two-deep ring, so that its first use does not pay the capture).  Needs one graph step done before.
        False if the set cannot have a graph of its own (host tensors, or both adopted sets are other tensors)."""
        slots = self._slots
        if not slots or not slots[0]["graphs"]:
            raise RuntimeError("precapture: run a graph-mode step first")
        (x_path, ema_x_path), _, x_omic, _, _, grade, index, sample_idx = batch
        given = dict(zip(self._IN_NAMES, (x_path, ema_x_path, x_omic, grade, index, sample_idx)))
        bnorm = float(x_path.shape[0] * (self.sync.world_size if self.sync is not None else 1))
        e = self._e_dev if self.variant != "miccai2022" else epoch / self.opt.niter_decay
        r_like = slots[0]["r"]
        st = slots.input_set(given, stage=False)
        return st is not None and self._graph(st, r_like, bnorm, e) is not None

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        """Everything a bit-identical resume needs.  The reference saves `model_state_dict` + `optimizer_state_dict`
        only (train_test_path_multi_distill.py:387-402) and silently loses the CRD banks, their normalisation
        constants Z, the embed heads' optimiser state, the EMA model and the step counter; the first two keys are kept
        reference-compatible, the rest is added."""
        rng = {}
        for name, mod in self.fix_model.named_modules():
            if hasattr(mod, "rng_step"):
                rng[name] = mod.rng_step.clone()
        return dict(model_state_dict=self.model.state_dict(), optimizer_state_dict=self.optimizer.state_dict(),
                    ema_model_state_dict=self.ema_model.state_dict(), teacher_state_dict=self.fix_model.state_dict(),
                    crd_kd_state_dict=self.criterion_kd.state_dict(),
                    crd_kd_path_state_dict=self.criterion_kd_path.state_dict(),
                    scheduler_state_dict=self.scheduler.state_dict(), iter_num=self.iter_num,
                    crd_criterion=self.crd_criterion,
                    teacher_rng_steps=rng,
                    gk_momentum_scale=None if self._mo_state is None else self._mo_state.clone(),
                    # draw counters of the on-device input pipeline and the host RNG behind the CRD rank draws
                    # (memory_new.py:311): without them a resumed run with step(None) / step.sampler draws other batches
                    input_rng=self._input_rng_state(),
                    # step counters / seeds of the `contrast_idx is None` draws (CL_utils/memory_new.draw_uniform_indices)
                    crd_draw_steps=[(None if c.contrast._draw_step is None else c.contrast._draw_step.clone(), c.contrast._draw_seed)
                                    for c in (self.criterion_kd, self.criterion_kd_path)])

    def _input_rng_state(self, load=None):
        """Device-side draw counters of step.sampler / step.loader (ContrastIndexSampler.step, DeviceAugment.step,
        ResidentTileLoader.batch_no) and numpy's global RNG state; `load` restores a dict this method returned."""
        loader = self.loader
        cells = dict(sampler=getattr(self.sampler, "step", None),
                     loader_sampler=getattr(getattr(loader, "sampler", None), "step", None),
                     loader_aug=getattr(getattr(loader, "aug", None), "step", None),
                     loader_batch_no=getattr(loader, "batch_no", None))
        if load is None:
            out = {k: (None if t is None else t.clone()) for k, t in cells.items()}
            # numpy's MT19937 state as tensors / plain scalars: `torch.load(weights_only=True)` (the default since
            # torch 2.6) rejects numpy globals, so the raw get_state() tuple would make the checkpoint unloadable
            name, key, pos, has_gauss, cached = np.random.get_state()
            out["numpy"] = dict(name=str(name), key=torch.from_numpy(key.astype(np.int64)), pos=int(pos),
                                has_gauss=int(has_gauss), cached_gaussian=float(cached))
            return out
        for k, t in cells.items():
            v = load.get(k)
            if v is None:
                continue
            if t is None:
                if k == "loader_batch_no" and loader is not None:
                    loader.batch_no = v.to(self.device).clone()
                    continue
                raise RuntimeError("checkpoint carries the draw counter %r but this step has no such component" % k)
            t.copy_(v)
        st = load.get("numpy")
        if st is not None:
            # NOTE: restores the PROCESS-GLOBAL numpy RNG (the reference draws its CRD ranks from it, memory_new.py:311)
            if isinstance(st, dict):
                st = (st["name"], np.asarray(st["key"].cpu().numpy(), dtype=np.uint32), int(st["pos"]), int(st["has_gauss"]),
                      float(st["cached_gaussian"]))
            np.random.set_state(st)

    def load_state_dict(self, sd):
        if sd.get("crd_criterion", "v3") != self.crd_criterion:      # (a checkpoint from before the option: "v3")
            raise ValueError("the checkpoint was written under crd_criterion %r, this step runs %r"
                             % (sd.get("crd_criterion", "v3"), self.crd_criterion))
        self.model.load_state_dict(sd["model_state_dict"])
        self.ema_model.load_state_dict(sd["ema_model_state_dict"])
        self.fix_model.load_state_dict(sd["teacher_state_dict"])
        for crd, key in ((self.criterion_kd, "crd_kd_state_dict"), (self.criterion_kd_path, "crd_kd_path_state_dict")):
            crd.load_state_dict(sd[key])      # (the bank's _load_from_state_dict tells from Z whether the first call is past)
        self.optimizer.load_state_dict(sd["optimizer_state_dict"])
        self.scheduler.load_state_dict(sd["scheduler_state_dict"])
        self.iter_num = sd["iter_num"]
        mo = sd.get("gk_momentum_scale")
        if mo is not None:
            if self._mo_state is None:
                self._mo_state = torch.zeros_like(mo, device=self.device)
                self._mo_init = torch.ones(1, device=self.device, dtype=torch.int32)
            self._mo_state.copy_(mo); self._mo_init.fill_(1)
        for name, mod in self.fix_model.named_modules():
            if hasattr(mod, "rng_step") and name in sd.get("teacher_rng_steps", {}):
                mod.rng_step.copy_(sd["teacher_rng_steps"][name])
        if sd.get("input_rng") is not None:
            self._input_rng_state(load=sd["input_rng"])
        for c, rec in zip((self.criterion_kd, self.criterion_kd_path), sd.get("crd_draw_steps") or ()):
            if rec[0] is not None:
                c.contrast._draw_step = rec[0].to(self.device).clone()
                c.contrast._draw_seed = rec[1]
        ops.bump_weight_epoch()      # packed MFMA weight images are rebuilt from the loaded parameters
        self._static = None          # a captured graph keeps pointing at valid buffers, but is rebuilt to be safe
        self._slots = None

    def static_inputs(self):
        """The graph path's resident input buffers (fill them in place to skip the device-to-device copy)."""
        st = self._static
        return None if st is None else {k: st[k] for k in self._IN_NAMES}


class _GatherRowsFn(torch.autograd.Function):
    """All-gather of feature rows with a local backward: forward returns the rows of every replica (rank order),
    backward returns the gradient of THIS replica's rows.  Every replica evaluates the same function of the gathered
    rows (the t-SVD penalty), so the partial derivative with respect to its own rows is complete as it stands; the
    gradient all-reduce then adds the replicas' parameter gradients."""

    @staticmethod
    def forward(ctx, x, sync):
        ctx.lo, ctx.n = sync.rank * x.shape[0], x.shape[0]
        return sync.all_gather_cat(x.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        return g[ctx.lo:ctx.lo + ctx.n].contiguous(), None


SURV_MAX_GLOBAL_BATCH = 4096      # one workgroup of ph_surv_stage1_loss_grad(_gathered), every row in LDS


class TeacherStage1Step:
    """The batch body of the stage-1 mean-teacher trainer (MICCAI-2022/train_test_MT.py:121-230) for the
    grading task: student PathomicNet forward/backward, EMA PathomicNet forward, three-branch NLL (:208-212),
    `pred_KD_loss` consistency (CL_utils/KD_losses.py:12-36; --num_teachers 1/2/3, :180-201), the optional vanilla
    CRD term on the fused features (--CRD_distill 1, CL_utils/CRD_criterion.py) and orthogonality term (--orth_loss
    True, CL_utils/orthogonal_loss.py), Adam, EMA update.  (--SP_distill names a class the reference never imports.)"""

    def __init__(self, opt, device="cuda", k=1, models=None, sync=None):
        """`sync`: a dist.ReplicaSync for data parallelism (one process per GPU, `opt.batch_size` tiles each).  Loss
        normalisers use the global batch, the vanilla CRD bank is updated identically on every replica, the
        cross-correlation of the orthogonality loss is all-reduced, and the t-SVD adjacency tensors are built over the
        global batch from all-gathered feature views (every replica computes the same auxiliary tensors; the penalty's
        gradient reaches this replica's rows only, the gradient all-reduce adds the replicas up).
        Under the survival task `sync` must provide `all_gather_into` (else NotImplementedError), and the global batch
        opt.batch_size x world_size is at most 4096 (the one-workgroup survival kernel, else ValueError): each step packs
        this replica's survival rows into one block, all-gathers it, and computes the Cox and consistency terms over the
        global batch (ops.SurvStage1GatheredFn), as the reference's nn.DataParallel does on its gathered outputs.  The
        survival outputs (`loss_cox*`, `loss_kd_*` and the survival part of `loss`) are then global-batch values, the same
        on every replica (like `loss_tsvd`); the CRD, masking and regulariser parts of `loss` stay partial per replica."""
        from .networks_new import define_net, define_optimizer, define_scheduler
        self.opt = opt
        self.device = torch.device(device)
        self.sync = sync
        _validate_opt(opt, "TeacherStage1Step", surv_ok=True)
        # survival task (--task surv --act_type Sigmoid --label_dim 1, train_test_MT.py:149-152): the three Cox terms and
        # MSE consistency terms in one launch (ops.SurvStage1LossFn); survtime / censor become step inputs
        self.surv = getattr(opt, "task", "grad") == "surv"
        if self.surv:
            if sync is not None:
                if not callable(getattr(sync, "all_gather_into", None)):
                    raise NotImplementedError("TeacherStage1Step: task 'surv' with data parallelism - the Cox risk sets span "
                                              "the global batch: the sync object must provide all_gather_into")
                if opt.batch_size * sync.world_size > SURV_MAX_GLOBAL_BATCH:
                    raise ValueError("TeacherStage1Step: task 'surv' with a global batch of %d x %d: the survival loss "
                                     "kernel holds at most %d rows" % (opt.batch_size, sync.world_size, SURV_MAX_GLOBAL_BATCH))
            if getattr(opt, "tSVD_loss", "False") == "True":
                raise NotImplementedError("TeacherStage1Step: task 'surv' with tSVD_loss (no reference vectors pin it)")
            if getattr(opt, "masking", 0):
                raise NotImplementedError("TeacherStage1Step: task 'surv' with masking (no reference vectors pin it)")
            if getattr(opt, "pred_distill", 1) == 1 and opt.num_teachers not in (1, 2, 3):
                raise NotImplementedError("TeacherStage1Step: task 'surv' with num_teachers %r (train_test_MT.py:180-201 "
                                          "builds 1, 2 or 3)" % (opt.num_teachers,))
            self._IN_NAMES = TeacherStage1Step._IN_NAMES + ("survtime", "censor")
        if models is None:
            self.model = define_net(opt, k).to(self.device)
            self.ema_model = define_net(opt, k).to(self.device)
        else:
            self.model, self.ema_model = models
        for p in self.ema_model.parameters():
            p.detach_()                                                             # train_test_MT.py:74-76
        # optional terms: vanilla CRD between the student's and the EMA teacher's fused features (:74-76,157-165; the
        # reference builds three criteria, appends all six embed heads to the optimiser and uses the `fuse` one) and the
        # orthogonality loss between the path and omic features (:79,216-218)
        self.crd_on = getattr(opt, "CRD_distill", 0) == 1
        self.orth_on = getattr(opt, "orth_loss", "False") == "True"
        if getattr(opt, "SP_distill", 0) == 1:
            raise NotImplementedError("--SP_distill: the reference's stage-1 trainer cannot run it either (its `Similarity` "
                                      "import is commented out, train_test_MT.py:27,169)")
        module_list = nn.ModuleList([self.model])
        if self.crd_on:
            from .CL_utils.CRD_criterion import CRDLoss as CRDLossV0
            self.CRD_criterion_path = CRDLossV0(opt).to(self.device)
            self.CRD_criterion_omic = CRDLossV0(opt).to(self.device)
            self.CRD_criterion_fuse = CRDLossV0(opt).to(self.device)
            for c in (self.CRD_criterion_path, self.CRD_criterion_omic, self.CRD_criterion_fuse):
                c.contrast.verbose = False
            # :84-90 appends all six heads to the optimiser, but only the `fuse` pair ever receives a gradient and
            # torch's Adam skips parameters whose .grad is None: the other four never change.  The flat fused Adam has
            # no "None" gradients (it would apply weight decay to them), so they are simply left out.
            module_list.append(self.CRD_criterion_fuse.embed_s); module_list.append(self.CRD_criterion_fuse.embed_t)
        if self.orth_on:
            from .CL_utils.orthogonal_loss import OrthLoss
            self.Orth_loss = OrthLoss()
        # t-SVD low-rank constraint of the MIA-2022 stage-1 trainer ("MIA 2022/train_test_tSVD.py":161-181,299-431):
        # adjacency tensors over n_views feature views per modality, auxiliary tensors from the tensor-nuclear-norm prox
        self.tsvd_on = getattr(opt, "tSVD_loss", "False") == "True"
        if self.tsvd_on:
            if opt.n_views not in (2, 4, 6, 8):
                raise ValueError("n_views %d (train_test_tSVD.py:309-363 builds 2, 4, 6 or 8 views)" % opt.n_views)
            if opt.tSVD_mode not in ("path", "omic", "pathomic"):
                raise ValueError(opt.tSVD_mode)
            self.mu = float(opt.mu)                                                              # :161 (never reset per epoch)
            gb = opt.batch_size * (sync.world_size if sync is not None else 1)
            from .tsvd import TSVD_MAX_ROWS
            if gb > TSVD_MAX_ROWS:
                raise ValueError("tSVD_loss: global batch %d (batch_size %d x world size %d) exceeds TSVD_MAX_ROWS = %d of the "
                                 "proximal update" % (gb, opt.batch_size, gb // opt.batch_size, TSVD_MAX_ROWS))
            z = lambda: [torch.zeros(gb, gb, device=self.device) for _ in range(opt.n_views)]
            self.adj_tensor1, self.aux_tensor1, self.adj_tensor2, self.aux_tensor2 = z(), z(), z(), z()   # :165-177
            self.path_TNN = self.omic_TNN = None
            self._batch_idx = 0
        self.optimizer = define_optimizer(opt, module_list if self.crd_on else self.model)      # :86-94
        self.module_list = module_list      # (what the reference's train() returns first)
        self.scheduler = define_scheduler(opt, self.optimizer)
        # a fusion gate that is off leaves linear_h_k / linear_z_k unread (fusion.py:45-46,52-53): they stay in the optimiser's
        # list as in the reference, where their .grad stays None and the update skips them - unless the regulariser reaches
        # them (`--reg_type all` sums |W| over every parameter and gives them a gradient)
        fusion = getattr(self.model, "fusion", None)
        unused = fusion.unused_parameters() if hasattr(fusion, "unused_parameters") else []
        self._unused_ids = set()
        if unused and opt.reg_type != "all" and hasattr(self.optimizer, "set_inactive"):
            self.optimizer.set_inactive(unused)
            self._unused_ids = {id(p) for p in unused}
        self.iter_num = opt.global_step
        self.model.train(); self.ema_model.train()
        self.ema_flat = FlatParams(list(self.ema_model.parameters()))
        for mod in self.ema_model.modules():
            if hasattr(mod, "_get_packed"):
                mod._follow_epoch = True
        self.optimizer.ema_flat = self.ema_flat
        n_model = len(list(self.model.parameters()))
        flat = self.optimizer.flat
        self.optimizer.ema_range = (0, flat.offsets[n_model] if n_model < len(flat.offsets) else flat.numel)
        self._want_graph = False
        self.record = None        # optional epoch.Stage1Record: every step ends with its launch (eager and captured alike)
        self._g_sets = StepGraphs(self.device, "stage-1", self._IN_NAMES, (self.model, self.ema_model))
        self._g_scal = self._g_ring = None      # the graph path's CRD weight | tau | mu of the penalty on the device
        self._ema_side = self._tsvd_side = None      # side streams, created on first use
        self._frozen_segs = self._surv_gather = None
        self._f32_bufs = {}
        if sync is not None:
            crds = (self.CRD_criterion_path, self.CRD_criterion_omic, self.CRD_criterion_fuse) if self.crd_on else ()
            sync.attach_parts(crds, (flat.flat, self.ema_flat.flat), (self.model, self.ema_model))
            if self.orth_on:
                self.Orth_loss.sync = sync

    def _as_f32(self, name, t):
        """survtime / censor as float32 (the survival kernel's type).  A float32 tensor passes as it is; a device tensor of
        another dtype is converted into a persistent buffer, so that its pointer stays put and a captured graph can adopt it
        (a fresh temporary every step would fill the adopted input sets with throwaway copies); a host tensor is converted
        on the host (it is staged or uploaded anyway)."""
        if t.dtype == torch.float32:
            return t
        if not t.is_cuda:
            return t.float()
        b = self._f32_bufs.get(name)
        if b is None or b.shape != t.shape or b.device != t.device:
            b = self._f32_bufs[name] = torch.empty(t.shape, device=t.device, dtype=torch.float32)
        b.copy_(t)
        return b

    def _ema_frozen(self):
        """update_ema_variables (:34-38, :229) covers EVERY parameter, output_range / output_shift included; the fused Adam step
        updates the EMA copy of the trained ones only.  Under surv the sigmoid head reads those two, so their EMA copies
        follow here (rate from the optimiser's device record: graph-replayable).  Grading leaves them alone: its head never
        reads them.  The student tensors that an option leaves unused (`_unused_ids`: no gradient, no Adam update) follow under
        both tasks: update_ema_variables still moves their EMA copies towards the unchanged student values."""
        opt_ = self.optimizer
        if self._frozen_segs is None:
            f, hi = opt_.flat, opt_.ema_range[1]
            left_out = lambda t: (self.surv and not t.requires_grad) or id(t) in self._unused_ids      # noqa: E731
            self._frozen_segs = [(s, min(e, hi)) for s, e in f.segments(left_out) if s < hi]
        f = opt_.flat
        for s, e in self._frozen_segs:
            check(lib().ph_ema_update_dev(ptr(self.ema_flat.flat[s:e]), ptr(f.flat[s:e]), e - s, ptr(opt_._hyper), stream()),
                  "ph_ema_update_dev")

    def _surv_gather_bufs(self, input_set, n):
        """The staging / gathered buffers of the survival all-gather (ops.surv_gather_buffers), allocated once per graph input
        set (captured graphs keep their addresses) and once for the eager steps; a new batch size replaces them."""
        holder = input_set if input_set is not None else self.__dict__
        bufs = holder.get("_surv_gather")
        if bufs is None or bufs[0].shape[1] != n:
            bufs = holder["_surv_gather"] = ops.surv_gather_buffers(n, self.sync.world_size, self.device)
        return bufs

    @staticmethod
    def pred_KD_loss(p_s, p_t, bnorm=None):
        """KD_losses.py:27-29 (grading, sample_KD False): sum(kl_div(p_s, exp(p_t))) / B on log-probabilities - the KL
        kernel at T = 1 (log_softmax of a log-probability vector is the vector itself).  `bnorm`: the global batch
        under data parallelism."""
        return ops.KLFn.apply(p_s, p_t.detach(), 1.0, float(bnorm or p_s.shape[0]))

    def start_epoch(self):
        """The t-SVD auxiliary update runs every opt.aux_iter batches of an epoch (:375): reset the batch counter."""
        self._batch_idx = 0

    def enable_graph(self):
        """Replay the device part of the step from captured HIP graphs (one per resident input set and per kind of step -
        with / without the t-SVD auxiliary update).  Call after at least two eager steps; shapes must stay fixed.  The
        per-step scalars that the eager path bakes into its launches (the CRD weight that drops at epoch 15, the t-SVD
        threshold Lambda / mu and the penalty's mu, Adam's bias corrections, the EMA rate) are read from device memory.
        Steps with the superpixel-masking terms (MIA-2023 stage 1) stay eager: their attention masks are built with host
        control flow."""
        self._want_graph = True

    def step(self, batch, epoch=0, batch_idx=None):
        opt = self.opt
        self.model.train()              # train_test_MT.py:110 `module_list.train()` per epoch (its test() leaves eval mode)
        if epoch >= 15:
            opt.CRD_weight = 0.01                                                                # train_test_MT.py:118-119
        views, x_grph, x_omic, censor, survtime, grade, index, sample_idx = batch
        sp_mask = x_path_m_v1 = x_path_m_v2 = None
        if len(views) == 6:      # the MIA-2023 loader (train_test_MT_SP_Masking.py:185): superpixel maps and two masked views
            x_path, sp_mask, ema_x_path, _, x_path_m_v1, x_path_m_v2 = views
        else:
            x_path, ema_x_path = views
        dev = self.device
        B = float(x_path.shape[0] * (self.sync.world_size if self.sync is not None else 1))   # global batch
        self.optimizer.ema_alpha = min(1 - 1 / (self.iter_num + 1), opt.ema_decay)
        masking_on = bool(getattr(opt, "masking", 0)) and epoch > opt.start_epoch
        # t-SVD schedule on the host: whether this batch updates the auxiliary tensors (:375), the threshold it uses and the
        # mu of the penalty, which is the value AFTER the update's `mu = min(mu * pho, max_mu)` (:413)
        do_aux, tau, mu_pen, bidx = False, 0.0, 0.0, 0
        if self.tsvd_on:
            bidx = self._batch_idx if batch_idx is None else batch_idx
            do_aux = bidx % opt.aux_iter == 0
            tau = opt.Lambda_global / self.mu
            mu_pen = min(self.mu * opt.pho, opt.max_mu) if do_aux else self.mu
        given = dict(x_path=x_path, ema_x_path=ema_x_path, x_omic=x_omic, grade=grade, index=index, sample_idx=sample_idx)
        if self.surv:
            given["survtime"] = self._as_f32("survtime", survtime)
            given["censor"] = self._as_f32("censor", censor)
        use_graph = (self._want_graph and not masking_on and self.iter_num - opt.global_step >= 2
                     and all(torch.is_tensor(t) for t in given.values()))
        out = None
        if use_graph:
            out = self._graph_step(given, B, do_aux, float(getattr(opt, "CRD_weight", 1.0)), tau, mu_pen)
        if out is None:
            loss_masking = None
            x_path, ema_x_path = x_path.to(dev, non_blocking=True), ema_x_path.to(dev, non_blocking=True)
            x_omic, grade = x_omic.to(dev, non_blocking=True), grade.to(dev, non_blocking=True)
            if masking_on:                                                                       # MIA-2023 :198-220
                # superpixel attention: mask the Path_K superpixels / Omic_K genes the fused prediction is most sensitive to
                # and ask the two masked views to agree with the mean teacher's predictions on the loader's masked views
                from . import superpixel as SPX
                if sp_mask is None:
                    raise ValueError("opt.masking needs the 6-view loader tuple (x_path, sp_mask, ema_x_path, ema_sp_mask, "
                                     "x_path_m_v1, x_path_m_v2)")
                for mod in self.model.modules():
                    if hasattr(mod, "_get_workspace"):
                        mod._multi_forward = True     # three taped forwards of the same trunk before one backward
                pm, om = SPX.superpixel_attention_mask(opt, self.optimizer, self.model, x_path, x_grph, x_omic, sp_mask, grade,
                                                       dev, getattr(opt, "num_superpixels_max", None))
                pred_m1 = self.model(x_path=SPX.apply_mask(x_path, pm), x_omic=x_omic)[5]            # :204-205
                pred_m2 = self.model(x_path=x_path, x_omic=SPX.apply_mask(x_omic, om))[5]            # :207-208
                with torch.no_grad():
                    ema_m1 = self.ema_model(x_path=x_path_m_v1.to(dev), x_omic=x_omic)[5]             # :211-215
                    ema_m2 = self.ema_model(x_path=x_path_m_v2.to(dev), x_omic=x_omic)[5]
                loss_masking = self.pred_KD_loss(pred_m1, ema_m1, B) + self.pred_KD_loss(pred_m2, ema_m2, B)   # :217-220
            out = self._device_body(x_path, ema_x_path, x_omic, grade, index.to(dev) if self.crd_on else index,
                                    sample_idx.to(dev) if self.crd_on else sample_idx, B, do_aux, getattr(opt, "CRD_weight", 1.0), tau, mu_pen,
                                    loss_masking, *((given["survtime"].to(dev, non_blocking=True),
                                                     given["censor"].to(dev, non_blocking=True)) if self.surv else ()))
        if self.tsvd_on:
            if do_aux:
                self.mu = mu_pen                                                                 # :413
            self._batch_idx = bidx + 1
        self.iter_num += 1
        if self.record is not None:
            self.record.count_rows(x_path.shape[0])      # the host's own row count (a replayed launch calls no Python)
        return out

    _IN_NAMES = ("x_path", "ema_x_path", "x_omic", "grade", "index", "sample_idx")

    def _graph_step(self, given, B, do_aux, crd_w, tau, mu_pen):
        """One step from a captured graph; None if no graph can serve it (capture failed: eager from now on).  One graph per
        input set (step_graph.py) and kind of step, with / without the t-SVD auxiliary update."""
        if self._g_scal is None:
            self._g_scal = torch.zeros(3, device=self.device, dtype=torch.float32)
            self._g_ring = PinnedRing((3,), torch.float32)
        st = self._g_sets.input_set(given)
        self._g_ring.upload(self._g_scal, [crd_w, tau, mu_pen])      # (pinned rows: no host sync per replayed step)
        hit = self._g_sets.graph(
            self, st, do_aux,
            lambda: self._device_body(st["x_path"], st["ema_x_path"], st["x_omic"], st["grade"], st["index"], st["sample_idx"], B,
                                      do_aux, self._g_scal[0], self._g_scal[1], self._g_scal[2], None, st.get("survtime"),
                                      st.get("censor"), st),
            # (the survival gather buffers, owned by the set, are allocated outside the capture)
            before=(lambda: self._surv_gather_bufs(st, st["x_path"].shape[0])) if self.surv and self.sync is not None else None)
        if hit is None:
            return None
        self.optimizer.prepare_step()
        self.optimizer._prepared = False
        hit[0].replay()
        return hit[1]

    def _device_body(self, x_path, ema_x_path, x_omic, grade, index, sample_idx, B, do_aux, crd_w, tau, mu_pen, loss_masking,
                     survtime=None, censor=None, input_set=None):
        """Everything of the step that runs on the device (capturable in one HIP graph).  `crd_w`, `tau`, `mu_pen`: floats on
        the eager path, 1-element device tensors under capture.  `survtime`, `censor`: device tensors of the survival task.
        `input_set`: the graph input set being captured (None: eager), which owns its survival gather buffers."""
        opt = self.opt
        dev = self.device
        if loss_masking is None:
            loss_masking = torch.zeros((), device=dev)
        # the mean teacher's forward (no_grad, :143-145) does not depend on the student's (:137): a second stream, joined
        # before the losses, as in DistillStep._device_body
        main = torch.cuda.current_stream()
        if self._ema_side is None:
            self._ema_side = torch.cuda.Stream(device=dev)
        eside = self._ema_side
        eside.wait_stream(main)
        with torch.cuda.stream(eside), torch.no_grad():
            ema_fuse_feat, ema_path_feat, ema_omic_feat, _, _, ema_pred, ema_pred_path, ema_pred_omic, _, _, _ = self.ema_model(
                x_path=ema_x_path, x_omic=x_omic)                                                # :143-145
            for t in (ema_fuse_feat, ema_path_feat, ema_omic_feat, ema_pred, ema_pred_path, ema_pred_omic):
                t.record_stream(main)
        fuse_feat, path_feat, omic_feat, _, _, pred, pred_path, pred_omic, _, _, _ = self.model(
            x_path=x_path, x_omic=x_omic)                                                        # :137
        main.wait_stream(eside)
        loss_CRD = torch.zeros((), device=dev)
        if self.crd_on:                                                                          # :157-165
            self.CRD_criterion_fuse.contrast.batch_norm_size = B
            loss_CRD = crd_w * self.CRD_criterion_fuse(
                fuse_feat, ema_fuse_feat.detach(), index, sample_idx).reshape(())
        kd = lambda p_s, p_t: self.pred_KD_loss(p_s, p_t, B)      # noqa: E731
        surv_terms = None
        if self.surv:
            # :149-152 + :180-203 with opt.task == "surv": lambda_cox * (three Cox terms) + KD_weight * (MSE consistency
            # terms) and its gradient with respect to the three predictions, one launch; NLL is absent (zero)
            nt = opt.num_teachers if getattr(opt, "pred_distill", 1) == 1 else 0
            if self.sync is None:
                loss_surv, surv_terms = ops.SurvStage1LossFn.apply(pred, pred_path, pred_omic, ema_pred, ema_pred_path,
                                                                   ema_pred_omic, survtime, censor, nt, float(opt.lambda_cox),
                                                                   float(getattr(opt, "KD_weight", 1.0)))
            else:
                # the risk sets span the global batch: pack, one all-gather, the gathered kernel (the values are those of
                # the concatenated batch, the same on every replica; the gradient reaches this replica's rows)
                loss_surv, surv_terms = ops.SurvStage1GatheredFn.apply(
                    pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor, nt,
                    float(opt.lambda_cox), float(getattr(opt, "KD_weight", 1.0)), self.sync,
                    *self._surv_gather_bufs(input_set, pred.shape[0]))
            loss_pred_KD = surv_terms[7] if nt > 0 else torch.zeros((), device=dev)
            loss_nll = torch.zeros((), device=dev)
            loss = loss_surv + loss_CRD + loss_masking
        elif getattr(opt, "pred_distill", 1) == 1:
            nt = opt.num_teachers
            kd_fuse = kd(pred, ema_pred)
            if nt == 1:
                kd_path, kd_omic = kd(pred_path, ema_pred_path), kd(pred_omic, ema_pred_omic)
            elif nt == 2:
                kd_path = (kd(pred_path, ema_pred_path) + kd(pred_path, ema_pred)) / 2.0
                kd_omic = (kd(pred_omic, ema_pred_omic) + kd(pred_omic, ema_pred)) / 2.0
            elif nt == 3:
                kd_path = (kd(pred_path, ema_pred_path) + kd(pred_path, ema_pred) + kd(pred_path, ema_pred_omic)) / 3.0
                kd_omic = (kd(pred_omic, ema_pred_omic) + kd(pred_omic, ema_pred) + kd(pred_omic, ema_pred_path)) / 3.0
            else:
                raise NotImplementedError("num_teachers in {1,2,3}")
            loss_pred_KD = getattr(opt, "KD_weight", 1.0) * (kd_fuse + kd_path + kd_omic)       # :203
        else:
            loss_pred_KD = torch.zeros((), device=dev)
        if not self.surv:
            nll = lambda p: ops.NLLFn.apply(p, grade, B)      # noqa: E731
            nll_path, nll_omic, nll_fuse = nll(pred_path), nll(pred_omic), nll(pred)
            loss_nll = nll_path + nll_omic + nll_fuse                                           # :208-212
            loss = opt.lambda_nll * loss_nll + loss_CRD + loss_pred_KD + loss_masking           # :217-218; MIA-2023 :303-304
        loss_reg = torch.zeros((), device=dev)
        if opt.reg_type != "none":      # :209 - the shipped stage-1 command keeps the default `omic` (options.py:132)
            from .networks_new import define_reg
            loss_reg = define_reg(opt, self.model)
            # split over the replicas, whose losses / gradients are summed (see DistillStep._add_reg)
            loss = loss + (opt.lambda_reg / (self.sync.world_size if self.sync is not None else 1)) * loss_reg
        loss_orth = torch.zeros((), device=dev)
        if self.orth_on:
            loss_orth = self.Orth_loss(path_feat, omic_feat)                                    # :216-218
            loss = loss + loss_orth
        loss_tsvd = torch.zeros((), device=dev)
        if self.tsvd_on:                                                                        # train_test_tSVD.py:299-431
            from . import tsvd as T
            if self.sync is not None:
                # the adjacency tensors span the global batch: gather every feature view (rank-ordered rows); the
                # backward of the gather hands this replica's rows their gradient
                fuse_feat, path_feat, omic_feat = (_GatherRowsFn.apply(t, self.sync) for t in (fuse_feat, path_feat, omic_feat))
                ema_fuse_feat, ema_path_feat, ema_omic_feat = (self.sync.all_gather_cat(t) for t in
                                                               (ema_fuse_feat, ema_path_feat, ema_omic_feat))
            if opt.n_views == 2:
                feats1 = [path_feat, ema_path_feat]                                             # :320-322
                feats2 = [omic_feat, ema_omic_feat]
            else:
                feats1 = [fuse_feat.detach(), ema_fuse_feat, path_feat, ema_path_feat]          # :311-313
                feats2 = [fuse_feat.detach(), ema_fuse_feat, omic_feat, ema_omic_feat]
                # n_views 6 / 8 add mixtures of the max-normalised mean-teacher features (:305-307, :341-363)
                for wa in (0.9, 0.8, 0.7, 0.6)[:opt.n_views - 4]:
                    feats1.append(T.maxnorm_mix(ema_path_feat, ema_omic_feat, wa, 1.0 - wa))
                    feats2.append(T.maxnorm_mix(ema_omic_feat, ema_path_feat, wa, 1.0 - wa))
            self.adj_tensor1 = T.update_adj_tensor(self.adj_tensor1, feats1)                    # :365-366
            self.adj_tensor2 = T.update_adj_tensor(self.adj_tensor2, feats2)
            if do_aux:
                # `if opt.tSVD_mode == "path" or "pathomic":` (:378, :398) is always true: both tensors are updated.  The two
                # proximal updates are independent and each fills only part of the device (up to 128 rows n_views / 2 + 1
                # workgroups, one per Fourier slice, ~5 ms at B = 128; above, (n_views / 2 + 1) x ~B / 32 workgroups per launch
                # of the tiled Jacobi): the second runs on a side stream beside the first.  The results land in the
                # PERSISTENT auxiliary tensors (captured graphs of other input sets / of the steps without an update read them)
                main = torch.cuda.current_stream()
                if self._tsvd_side is None:
                    self._tsvd_side = torch.cuda.Stream(device=dev)
                side = self._tsvd_side
                side.wait_stream(main)
                tnns = {}
                for adj, auxs, name, strm in ((self.adj_tensor2, self.aux_tensor2, "2", side),
                                              (self.adj_tensor1, self.aux_tensor1, "1", main)):
                    with torch.cuda.stream(strm):
                        stack = torch.stack([a.detach() for a in adj], dim=2)
                        aux, tnns[name] = T.update_aux(stack, tau)                              # :382, :402
                        for v in range(opt.n_views):
                            auxs[v].copy_(aux[:, :, v])
                        if strm is side:
                            stack.record_stream(main); aux.record_stream(main)
                main.wait_stream(side)
                if torch.is_tensor(tnns["2"]):
                    tnns["2"].record_stream(main)
                self.path_TNN, self.omic_TNN = tnns["1"], tnns["2"]
            if opt.tSVD_mode in ("path", "pathomic"):                                           # :418-431
                loss_tsvd = loss_tsvd + T.tsvd_penalty(self.adj_tensor1, self.aux_tensor1, mu_pen)
            if opt.tSVD_mode in ("omic", "pathomic"):
                loss_tsvd = loss_tsvd + T.tsvd_penalty(self.adj_tensor2, self.aux_tensor2, mu_pen)
            loss = loss + loss_tsvd
        _backward_and_update(self, loss)                                                        # + EMA (:229) fused
        if self.surv or self._unused_ids:
            self._ema_frozen()
        if self.tsvd_on:
            # the adjacency tensors are kept as VALUES: with their grad_fn they would keep this step's autograd graph - and the
            # AccumulateGrad nodes of every parameter, bound to the stream of this step - alive into the next one (a capture of
            # the next step then runs them on the wrong stream: the runtime crashes in hipStreamEndCapture)
            self.adj_tensor1 = [a.detach() for a in self.adj_tensor1]
            self.adj_tensor2 = [a.detach() for a in self.adj_tensor2]
        out = dict(loss=loss.detach(), loss_nll=loss_nll.detach(), loss_pred_KD=loss_pred_KD.detach(),
                   loss_CRD=loss_CRD.detach(), loss_orth=loss_orth.detach(), loss_tsvd=loss_tsvd.detach(),
                   loss_pred_KD_masking=loss_masking.detach(), loss_reg=loss_reg.detach(),
                   pred=pred.detach(), pred_path=pred_path.detach(), pred_omic=pred_omic.detach())
        if surv_terms is not None:
            out.update(loss_cox=surv_terms[6], loss_cox_fuse=surv_terms[0], loss_cox_path=surv_terms[1],
                       loss_cox_omic=surv_terms[2], loss_kd_fuse=surv_terms[3], loss_kd_path=surv_terms[4],
                       loss_kd_omic=surv_terms[5])
        else:
            out.update(loss_nll_fuse=nll_fuse.detach(), loss_nll_path=nll_path.detach(), loss_nll_omic=nll_omic.detach())
        if self.record is not None:
            # the step's last launch; the nuclear norms are added only on a step that ran the auxiliary update (:392, :409)
            self.record.add(out, grade, (self.path_TNN, self.omic_TNN) if self.tsvd_on and do_aux else None, survtime, censor)
        return out

"""torch.autograd glue over the C-ABI: every Function's forward/backward is a call into
libpathomic_hip.so on raw device pointers + the current HIP stream.  torch supplies memory and the
autograd tape only; there is no eager-PyTorch compute fallback."""
import ctypes as C

import torch

from . import _lib
from ._lib import lib, check, ptr, stream, require_cuda

ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3
EW_RELU, EW_GATE, EW_RELU_BWD, EW_ADD, EW_ELU_BWD, EW_MUL = 0, 1, 2, 3, 4, 5
PREC_BF16, PREC_BF16X6, PREC_BF16X3, PREC_FP16X3, PREC_FP16X1 = 0, 1, 2, 3, 4

_precision = PREC_BF16
_fwd_only_precision = None      # optional other arithmetic for forward-only (no_grad) trunk forwards, see set_precision
_backward_precision = None      # optional other arithmetic for the backward's dgrad / wgrad kernels
_weight_epoch = 0


def bump_weight_epoch():
    """Call after parameters were modified through raw device pointers (fused Adam / EMA kernels), so that
    cached MFMA weight packings are refreshed."""
    global _weight_epoch
    _weight_epoch += 1


def weight_epoch():
    return _weight_epoch


def set_precision(mode):
    """Arithmetic of the ResNet trunk:
      'bf16'      perf mode: bf16 operands and activations, fp32 accumulation and statistics;
      'bf16x6'    parity mode: fp32 activations, operands split into three bf16 planes, six MFMA products (fp32-equivalent);
      'bf16x3'    fp32 activations, the three leading products only (16-bit operands, ~2^-16 per product): half the matrix work;
      'fp16x3'    half-pair mode: every tensor a convolution reads (activations, BatchNorm-backward dz under a per-tensor
                  power-of-two scale) is stored as two fp16 planes x = hi + lo * 2^-11 (22 significant bits, 4 B per element),
                  conv outputs and gradients stay fp32, three fp16 MFMA products per k-step (hi*hi, hi*lo, lo*hi: ~2^-22 per
                  product, fp32 accumulation) - the cheapest arithmetic that meets the 1e-3 parity tolerance everywhere;
      'fp16x3/x1' 'fp16x3' for every forward, ONE fp16 product (the hi planes) in the backward's dgrad / wgrad kernels;
      'bf16x6/x3' parity mode for every forward, three products in the backward's dgrad / wgrad kernels;
      'bf16x6+x3' parity mode for every forward that is followed by a backward (the student), 'bf16x3' for the forward-only
                  networks (the no_grad EMA / teacher forwards of train_test_path_multi_distill.py:253-256)."""
    global _precision, _fwd_only_precision, _backward_precision
    _backward_precision = None
    names = {"bf16": PREC_BF16, "bf16x6": PREC_BF16X6, "bf16x3": PREC_BF16X3, "fp16x3": PREC_FP16X3, PREC_BF16: PREC_BF16,
             PREC_BF16X6: PREC_BF16X6, PREC_BF16X3: PREC_BF16X3, PREC_FP16X3: PREC_FP16X3}
    if mode == "bf16x6+x3":
        _precision, _fwd_only_precision = PREC_BF16X6, PREC_BF16X3
    elif mode == "fp16x3/x1":
        # half-pair forward (logits, losses, GK-Refine weights as in 'fp16x3'); the backward's dgrad / wgrad multiply the hi
        # planes alone: one fp16 product on 11-bit operands with fp32 accumulation (gradients at ~1e-4 of their scale)
        _precision, _fwd_only_precision, _backward_precision = PREC_FP16X3, None, PREC_FP16X1
    elif mode == "bf16x6/x3":
        # every FORWARD in parity arithmetic (logits, losses, GK-Refine weights as in 'bf16x6'), the backward's dgrad /
        # wgrad kernels with three products
        _precision, _fwd_only_precision, _backward_precision = PREC_BF16X6, None, PREC_BF16X3
    else:
        _precision, _fwd_only_precision = names[mode], None


def get_backward_precision():
    return _backward_precision


def get_precision(fwd_only=False):
    """The trunk arithmetic in force (for a forward-only forward when `fwd_only`)."""
    return _fwd_only_precision if (fwd_only and _fwd_only_precision is not None) else _precision


def _f32(t):
    t = require_cuda(t)
    if t.dtype != torch.float32:
        raise RuntimeError("expected float32 tensor")
    return t.contiguous()


_ones_cache = {}


def _ones(n, device):
    key = (n, device)
    if key not in _ones_cache:
        _ones_cache[key] = torch.ones(n, device=device, dtype=torch.float32)
    return _ones_cache[key]


def sgemm(A, Bm, bias, out, M, N, K, sam, sak, sbk, sbn, act=ACT_NONE, accumulate=False, ldc=None):
    check(lib().ph_sgemm(ptr(A), ptr(Bm), ptr(bias), ptr(out), M, N, K, sam, sak, sbk, sbn, N if ldc is None else ldc, act,
                         int(accumulate), stream()), "ph_sgemm")
    return out


def linear_fwd(x, w, b, act=ACT_NONE):
    """y[B,N] = act(x[B,K] @ w[N,K]^T + b)   (nn.Linear)"""
    x, w = _f32(x), _f32(w)
    Bn, K = x.shape
    N = w.shape[0]
    y = torch.empty(Bn, N, device=x.device, dtype=torch.float32)
    if K >= 4096 and Bn * N <= 256 * 256:
        nsplit = 128 if K >= 8192 else 32     # 64-256 workgroups: a 16641-deep K in 5 LDS steps per workgroup instead of 17
        part = torch.empty(nsplit * Bn * N, device=x.device, dtype=torch.float32)
        check(lib().ph_sgemm_splitk(ptr(x), ptr(w), ptr(b), ptr(y), ptr(part), nsplit, Bn, N, K, K, 1, 1, K, N, act,
                                    stream()), "ph_sgemm_splitk")
        return y
    return sgemm(x, w, b, y, Bn, N, K, K, 1, 1, K, act)


def _bias_grad(g):
    """db[N] = 1^T dY of dY [B, N]"""
    Bn, N = g.shape
    db = torch.empty(N, device=g.device, dtype=torch.float32)
    return sgemm(_ones(Bn, g.device), g, None, db, 1, N, Bn, 0, 1, N, 1)


def _linear_grads(needs, g, x, w, has_bias):
    """(dx, dw, db) of y = x @ w^T + b for dY = g, each None where needs[i] is false (db also without a bias)"""
    Bn, K = x.shape
    N = w.shape[0]
    dx = dw = db = None
    if needs[0]:
        dx = torch.empty_like(x)
        sgemm(g, w, None, dx, Bn, K, N, N, 1, K, 1)              # dX = dY @ W
    if needs[1]:
        dw = torch.empty_like(w)
        sgemm(g, x, None, dw, N, K, Bn, 1, N, K, 1)              # dW = dY^T @ X
    if has_bias and needs[2]:
        db = _bias_grad(g)
    return dx, dw, db


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return linear_fwd(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return _linear_grads(ctx.needs_input_grad, _f32(g), x, w, ctx.has_bias)


# ---- a linear map over a row-wise concatenation (x_0 | x_1 | ...), some blocks followed by a column of ones, without forming
# the concatenation: a sum of GEMMs over column blocks of the weight (the fusion head's skip connection and linear gate,
# fusion.py:43,61).  `blocks` is a list of (x_i [B, k_i] contiguous, one_follows).
def _cat_layout(blocks):
    """[(column offset of block i, k_i)], [columns that multiply an appended 1], total width"""
    offs, ones, off = [], [], 0
    for x, one in blocks:
        offs.append((off, x.shape[1]))
        off += x.shape[1]
        if one:
            ones.append(off)
            off += 1
    return offs, ones, off


def cat_linear_fwd(blocks, w, b):
    """y[B,N] = (x_0 | [1] | x_1 | [1] | ...) @ w[N,Kt]^T + b"""
    w = _f32(w)
    blocks = [(_f32(x), one) for x, one in blocks]
    offs, ones, Kt = _cat_layout(blocks)
    N = w.shape[0]
    if Kt != w.shape[1]:
        raise RuntimeError("cat_linear: blocks span %d columns, the weight has %d" % (Kt, w.shape[1]))
    Bn = blocks[0][0].shape[0]
    y = torch.empty(Bn, N, device=w.device, dtype=torch.float32)
    for i, ((x, _), (off, k)) in enumerate(zip(blocks, offs)):
        sgemm(x, w[:, off:], b if i == 0 else None, y, Bn, N, k, k, 1, 1, Kt, accumulate=i > 0)
    if len(ones) == 2:      # both appended-1 columns in one K = 2 product: A is a broadcast 1, B steps from column to column
        sgemm(_ones(1, w.device), w[:, ones[0]:], None, y, Bn, N, 2, 0, 0, ones[1] - ones[0], Kt, accumulate=True)
    else:
        for c in ones:
            sgemm(_ones(1, w.device), w[:, c:], None, y, Bn, N, 1, 0, 0, 1, Kt, accumulate=True)
    return y


class CatLinearFn(torch.autograd.Function):
    """cat_linear_fwd taped: every block's input gradient from its column block of the weight, the weight gradient
    written block by block into column slices of one [N, Kt] tensor (ldc = Kt), the appended-1 columns get 1^T dY."""

    @staticmethod
    def forward(ctx, w, b, ones_after, *xs):
        blocks = list(zip(xs, ones_after))
        ctx.save_for_backward(w, *xs)
        ctx.ones_after, ctx.has_bias = tuple(ones_after), b is not None
        return cat_linear_fwd(blocks, w, b)

    @staticmethod
    def backward(ctx, g):
        w, *xs = ctx.saved_tensors
        g = _f32(g)
        offs, ones, Kt = _cat_layout(list(zip(xs, ctx.ones_after)))
        Bn, N = g.shape
        one = _ones(1, g.device)
        dxs = []
        for i, (x, (off, k)) in enumerate(zip(xs, offs)):
            dx = None
            if ctx.needs_input_grad[3 + i]:
                dx = torch.empty_like(x)
                sgemm(g, w[:, off:], None, dx, Bn, k, N, N, 1, Kt, 1)              # dX_i = dY @ W[:, block i]
            dxs.append(dx)
        dw = db = None
        if ctx.needs_input_grad[0]:
            dw = torch.empty_like(w)
            for x, (off, k) in zip(xs, offs):
                sgemm(g, x, None, dw[:, off:], N, k, Bn, 1, N, k, 1, ldc=Kt)       # dW[:, block i] = dY^T @ X_i
            for c in ones:
                sgemm(g, one, None, dw[:, c:], N, 1, Bn, 1, N, 0, 0, ldc=Kt)       # dW[:, c] = dY^T 1
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = _bias_grad(g)
        return (dw, db, None) + tuple(dxs)


def cat_linear(blocks, w, b):
    return CatLinearFn.apply(w, b, tuple(one for _, one in blocks), *[_f32(x) for x, _ in blocks])


# ---- autograd forms of the SNN / fusion operators (stage-1 teacher training).  The frozen teacher of the
# stage-2 hot path keeps its fused forward-only calls; these are used when a gradient is required.
class LinearActFn(torch.autograd.Function):
    """y = act(x @ w^T + b) with act in {none, relu, elu} fused into the GEMM epilogue; backward from the saved y."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        y = linear_fwd(x, w, b, act)
        ctx.save_for_backward(x, w, y)
        ctx.act, ctx.has_bias = act, b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        g = _f32(g)
        if ctx.act == ACT_RELU:
            g = eltwise(g, y, EW_RELU_BWD)
        elif ctx.act == ACT_ELU:
            g = eltwise(g, y, EW_ELU_BWD)
        elif ctx.act != ACT_NONE:
            raise NotImplementedError("LinearActFn backward: activation %d" % ctx.act)
        return _linear_grads(ctx.needs_input_grad, g, x, w, ctx.has_bias) + (None,)


class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = eltwise(x, None, EW_RELU)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return eltwise(_f32(g), y, EW_RELU_BWD)


class DropoutFn(torch.autograd.Function):
    """(Alpha-)dropout with the counter-based RNG of ph_dropout_dev; the backward re-creates the mask from the step
    counter value of the forward call (a saved 8-byte device copy), so no mask tensor is stored."""

    @staticmethod
    def forward(ctx, x, p, seed, site_offset, step_counter, alpha):
        x = _f32(x)
        y = torch.empty_like(x)
        check(lib().ph_dropout_dev_to(ptr(x), ptr(y), y.numel(), p, seed, site_offset, ptr(step_counter), int(alpha), stream()),
              "ph_dropout_dev_to")
        if ctx.needs_input_grad[0]:      # (the frozen teacher's dropouts never run a backward: no 8-byte copy kernel for them)
            ctx.save_for_backward(step_counter.clone())
        ctx.args = (p, seed, site_offset, int(alpha))
        return y

    @staticmethod
    def backward(ctx, g):
        (ctr,) = ctx.saved_tensors
        p, seed, site_offset, alpha = ctx.args
        g = _f32(g)
        d = torch.empty_like(g)
        check(lib().ph_dropout_bwd_dev_to(ptr(g), ptr(d), d.numel(), p, seed, site_offset, ptr(ctr), alpha, stream()),
              "ph_dropout_bwd_dev_to")
        return d, None, None, None, None, None


class GateFn(torch.autograd.Function):
    """y = sigmoid(z) * h  (fusion.py:44-45)"""

    @staticmethod
    def forward(ctx, z, h):
        z, h = _f32(z), _f32(h)
        ctx.save_for_backward(z, h)
        return eltwise(z, h, EW_GATE)

    @staticmethod
    def backward(ctx, g):
        z, h = ctx.saved_tensors
        g = _f32(g)
        dz, dh = torch.empty_like(z), torch.empty_like(h)
        check(lib().ph_gate_bwd(ptr(g), ptr(z), ptr(h), ptr(dz), ptr(dh), z.numel(), stream()), "ph_gate_bwd")
        return dz, dh


class OuterFn(torch.autograd.Function):
    """o12[b] = vec(o1e[b] (x) o2e[b]) with an optional appended 1 on both operands (fusion.py:43,56-58)"""

    @staticmethod
    def forward(ctx, o1, o2, append_one):
        o1, o2 = _f32(o1), _f32(o2)
        ctx.save_for_backward(o1, o2)
        ctx.append_one = int(append_one)
        return outer(o1, o2, ctx.append_one)

    @staticmethod
    def backward(ctx, g):
        o1, o2 = ctx.saved_tensors
        g = _f32(g)
        d1, d2 = torch.empty_like(o1), torch.empty_like(o2)
        check(lib().ph_outer_bwd(ptr(g), ptr(o1), ptr(o2), ptr(d1), ptr(d2), o1.shape[0], o1.shape[1], o2.shape[1],
                                 ctx.append_one, stream()), "ph_outer_bwd")
        return d1, d2, None


class BN1dFn(torch.autograd.Function):
    """nn.BatchNorm1d (training statistics) optionally fused with ReLU."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, relu, update_running):
        x = _f32(x)
        Bn, Cn = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(Cn, device=x.device, dtype=torch.float32)
        invstd = torch.empty_like(mean)
        check(lib().ph_bn1d_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(invstd),
                                ptr(rm) if update_running else None, ptr(rv), ptr(nbt), Bn, Cn, 1e-5, 0.1, int(relu),
                                stream()), "ph_bn1d_fwd")
        ctx.save_for_backward(x, y, mean, invstd, gamma)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, mean, invstd, gamma = ctx.saved_tensors
        g = _f32(g)
        Bn, Cn = x.shape
        dx = torch.empty_like(x)
        dg = torch.empty_like(gamma)
        db = torch.empty_like(gamma)
        check(lib().ph_bn1d_bwd(ptr(g), ptr(y), ptr(x), ptr(mean), ptr(invstd), ptr(gamma), ptr(dx), ptr(dg), ptr(db),
                                Bn, Cn, int(ctx.relu), stream()), "ph_bn1d_bwd")
        return dx, dg, db, None, None, None, None, None


def bn1d_eval(x, bn, relu):
    """nn.BatchNorm1d in eval mode (running statistics), optionally + ReLU; forward only."""
    x = _f32(x)
    y = torch.empty_like(x)
    check(lib().ph_bn1d_eval(ptr(x), ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), ptr(y),
                             x.shape[0], x.shape[1], bn.eps, int(relu), stream()), "ph_bn1d_eval")
    return y


class BN1dEvalFn(torch.autograd.Function):
    """bn1d_eval with a backward to the input (eval-mode BatchNorm1d is a fixed per-channel scale): used when a
    gradient flows through an eval-mode network to its inputs (MIA-2023 superpixel attention masks)."""

    @staticmethod
    def forward(ctx, x, bn, relu):
        y = bn1d_eval(x, bn, relu)
        ctx.save_for_backward(y)
        ctx.bn, ctx.relu = bn, relu
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        bn = ctx.bn
        g = _f32(g)
        dx = torch.empty_like(y)
        check(lib().ph_bn1d_eval_bwd(ptr(g), ptr(y), ptr(bn.weight), ptr(bn.running_var), ptr(dx), y.shape[0], y.shape[1],
                                     bn.eps, int(ctx.relu), stream()), "ph_bn1d_eval_bwd")
        return dx, None, None


class LogSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty_like(x)
        check(lib().ph_log_softmax(ptr(x), ptr(y), x.shape[0], x.shape[1], stream()), "ph_log_softmax")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(y)
        check(lib().ph_log_softmax_bwd(ptr(g), ptr(y), ptr(dx), y.shape[0], y.shape[1], stream()), "ph_log_softmax_bwd")
        return dx


class NLLFn(torch.autograd.Function):
    """F.nll_loss(pred, grade) with mean reduction over `bnorm` samples (the global batch under DDP)."""

    @staticmethod
    def forward(ctx, pred, grade, bnorm):
        pred = _f32(pred)
        grade = require_cuda(grade).contiguous()
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        check(lib().ph_nll_fwd(ptr(pred), ptr(grade), ptr(loss), pred.shape[0], pred.shape[1], 1.0 / bnorm, stream()),
              "ph_nll_fwd")
        ctx.save_for_backward(grade)
        ctx.shape = tuple(pred.shape)
        ctx.bnorm = bnorm
        return loss

    @staticmethod
    def backward(ctx, g):
        grade, = ctx.saved_tensors
        g = _f32(g)
        d = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib().ph_nll_bwd(ptr(g), ptr(grade), ptr(d), ctx.shape[0], ctx.shape[1], 1.0 / ctx.bnorm, stream()),
              "ph_nll_bwd")
        return d, None, None


class KLFn(torch.autograd.Function):
    """DistillKL (reference KD_loss.py:13-17); gradient w.r.t. y_s only (y_t is detached on the hot path)."""

    @staticmethod
    def forward(ctx, y_s, y_t, T, bnorm):
        y_s, y_t = _f32(y_s), _f32(y_t)
        loss = torch.empty((), device=y_s.device, dtype=torch.float32)
        check(lib().ph_kl_fwd(ptr(y_s), ptr(y_t), ptr(loss), y_s.shape[0], y_s.shape[1], T, 1.0 / bnorm, stream()),
              "ph_kl_fwd")
        ctx.save_for_backward(y_s, y_t)
        ctx.T, ctx.bnorm = T, bnorm
        return loss

    @staticmethod
    def backward(ctx, g):
        y_s, y_t = ctx.saved_tensors
        g = _f32(g)
        d = torch.empty_like(y_s)
        check(lib().ph_kl_bwd(ptr(g), ptr(y_s), ptr(y_t), ptr(d), y_s.shape[0], y_s.shape[1], ctx.T, 1.0 / ctx.bnorm,
                              stream()), "ph_kl_bwd")
        return d, None, None, None


class SigmoidRangeFn(torch.autograd.Function):
    """The survival head (networks_new.py:236-237,327-328, resnets.py:252-253): sigmoid(hazard) * output_range +
    output_shift, the two read from the module's parameters in device memory (they carry no gradient: requires_grad=False
    in the reference)."""

    @staticmethod
    def forward(ctx, hazard, output_range, output_shift):
        h = _f32(hazard)
        r, s = _f32(output_range.detach()), _f32(output_shift.detach())
        pred = torch.empty_like(h)
        sigma = torch.empty_like(h)
        check(lib().ph_sigmoid_range_fwd(ptr(h), ptr(r), ptr(s), ptr(pred), ptr(sigma), h.numel(), stream()),
              "ph_sigmoid_range_fwd")
        ctx.save_for_backward(sigma, r)
        return pred

    @staticmethod
    def backward(ctx, g):
        sigma, r = ctx.saved_tensors
        g = _f32(g)
        dh = torch.empty_like(sigma)
        check(lib().ph_sigmoid_range_bwd(ptr(g), ptr(sigma), ptr(r), ptr(dh), sigma.numel(), stream()), "ph_sigmoid_range_bwd")
        return dh, None, None


def apply_act(act, hazard, owner):
    """The head of the three networks: log-softmax (grading) or the sigmoid range head of the survival task, whose range and
    shift are `owner`'s output_range / output_shift parameters.  Any other activation raises."""
    if isinstance(act, torch.nn.LogSoftmax):
        return LogSoftmaxFn.apply(hazard)
    if isinstance(act, torch.nn.Sigmoid):
        return SigmoidRangeFn.apply(hazard, owner.output_range, owner.output_shift)
    raise NotImplementedError("act %r: the log-softmax (grading) and sigmoid-range (survival) heads are built"
                              % type(act).__name__)


# ---- what the two survival autograd functions share
def _surv_prepare(pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor):
    """-> the eight flattened rows in the order the C entries take them (an absent teacher row is None), out [9] and
    d [3, n] = d total / d (pred, pred_path, pred_omic) for the entry to fill"""
    ps = [_f32(p).reshape(-1) for p in (pred, pred_path, pred_omic)]
    qs = [None if q is None else _f32(q.detach()).reshape(-1) for q in (ema_pred, ema_pred_path, ema_pred_omic)]
    rows = ps + qs + [_f32(survtime).reshape(-1), _f32(censor).reshape(-1)]
    out = torch.empty(9, device=ps[0].device, dtype=torch.float32)
    d = torch.empty(3, ps[0].shape[0], device=ps[0].device, dtype=torch.float32)
    return rows, out, d


def _surv_result(ctx, preds, out, d):
    """(total, terms[8]) from `out`; d and the predictions' shapes kept for _surv_backward"""
    ctx.save_for_backward(d)
    ctx.shapes = tuple(p.shape for p in preds)
    terms = out[:8]
    ctx.mark_non_differentiable(terms)
    return out[8], terms


def _surv_backward(ctx, g):
    d, = ctx.saved_tensors
    return tuple((d[k] * g).reshape(ctx.shapes[k]) for k in range(3))


class SurvStage1LossFn(torch.autograd.Function):
    """The survival block of the stage-1 teacher step in one launch (ph_surv_stage1_loss_grad): the three Cox terms
    (train_test_MT.py:149-152) and the MSE consistency terms (:180-201, KD_losses.py:20-22).  Returns (total, terms[6]) with
    total = lambda_cox * (cox terms) + kd_weight * (kd terms); the gradient of `total` is computed in the forward, the
    backward scales it by the incoming gradient (as utils._CoxFn).  num_teachers 0: no consistency terms.  `terms`: cox_fuse,
    cox_path, cox_omic, kd_fuse, kd_path, kd_omic, loss_cox (their sum), loss_pred_KD (kd_weight x the kd sum)."""

    @staticmethod
    def forward(ctx, pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor, num_teachers,
                lambda_cox, kd_weight):
        rows, out, d = _surv_prepare(pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor)
        check(lib().ph_surv_stage1_loss_grad(*map(ptr, rows), d.shape[1], int(num_teachers), float(lambda_cox), float(kd_weight),
                                             ptr(out), ptr(d), stream()), "ph_surv_stage1_loss_grad")
        return _surv_result(ctx, (pred, pred_path, pred_omic), out, d)

    @staticmethod
    def backward(ctx, g, g_terms):
        return _surv_backward(ctx, g) + (None,) * 8


def surv_gather_buffers(n, world, device):
    """The persistent buffers of SurvStage1GatheredFn: this replica's staging block [8, n] and the all-gathered blocks
    [world, 8, n] (layout: include/pathomic_hip.h, ph_surv_pack_rows)."""
    return (torch.empty(8, n, device=device, dtype=torch.float32),
            torch.empty(world, 8, n, device=device, dtype=torch.float32))


class SurvStage1GatheredFn(torch.autograd.Function):
    """SurvStage1LossFn under data parallelism, over the GLOBAL batch: the reference's nn.DataParallel computes the Cox and
    consistency terms on the outputs gathered from every replica (train_test_MT.py:63-64), so every risk set spans all
    replicas' rows.  Forward: pack this replica's eight survival rows into `staging` (ph_surv_pack_rows), ONE all-gather
    into `gathered` (sync.all_gather_into, rank-ordered), then the gathered kernel (ph_surv_stage1_loss_grad_gathered).
    Returns the same (total, terms[8]) as SurvStage1LossFn on the concatenated batch, bitwise, identical on every replica.
    Backward: d total / d (this replica's rows) x the incoming gradient, no collective - every replica evaluates the same
    function of the gathered rows, so the partial derivative with respect to its own rows is complete, and the gradient
    all-reduce adds the replicas' parameter gradients up (as train_step._GatherRowsFn for the t-SVD term).  `staging`,
    `gathered`: surv_gather_buffers(n, world); the caller keeps them so that a captured graph reuses their addresses."""

    @staticmethod
    def forward(ctx, pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor, num_teachers,
                lambda_cox, kd_weight, sync, staging, gathered):
        rows, out, d = _surv_prepare(pred, pred_path, pred_omic, ema_pred, ema_pred_path, ema_pred_omic, survtime, censor)
        n, W, nt = d.shape[1], sync.world_size, int(num_teachers)
        if tuple(staging.shape) != (8, n) or tuple(gathered.shape) != (W, 8, n):
            raise ValueError("SurvStage1GatheredFn: staging must be [8, %d] and gathered [%d, 8, %d], got %s and %s"
                             % (n, W, n, tuple(staging.shape), tuple(gathered.shape)))
        check(lib().ph_surv_pack_rows(*map(ptr, rows), n, nt, ptr(staging), stream()), "ph_surv_pack_rows")
        sync.all_gather_into(gathered, staging)
        check(lib().ph_surv_stage1_loss_grad_gathered(ptr(gathered), W, n, sync.rank, nt, float(lambda_cox), float(kd_weight),
                                                      ptr(out), ptr(d), stream()), "ph_surv_stage1_loss_grad_gathered")
        return _surv_result(ctx, (pred, pred_path, pred_omic), out, d)

    @staticmethod
    def backward(ctx, g, g_terms):
        return _surv_backward(ctx, g) + (None,) * 11


def surv_loss_terms(pred, pred_path, pred_omic, survtime, censor):
    """Forward-only Cox terms (fuse, path, omic) of one batch: the evaluation's per-batch loss, as a [3] device tensor."""
    ps = [_f32(p).reshape(-1) for p in (pred, pred_path, pred_omic)]
    t, c = _f32(survtime).reshape(-1), _f32(censor).reshape(-1)
    out = torch.empty(9, device=ps[0].device, dtype=torch.float32)
    check(lib().ph_surv_stage1_loss_grad(ptr(ps[0]), ptr(ps[1]), ptr(ps[2]), None, None, None, ptr(t), ptr(c), ps[0].shape[0],
                                         0, 1.0, 0.0, ptr(out), None, stream()), "ph_surv_stage1_loss_grad")
    return out[:3]


def cindex_counts(survtime, event, hazards):
    """Concordance counts of up to three risk vectors against one (survtime, event) pair (ph_cindex_counts): an int64
    [len(hazards), 3] device tensor of comparable, concordant and tied pairs."""
    t, e = _f32(survtime).reshape(-1), _f32(event).reshape(-1)
    hs = [_f32(h).reshape(-1) for h in hazards]
    if not 1 <= len(hs) <= 3 or any(h.shape[0] != t.shape[0] for h in hs) or e.shape[0] != t.shape[0]:
        raise ValueError("cindex_counts: 1 to 3 risk vectors, each as long as survtime and event")
    out = torch.empty(len(hs), 3, device=t.device, dtype=torch.int64)
    hp = [ptr(h) for h in hs] + [None] * (3 - len(hs))
    check(lib().ph_cindex_counts(ptr(t), ptr(e), hp[0], hp[1], hp[2], len(hs), t.shape[0], ptr(out), stream()),
          "ph_cindex_counts")
    return out


AGG_FUN = {"mean": 0, "max": 1}          # PH_AGG_MEAN, PH_AGG_MAX


def _pred_grade(pred, grade, what):
    pred = _f32(pred)
    if pred.dim() != 2 or grade.numel() != pred.shape[0]:
        raise ValueError("%s: pred [N, C] float32 and one grade per row" % what)
    return pred, require_cuda(grade, "grade").reshape(-1).long().contiguous()


def rank_counts(pred, grade, out=None):
    """The counts behind the micro-averaged ROC-AUC and average precision (ph_rank_counts) of scores pred [N, C] against
    the labels grade [N]: an int64 [5] device tensor {P, concordant, tied, bad, ap_sum}, the last word holding the BITS of
    the float64 sum (`out[4:5].view(torch.float64)`).  `out`: five int64 words of a caller's buffer to fill instead."""
    pred, grade = _pred_grade(pred, grade, "rank_counts")
    N, C = pred.shape
    nbytes = lib().ph_rank_counts_workspace_bytes(N, C)
    if nbytes == 0:
        raise ValueError("rank_counts: N >= 1, C >= 1 and N * C <= 1048576 (got %d x %d)" % (N, C))
    if out is None:
        out = torch.empty(5, device=pred.device, dtype=torch.int64)
    ws = torch.empty(nbytes // 8, device=pred.device, dtype=torch.float64)
    check(lib().ph_rank_counts(ptr(pred), ptr(grade), N, C, ptr(out), out.data_ptr() + 32, ptr(ws), stream()), "ph_rank_counts")
    return out


def rank_counts_classes(pred, grade, out=None):
    """The counts of `rank_counts` for every one-vs-rest column of pred [N, C] in one call (ph_rank_counts_classes; a memset
    and two launches whatever C is): an int64 [5 * C] device tensor, words 4 c .. 4 c + 3 = {P_c, concordant_c, tied_c, bad_c}
    and word 4 C + c the BITS of the float64 ap_sum_c (`out[4 * C:].view(torch.float64)`).  `out`: 5 C int64 words of a
    caller's buffer to fill instead."""
    pred, grade = _pred_grade(pred, grade, "rank_counts_classes")
    N, C = pred.shape
    nbytes = lib().ph_rank_counts_classes_workspace_bytes(N, C)
    if nbytes == 0:
        raise ValueError("rank_counts_classes: 1 <= N <= 1048576 and 1 <= C <= 16 (got %d x %d)" % (N, C))
    if out is None:
        out = torch.empty(5 * C, device=pred.device, dtype=torch.int64)
    ws = torch.empty(nbytes // 8, device=pred.device, dtype=torch.float64)
    check(lib().ph_rank_counts_classes(ptr(pred), ptr(grade), N, C, ptr(out), out.data_ptr() + 32 * C, ptr(ws), stream()),
          "ph_rank_counts_classes")
    return out


def roc_points(pred, grade, cls):
    """The ROC curve's integer points at every distinct threshold (ph_roc_points) of column `cls` of pred [N, C] one-vs-rest
    (M = N elements), or with cls = "micro" (or -1) of all M = N * C (score, label) pairs: an int32 [2 + 3 * M] device tensor
    {points, bad, fps [M], tps [M], thr [M] (the BITS of the float32 thresholds: `.view(torch.float32)`)}; the first `points`
    entries of the three arrays are the curve in descending threshold order, the rest is left unwritten."""
    pred, grade = _pred_grade(pred, grade, "roc_points")
    N, C = pred.shape
    if isinstance(cls, str):
        if cls != "micro":
            raise ValueError('roc_points: cls is a class index or "micro", got %r' % (cls,))
        cls = -1
    cls = int(cls)
    nbytes = lib().ph_roc_points_workspace_bytes(N, C)
    if nbytes == 0 or not -1 <= cls < C or (cls == -1 and N * C > 1 << 20):
        raise ValueError("roc_points: 1 <= N <= 1048576, 1 <= C <= 16, cls in [0, C) or \"micro\" with N * C <= 1048576 "
                         "(got %d x %d, cls %d)" % (N, C, cls))
    M = N if cls >= 0 else N * C
    out = torch.empty(2 + 3 * M, device=pred.device, dtype=torch.int32)
    ws = torch.empty(nbytes // 4, device=pred.device, dtype=torch.int32)
    base = out.data_ptr()
    check(lib().ph_roc_points(ptr(pred), ptr(grade), N, C, cls, base + 8, base + 8 + 4 * M, base + 8 + 8 * M, base, ptr(ws),
                              stream()), "ph_roc_points")
    return out


SURV_MAX_N, SURV_MAX_K, SURV_MAX_G, SURV_MAX_P = 1 << 20, 7, 8, 28      # the limits of csrc/survstrata.hip


def _i32_out(t, n, what):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError("%s: a contiguous int32 tensor of %d entries" % (what, n))
    return require_cuda(t, what)


def surv_strata(hazard, q, cuts, group, sizes, bad):
    """Risk strata of hazard f32 [N] at the percentiles q (a host sequence of K percents): ph_surv_strata fills the caller's
    device tensors cuts float64 [K] (numpy's linear percentile of the float64 hazards, with the reference's 2.99997 patch),
    group int32 [N] (the first i with hazard < cuts[i], else K), sizes int32 [K + 1] and bad int32 [1] (non-finite hazards).
    Nothing is read back."""
    import numpy as np
    hazard = _f32(hazard).reshape(-1)
    qh = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    N, K = hazard.shape[0], qh.shape[0]
    nbytes = lib().ph_surv_strata_workspace_bytes(N, K)
    if nbytes == 0 or not bool(np.all((qh >= 0.0) & (qh <= 100.0))):
        raise ValueError("surv_strata: 2 <= N <= 1048576 and 1 to 7 percentiles in [0, 100] (got N = %d, q = %r)" % (N, qh.tolist()))
    if cuts.dtype != torch.float64 or cuts.numel() != K or not cuts.is_contiguous():
        raise ValueError("surv_strata: cuts is a contiguous float64 tensor of %d entries" % K)
    _i32_out(group, N, "group"); _i32_out(sizes, K + 1, "sizes"); _i32_out(bad, 1, "bad")
    ws = torch.empty(nbytes, device=hazard.device, dtype=torch.uint8)
    check(lib().ph_surv_strata(ptr(hazard), N, qh.ctypes.data, K, ptr(require_cuda(cuts, "cuts")), ptr(group), ptr(sizes), ptr(bad),
                               ptr(ws), stream()), "ph_surv_strata")


def surv_table(survtime, event, group, G, times, at_risk, observed, censored, npoints):
    """lifelines' event table per group (ph_surv_table) of survtime, event f32 [N] and group int32 [N] with G groups, into the
    caller's device tensors times f32 [N], at_risk / observed / censored int32 [N, G] and npoints int32 [2] (slots, rows left
    out); the rows from npoints[0] on stay unwritten.  Nothing is read back."""
    survtime, event = _f32(survtime).reshape(-1), _f32(event).reshape(-1)
    N, G = survtime.shape[0], int(G)
    nbytes = lib().ph_surv_table_workspace_bytes(N, G)
    if nbytes == 0 or event.shape[0] != N:
        raise ValueError("surv_table: survtime and event [N] with 2 <= N <= 1048576, 1 <= G <= 8 (got %d, %d, G = %d)"
                         % (N, event.shape[0], G))
    _i32_out(group, N, "group")
    if times.dtype != torch.float32 or times.numel() != N or not times.is_contiguous():
        raise ValueError("surv_table: times is a contiguous float32 tensor of %d entries" % N)
    for name, t in (("at_risk", at_risk), ("observed", observed), ("censored", censored)):
        _i32_out(t, N * G, name)
    _i32_out(npoints, 2, "npoints")
    ws = torch.empty(nbytes, device=survtime.device, dtype=torch.uint8)
    check(lib().ph_surv_table(ptr(survtime), ptr(event), ptr(group), N, G, ptr(require_cuda(times, "times")), ptr(at_risk),
                              ptr(observed), ptr(censored), ptr(npoints), ptr(ws), stream()), "ph_surv_table")


def surv_logrank_km(at_risk, observed, npoints, G, pairs, stat, surv):
    """The log-rank sums (O - E, V) of the group pairs `pairs` (a host sequence of (a, b)) into stat float64 [P, 2] and the
    Kaplan-Meier estimate of every group at every slot into surv float64 [N, G] (ph_surv_logrank_km), from the table of
    `surv_table` on the device.  Nothing is read back."""
    import numpy as np
    G = int(G)
    ph = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = ph.shape[0]
    N = at_risk.numel() // max(G, 1)
    nbytes = lib().ph_surv_logrank_km_workspace_bytes(N, G, P)
    if nbytes == 0 or (P and (ph.min() < 0 or ph.max() >= G or bool((ph[:, 0] == ph[:, 1]).any()))):
        raise ValueError("surv_logrank_km: 2 <= N <= 1048576, 1 <= G <= 8, at most 28 pairs of two different groups in [0, G) "
                         "(got N = %d, G = %d, pairs %r)" % (N, G, ph.tolist()))
    _i32_out(at_risk, N * G, "at_risk"); _i32_out(observed, N * G, "observed"); _i32_out(npoints, 2, "npoints")
    for name, t, n in (("stat", stat, 2 * P), ("surv", surv, N * G)):
        if t.dtype != torch.float64 or t.numel() != n or not t.is_contiguous():
            raise ValueError("surv_logrank_km: %s is a contiguous float64 tensor of %d entries" % (name, n))
    ws = torch.empty(nbytes, device=at_risk.device, dtype=torch.uint8)
    check(lib().ph_surv_logrank_km(ptr(at_risk), ptr(observed), ptr(npoints), N, G, ph.ctypes.data if P else None, P,
                                   ptr(require_cuda(stat, "stat")) if P else None, ptr(require_cuda(surv, "surv")), ptr(ws),
                                   stream()), "ph_surv_logrank_km")


def confusion_counts(pred, grade, out=None):
    """int64 [C, C] device tensor: row = true grade, column = arg-max of the row of pred (first maximum), ph_confusion_counts."""
    pred, grade = _pred_grade(pred, grade, "confusion_counts")
    N, C = pred.shape
    if not 1 <= C <= 16 or N < 1:
        raise ValueError("confusion_counts: N >= 1 and 1 <= C <= 16 (got %d x %d)" % (N, C))
    if out is None:
        out = torch.empty(C, C, device=pred.device, dtype=torch.int64)
    check(lib().ph_confusion_counts(ptr(pred), ptr(grade), N, C, ptr(out), stream()), "ph_confusion_counts")
    return out


def group_csr(group_of_row, num_groups):
    """The CSR ph_group_agg reads, from a HOST sequence of one dense group id per row: (offsets int32 [G + 1] numpy,
    order int32 [N] numpy), the rows of a group ascending."""
    import numpy as np
    g = np.asarray(group_of_row, dtype=np.int64).reshape(-1)
    if g.size and (g.min() < 0 or g.max() >= num_groups):
        raise ValueError("group ids must lie in [0, %d)" % num_groups)
    order = np.argsort(g, kind="stable").astype(np.int32)
    offsets = np.zeros(num_groups + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(g, minlength=num_groups))
    return offsets, order


def _group_call(name, entry, x, offsets_dev, order_dev, offsets_host, scalar, refusal):
    """The body of `group_agg` and `group_quantile`: the checks of x and the CSR, out [G, C], the C call `entry` with its
    one extra `scalar`, and its -22 as a ValueError with the text `refusal`."""
    import numpy as np
    x = _f32(x)
    oh = np.ascontiguousarray(offsets_host, dtype=np.int32)
    G = oh.shape[0] - 1
    if x.dim() != 2 or order_dev.numel() != x.shape[0] or offsets_dev.numel() != G + 1:
        raise ValueError("%s: x [N, C], order [N], offsets [G + 1]" % name)
    if offsets_dev.dtype != torch.int32 or order_dev.dtype != torch.int32:
        raise ValueError("%s: offsets and order are int32" % name)
    out = torch.empty(G, x.shape[1], device=x.device, dtype=torch.float32)
    rc = entry(ptr(x), ptr(require_cuda(offsets_dev).contiguous()), ptr(require_cuda(order_dev).contiguous()),
               oh.ctypes.data, x.shape[0], x.shape[1], G, scalar, ptr(out), stream())
    if rc == -22:
        raise ValueError("ph_%s refused the groups: %s" % (name, refusal))
    check(rc, "ph_" + name)
    return out


def group_agg(x, offsets_dev, order_dev, offsets_host, fun):
    """out [G, C] = mean or max of the rows of x [N, C] per group (ph_group_agg); offsets_host: the numpy int32 copy of
    offsets_dev (the entry checks it on the host: an empty group raises)."""
    if fun not in AGG_FUN:
        raise ValueError('agg must be "mean" or "max", got %r' % (fun,))
    return _group_call("group_agg", lib().ph_group_agg, x, offsets_dev, order_dev, offsets_host, AGG_FUN[fun],
                       "offsets must start at 0, end at N and leave no group empty")


QUANTILE_MAX_GROUP = 4096                 # PH_QUANTILE_MAX_GROUP


def group_quantile(x, offsets_dev, order_dev, offsets_host, q):
    """out [G, C] = the q-quantile (a fraction in [0, 1]; numpy's percentile, method "linear"; 0.5 = pandas' median) of the
    rows of x [N, C] per group (ph_group_quantile), over the CSR of `group_agg`.  A NaN in a group's column gives NaN.
    One launch, nothing read back; groups of at most 4096 rows."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("group_quantile: q is a fraction in [0, 1], got %r" % (q,))
    return _group_call("group_quantile", lib().ph_group_quantile, x, offsets_dev, order_dev, offsets_host, q,
                       "offsets must start at 0, end at N, leave no group empty and none larger than %d rows "
                       "(N <= 16777216, C <= 4096)" % QUANTILE_MAX_GROUP)


class L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty_like(x)
        nrm = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        check(lib().ph_l2norm_fwd(ptr(x), ptr(y), ptr(nrm), x.shape[0], x.shape[1], stream()), "ph_l2norm_fwd")
        ctx.save_for_backward(y, nrm)
        return y

    @staticmethod
    def backward(ctx, g):
        y, nrm = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(y)
        check(lib().ph_l2norm_bwd(ptr(g), ptr(y), ptr(nrm), ptr(dx), y.shape[0], y.shape[1], stream()), "ph_l2norm_bwd")
        return dx


def eltwise(a, b, op):
    a = _f32(a)
    out = torch.empty_like(a)
    check(lib().ph_eltwise(ptr(a), ptr(b), ptr(out), a.numel(), op, stream()), "ph_eltwise")
    return out


def dropout_(x, p, seed, site_offset, step_counter, alpha=False):
    """In-place (alpha-)dropout; `step_counter` is a device uint64 advanced once per forward so that the launch
    is replayable inside a captured HIP graph."""
    if p > 0:
        check(lib().ph_dropout_dev(ptr(x), x.numel(), p, seed, site_offset, ptr(step_counter), int(alpha), stream()),
              "ph_dropout_dev")
    return x


def counter_inc(counter):
    check(lib().ph_counter_inc(ptr(counter), stream()), "ph_counter_inc")


def outer(o1, o2, append_one):
    o1, o2 = _f32(o1), _f32(o2)
    Bn, D1 = o1.shape
    D2 = o2.shape[1]
    out = torch.empty(Bn, (D1 + append_one) * (D2 + append_one), device=o1.device, dtype=torch.float32)
    check(lib().ph_outer(ptr(o1), ptr(o2), ptr(out), Bn, D1, D2, int(append_one), stream()), "ph_outer")
    return out


def void_array(ptrs):
    arr = (C.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


# ---------------------------------------------------------------- L1 weight regulariser (define_reg)
_flat_registry = {}     # untyped-storage pointer of a FlatParams buffer -> weakref to it (train_step.FlatParams registers)


def register_flat(fp):
    import weakref
    _flat_registry[fp.flat.untyped_storage().data_ptr()] = weakref.ref(fp)


def _l1_segments(tensors):
    """[(param pointer, element count, gradient pointer or None, tensors covered)]: runs of parameters that sit back
    to back in one FlatParams buffer (16-byte aligned, zero padding in between: |0| = 0, sgn(0) = 0) become ONE
    segment whose gradient goes straight into the flat gradient buffer; anything else is a segment of its own."""
    segs = []
    for t in tensors:
        t = require_cuda(t, "parameter")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("define_reg expects contiguous float32 parameters")
        ref = _flat_registry.get(t.untyped_storage().data_ptr())
        fp = ref() if ref is not None else None
        if fp is not None and fp.flat.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
            off = (t.data_ptr() - fp.flat.data_ptr()) // 4
            end = off + (t.numel() + 3) // 4 * 4
            direct = (fp.grad is not None and t.requires_grad and t.grad is not None
                      and t.grad.data_ptr() == fp.grad.data_ptr() + 4 * off)
            last = segs[-1] if segs else None
            if (last is not None and last["fp"] is fp and last["end"] == off and last["direct"] == direct):
                last["end"] = end
                last["tensors"].append(t)
                continue
            segs.append(dict(fp=fp, off=off, end=end, direct=direct, tensors=[t]))
        else:
            segs.append(dict(fp=None, off=0, end=t.numel(), direct=False, tensors=[t]))
    return segs


class L1RegFn(torch.autograd.Function):
    """sum_i |W_i|.sum() of the reference's regularize_* helpers (utils.py:60-198) as a device scalar.  Backward:
    sgn(W) * upstream, accumulated IN PLACE into the flat gradient buffer where the parameter's .grad is a view of it
    (the optimiser's zero_grad() runs before backward() in every step class), returned to autograd otherwise."""

    @staticmethod
    def forward(ctx, *tensors):
        segs = _l1_segments(tensors)
        dev = tensors[0].device
        out = torch.zeros(1, device=dev, dtype=torch.float32)
        scratch = torch.empty(1024, device=dev, dtype=torch.float32)
        for sg in segs:
            w = sg["fp"].flat[sg["off"]:sg["end"]] if sg["fp"] is not None else sg["tensors"][0].reshape(-1)
            check(lib().ph_l1_sum(ptr(w), w.numel(), ptr(scratch), ptr(out), 1, stream()), "ph_l1_sum")
        ctx.segs = segs
        ctx.tensors = tensors
        return out[0]

    @staticmethod
    def backward(ctx, g):
        g = g.reshape(1).float().contiguous()
        grads = {}
        for sg in ctx.segs:
            if sg["direct"]:
                fp = sg["fp"]
                check(lib().ph_l1_sign_axpy(ptr(fp.flat[sg["off"]:sg["end"]]), ptr(fp.grad[sg["off"]:sg["end"]]),
                                            sg["end"] - sg["off"], ptr(g), 1.0, stream()), "ph_l1_sign_axpy")
                continue
            for t in sg["tensors"]:
                if not t.requires_grad:
                    continue
                d = torch.zeros_like(t)
                check(lib().ph_l1_sign_axpy(ptr(t), ptr(d), t.numel(), ptr(g), 1.0, stream()), "ph_l1_sign_axpy")
                grads[id(t)] = d
        return tuple(grads.get(id(t)) for t in ctx.tensors)


def l1_norm_sum(tensors):
    tensors = list(tensors)
    if not tensors:
        return None        # the reference's helpers return None when nothing matched (the caller's `lambda_reg * None` raises)
    return L1RegFn.apply(*tensors)

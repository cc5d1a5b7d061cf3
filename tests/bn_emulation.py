"""References of the BatchNorm, ReLU, pooling and stem-backward kernels of the ResNet trunk (csrc/bn_act.hip) for
tests/test_gpu_bn_act.py, and the case tables of that sweep.  The layout is that of tests/head_emulation.py.

Every operator is one function of (inputs, dt, defect).  dt = float64 is the reference of the definition: nn.BatchNorm2d in training
mode (biased batch variance, unbiased running variance), ReLU, MaxPool2d(3, 2, 1) with the first maximum's position, the global
average pool, and their gradients; tests/test_bn_emulation_cpu.py checks these against torch float64 (F.batch_norm, F.max_pool2d
with return_indices, F.adaptive_avg_pool2d and autograd).  dt = float32 restates the kernel in its summation order - per-thread
partial sums over pl, pl + npl, .., the sh[..] combine over q, blocks of per = ceil(npix / nb) pixels, the 32-lane row walk of the
stem kernels, the q < 32 combine of the average pool, the 256-thread strided double sums of the finalize kernels - and ends with
the output type's rounding: bf16 round-to-nearest-even, or the half-pair split hi = fp16(x), lo = fp16((x - hi) * 2^11) with
saturation at +-65504.  The float64 form carries no output rounding.  An output array of a case is compared in one of two classes:

  exact   named in the entry's `exact`: the inputs come from dyadic grids (y = k/4 with |k| <= 8, scale in +-{1/2, 1, 2}, shift =
          j/4, gradients small integers over 8) on which every product and sum the kernel forms is exact in float32, so an fma and
          two roundings cannot differ and every mask is bit-determined; or the array is a copy, a maximum or a rounding of inputs
          (arg-max codes, amax rows, dzs, pack_input).  The float64 reference, cast to the output type, equals the float32
          restatement bit for bit (checked on the CPU) and the device must equal it too: no outlier allowance.
  real    everything else, on normal random data: within MARGIN (4) x the float32 restatement's error against float64 on the same
          inputs, plus FLOOR[operator] x max |ref| (4 x the largest excess of the MI355X over the restatement; the figures are in
          the docstring of tests/test_gpu_bn_act.py, which prints them on every run).

Tensors are NHWC float32 arrays holding values the mode's storage type represents (bf16 in PH_PREC_BF16, half pairs where a
half-pair image is read), so the conversion to the device type loses nothing.

tests/test_bn_emulation_cpu.py shows that the tolerances accept the restatement and reject every injected defect by a factor of 4
or more (an exact array rejects by not being equal)."""
import ctypes as C

import numpy as np

from tests.dense_emulation import err, scale, _fma      # noqa: F401  (err / scale are part of this module's interface)

F32, F64 = np.float32, np.float64
MARGIN = 4.0
OK, EINVAL = 0, -22
BF16, BF16X6, FP16X3 = 0, 1, 3                          # PH_PREC_* of the tensors (csrc/ph_common.h)
PRECS = (BF16, BF16X6, FP16X3)
PNAME = {BF16: "bf16", BF16X6: "bf16x6", FP16X3: "fp16x3"}
BWD_BLOCKS_MAX, STEM_ROWS, EW_BLOCKS, EW_ITEMS = 1024, 16, 2048, 4

# Relative floor per operator, in units of max |ref|: 4 x the measured excess of the device's error over the restatement's (the
# kernels' `a * b + c` are contracted to fmas where hipcc chooses, rsqrtf and the divisions are the device's).  An operator without an
# entry never exceeded its restatement.
FLOOR = {"bn_finalize": 4 * 5.37e-8, "avgpool_bwd": 4 * 9.573e-10, "bn_eval_params": 4 * 7.882e-10}

vp, i32, f32, f64, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
# the test entry points at the end of csrc/bn_act.hip (not part of include/pathomic_hip.h)
SIGNATURES = {
    "ph_debug_bn_pack_input": [vp, vp, i32, i32, i32, i32, vp],
    "ph_debug_bn_finalize": [vp, i32, i32, f64, f32, f32] + [vp] * 10,
    "ph_debug_bn_eval_params": [vp] * 9 + [i32, f32, vp],
    "ph_debug_bn_apply": [vp] * 9 + [sz, i32, i32, i32, i32, vp],
    "ph_debug_bn_relu_maxpool": [vp] * 7 + [i32] * 5 + [vp],
    "ph_debug_bn_avgpool": [vp, vp, i32, i32, i32, i32, vp],
    "ph_debug_bn_avgpool_t": [vp, vp, i32, i32, i32, i32, vp],
    "ph_debug_bn_avgpool_bwd": [vp, vp, i32, i32, i32, i32, i32, vp],
    "ph_debug_bn_bwd_parts": [sz, i32],
    "ph_debug_bn_stem_bwd_parts": [i32, i32],
    "ph_debug_bn_bwd_reduce": [vp] * 6 + [sz, i32, i32, vp, vp, vp, vp],
    "ph_debug_bn_bwd_finalize": [vp, i32, i32, f64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "ph_debug_bn_bwd_finalize_fused": [vp, i32, i32, f64, vp, vp, vp, vp, vp, i32, vp],
    "ph_debug_bn_bwd_apply": [vp] * 9 + [sz, i32, i32, vp, vp, vp, vp],
    "ph_debug_bn_stem_bwd_reduce": [vp] * 9 + [i32] * 5 + [vp, i32, vp],
    "ph_debug_bn_stem_bwd_apply": [vp] * 11 + [i32] * 5 + [vp, vp],
}


def bind(L):
    """Declare the ph_debug_bn_* entries of the loaded library L (AttributeError if one is missing)."""
    for name, args in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = i32, args
    return L


def base_op(op):
    """The operator of a suite: the suite's name without its class ("bn_apply_exact", "bn_apply_stride" -> "bn_apply")."""
    for suffix in ("_exact", "_stride", "_clamp"):
        if op.endswith(suffix):
            op = op[:-len(suffix)]
    return "bn_bwd_finalize" if op == "dzs" else op


def tolerance(op, ref, rest):
    return MARGIN * err(ref, rest) + FLOOR.get(base_op(op), 0.0) * scale(ref)


def cast(e, k):
    """The float64 reference array k of suite entry e as the device stores it (what an array of the exact class must equal)."""
    ref = e["ref"][k]
    if ref.dtype.kind != "f" or ref.dtype == np.float16:
        return ref
    kind = {"out": "T", "x4": "T", "dx": "TY", "dy": "T"}.get(k, "f32")
    return round_to(ref.astype(F32), kind, e["inp"].get("prec", BF16X6))


def entry_tolerance(e, k):
    return tolerance(e["op"], e["ref"][k], e["rest"][k])


# ------------------------------------------------------------------------------------------------ storage types
def bf16r(x):
    """float32 -> bf16 (round to nearest even) -> float32."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def hp_split(x):
    """The half-pair split of float32 x: (hi, lo) as float16, x ~ hi + lo 2^-11, saturating at +-65504."""
    x = np.clip(np.asarray(x, dtype=F32), F32(-65504), F32(65504))
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(F32)) * F32(2048)).astype(np.float16)
    return hi, lo


def hp_join(hi, lo):
    return hi.astype(F32) + lo.astype(F32) * F32(1.0 / 2048)


def hpr(x):
    return hp_join(*hp_split(x))


def round_to(x, kind, prec):
    """float32 x as stored: kind "T" = an activation as the convolutions read it (bf16 | float | half pair), "TY" = a convolution
    output or a gradient (bf16 | float | float), anything else = float32."""
    x = np.asarray(x, dtype=F32)
    if kind in ("T", "TY") and prec == BF16:
        return bf16r(x)
    if kind == "T" and prec == FP16X3:
        return hpr(x)
    return x


def _o(x, kind, prec, dt):
    """An output: unrounded in the float64 reference, as stored in the restatement."""
    return x if dt is F64 else round_to(x, kind, prec)


def _madd(a, b, c, dt):
    """a * b + c: one fma in float32 (hipcc contracts, and bn_apply asks for it), plain in float64."""
    return _fma(np.asarray(a), np.asarray(b), np.asarray(c)) if dt is F32 else a * b + c


def _butterfly(w):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    return w


def _nbr(v, by=8):
    """Per-channel constants of the neighbouring channel group."""
    return np.roll(v, -by, axis=-1)


def ew_grid(n8):
    """Blocks of the grid-stride elementwise passes (C / 8 divides 256)."""
    b = (n8 + 255) // 256
    return b if b <= EW_BLOCKS else max(EW_BLOCKS, (b + EW_ITEMS - 1) // EW_ITEMS)


def _drop(out, n8, defect):
    """The elements (of arrays shaped [.., C] with n8 eight-channel vectors) that a dropped block / iteration leaves unwritten."""
    i = np.arange(n8)
    g = ew_grid(n8) * 256
    if defect == "drop_last_block":
        lost = i >= (n8 // 256) * 256
    else:                                    # drop_tail_iter: the iteration after which `more` is false, where there was a prefetch
        lost = (i >= g) & (i + g >= n8)
    assert lost.any()
    res = {}
    for k, a in out.items():
        a = np.array(a, dtype=F32).reshape(n8, 8)
        a[lost] = np.nan
        res[k] = a.reshape(np.shape(out[k]))
    return res


def _seed(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def _act(rng, shape, kind, prec, exact, grid=4, kmax=8):
    """An input tensor: dyadic grid (exact class) or normal random data rounded to its storage type."""
    if exact:
        return (rng.integers(-kmax, kmax + 1, shape) / grid).astype(F32)
    return round_to(rng.standard_normal(shape).astype(F32), kind, prec)


def _chan(rng, C, exact, what):
    """Per-channel constants: "scale" (no zeros, both signs), "shift", "pos" (an invstd), "small" (c1 / c2)."""
    if exact:
        if what in ("scale", "pos"):
            s = rng.choice(np.array([0.5, 1.0, 2.0]), C)
            return (s * (rng.choice(np.array([-1.0, 1.0]), C) if what == "scale" else 1.0)).astype(F32)
        return (rng.integers(-4, 5, C) / (4 if what == "shift" else 16)).astype(F32)
    if what == "scale":
        return (rng.uniform(0.5, 1.5, C) * rng.choice(np.array([-1.0, 1.0]), C)).astype(F32)
    if what == "pos":
        return rng.uniform(0.5, 2.0, C).astype(F32)
    return (rng.standard_normal(C) * (0.5 if what == "shift" else 0.05)).astype(F32)


# ------------------------------------------------------------------------------------------------ pack_input
def pack_input(i, dt, defect=None):
    """NCHW float32 -> NHWC4 of the activation type, channel 3 zero.  Half-pair mode: planes [2][npix][4] fp16 (hi, lo)."""
    x, prec = i["x"], i["prec"]
    B, _, H, W = x.shape
    v = np.zeros((B * H * W, 4), dt)
    v[:, :3] = x.transpose(0, 2, 3, 1).reshape(-1, 3)
    if defect == "ch3_nonzero":
        v[:, 3] = v[:, 2]
    if dt is F64:
        out = {"x4": v}
        if prec == FP16X3:
            out["hi"], out["lo"] = hp_split(v.astype(F32))      # (bit-determined: the split of the input itself)
        return out
    if prec != FP16X3:
        return {"x4": round_to(v, "T", prec)}
    hi, lo = hp_split(v)
    if defect == "planes_swapped":
        hi, lo = lo, hi
    return {"x4": hp_join(hi, lo), "hi": hi, "lo": lo}


# ------------------------------------------------------------------------------------------------ finalize kernels
def _dsum(p, kernel):
    """Sum of p [nparts][C] over the parts in double.  kernel: 256 threads add parts tid, tid + 256, .., the 64-lane butterfly, the four
    wave sums one after the other; else numpy's long double."""
    if not kernel:
        return p.astype(np.longdouble).sum(0).astype(F64)
    n, Cc = p.shape
    a = np.concatenate([p.astype(F64), np.zeros((-n % 256, Cc))]).reshape(-1, 256, Cc)
    acc = np.zeros((256, Cc))
    for r in range(a.shape[0]):
        acc = acc + a[r]
    w = _butterfly(acc.reshape(4, 64, Cc).transpose(0, 2, 1))[..., 0]          # [4][C]
    return ((w[0] + w[1]) + w[2]) + w[3]


def bn_finalize(i, dt, defect=None):
    """parts [nparts][2][C] (sum x, sum x^2) -> mean, invstd, scale, shift and the running statistics (momentum m: new = (1 - m) old
    + m batch, the batch variance unbiased) of nn.BatchNorm2d in training mode."""
    k = dt is F32
    cnt, eps, mom = F64(i["count"]), F64(F32(i["eps"])), i["momentum"]
    s1, s2 = _dsum(i["parts"][:, 0], k), _dsum(i["parts"][:, 1], k)
    m = s1 / cnt
    var = s2 / cnt - m * m
    if defect != "var_unclamped":
        var = np.maximum(var, 0.0)
    with np.errstate(invalid="ignore"):
        istd = 1.0 / np.sqrt(var + eps)
    gamma, beta = i["gamma"].astype(dt), i["beta"].astype(dt)
    out = {"mean": m.astype(dt), "invstd": istd.astype(dt)}
    out["scale"] = gamma * out["invstd"]
    out["shift"] = _madd(-out["mean"], out["scale"], beta, dt)
    if i["running"] is not None:
        unb = var if (cnt <= 1 or defect == "biased_running") else var * cnt / (cnt - 1.0)
        a, b = dt(1) - dt(F32(mom)), dt(F32(mom))
        if defect == "momentum_swapped":
            a, b = b, a
        out["running_mean"] = _madd(a, i["running"][0].astype(dt), b * m.astype(dt), dt)
        out["running_var"] = _madd(a, i["running"][1].astype(dt), b * unb.astype(dt), dt)
        if i["nbt"] is not None:
            out["nbt"] = np.array([i["nbt"] + (len(gamma) if defect == "nbt_per_channel" else 1)], np.int64)
    return out


def bn_eval_params(i, dt, defect=None):
    """Eval mode: every unit's mean / invstd / scale / shift from its running statistics; the units one after the other."""
    res = {k: [] for k in ("mean", "invstd", "scale", "shift")}
    for u in i["units"]:
        rm, rv, g, b = (u[k].astype(dt) for k in ("running_mean", "running_var", "gamma", "beta"))
        istd = (dt(1) / np.sqrt(rv + dt(F32(i["eps"])))).astype(dt)
        sc = g * istd
        for k, v in (("mean", rm), ("invstd", istd), ("scale", sc), ("shift", _madd(-rm, sc, b, dt))):
            res[k].append(v)
    return {k: np.concatenate(v) for k, v in res.items()}


def dz_scale(bound):
    """float32 bound -> (2^e, 2^-e) with bound 2^e in [2^9, 2^10), e clamped to +-100; 1 for a bound of 0 or infinity."""
    e = 0
    if bound > 0 and np.isfinite(bound):
        e = 9 - (int(np.frexp(F64(bound))[1]) - 1)
    e = max(-100, min(100, e))
    return e


def bn_bwd_finalize(i, dt, defect=None):
    """parts [nparts][nrow][C] -> dbeta = sum dz, dgamma = sum dz xhat, c1 = dbeta / count, c2 = dgamma / count; nrow = 3: the second sum
    is row `row2` times invstd.  dzs (with amax, gamma, invstd): the power-of-two pair of the half-pair dz tensor."""
    k = dt is F32
    p, row2 = i["parts"], i["row2"]
    if defect == "row2_swapped":
        row2 = 3 - row2
    s1, s2 = _dsum(p[:, 0], k), _dsum(p[:, row2], k)
    if i["fused"] and defect != "s2_no_invstd":
        s2 = s2 * i["invstd"].astype(F64)
    cnt = F64(i["count"])
    out = {"c1": (s1 / cnt).astype(dt), "c2": (s2 / cnt).astype(dt)}
    if i["dgb"]:
        out["dbeta"], out["dgamma"] = s1.astype(dt), s2.astype(dt)
    if i["amax"] is not None:
        g = np.abs(i["gamma"].astype(dt) * i["invstd"].astype(dt)).astype(dt).max()
        bound = dt(i["amax"].astype(dt).max() * g)
        e = dz_scale(bound) + (1 if defect == "dzs_exp_off" else 0)
        out["dzs"] = np.array([np.ldexp(1.0, e), np.ldexp(1.0, e if defect == "dzs_not_reciprocal" else -e)], F32)
    return out


# ------------------------------------------------------------------------------------------------ bn_apply
def bn_apply(i, dt, defect=None):
    """out = relu?(y scale + shift + [res | y_r scale_r + shift_r | T(relu(y_r scale_r + shift_r))]); relu bit 0: on the sum, bit 1: on
    the shortcut term, which is then an activation of its own and rounded to the activation type (bf16) like one."""
    prec, C = i["prec"], i["C"]
    sc, sh = i["scale"].astype(dt), i["shift"].astype(dt)
    if defect == "neighbour_cg":
        sc, sh = _nbr(sc), _nbr(sh)
    v = _madd(i["y"].astype(dt), sc, sh, dt)
    if i["res"] is not None:
        v = v + i["res"].astype(dt)
    elif i["y_r"] is not None:
        t = _madd(i["y_r"].astype(dt), i["scale_r"].astype(dt), i["shift_r"].astype(dt), dt)
        if i["relu"] & 2:
            t = np.where(t > 0, t, dt(0))
            if prec != FP16X3 and defect != "shortcut_unrounded":
                t = round_to(t.astype(F32), "T", prec).astype(dt)
        v = v + t
    pre = v
    if i["relu"] & 1:
        v = np.where(v > 0, v, dt(0))
    out = {"out": _o(v, "T", prec, dt)}
    if i["out32"]:
        out["out32"] = pre if defect == "out32_differs" else v
    if defect in ("drop_last_block", "drop_tail_iter"):
        out = _drop(out, i["npix"] * C // 8, defect)
    return out


# ------------------------------------------------------------------------------------------------ max pool
def _maxpool(a, y, defect=None):
    """a [B][H][W][C] (>= 0) -> its 3 x 3 / stride 2 / pad 1 maximum, the window position kh * 3 + kw of the first maximum in row-major
    order and y there.  Padding never counts."""
    B, H, W, Cc = a.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    if defect == "pad_counted":            # out-of-image taps read the clamped coordinate
        ap, yp = (np.pad(t, ((0, 0), (1, 2), (1, 2), (0, 0)), mode="edge") for t in (a, y))
    else:
        ap = np.pad(a, ((0, 0), (1, 2), (1, 2), (0, 0)), constant_values=-np.inf)
        yp = np.pad(y, ((0, 0), (1, 2), (1, 2), (0, 0)))
    best = np.full((B, OH, OW, Cc), -np.inf, a.dtype)
    code = np.zeros((B, OH, OW, Cc), np.uint8)
    raw = np.zeros((B, OH, OW, Cc), y.dtype)
    for kh in range(3):
        for kw in range(3):
            t = ap[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            up = (t >= best) if defect == "last_max" else (t > best)
            up &= np.isfinite(t)
            best = np.where(up, t, best)
            code = np.where(up, np.uint8(kw * 3 + kh if defect == "code_kw_kh" else kh * 3 + kw), code)
            raw = np.where(up, yp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2], raw)
    return best, code, raw


def bn_relu_maxpool(i, dt, defect=None):
    prec = i["prec"]
    y = i["y"].astype(dt)
    a = _madd(y, i["scale"].astype(dt), i["shift"].astype(dt), dt)
    best, code, raw = _maxpool(np.where(a > 0, a, dt(0)), y, defect)
    out = {"out": _o(best, "T", prec, dt)}
    if prec == FP16X3:
        out["out32"] = best
    if i["idx"]:
        out["idx"] = code
        if i["raw"]:
            out["raw"] = raw
    if defect == "oh_floor" and y.shape[1] % 2:
        out = {k: np.where(np.arange(v.shape[1])[None, :, None, None] < y.shape[1] // 2, v,
                           np.nan if v.dtype.kind == "f" else 255).astype(v.dtype) for k, v in out.items()}
    return out


# ------------------------------------------------------------------------------------------------ average pool
def avgpool(i, dt, defect=None):
    """x [B][HW][C] -> its mean over the pixels [B][C].  Kernel: lane pl of 32 adds pixels pl, pl + 32, ..; the 32 lane sums are added
    one after the other; one division by HW."""
    x = i["x"].astype(dt)
    B, HW, Cc = x.shape
    if dt is F64:
        return {"out": x.mean(1)}
    a = np.concatenate([x, np.zeros((B, -HW % 32, Cc), F32)], 1).reshape(B, -1, 32, Cc)
    s = np.zeros((B, 32, Cc), F32)
    for r in range(a.shape[1]):
        s = s + a[:, r]
    t = np.zeros((B, Cc), F32)
    for q in range(32):
        t = t + s[:, q]
    return {"out": t / F32(a.shape[1] * 32 if defect == "lane_rounded_count" else HW)}


def avgpool_bwd(i, dt, defect=None):
    """dx [B][HW][C] (+)= g [B][C] / HW.  The kernel multiplies by the float32 reciprocal."""
    B, HW, Cc = i["B"], i["HW"], i["C"]
    g = i["g"].astype(dt)
    gb = np.broadcast_to(g[:, None, :], (B, HW, Cc))
    acc = i["accumulate"] and defect != "no_accumulate"
    if dt is F64:
        v = gb / F64(HW) + (i["dx"].astype(F64) if acc else 0.0)
    else:
        inv = np.broadcast_to(F32(1) / F32(HW), (B, HW, Cc))
        v = _fma(gb, inv, i["dx"]) if acc else gb * inv
    return {"dx": _o(np.array(v), "TY", i["prec"], dt)}


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_bwd_parts(npix, C):
    return max(1, min(BWD_BLOCKS_MAX, (npix * (C // 8) + 2047) // 2048))


def _masked_dz(i, dt, defect):
    g, y = i["g"].astype(dt), i["y"].astype(dt)
    if i["a"] is not None:
        a = i["a"]
        return np.where((a >= 0) if defect == "relu_ge" else (a > 0), g, dt(0))
    if i["mscale"] is not None:
        if defect == "mask_from_a":
            return np.where(i["a_block"] > 0, g, dt(0))
        t = _madd(y, i["mscale"].astype(dt), i["mshift"].astype(dt), dt)
        return np.where((t >= 0) if defect == "relu_ge" else (t > 0), g, dt(0))
    return g


def bn_bwd_reduce(i, dt, defect=None):
    """g, y [npix][C] -> parts [nb][2][C]: per block of per = ceil(npix / nb) pixels the sums of dz and of dz xhat, dz = g where the ReLU let
    the activation through (a > 0, or y mscale + mshift > 0, or everywhere); amax [nb]: the block's largest |dz|."""
    npix, Cc = i["npix"], i["C"]
    nb, npl = bn_bwd_parts(npix, Cc), 256 // (Cc // 8)
    per = (npix + nb - 1) // nb
    dz = _masked_dz(i, dt, defect)
    mu, istd = i["mean"].astype(dt), i["invstd"].astype(dt)
    if defect == "neighbour_cg":
        mu, istd = _nbr(mu), _nbr(istd)
    t = dz * (i["y"].astype(dt) - mu)
    iters = (per + npl - 1) // npl
    rows = nb * iters * npl

    def blocks(v):           # [nb][iters][npl][C]: block b owns pixels b per .. min(npix, (b + 1) per), zero beyond
        w = np.zeros((nb, iters * npl, Cc), v.dtype)
        full = min(nb, npix // per)
        w[:full, :per] = v[:full * per].reshape(full, per, Cc)
        if full < nb and npix > full * per:
            w[full, :npix - full * per] = v[full * per:]
        return w.reshape(nb, iters, npl, Cc)
    dzb, tb = blocks(dz), blocks(t)
    if defect == "drop_ragged":          # the iteration in which only some lanes still own a pixel
        own = blocks(np.ones((npix, Cc), dz.dtype))[..., 0]
        ragged = (own.sum(2) > 0) & (own.sum(2) < npl)
        assert ragged.any()
        dzb, tb = dzb * ~ragged[:, :, None, None], tb * ~ragged[:, :, None, None]
    out = {}
    if dt is F64:
        out["parts"] = np.stack([dzb.sum((1, 2)), (tb * istd).sum((1, 2))], 1)
    else:
        s1, s2 = np.zeros((nb, npl, Cc), F32), np.zeros((nb, npl, Cc), F32)
        ib = np.broadcast_to(istd, s1.shape)
        for r in range(iters):
            s1 = s1 + dzb[:, r]
            s2 = _fma(tb[:, r], ib, s2)
        p1, p2 = np.zeros((nb, Cc), F32), np.zeros((nb, Cc), F32)
        for q in range(npl):
            p1, p2 = p1 + s1[:, q], p2 + s2[:, q]
        out["parts"] = np.stack([p1, p2], 1)
    assert rows >= npix
    if i["amax"]:
        out["amax"] = np.abs(dzb).max((1, 2, 3)).astype(F32)
    return out


def bn_bwd_apply(i, dt, defect=None):
    """dy = gamma invstd (dz - c1 - xhat c2); half-pair mode stores dy dzs[0] as pairs, "dy" is the decoded tensor times dzs[1]."""
    prec, Cc = i["prec"], i["C"]
    dz = _masked_dz(i, dt, defect)
    mu, istd, ga, c1, c2 = (i[k].astype(dt) for k in ("mean", "invstd", "gamma", "c1", "c2"))
    if defect == "neighbour_cg":
        mu, istd, ga, c1, c2 = (_nbr(v) for v in (mu, istd, ga, c1, c2))
    xh = (i["y"].astype(dt) - mu) * istd
    v = (ga * istd) * _madd(-xh, c2, dz - c1, dt)
    if i["dzs"] is not None and dt is F32:
        v = hpr(v * i["dzs"][0]) * i["dzs"][1]
    out = {"dy": _o(v, "T" if i["dzs"] is None else "f32", prec, dt)}
    if defect in ("drop_last_block", "drop_tail_iter"):
        out = _drop(out, i["npix"] * Cc // 8, defect)
    return out


# ------------------------------------------------------------------------------------------------ stem backward
def stem_scatter(dpool, idx, H, W):
    """The max-pool backward by its definition: every window sends its gradient to the pixel its arg-max code names."""
    B, OH, OW, Cc = dpool.shape
    dz = np.zeros((B, H, W, Cc), dpool.dtype)
    b, ph, pw, c = np.meshgrid(np.arange(B), np.arange(OH), np.arange(OW), np.arange(Cc), indexing="ij")
    kh, kw = idx // 3, idx % 3
    np.add.at(dz, (b, 2 * ph - 1 + kh, 2 * pw - 1 + kw, c), dpool)
    return dz


def _stem_gather(dpool, idx, H, W, defect=None):
    """The same per input pixel, in the kernel's order: the (up to) four windows (h >> 1 | (h + 1) >> 1) x (w >> 1 | (w + 1) >> 1)."""
    B, OH, OW, Cc = dpool.shape
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    dz = np.zeros((B, H, W, Cc), dpool.dtype)
    for a in (0, 1):
        for c in (0, 1):
            ph, pw = (h + a) >> 1, (w + c) >> 1
            ok = ~((a == 1) & (ph == h >> 1)) & ~((c == 1) & (pw == w >> 1)) & (ph < OH) & (pw < OW)
            if defect == "window_missing" and a == 1:
                ok = ok & (h % 2 == 0)
            code = (h - (2 * ph - 1)) * 3 + (w - (2 * pw - 1))
            phc, pwc = np.minimum(ph, OH - 1) + 0 * pw, np.minimum(pw, OW - 1) + 0 * ph
            hit = ok[None, :, :, None] & (idx[:, phc, pwc] == code[None, :, :, None])
            dz = dz + np.where(hit, dpool[:, phc, pwc], dpool.dtype.type(0))
    return dz


def stem_blocks(B, H):
    return (B * H + STEM_ROWS - 1) // STEM_ROWS


def _walk(rows, nb, per):
    """rows [R][W][64] -> [nb][per][ceil(W / 32)][32][64]: block, its row, the lane's step, the lane; zero beyond."""
    R, W, Cc = rows.shape
    w = np.zeros((nb * per, -(-W // 32) * 32, Cc), rows.dtype)
    w[:R, :W] = rows
    return w.reshape(nb, per, -1, 32, Cc)


def _lane_sums(dzw, xhw, dt):
    """Per-block sums of dz and dz xhat over a _walk()."""
    if dt is F64:
        return np.stack([dzw.sum((1, 2, 3)), (dzw * xhw).sum((1, 2, 3))], 1)
    nb, per, steps = dzw.shape[:3]
    s1, s2 = np.zeros((nb, 32, 64), F32), np.zeros((nb, 32, 64), F32)
    for r in range(per):
        for j in range(steps):
            s1 = s1 + dzw[:, r, j]
            s2 = _fma(dzw[:, r, j], xhw[:, r, j], s2)
    p1, p2 = np.zeros((nb, 64), F32), np.zeros((nb, 64), F32)
    for q in range(32):
        p1, p2 = p1 + s1[:, q], p2 + s2[:, q]
    return np.stack([p1, p2], 1)


def stem_bwd_reduce(i, dt, defect=None):
    """dpool [B][OH][OW][64], idx, y [B][H][W][64] -> parts [ceil(B H / 16)][2][64].  form "pixel": a block owns 16 image rows, dz = the
    scattered gradient where bn(y) > 0.  form "pooled" / "raw" (even H): a block owns 8 pooled rows and sums over windows, y read at
    the arg-max (through idx, or from raw); amax = 4 x the block's largest masked window gradient.  "sums": the rows added up."""
    B, H, W = i["B"], i["H"], i["W"]
    sc, sf, mu, istd = (i[k].astype(dt) for k in ("scale", "shift", "mean", "invstd"))
    nb = stem_blocks(B, H)
    dp, y = i["dpool"].astype(dt), i["y"].astype(dt)
    out = {}
    if i["form"] == "pixel":
        dz = stem_scatter(dp, i["idx"], H, W) if dt is F64 else _stem_gather(dp, i["idx"], H, W, defect)
        dz = np.where(_madd(y, sc, sf, dt) > 0, dz, dt(0))
        xh = (y - mu) * istd
        out["parts"] = _lane_sums(_walk(dz.reshape(B * H, W, 64), nb, STEM_ROWS), _walk(xh.reshape(B * H, W, 64), nb, STEM_ROWS), dt)
    else:
        z = i["raw"].astype(dt)                     # y at the arg-max (the pooled form gathers the same values through idx)
        OH, OW = z.shape[1:3]
        dz = np.where(_madd(z, sc, sf, dt) > 0, dp, dt(0))
        xh = (z - mu) * istd
        dzw = _walk(dz.reshape(B * OH, OW, 64), nb, STEM_ROWS // 2)
        out["parts"] = _lane_sums(dzw, _walk(xh.reshape(B * OH, OW, 64), nb, STEM_ROWS // 2), dt)
        if i["amax"]:
            out["amax"] = (np.abs(dzw).max((1, 2, 3, 4)) * (1 if defect == "amax_no_4" else 4)).astype(F32)
    out["sums"] = out["parts"].astype(F64).sum(0) if dt is F64 else out["parts"].astype(F64).sum(0).astype(F32)
    return out


def stem_bwd_apply(i, dt, defect=None):
    """dy0 = gamma invstd (dz - c1 - xhat c2) with dz the scattered, masked gradient; half-pair mode as bn_bwd_apply."""
    B, H, W, prec = i["B"], i["H"], i["W"], i["prec"]
    sc, sf, mu, istd, ga, c1, c2 = (i[k].astype(dt) for k in ("scale", "shift", "mean", "invstd", "gamma", "c1", "c2"))
    dp, y = i["dpool"].astype(dt), i["y"].astype(dt)
    dz = stem_scatter(dp, i["idx"], H, W) if dt is F64 else _stem_gather(dp, i["idx"], H, W, defect)
    dz = np.where(_madd(y, sc, sf, dt) > 0, dz, dt(0))
    xh = (y - mu) * istd
    v = (ga * istd) * _madd(-xh, c2, dz - c1, dt)
    if i["dzs"] is not None and dt is F32:
        v = hpr(v * i["dzs"][0]) * i["dzs"][1]
    return {"dy": _o(v, "T" if i["dzs"] is None else "f32", prec, dt)}


# ------------------------------------------------------------------------------------------------ the case tables
APPLY_C, APPLY_NPIX = (64, 128, 256, 512), (1, 3, 33)
# (name, res, y_r, relu, out32, res_as_t, modes)
APPLY_VARIANTS = (("plain", 0, 0, 0, 0, 0, PRECS), ("plain relu", 0, 0, 1, 0, 0, PRECS), ("res", 1, 0, 1, 0, 0, PRECS),
                  ("y_r relu1", 0, 1, 1, 0, 0, PRECS), ("y_r relu3", 0, 1, 3, 0, 0, PRECS), ("hp out32", 0, 0, 1, 1, 0, (FP16X3,)),
                  ("hp res out32", 1, 0, 1, 1, 0, (FP16X3,)), ("hp res_as_t", 1, 0, 1, 0, 1, (FP16X3,)),
                  ("hp res_as_t out32", 1, 0, 1, 1, 1, (FP16X3,)))
# eight-channel vectors of the three grid-stride shapes; the tensor has ceil(n8 / (C / 8)) pixels (a whole number of pixels, still
# inside the same last block): one block and a few vectors past 2048 blocks, two to three iterations with a ragged last one, and a
# grid above 2048 blocks
STRIDE_N8 = (2048 * 256 + 264, 4097 * 256 + 8, 8193 * 256 - 100)
POOL_SHAPES = ((1, 2, 2), (2, 5, 7), (1, 6, 5), (3, 8, 66))
AVG_B, AVG_HW, AVG_C = (1, 3), (1, 31, 32, 33, 49, 256), (64, 512)
FIN_NPARTS, FIN_C = (1, 255, 257, 1000), (64, 512)
BWD_C, BWD_NPIX, BWD_CLAMP_NPIX = (64, 128, 256, 512), (5, 33, 300, 1000), 262144 + 77
BFIN_NPARTS = (1, 3, 256, 257, 1024)
STEM_SHAPES = ((5, 6, 10), (2, 16, 70), (1, 7, 9), (3, 5, 66))
PACK_SHAPES = ((2, 3, 5), (1, 17, 16))
EVAL_WIDTHS = (64, 128, 256, 512)


def stride_npix(n8, C):
    return -(-n8 // (C // 8))


def _entry(op, name, inp, fn, defects=(), exact=()):
    """One case of one operator: inputs, float64 reference, float32 restatement, the restatement with each defect; `exact` names the
    output arrays of the exact class (all of them: True)."""
    ref = fn(inp, F64)
    return dict(op=op, name=name, inp=inp, ref=ref, rest=fn(inp, F32), defects={d: fn(inp, F32, d) for d in defects},
                exact=set(ref) if exact is True else set(exact or ()))


STRIDE_PERIOD = 4099          # pixels (a prime: no multiple of a block, of the grid's stride or of a channel-group count)


def _tiled_entry(op, name, inp, npix, fn):
    """A case of an ELEMENTWISE operator on npix pixels whose tensors repeat the STRIDE_PERIOD pixels of `inp`: reference and restatement
    are those of the period, repeated (what makes tensors of 17 M elements cheap to state).  The defect is the dropped tail iteration."""
    e = _entry(op, name, inp, fn, (), True if op == "bn_apply_stride" else ())

    def rep(a):
        return a if not isinstance(a, np.ndarray) or a.shape[:1] != (STRIDE_PERIOD,) else np.tile(a, (-(-npix // STRIDE_PERIOD), 1))[:npix]
    e["inp"] = {k: rep(v) for k, v in inp.items()}
    e["inp"]["npix"] = npix
    e["ref"], e["rest"] = ({k: rep(v) for k, v in e[w].items()} for w in ("ref", "rest"))
    if npix * inp["C"] // 8 < 2 * EW_BLOCKS * 256:
        e["defects"] = {"drop_tail_iter": _drop(e["rest"], npix * inp["C"] // 8, "drop_tail_iter")}
    return e


def _apply_inp(prec, npix, C, var, exact, seed):
    name, res, yr, relu, out32, rat, _ = var
    r = _seed(1, prec, npix, C, seed, exact)
    i = dict(prec=prec, npix=npix, C=C, relu=relu, out32=out32, res_as_t=rat, res=None, y_r=None, scale_r=None, shift_r=None,
             y=_act(r, (npix, C), "TY", prec, exact), scale=_chan(r, C, exact, "scale"), shift=_chan(r, C, exact, "shift"))
    if res:
        i["res"] = _act(r, (npix, C), "T" if rat else "TY", prec, exact)
    if yr:
        # relu & 2, exact class, bf16: a finer grid, so that the shortcut term is exact in float32 and NOT representable in bf16
        i["y_r"] = _act(r, (npix, C), "TY", prec, exact)
        if exact and relu & 2 and prec == BF16:
            i["y_r"] = bf16r(i["y_r"] + F32(1.0 / 128) * r.integers(0, 2, (npix, C)).astype(F32))
        i["scale_r"], i["shift_r"] = _chan(r, C, exact, "scale"), _chan(r, C, exact, "shift")
    return i


def _bwd_inp(prec, npix, C, mask, exact, seed, hp_dzs=False):
    r = _seed(2, prec, npix, C, seed, exact)
    i = dict(prec=prec, npix=npix, C=C, mask=mask, a=None, mscale=None, mshift=None, amax=prec == FP16X3,
             g=(r.integers(-8, 9, (npix, C)) / 8).astype(F32) if exact else _act(r, (npix, C), "TY", prec, False),
             y=_act(r, (npix, C), "TY", prec, exact), mean=_chan(r, C, exact, "shift"), invstd=_chan(r, C, exact, "pos"))
    blk = _act(r, (npix, C), "TY", prec, exact)
    i["a_block"] = np.where(blk > 0, blk, F32(0))               # a block output: zeros where the ReLU cut
    if mask == "a":
        i["a"] = i["a_block"]
    elif mask == "m":
        i["mscale"], i["mshift"] = _chan(r, C, exact, "scale"), _chan(r, C, exact, "shift")
    i["gamma"], i["c1"], i["c2"] = _chan(r, C, exact, "scale"), _chan(r, C, exact, "small"), _chan(r, C, exact, "small")
    i["dzs"] = None
    if hp_dzs:                                                  # the scale the finalize pass derives from this tensor's amax rows
        am = bn_bwd_reduce(i, F32)["amax"]
        i["amax_rows"] = am
        i["dzs"] = bn_bwd_finalize(dict(parts=np.zeros((1, 2, C), F32), row2=1, fused=False, count=1.0, dgb=False, amax=am,
                                        gamma=i["gamma"], invstd=i["invstd"]), F32)["dzs"]
    return i


def _pool_ref_inputs(r, B, H, W, prec, exact):
    """A stem: y, scale, shift and the forward's idx / raw by the reference (never by the forward kernel)."""
    y = _act(r, (B, H, W, 64), "TY", prec, exact)
    sc, sf = np.abs(_chan(r, 64, exact, "scale")) * np.where(np.arange(64) % 5 == 4, -1, 1).astype(F32), _chan(r, 64, exact, "shift")
    if exact:
        sf[::8] = -8                             # every eighth channel: all zeros after the ReLU, every window a tie of zeros
    a = y.astype(F64) * sc + sf
    _, idx, raw = _maxpool(np.where(a > 0, a, 0.0), y)
    return y, sc, sf, idx, raw


def _stem_inp(prec, B, H, W, form, exact, seed, amax=False, hp_dzs=False):
    r = _seed(3, prec, B, H, W, seed, exact)
    y, sc, sf, idx, raw = _pool_ref_inputs(r, B, H, W, prec, exact)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    i = dict(prec=prec, B=B, H=H, W=W, form=form, y=y, scale=sc, shift=sf, idx=idx, raw=raw, amax=amax,
             dpool=(r.integers(-8, 9, (B, OH, OW, 64)) / 8).astype(F32) if exact else _act(r, (B, OH, OW, 64), "TY", prec, False),
             mean=_chan(r, 64, exact, "shift"), invstd=_chan(r, 64, exact, "pos"), gamma=_chan(r, 64, exact, "scale"),
             c1=_chan(r, 64, exact, "small"), c2=_chan(r, 64, exact, "small"), dzs=None)
    if hp_dzs:
        am = stem_bwd_reduce(dict(i, form="raw", amax=True), F32)["amax"]
        i["amax_rows"] = am
        i["dzs"] = bn_bwd_finalize(dict(parts=np.zeros((1, 2, 64), F32), row2=1, fused=False, count=1.0, dgb=False, amax=am,
                                        gamma=i["gamma"], invstd=i["invstd"]), F32)["dzs"]
    return i


def _const_channel():
    """A float32 v whose square rounds DOWN to float32: sums of n copies of v and of fl(v^2) give a negative variance in double."""
    for k in range(1, 200):
        v = F32(1.0 + k / 128.0 + 1.0 / 4096)
        if F64(F32(F64(v) * F64(v))) < F64(v) * F64(v):
            return v
    raise AssertionError


def _fin_inp(nparts, C, running, count1, seed):
    r = _seed(4, nparts, C, seed)
    if count1:
        x = r.standard_normal((1, 1, C)).astype(F32)
        parts, cnt = np.concatenate([x, x * x], 1), 1.0
    else:
        n = 16                                   # pixels per part
        x = (r.standard_normal((nparts, n, C)) * r.uniform(0.5, 3, C) + r.standard_normal(C)).astype(F64)
        parts = np.stack([x.sum(1), (x * x).sum(1)], 1).astype(F32)
        v = _const_channel()
        parts[:, 0, 1], parts[:, 1, 1] = F32(n) * v, F32(n) * F32(F64(v) * F64(v))          # the constant channel: the clamp is taken
        cnt = float(nparts * n)
    i = dict(parts=parts, count=cnt, eps=1e-5, momentum=0.1, gamma=_chan(r, C, False, "scale"), beta=_chan(r, C, False, "shift"),
             running=None, nbt=None, nparts=nparts, C=C)
    if running:
        i["running"] = (r.standard_normal(C).astype(F32), r.uniform(0.5, 2, C).astype(F32))
        i["nbt"] = 41 + nparts
    return i


def _suite(op):
    out = []
    if op == "pack_input":
        for B, H, W in PACK_SHAPES:
            for prec in PRECS:
                r = _seed(5, B, H, W, prec)
                x = (r.standard_normal((B, 3, H, W)) * 3).astype(F32)
                x.flat[:6] = (0.0, -0.0, 65504.0, 1e5, -1e5, 2.0 ** -20)          # zeros, the largest half, saturation, a tiny value
                out.append(_entry(op, "B%d H%d W%d %s" % (B, H, W, PNAME[prec]), dict(x=x, prec=prec, B=B, H=H, W=W), pack_input,
                                  ("ch3_nonzero",) + (("planes_swapped",) if prec == FP16X3 else ()), True))
    elif op in ("bn_apply_exact", "bn_apply"):
        ex = op == "bn_apply_exact"
        for C in APPLY_C:
            for npix in APPLY_NPIX:
                for var in APPLY_VARIANTS:
                    for prec in var[6]:
                        i = _apply_inp(prec, npix, C, var, ex, 0)
                        dfs = ["neighbour_cg"]
                        if (npix * C // 8) % 256 and npix * C // 8 > 256:
                            dfs.append("drop_last_block")
                        if var[3] & 2 and prec == BF16 and ex and npix == 33:
                            dfs.append("shortcut_unrounded")
                        if var[4] and ex and npix > 1:
                            dfs.append("out32_differs")
                        out.append(_entry(op, "C%d npix%d %s %s" % (C, npix, var[0], PNAME[prec]), i, bn_apply,
                                          dfs if npix > 1 else (), ex))
    elif op == "bn_apply_stride":
        for C in (64, 512):
            for n, n8 in enumerate(STRIDE_N8):
                npix = stride_npix(n8, C)
                out.append(_tiled_entry(op, "C%d n8 %d res bf16" % (C, npix * C // 8), _apply_inp(BF16, STRIDE_PERIOD, C, APPLY_VARIANTS[2], True, 1 + n),
                                        npix, bn_apply))
    elif op in ("bn_relu_maxpool_exact", "bn_relu_maxpool"):
        ex = op == "bn_relu_maxpool_exact"
        for B, H, W in POOL_SHAPES:
            for idx, raw in ((0, 0), (1, 0), (1, 1)):
                for prec in PRECS:
                    r = _seed(6, B, H, W, prec, ex)
                    y, sc, sf, _, _ = _pool_ref_inputs(r, B, H, W, prec, ex)
                    i = dict(prec=prec, B=B, H=H, W=W, C=64, y=y, scale=sc, shift=sf, idx=idx, raw=raw)
                    dfs = ()
                    if ex and idx:
                        dfs = ("last_max", "code_kw_kh", "pad_counted") + (("oh_floor",) if H % 2 else ())
                    # real data: `out` alone is compared (an arg-max may differ between two roundings of near-equal taps)
                    if not ex:
                        i = dict(i, idx=0, raw=0)
                        if idx:
                            continue
                    out.append(_entry(op, "B%d H%d W%d idx%d raw%d %s" % (B, H, W, idx, raw, PNAME[prec]), i, bn_relu_maxpool, dfs, ex))
    elif op in ("avgpool", "avgpool_t"):
        for B in AVG_B:
            for HW in AVG_HW:
                for C in AVG_C:
                    for prec in PRECS:
                        r = _seed(7, B, HW, C, prec)
                        x = _act(r, (B, HW, C), "T" if op == "avgpool_t" else "TY", prec, False) + F32(0.5)
                        x = round_to(x, "T" if op == "avgpool_t" else "TY", prec)
                        out.append(_entry(op, "B%d HW%d C%d %s" % (B, HW, C, PNAME[prec]), dict(x=x, prec=prec, B=B, HW=HW, C=C), avgpool,
                                          ("lane_rounded_count",) if HW % 32 else ()))
    elif op == "avgpool_bwd":
        for B in AVG_B:
            for HW in AVG_HW:
                for C in AVG_C:
                    for acc in (0, 1):
                        for prec in PRECS:
                            ex = HW & (HW - 1) == 0                  # a power of two: g / HW is exact on the dyadic grid
                            r = _seed(8, B, HW, C, prec, acc)
                            g = (r.integers(-8, 9, (B, C)) / 8).astype(F32) if ex else r.standard_normal((B, C)).astype(F32)
                            i = dict(prec=prec, B=B, HW=HW, C=C, accumulate=acc, g=g, dx=_act(r, (B, HW, C), "TY", prec, ex) if acc else None)
                            out.append(_entry(op, "B%d HW%d C%d acc%d %s" % (B, HW, C, acc, PNAME[prec]), i, avgpool_bwd,
                                              ("no_accumulate",) if acc else (), ex))
    elif op == "bn_finalize":
        for nparts in FIN_NPARTS:
            for C in FIN_C:
                for running in (0, 1):
                    i = _fin_inp(nparts, C, running, False, 0)
                    dfs = ("var_unclamped",) + (("biased_running", "momentum_swapped", "nbt_per_channel") if running else ())
                    out.append(_entry(op, "nparts%d C%d running%d" % (nparts, C, running), i, bn_finalize, dfs, ("nbt",) if running else ()))
        for running in (0, 1):
            out.append(_entry(op, "count1 C64 running%d" % running, _fin_inp(1, 64, running, True, 1), bn_finalize,
                              ("momentum_swapped", "nbt_per_channel") if running else (), ("nbt",) if running else ()))
    elif op == "bn_eval_params":
        for n in (1, 20):
            r = _seed(9, n)
            units = [dict(C=EVAL_WIDTHS[(u + n) % 4], **{k: _chan(r, EVAL_WIDTHS[(u + n) % 4], False, w) for k, w in
                          (("gamma", "scale"), ("beta", "shift"), ("running_mean", "shift"), ("running_var", "pos"))}) for u in range(n)]
            out.append(_entry(op, "%d units" % n, dict(units=units, eps=1e-5, n=n), bn_eval_params, (), ("mean",)))
    elif op in ("bn_bwd_reduce_exact", "bn_bwd_reduce", "bn_bwd_apply_exact", "bn_bwd_apply"):
        ex, red = op.endswith("_exact"), "reduce" in op
        fn = bn_bwd_reduce if red else bn_bwd_apply
        for C in BWD_C:
            for npix in BWD_NPIX:
                for mask in ("a", "m", "none"):
                    for prec in PRECS:
                        if ex and not red and prec != BF16X6:
                            continue               # (the apply pass's output is exact only before its rounding: fp32 tensors)
                        i = _bwd_inp(prec, npix, C, mask, ex, 0, hp_dzs=not red and prec == FP16X3)
                        dfs = []
                        if npix > 5 and (ex or prec != BF16 or red):
                            dfs.append("neighbour_cg")
                            if mask == "a" or (mask == "m" and ex):      # (real data: y mscale + mshift is never exactly 0)
                                dfs.append("relu_ge")
                            if mask == "m":
                                dfs.append("mask_from_a")
                            if red and (-(-npix // bn_bwd_parts(npix, C))) % (256 // (C // 8)):
                                dfs.append("drop_ragged")
                            if not red and (npix * C // 8) % 256 and npix * C // 8 > 256:
                                dfs.append("drop_last_block")
                        exact = (("amax",) if i["amax"] else ()) if red else ()
                        out.append(_entry(op, "C%d npix%d mask-%s %s" % (C, npix, mask, PNAME[prec]), i, fn, dfs,
                                          True if ex else exact))
    elif op == "bn_bwd_reduce_clamp":
        i = _bwd_inp(BF16, BWD_CLAMP_NPIX, 64, "a", False, 2)
        out.append(_entry(op, "C64 npix%d mask-a bf16" % BWD_CLAMP_NPIX, i, bn_bwd_reduce))
    elif op == "bn_bwd_apply_stride":
        for C in (64, 512):
            for n, n8 in enumerate(STRIDE_N8):
                npix = stride_npix(n8, C)
                out.append(_tiled_entry(op, "C%d n8 %d mask-a bf16" % (C, npix * C // 8), _bwd_inp(BF16, STRIDE_PERIOD, C, "a", False, 3 + n), npix,
                                        bn_bwd_apply))
    elif op == "bn_bwd_finalize":
        for nparts in BFIN_NPARTS:
            for dgb in (0, 1):
                for fused, row2 in ((0, 1), (1, 1), (1, 2)):
                    C = 64 if nparts % 2 else 128
                    r = _seed(10, nparts, dgb, fused, row2)
                    i = dict(parts=r.standard_normal((nparts, 3 if fused else 2, C)).astype(F32), row2=row2, fused=fused, count=float(nparts * 49),
                             dgb=dgb, amax=None, gamma=_chan(r, C, False, "scale"), invstd=_chan(r, C, False, "pos"), nparts=nparts, C=C)
                    dfs = ("s2_no_invstd", "row2_swapped") if fused else ()
                    if not fused:
                        i["amax"] = np.abs(r.standard_normal(max(1, nparts // 2))).astype(F32)
                        dfs = ("dzs_exp_off", "dzs_not_reciprocal")
                    out.append(_entry(op, "nparts%d dgb%d fused%d row2 %d" % (nparts, dgb, fused, row2), i, bn_bwd_finalize, dfs,
                                      ("dzs",) if not fused else ()))
    elif op == "dzs":
        # bounds across the binades: amax = 1.5 2^j, max |gamma invstd| = 1 (exact products); j beyond +-91 / 109: the clamp; 0; infinity
        for j in list(range(-120, 121, 7)) + ["zero", "inf"]:
            am = np.array([0.0 if j == "zero" else (np.inf if j == "inf" else np.ldexp(1.5, j)), 0.0, 0.0], F32)
            i = dict(parts=np.ones((1, 2, 64), F32), row2=1, fused=False, count=1.0, dgb=0, amax=am, j=j, nparts=1, C=64,
                     gamma=np.where(np.arange(64) == 7, -2.0, 0.25).astype(F32), invstd=np.where(np.arange(64) == 7, 0.5, 1.0).astype(F32))
            out.append(_entry(op, "bound 1.5 2^%s" % j, i, bn_bwd_finalize,
                              ("dzs_exp_off", "dzs_not_reciprocal") if j not in ("zero", "inf") and abs(j) < 90 else (), True))
    elif op in ("stem_bwd_reduce_exact", "stem_bwd_reduce"):
        ex = op.endswith("_exact")
        for B, H, W in STEM_SHAPES:
            for prec in PRECS:
                forms = ("pixel",) if H % 2 else ("raw", "pooled", "pixel")
                for form in forms:
                    i = _stem_inp(prec, B, H, W, form, ex, 0, amax=form != "pixel" and prec == FP16X3)
                    dfs = ()
                    if form == "pixel" and (ex or prec != BF16):
                        dfs = ("window_missing",)
                    if i["amax"]:
                        dfs = ("amax_no_4",)
                    out.append(_entry(op, "B%d H%d W%d %s %s" % (B, H, W, form, PNAME[prec]), i, stem_bwd_reduce, dfs,
                                      True if ex else (("amax",) if i["amax"] else ())))
    elif op in ("stem_bwd_apply_exact", "stem_bwd_apply"):
        ex = op.endswith("_exact")
        for B, H, W in STEM_SHAPES:
            for prec in PRECS:
                if ex:
                    # gamma invstd = 1, c1 = c2 = 0: dy0 is the scattered, masked gradient itself
                    i = _stem_inp(prec, B, H, W, "pixel", True, 1)
                    i.update(gamma=np.ones(64, F32), invstd=np.ones(64, F32), c1=np.zeros(64, F32), c2=np.zeros(64, F32))
                else:
                    i = _stem_inp(prec, B, H, W, "pixel", False, 1, hp_dzs=prec == FP16X3 and H % 2 == 0)
                out.append(_entry(op, "B%d H%d W%d %s" % (B, H, W, PNAME[prec]), i, stem_bwd_apply,
                                  ("window_missing",) if ex or prec != BF16 else (), ex))
    else:
        raise KeyError(op)
    return out


OPS = ("pack_input", "bn_apply_exact", "bn_apply", "bn_apply_stride", "bn_relu_maxpool_exact", "bn_relu_maxpool", "avgpool", "avgpool_t",
       "avgpool_bwd", "bn_finalize", "bn_eval_params", "bn_bwd_reduce_exact", "bn_bwd_reduce", "bn_bwd_reduce_clamp", "bn_bwd_finalize",
       "dzs", "bn_bwd_apply_exact", "bn_bwd_apply", "bn_bwd_apply_stride", "stem_bwd_reduce_exact", "stem_bwd_reduce",
       "stem_bwd_apply_exact", "stem_bwd_apply")
# (operator name for FLOOR / excess: the suite's name without its class)
_cache = {}


def suite(op):
    """The cases of one operator (computed once per process; treat the arrays as read-only)."""
    if op not in _cache:
        _cache[op] = _suite(op)
    return _cache[op]

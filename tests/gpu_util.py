"""Helpers shared by the -m gpu parity tests (they call the product through its C-ABI / module API and
compare with the CPU oracle)."""
import ctypes

import numpy as np
import torch

# kernel families of the tap-conv / weight-gradient launchers, in the bit order of ph_debug_dispatch_mask (csrc/ph_kernels.h PH_DK_*)
DISPATCH_FAMILIES = ["gen1_bf16", "gen1_hp16", "gen1_f32", "tap2", "tap2_masked", "tap2_l1", "tap3", "tap3_hp", "tap4", "tap5",
                     "tap6", "tap6b", "tap7", "wgrad_bf16", "wgrad_hp16", "wgrad_f32",
                     # the dense GEMMs (dense.hip): 16 x 16 tiles, 64 x 64 tiles, split-K + finish
                     "sgemm16", "sgemm64", "sgemm_splitk"]

GUARD = 4096          # bytes of sentinel on each side of an output (a multiple of 256: the half-pair alignment is kept)
SENTINEL = 0x5A


class Guarded:
    """An output tensor of `shape` / `dtype` inside a byte buffer with sentinel guard bands."""

    def __init__(self, shape, dtype, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        es = torch.empty((), dtype=dtype).element_size()
        self.nbytes = n * es
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 256 == 0

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.nbytes:]])
        return bool((g == SENTINEL).all())

    def snapshot(self):
        return self.buf.clone()


def dispatch_lib():
    """The library with its (non-public) dispatch-record hooks bound: ph_debug_dispatch_mask / ph_debug_dispatch_reset."""
    from multimodal_learning_amd._lib import lib
    L = lib()
    L.ph_debug_dispatch_mask.restype = ctypes.c_uint
    L.ph_debug_dispatch_mask.argtypes = []
    L.ph_debug_dispatch_reset.restype = None
    L.ph_debug_dispatch_reset.argtypes = []
    return L


def dispatched(L):
    """The kernel families launched since the last ph_debug_dispatch_reset()."""
    m = L.ph_debug_dispatch_mask()
    return {f for i, f in enumerate(DISPATCH_FAMILIES) if m >> i & 1}


def nhwc(x, dtype):
    """NCHW cpu fp32 -> NHWC cuda tensor of the activation dtype."""
    return x.permute(0, 2, 3, 1).contiguous().to("cuda").to(dtype)


def hp_pack(x, scale=1.0):
    """fp32 cuda tensor whose innermost extent is a multiple of 64 -> the half-pair storage of PH_PREC_FP16X3 (same shape and
    byte size, an opaque float32 container; include/pathomic_hip.h: ph_hp_pack)."""
    from multimodal_learning_amd._lib import lib, ptr, stream, check
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib().ph_hp_pack(ptr(x), ptr(out), x.numel(), float(scale), stream()), "ph_hp_pack")
    return out


def hp_unpack(x):
    from multimodal_learning_amd._lib import lib, ptr, stream, check
    out = torch.empty_like(x)
    check(lib().ph_hp_unpack(ptr(x), ptr(out), x.numel(), stream()), "ph_hp_unpack")
    return out


def nchw_cpu(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def _d(a):
    if torch.is_tensor(a):
        return a.detach().double().cpu()
    return torch.as_tensor(np.asarray(a)).double()


def maxerr(a, b):
    a, b = _d(a), _d(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item(), a.abs().max().item()


def assert_close(ref, got, atol, rtol=0.0, what=""):
    err, mx = maxerr(ref, got)
    assert err <= atol + rtol * mx, f"{what}: max|err| {err:.3e} > {atol:.1e} + {rtol:.1e}*{mx:.3e}"
    return err


class Report:
    """Collects every comparison of a test, prints the whole table, fails at the end if any exceeded its
    tolerance (one GPU round trip shows all errors instead of the first)."""

    def __init__(self, title):
        self.title, self.rows = title, []

    def close(self, ref, got, atol, rtol=0.0, what=""):
        err, mx = maxerr(ref, got)
        self.rows.append((what, err, mx, atol + rtol * mx))
        return err

    def add(self, what, err, mx, tol):
        """A row whose error and tolerance the caller worked out."""
        self.rows.append((what, err, mx, tol))
        return err

    def finish(self):
        print(f"\n== {self.title}")
        bad = []
        for what, err, mx, tol in self.rows:
            flag = "" if err <= tol else "   <-- FAIL"
            print(f"   {what:<34s} max|err| {err:9.3e}   max|ref| {mx:9.3e}   tol {tol:9.3e}{flag}")
            if err > tol:
                bad.append(what)
        assert not bad, f"{self.title}: out of tolerance: {bad}"


def assert_same(a, b, path="r"):
    """Exact equality of two nested results (dicts, lists / tuples, numpy arrays with dtype, floats, None)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            assert_same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, "%s[%d]" % (path, k))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, float) and a != a:
        assert b != b, path
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


def count_host_reads(monkeypatch):
    """Wrap torch.Tensor's cpu / item / tolist / numpy so that each call counts; returns the dict whose "n" is the count."""
    calls = {"n": 0}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            calls["n"] += 1
            return orig(self, *a, **k)
        return f
    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    return calls

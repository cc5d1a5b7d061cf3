"""Host side of ph_group_quantile (csrc/evalmetrics.hip) without a GPU: the symbol is bound with the
declared signature, the ABI version stays 1, and every refused argument comes back as PH_EINVAL before any HIP call -
pointers are never dereferenced on the host (the one host array, the copy of the offsets, is a real one)."""
import ctypes as C

import numpy as np

EINVAL = -22


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_symbol_signature_and_abi_version():
    from multimodal_learning_amd import _lib as B, ops
    L = _lib()
    assert L.ph_abi_version() == 1
    name = "ph_group_quantile"
    assert name in B.SIGNATURES and hasattr(L, name)
    fn = getattr(L, name)
    assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1]
    assert fn.argtypes[7] is C.c_double and len(fn.argtypes) == 10
    assert ops.AGG_FUN == {"mean": 0, "max": 1} and ops.QUANTILE_MAX_GROUP == 4096
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pathomic_hip.h")).read()
    assert "#define PH_QUANTILE_MAX_GROUP 4096" in hdr and "int ph_group_quantile(" in hdr


def _call(off, N=9, Cc=3, G=3, q=0.5, x=True, o=True, r=True, out=True):
    p = C.c_void_p(4096)                       # a non-null placeholder
    f = lambda on: p if on else None
    return _lib().ph_group_quantile(f(x), f(o), f(r), None if off is None else off.ctypes.data, N, Cc, G, q, f(out), None)


def test_refuses_null_pointers_and_sizes_out_of_range():
    good = np.array([0, 4, 5, 9], dtype=np.int32)
    for kw in (dict(x=False), dict(o=False), dict(r=False), dict(out=False)):
        assert _call(good, **kw) == EINVAL, kw
    assert _call(None) == EINVAL
    for kw in (dict(N=0), dict(N=-9), dict(N=(1 << 24) + 1), dict(Cc=0), dict(Cc=-1), dict(Cc=4097), dict(G=0), dict(G=-3),
               dict(G=10)):
        assert _call(good, **kw) == EINVAL, kw


def test_refuses_q_outside_the_unit_interval():
    good = np.array([0, 4, 5, 9], dtype=np.int32)
    for q in (-1e-9, 1.0 + 1e-9, float("nan"), -1.0, 2.0, 50.0, float("inf"), float("-inf")):
        assert _call(good, q=q) == EINVAL, q


def test_refuses_empty_groups_and_bad_end_offsets():
    for off in ([0, 4, 4, 9],          # an empty group
                [0, 0, 5, 9], [0, 5, 9, 9], [0, 6, 5, 9],      # first / last empty, a decreasing offset
                [1, 4, 5, 9], [0, 4, 5, 8]):                    # does not start at 0 / end at N
        assert _call(np.array(off, dtype=np.int32)) == EINVAL, off


def test_refuses_a_group_of_4097_rows():
    for off in ([0, 4097], [0, 1, 4098], [0, 4097, 4098]):
        a = np.array(off, dtype=np.int32)
        assert _call(a, N=int(a[-1]), G=len(off) - 1) == EINVAL, off

"""Host side of ph_surv_strata, ph_surv_table and ph_surv_logrank_km (csrc/survstrata.hip) without a
GPU: the symbols are bound with the declared signatures, the workspace queries give the documented sizes (0 for a refused
shape), and a NULL pointer or a value outside the documented ranges returns PH_EINVAL before any HIP call.  Every call here
returns before a launch; the device pointers are placeholders that are never dereferenced (q and pairs are HOST arrays and
are read)."""
import ctypes as C

import numpy as np
import pytest

OK, EINVAL = 0, -22
NAMES = ("ph_surv_strata_workspace_bytes", "ph_surv_strata", "ph_surv_table_workspace_bytes", "ph_surv_table",
         "ph_surv_logrank_km_workspace_bytes", "ph_surv_logrank_km")
MAX = 1 << 20
BAD_N = (1, 0, -5, MAX + 1, 1 << 30)


@pytest.fixture(scope="module")
def L():
    import multimodal_learning_amd as m
    m.build()
    return m.lib()


p = C.c_void_p(4096)                           # a non-null placeholder


def _q(*v):
    return np.asarray(v, dtype=np.float64)


def _pairs(*v):
    return np.asarray(v, dtype=np.int32).reshape(-1, 2)


def _each_null(call, args, required):
    for i in required:
        a = list(args)
        a[i] = None
        assert call(*a) == EINVAL, (call.__name__, i)


def test_symbols_are_bound_and_the_abi_version_stays(L):
    from multimodal_learning_amd import _lib as B
    assert L.ph_abi_version() == 1
    hdr = open(B.CSRC + "/../../include/pathomic_hip.h").read()
    for name in NAMES:
        assert name in B.SIGNATURES and hasattr(L, name) and (" %s(" % name) in hdr, name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name


def test_strata_argument_rule(L):
    assert L.ph_surv_strata_workspace_bytes(2, 1) == 64 and L.ph_surv_strata_workspace_bytes(MAX, 7) == 64
    q = _q(33, 66)
    for N in BAD_N:
        assert L.ph_surv_strata_workspace_bytes(N, 2) == 0, N
        assert L.ph_surv_strata(p, N, q.ctypes.data, 2, p, p, p, p, p, None) == EINVAL, N
    seven = _q(*range(10, 90, 10))
    for K in (0, 8, -1, 1 << 20):
        assert L.ph_surv_strata_workspace_bytes(300, K) == 0, K
        assert L.ph_surv_strata(p, 300, seven.ctypes.data, K, p, p, p, p, p, None) == EINVAL, K
    for bad in (float("nan"), -1.0, 101.0, float("inf"), -1e-9, 100.0000001):
        for at in (0, 1):
            q = _q(33, 66)
            q[at] = bad
            assert L.ph_surv_strata(p, 300, q.ctypes.data, 2, p, p, p, p, p, None) == EINVAL, (bad, at)
    q = _q(33, 66)
    _each_null(L.ph_surv_strata, (p, 300, q.ctypes.data, 2, p, p, p, p, p, None), (0, 2, 4, 5, 6, 7, 8))


def test_table_argument_rule(L):
    assert L.ph_surv_table_workspace_bytes(2, 1) == 8 and L.ph_surv_table_workspace_bytes(300, 3) == 1200
    assert L.ph_surv_table_workspace_bytes(MAX, 8) == 4 * MAX
    for N in BAD_N:
        assert L.ph_surv_table_workspace_bytes(N, 3) == 0, N
        assert L.ph_surv_table(p, p, p, N, 3, p, p, p, p, p, p, None) == EINVAL, N
    for G in (0, 9, -1, 1 << 20):
        assert L.ph_surv_table_workspace_bytes(300, G) == 0, G
        assert L.ph_surv_table(p, p, p, 300, G, p, p, p, p, p, p, None) == EINVAL, G
    _each_null(L.ph_surv_table, (p, p, p, 300, 3, p, p, p, p, p, p, None), (0, 1, 2, 5, 6, 7, 8, 9, 10))


def test_logrank_km_argument_rule(L):
    assert L.ph_surv_logrank_km_workspace_bytes(300, 3, 2) == 8 * 2 * (4 + 6)
    assert L.ph_surv_logrank_km_workspace_bytes(2, 1, 0) == 8 * 2 and L.ph_surv_logrank_km_workspace_bytes(256, 8, 28) == 8 * (56 + 16)
    assert L.ph_surv_logrank_km_workspace_bytes(MAX, 8, 28) == 8 * 4096 * (56 + 16)
    pr = _pairs((0, 1), (1, 2))
    for N in BAD_N:
        assert L.ph_surv_logrank_km_workspace_bytes(N, 3, 2) == 0, N
        assert L.ph_surv_logrank_km(p, p, p, N, 3, pr.ctypes.data, 2, p, p, p, None) == EINVAL, N
    for G in (0, 9, -1):
        assert L.ph_surv_logrank_km_workspace_bytes(300, G, 0) == 0, G
        assert L.ph_surv_logrank_km(p, p, p, 300, G, None, 0, None, p, p, None) == EINVAL, G
    many = _pairs(*[(a, b) for a in range(8) for b in range(a + 1, 8)], (1, 0))
    assert many.shape[0] == 29
    for P in (29, -1, 1 << 20):
        assert L.ph_surv_logrank_km_workspace_bytes(300, 8, P) == 0, P
        assert L.ph_surv_logrank_km(p, p, p, 300, 8, many.ctypes.data, P, p, p, p, None) == EINVAL, P
    # a pair index outside [0, G), or a group against itself
    for bad in ((0, 3), (3, 0), (-1, 1), (1, -1), (0, 1 << 20), (1, 1)):
        pr = _pairs((0, 1), bad)
        assert L.ph_surv_logrank_km(p, p, p, 300, 3, pr.ctypes.data, 2, p, p, p, None) == EINVAL, bad
    pr = _pairs((0, 1), (1, 2))
    _each_null(L.ph_surv_logrank_km, (p, p, p, 300, 3, pr.ctypes.data, 2, p, p, p, None), (0, 1, 2, 5, 7, 8, 9))
    # P == 0: pairs and stat may be NULL, the rest may not
    _each_null(L.ph_surv_logrank_km, (p, p, p, 300, 3, None, 0, None, p, p, None), (0, 1, 2, 8, 9))

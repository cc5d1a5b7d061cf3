"""Host side of the evaluation-tail entries (csrc/evalmetrics.hip) without a GPU: the symbols are bound
with the declared signatures, and every refused argument comes back as PH_EINVAL before any HIP call - pointers are never
dereferenced on the host (the one host array, ph_group_agg's copy of the offsets, is a real one)."""
import ctypes as C

import numpy as np

EINVAL = -22
NAMES = ("ph_rank_counts_workspace_bytes", "ph_rank_counts", "ph_confusion_counts", "ph_group_agg")


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_new_symbols_and_abi_version():
    from multimodal_learning_amd import _lib as B
    L = _lib()
    assert L.ph_abi_version() == 1
    for name in NAMES:
        assert name in B.SIGNATURES and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name


def test_rank_counts_refuses_bad_arguments():
    L = _lib()
    p = C.c_void_p(4096)                       # a non-null placeholder
    assert L.ph_rank_counts_workspace_bytes(4500, 3) == 8 * ((13500 + 255) // 256)
    assert L.ph_rank_counts_workspace_bytes(1, 1) == 8 and L.ph_rank_counts_workspace_bytes(1 << 20, 1) == 8 * 4096
    for N, Cc in ((0, 3), (-1, 3), (4, 0), (4, -3), ((1 << 20) // 3 + 1, 3), ((1 << 20) + 1, 1), (1 << 30, 1 << 30)):
        assert L.ph_rank_counts_workspace_bytes(N, Cc) == 0, (N, Cc)
        assert L.ph_rank_counts(p, p, N, Cc, p, p, p, None) == EINVAL, (N, Cc)
    for k in (0, 1, 4, 5, 6):
        args = [p, p, 300, 3, p, p, p, None]
        args[k] = None
        assert L.ph_rank_counts(*args) == EINVAL, k


def test_confusion_counts_refuses_bad_arguments():
    L = _lib()
    p = C.c_void_p(4096)
    for N, Cc in ((0, 3), (-5, 3), (10, 0), (10, -1), (10, 17)):
        assert L.ph_confusion_counts(p, p, N, Cc, p, None) == EINVAL, (N, Cc)
    for k in (0, 1, 4):
        args = [p, p, 10, 3, p, None]
        args[k] = None
        assert L.ph_confusion_counts(*args) == EINVAL, k


def test_group_agg_refuses_bad_arguments_and_empty_groups():
    L = _lib()
    p = C.c_void_p(4096)
    good = np.array([0, 4, 5, 9], dtype=np.int32)

    def call(off, N=9, Cc=3, G=3, fun=1, x=p, o=p, r=p, out=p):
        return L.ph_group_agg(x, o, r, None if off is None else off.ctypes.data, N, Cc, G, fun, out, None)

    for kw in (dict(x=None), dict(o=None), dict(r=None), dict(out=None)):
        assert call(good, **kw) == EINVAL, kw
    assert call(None) == EINVAL
    for kw in (dict(N=0), dict(N=-9), dict(N=(1 << 24) + 1), dict(Cc=0), dict(Cc=4097), dict(G=0), dict(G=10), dict(fun=2), dict(fun=-1)):
        assert call(good, **kw) == EINVAL, kw
    for off in ([0, 4, 4, 9],          # an empty group
                [0, 0, 5, 9], [0, 5, 9, 9], [0, 6, 5, 9],      # first / last empty, a decreasing offset
                [1, 4, 5, 9], [0, 4, 5, 8]):                    # does not start at 0 / end at N
        assert call(np.array(off, dtype=np.int32)) == EINVAL, off

"""Host side of ph_rank_counts_classes and ph_roc_points (csrc/evalmetrics.hip) without a GPU: the
symbols are bound with the declared signatures, the workspace queries give the documented sizes, and a NULL pointer, a size
outside the documented range or a cls outside [-1, C) returns PH_EINVAL before any HIP call.  Every call here returns
before a launch; the pointers are placeholders that are never dereferenced."""
import ctypes as C

import pytest

OK, EINVAL = 0, -22
NAMES = ("ph_rank_counts_classes_workspace_bytes", "ph_rank_counts_classes", "ph_roc_points_workspace_bytes", "ph_roc_points")
MAX = 1 << 20


@pytest.fixture(scope="module")
def L():
    import multimodal_learning_amd as m
    m.build()
    return m.lib()


p = C.c_void_p(4096)                           # a non-null placeholder


def _each_null(call, args, required):
    for i in required:
        a = list(args)
        a[i] = None
        assert call(*a) == EINVAL, (call.__name__, i)


def test_symbols_are_bound_and_the_abi_version_stays(L):
    from multimodal_learning_amd import _lib as B
    assert L.ph_abi_version() == 1
    for name in NAMES:
        assert name in B.SIGNATURES and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name


BAD_SHAPES = ((0, 3), (-1, 3), (4, 0), (4, -3), (4, 17), (MAX + 1, 1), (MAX + 1, 3), (1 << 30, 1 << 30))


def test_rank_counts_classes_argument_rule(L):
    assert L.ph_rank_counts_classes_workspace_bytes(4500, 3) == 8 * 3 * ((4500 + 255) // 256)
    assert L.ph_rank_counts_classes_workspace_bytes(1, 1) == 8
    assert L.ph_rank_counts_classes_workspace_bytes(256, 16) == 8 * 16 and L.ph_rank_counts_classes_workspace_bytes(257, 16) == 8 * 32
    assert L.ph_rank_counts_classes_workspace_bytes(MAX, 16) == 8 * 16 * 4096        # N alone is bounded, not N * C
    for N, Cc in BAD_SHAPES:
        assert L.ph_rank_counts_classes_workspace_bytes(N, Cc) == 0, (N, Cc)
        assert L.ph_rank_counts_classes(p, p, N, Cc, p, p, p, None) == EINVAL, (N, Cc)
    _each_null(L.ph_rank_counts_classes, (p, p, 300, 3, p, p, p, None), (0, 1, 4, 5, 6))


def test_roc_points_argument_rule(L):
    assert L.ph_roc_points_workspace_bytes(4500, 3) == 12 * 13500
    assert L.ph_roc_points_workspace_bytes(1, 1) == 12
    assert L.ph_roc_points_workspace_bytes(MAX // 16, 16) == 12 * MAX
    # N * C above 1048576: only the per-class problems (N elements) are served
    assert L.ph_roc_points_workspace_bytes(MAX // 16 + 1, 16) == 12 * (MAX // 16 + 1)
    assert L.ph_roc_points_workspace_bytes(MAX, 3) == 12 * MAX
    for N, Cc in BAD_SHAPES:
        assert L.ph_roc_points_workspace_bytes(N, Cc) == 0, (N, Cc)
        for cls in (-1, 0):
            assert L.ph_roc_points(p, p, N, Cc, cls, p, p, p, p, p, None) == EINVAL, (N, Cc, cls)
    for cls in (-2, 3, 4, 1 << 20, -(1 << 31)):
        assert L.ph_roc_points(p, p, 300, 3, cls, p, p, p, p, p, None) == EINVAL, cls
    assert L.ph_roc_points(p, p, MAX // 16 + 1, 16, -1, p, p, p, p, p, None) == EINVAL      # the micro problem does not fit
    for cls in (-1, 0, 2):
        _each_null(L.ph_roc_points, (p, p, 300, 3, cls, p, p, p, p, p, None), (0, 1, 5, 6, 7, 8, 9))

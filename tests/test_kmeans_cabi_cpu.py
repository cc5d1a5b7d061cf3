"""Host-side argument checks of ph_crd_kmeans_centers (csrc/crd_kmeans.hip) without a GPU: every PH_EINVAL is returned before
anything is launched, and the workspace size follows the documented layout."""
import ctypes

import pytest

EINVAL = -22


@pytest.fixture(scope="module")
def L():
    import multimodal_learning_amd as m
    m.build()
    return m.lib()


def test_workspace_bytes_follow_the_layout(L):
    # per bank, class and 256-row chunk: k x 128 partial sums, k counts, 256 running minima, 2 x 2 pick candidates
    for C, rows, k in ((3, 1, 2), (3, 256, 2), (3, 257, 4), (9, 513, 8), (3, 21846, 4)):
        chunks = (rows + 255) // 256
        assert L.ph_crd_kmeans_centers_workspace_bytes(C, rows, k) == 2 * C * chunks * (k * 128 + k + 256 + 4) * 4
    assert L.ph_crd_kmeans_centers_workspace_bytes(3, 0, 2) == L.ph_crd_kmeans_centers_workspace_bytes(3, 1, 2)
    assert L.ph_crd_kmeans_centers_workspace_bytes(0, 10, 2) == 0 and L.ph_crd_kmeans_centers_workspace_bytes(3, 10, 0) == 0


def test_argument_errors_return_before_any_launch(L):
    buf = (ctypes.c_float * 64)()                       # host memory: never dereferenced, 16-byte aligned or rejected for it
    p = ctypes.addressof(buf)
    p += -p % 16
    good = dict(mem1=p, mem2=p, members=p, offsets=p, C=3, rows=10, n=100, D=128, k=2, T=4, ws=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.ph_crd_kmeans_centers(a["mem1"], a["mem2"], a["members"], a["offsets"], a["C"], a["rows"], a["n"], a["D"], a["k"],
                                       a["T"], None, None, a["ws"], None)
    for kw in (dict(D=64), dict(k=1), dict(k=9), dict(k=0), dict(T=0), dict(C=0), dict(mem1=None), dict(mem2=None),
               dict(members=None), dict(offsets=None), dict(ws=None), dict(mem1=p + 4)):
        assert call(**kw) == EINVAL, kw

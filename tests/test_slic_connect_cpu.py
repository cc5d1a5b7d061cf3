"""The connectivity pass over SLIC label maps without a GPU: the restatement
(tests/slic_connect_emulation.py) on literal counts and on hand-made maps whose result can be read off, the properties
of the rule, defects that the cases must tell from the rule, and the host side of the two C-ABI entries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_connect_emulation as CE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


# ---- symbols and arguments -------------------------------------------------------------------------------------------
def test_symbols_are_bound_with_the_arity_of_the_header():
    from multimodal_learning_amd import _lib as B
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "pathomic_hip.h")).read()
    for name, nargs in (("ph_slic_connect_workspace_bytes", 4), ("ph_slic_connect", 9)):
        assert name in B.SIGNATURES and hasattr(L, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(decl.split(",")) == nargs == len(B.SIGNATURES[name][1]), name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name
    assert L.ph_abi_version() == 1


def test_workspace_bytes_on_the_host():
    L = _lib()
    prev = 0
    for n in (1, 2, 3, 9, 64, 256, 65535):
        b = L.ph_slic_connect_workspace_bytes(n, 1024, 1024, 100)
        assert b > prev and b >= n * (1024 * 1024 * 8 + 100 * 8)
        prev = b
    assert L.ph_slic_connect_workspace_bytes(1, 1, 1, 1) > 0
    assert L.ph_slic_connect_workspace_bytes(65535, 8192, 8192, 2048) >= 65535 * 8192 * 8192 * 8      # no 32-bit overflow
    for bad in ((0, 64, 64, 8), (-1, 64, 64, 8), (65536, 64, 64, 8), (1, 0, 64, 8), (1, 64, 0, 8), (1, 8193, 64, 8), (1, 64, 8193, 8),
                (1, 64, 64, 0), (1, 64, 64, 2049), (1, 64, 64, -3)):
        assert L.ph_slic_connect_workspace_bytes(*bad) == 0, bad


def test_every_bad_argument_is_refused_before_any_launch():
    """Nothing is dereferenced on the host and nothing launched: the codes come back without a device."""
    L = _lib()
    p = C.c_void_p(4096)
    good = dict(i=p, o=p, n=1, H=64, W=64, N=8, ms=4, ws=p)
    call = lambda **k: (lambda a: L.ph_slic_connect(a["i"], a["o"], a["n"], a["H"], a["W"], a["N"], a["ms"], a["ws"], None))({**good, **k})
    for bad in (dict(i=None), dict(o=None), dict(ws=None), dict(n=0), dict(n=-1), dict(n=65536), dict(H=0), dict(W=0), dict(H=8193),
                dict(W=8193), dict(H=-1), dict(N=0), dict(N=2049), dict(N=-1), dict(ms=0), dict(ms=-5)):
        assert call(**bad) == -22, bad


# ---- literal counts --------------------------------------------------------------------------------------------------
def _properties(labels, N, min_size, out, info):
    lab, o = labels.astype(np.int64), out.astype(np.int64)
    assert o.min() >= 0 and o.max() < N
    assert set(np.unique(o)) == set(np.unique(lab))
    stay = info["principal"] | info["kept_mask"]
    untouched = np.isin(info["comp"], info["roots"][stay])
    assert np.array_equal(o[untouched], lab[untouched])
    assert info["components_after"] <= np.unique(lab).size + info["kept"] + 1


@pytest.mark.parametrize("name", list(CE.TABLE))
def test_restatement_reproduces_the_literal_counts(name):
    _, _, _, labels, N, min_size = CE.table_labels(name)
    want = CE.TABLE[name][3]
    out, info = CE.connect(labels, N, min_size, return_info=True)
    got = (N, min_size, info["components"], info["merged"], info["kept"], info["changed"], info["components_after"])
    assert got == want
    assert out.dtype == np.int16 and out.shape == labels.shape
    _properties(labels, N, min_size, out, info)
    assert np.array_equal(CE.connect(labels, N, 1), labels)                # min_size = 1: the identity


# ---- hand-made maps --------------------------------------------------------------------------------------------------
def test_checkerboard_collapses_onto_column_zero_and_the_rest():
    cb = CE.checkerboard()
    out, info = CE.connect(cb, 2, 4096, return_info=True)
    assert info["components"] == 4096 and info["merged"] == 4094
    want = np.ones((64, 64), dtype=np.int16)
    want[:, 0] = 0
    assert np.array_equal(out, want)
    _properties(cb, 2, 4096, out, info)
    assert np.array_equal(CE.connect(cb, 2, 1), cb)


def test_of_two_equal_components_the_one_with_the_lower_first_pixel_stays():
    lab = np.zeros((5, 9), dtype=np.int16)
    lab[1:3, 1:3] = 1                                   # first pixel 10, 4 pixels
    lab[2:4, 5:7] = 1                                   # first pixel 23, 4 pixels
    out = CE.connect(lab, 2, 100)
    want = lab.copy()
    want[2:4, 5:7] = 0
    assert np.array_equal(out, want)


def test_min_size_is_a_strict_bound():
    lab = np.zeros((6, 12), dtype=np.int16)
    lab[1:3, 1:4] = 1                                   # principal of label 1: 6 pixels
    lab[4, 6:10] = 1                                    # 4 pixels
    assert np.array_equal(CE.connect(lab, 2, 4), lab)   # exactly min_size: kept
    want = lab.copy()
    want[4, 6:10] = 0
    assert np.array_equal(CE.connect(lab, 2, 5), want)  # min_size - 1 pixels: merged


def test_fragment_at_the_origin_and_row_zero_take_the_left_neighbour():
    lab = np.array([[1, 0, 2, 0, 0], [0, 0, 0, 0, 0], [1, 1, 2, 2, 0]], dtype=np.int16)
    out = CE.connect(lab, 3, 10)
    assert np.array_equal(out, np.array([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 2, 2, 0]], dtype=np.int16))


def test_labels_outside_the_table_stay():
    lab = np.array([[0, -1, 0, 0], [0, 0, 5, 0], [1, 0, 0, 0]], dtype=np.int16)
    out = CE.connect(lab, 2, 100)
    assert out[0, 1] == -1 and out[1, 2] == 5 and out[2, 0] == 1


def test_serpentine_is_one_component():
    lab = CE.serpentine()
    comp = CE.components(lab)
    assert (comp[lab == 0] == 0).all() and np.unique(comp[lab == 1]).size == 96 // 2


# ---- injected defects ------------------------------------------------------------------------------------------------
def _all_cases():
    for name in CE.TABLE:
        _, _, _, labels, N, min_size = CE.table_labels(name)
        yield labels, N, min_size
    yield CE.checkerboard(), 2, 4096
    lab = np.zeros((5, 9), dtype=np.int16); lab[1:3, 1:3] = 1; lab[2:4, 5:7] = 1
    yield lab, 2, 100
    lab = np.zeros((6, 12), dtype=np.int16); lab[1:3, 1:4] = 1; lab[4, 6:10] = 1
    yield lab, 2, 4


@pytest.mark.parametrize("defect", ["eight", "le", "tie_high", "left_first", "one_level", "principal_by_first"])
def test_every_injected_defect_fails_a_case(defect):
    failing = sum(not np.array_equal(CE.connect(l, N, ms, **{defect: True}), CE.connect(l, N, ms)) for l, N, ms in _all_cases())
    print(defect, "changes", failing, "cases")
    assert failing >= 1

"""Host side of the epoch entries (csrc/epochrec.hip) without a GPU: the symbols are bound with the
declared signatures, the header declares what the binding uses, and every refused argument comes back as PH_EINVAL before any
HIP call - device pointers are never dereferenced on the host (the two host arrays of ph_epoch_record_add are real ones)."""
import ctypes as C
import os
import re

EINVAL = -22
NAMES = ("ph_epoch_record_add", "ph_store_rows", "ph_sim_audit_workspace_bytes", "ph_sim_audit")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_new_symbols_header_and_abi_version():
    from multimodal_learning_amd import _lib as B
    from multimodal_learning_amd import epoch
    L = _lib()
    assert L.ph_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "pathomic_hip.h")).read()
    for name in NAMES:
        assert name in B.SIGNATURES and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(decl.split(",")) == len(B.SIGNATURES[name][1]), name
    defs = dict(re.findall(r"#define (PH_(?:EPOCHREC|REC)_[A-Z_]+) (\d+)", hdr))
    assert int(defs["PH_EPOCHREC_WORDS"]) == epoch.REC_WORDS and int(defs["PH_EPOCHREC_MAX_SCALARS"]) == 16
    assert (int(defs["PH_REC_ADD"]), int(defs["PH_REC_ADD_POSITIVE"])) == (epoch.REC_ADD, epoch.REC_ADD_POSITIVE)


def _scalars(n, ptr=4096, mode=0):
    return (C.c_void_p * max(n, 1))(*([ptr] * n)), (C.c_int32 * max(n, 1))(*([mode] * n))


def test_epoch_record_add_refuses_bad_arguments():
    L = _lib()
    p = C.c_void_p(4096)

    def call(rec=p, ns=2, sp=None, md=None, wvec=p, nw=5, pred=p, grade=p, B=8, Cc=3, row0=p, row1=p, nrow=8, ptr=4096, mode=1):
        a, b = _scalars(ns, ptr, mode)
        return L.ph_epoch_record_add(rec, C.cast(a, C.c_void_p) if sp is None else sp, C.cast(b, C.c_void_p) if md is None else md,
                                     ns, wvec, nw, pred, grade, B, Cc, row0, row1, nrow, None)

    null = C.c_void_p(None)
    for kw in (dict(rec=None), dict(rec=C.c_void_p(4100)), dict(ns=-1), dict(ns=17), dict(nw=-1), dict(nw=17), dict(wvec=None),
               dict(wvec=C.c_void_p(4098)), dict(pred=None), dict(grade=None), dict(B=0), dict(B=-3), dict(B=(1 << 20) + 1),
               dict(Cc=0), dict(Cc=17), dict(pred=C.c_void_p(4098)), dict(grade=C.c_void_p(4100)), dict(row0=None),
               dict(nrow=0), dict(nrow=(1 << 20) + 1), dict(row1=C.c_void_p(4097)), dict(ptr=0), dict(ptr=4097), dict(mode=2),
               dict(mode=-1)):
        assert call(**kw) == EINVAL, kw
    # the host arrays themselves missing; and a call with nothing to add
    a, b = _scalars(2)
    assert L.ph_epoch_record_add(p, None, C.cast(b, C.c_void_p), 2, None, 0, None, None, 0, 0, None, None, 0, None) == EINVAL
    assert L.ph_epoch_record_add(p, C.cast(a, C.c_void_p), None, 2, None, 0, None, None, 0, 0, None, None, 0, None) == EINVAL
    assert L.ph_epoch_record_add(p, None, None, 0, None, 0, None, None, 0, 0, None, None, 0, None) == EINVAL
    assert null.value is None


def test_store_rows_refuses_bad_arguments():
    L = _lib()
    p = C.c_void_p(4096)

    def call(rows=p, index=p, B=4, D=3, store=p, n=10, softmax=0, skipped=p):
        return L.ph_store_rows(rows, index, B, D, store, n, softmax, skipped, None)

    for kw in (dict(rows=None), dict(index=None), dict(store=None), dict(skipped=None), dict(rows=C.c_void_p(4097)),
               dict(store=C.c_void_p(4098)), dict(index=C.c_void_p(4100)), dict(skipped=C.c_void_p(4100)), dict(B=0), dict(B=-1),
               dict(B=65537), dict(D=0), dict(D=4097), dict(n=0), dict(n=-5), dict(n=(1 << 31) + 1), dict(softmax=2),
               dict(softmax=-1)):
        assert call(**kw) == EINVAL, kw


def test_sim_audit_refuses_bad_arguments_and_sizes_its_workspace():
    L = _lib()
    p = C.c_void_p(4096)
    ws = L.ph_sim_audit_workspace_bytes
    # two float [n] vectors rounded up to 256 bytes + 8 words per workgroup (tiles of 64 rows x min(tiles, 16) ranges)
    assert ws(1, 1, 1) == 2 * 256 + 64 and ws(64, 3, 512) == 2 * 256 + 64 and ws(65, 3, 3) == 2 * 512 + 64 * 4
    assert ws(65536, 128, 128) == 2 * 4 * 65536 + 64 * 1024 * 16
    for n, Df, Dp in ((0, 3, 3), (-1, 3, 3), (65537, 3, 3), (10, 0, 3), (10, 3, 0), (10, 513, 3), (10, 3, 513), (1 << 30, 1, 1)):
        assert ws(n, Df, Dp) == 0, (n, Df, Dp)
        assert L.ph_sim_audit(p, p, p, n, Df, Dp, p, p, p, None) == EINVAL, (n, Df, Dp)
    for k in (0, 1, 6, 7, 8):                                   # labels (2) may be NULL: one class
        args = [p, p, p, 100, 128, 3, p, p, p, None]
        args[k] = None
        assert L.ph_sim_audit(*args) == EINVAL, k
    for k, bad in ((0, 4098), (1, 4097), (2, 4100), (6, 4100), (7, 4100), (8, 4096 + 128)):
        args = [p, p, p, 100, 128, 3, p, p, p, None]
        args[k] = C.c_void_p(bad)
        assert L.ph_sim_audit(*args) == EINVAL, (k, bad)


def test_python_wrappers_refuse_before_the_library():
    """The ValueError paths of epoch.sim_audit / the audit functions that need no device tensor."""
    import pytest
    import torch
    from multimodal_learning_amd import evaluate
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):                           # host tensors: no CPU fallback
        evaluate.feature_audit_device(x, x, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        evaluate.feature_audit_device(x, x, None)

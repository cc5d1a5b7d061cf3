"""Host side of ph_stage1_record_add (csrc/epochrec.hip) without a GPU: the symbol is bound with the
declared signature, the header declares what the binding uses, and every refused argument comes back as PH_EINVAL before any
HIP call - device pointers are never dereferenced on the host (the two host arrays are real ones)."""
import ctypes as C
import os
import re

EINVAL = -22
NAME = "ph_stage1_record_add"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_symbol_header_and_constants():
    import multimodal_learning_amd as m
    from multimodal_learning_amd import _lib as B
    from multimodal_learning_amd import epoch
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "pathomic_hip.h")).read()
    assert NAME in B.SIGNATURES and hasattr(L, NAME)
    fn = getattr(L, NAME)
    assert fn.restype is B.SIGNATURES[NAME][0] and list(fn.argtypes) == B.SIGNATURES[NAME][1]
    decl = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(B.SIGNATURES[NAME][1]) == 19
    assert int(re.search(r"#define PH_STAGE1REC_WORDS (\d+)", hdr).group(1)) == epoch.S1_WORDS
    assert len(epoch.Stage1Record.SCALARS) == len(epoch.Stage1Record.MODES) <= 16
    for name in ("train_teacher", "Stage1Record", "teacher_epoch_end_plan"):
        assert name in m.__all__ and hasattr(m, name)


def _scalars(n, ptr=4096, mode=0):
    return (C.c_void_p * max(n, 1))(*([ptr] * n)), (C.c_int32 * max(n, 1))(*([mode] * n))


def _call(L, rec=4096, ns=2, sp=0, md=0, heads=(4096, 4096, 4096), nh=3, grade=4096, B=8, Cc=3,
          surv=(4096, 4096, 4096, 4096, 4096, 4096), cap=64, ptr=4096, mode=1):
    a, b = _scalars(ns, ptr, mode)
    v = lambda x: C.c_void_p(x) if x else None      # noqa: E731
    return L.ph_stage1_record_add(v(rec), C.cast(a, C.c_void_p) if sp == 0 else v(sp), C.cast(b, C.c_void_p) if md == 0 else v(md),
                                  ns, v(heads[0]), v(heads[1]), v(heads[2]), nh, v(grade), B, Cc, v(surv[0]), v(surv[1]),
                                  v(surv[2]), v(surv[3]), v(surv[4]), v(surv[5]), cap, None)


def test_refuses_bad_arguments():
    L = _lib()
    p = 4096
    none6 = (None,) * 6
    bad = [dict(rec=None), dict(rec=4100), dict(ns=-1), dict(ns=17), dict(nh=-1), dict(nh=4), dict(ptr=0), dict(ptr=4097),
           dict(mode=2), dict(mode=-1), dict(sp=None), dict(md=None),
           # heads: exactly the first n_heads given, aligned, with a label vector
           dict(heads=(None, p, p)), dict(heads=(p, None, p)), dict(heads=(p, p, None)), dict(nh=2), dict(nh=1), dict(nh=0),
           dict(heads=(p, p, None), nh=2, grade=None), dict(heads=(4098, p, p)), dict(heads=(p, p, 4097)), dict(grade=None),
           dict(grade=4100), dict(heads=(None,) * 3, nh=0),          # (a label vector without a head)
           # every range edge
           dict(B=0), dict(B=-3), dict(B=65537), dict(Cc=0), dict(Cc=17), dict(cap=0), dict(cap=-1), dict(cap=(1 << 20) + 1),
           dict(heads=(None,) * 3, nh=0, grade=None, B=0), dict(heads=(None,) * 3, nh=0, grade=None, B=65537)]
    # survival pointers given only in part, or misaligned
    for k in range(6):
        part = [p] * 6
        part[k] = None
        bad.append(dict(surv=tuple(part)))
        only = [None] * 6
        only[k] = p
        bad.append(dict(surv=tuple(only)))
        mis = [p] * 6
        mis[k] = 4098
        bad.append(dict(surv=tuple(mis)))
    for kw in bad:
        assert _call(L, **kw) == EINVAL, kw
    # nothing to add
    assert _call(L, ns=0, heads=(None,) * 3, nh=0, grade=None, surv=none6) == EINVAL
    # the sizes that do not apply are not looked at: no heads -> C is free; no survival rows -> cap is free.  (These calls would
    # launch, so they are made only with an argument that is refused for another reason: the record pointer.)
    assert _call(L, rec=None, heads=(None,) * 3, nh=0, grade=None, Cc=0) == EINVAL


def test_python_wrappers_refuse_before_the_library():
    """The ValueError / RuntimeError paths of epoch.stage1_record_add and Stage1Record that need no device tensor.  (The
    inclusive edges B = 1 / 65536, C = 1 / 16, cap = 1 / 1048576, 16 scalars, 3 heads are accepted calls: they launch, and
    tests/test_gpu_epoch_stage1.py makes them on the device.)"""
    import pytest
    import torch
    from multimodal_learning_amd import epoch
    buf = torch.zeros(epoch.S1_WORDS, dtype=torch.int64)
    with pytest.raises(RuntimeError):                                 # host tensors: no CPU fallback
        epoch.stage1_record_add(buf, [torch.zeros(1)], [0])
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, [torch.zeros(1)] * 17, [0] * 17)
    with pytest.raises(ValueError):
        epoch.stage1_record_add(buf, cols=[torch.zeros(2)] * 5)       # columns without a store
    from types import SimpleNamespace
    with pytest.raises(NotImplementedError):
        epoch.Stage1Record(SimpleNamespace(sync=object(), surv=False, device="cpu"), 16)
    with pytest.raises(ValueError):
        epoch.Stage1Record(SimpleNamespace(sync=None, surv=True, device="cpu"), 0)
    with pytest.raises(ValueError):
        epoch.Stage1Record(SimpleNamespace(sync=None, surv=True, device="cpu"), (1 << 20) + 1)
    rec = epoch.Stage1Record(SimpleNamespace(sync=None, surv=True, device="cpu"), 8)
    rec.count_rows(1)
    with pytest.raises(ValueError, match="2 <= rows <= 8"):
        rec.cindex()

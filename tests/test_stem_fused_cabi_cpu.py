"""CPU-side checks of the fused stem backward's switch (ph_resnet_plan_set_stem_fused): declared in include/pathomic_hip.h, bound
in _lib.SIGNATURES with the same arity, exported, and a null plan is PH_EINVAL before anything else happens."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ph_resnet_plan_set_stem_fused"


def test_setter_is_declared_bound_and_exported():
    import multimodal_learning_amd as m
    from multimodal_learning_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pathomic_hip.h")).read()
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert decl, "not in the header"
    assert NAME in _lib.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 2
    assert hasattr(m.lib(), NAME)


def test_setter_rejects_a_null_plan_and_accepts_a_plan():
    import multimodal_learning_amd as m
    L = m.lib()
    for on in (0, 1):
        assert getattr(L, NAME)(None, on) == -22      # PH_EINVAL
    p = L.ph_resnet_plan_create(2, 64, 64, 0)
    assert p
    try:
        for on in (0, 1, 7):
            assert getattr(L, NAME)(p, on) == 0
    finally:
        L.ph_resnet_plan_destroy(p)

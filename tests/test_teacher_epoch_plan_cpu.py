"""train_step.teacher_epoch_end_plan over its window edges (MICCAI-2022/train_test_MT.py:269, :288, :295; the two MIA stage-1
trainers agree): epochs total - 16 .. total, 15 and 16, opt.measure on and off."""
from types import SimpleNamespace

import pytest

VARIANTS = ("miccai2022", "mia2022", "mia2023")


def _opt(niter, niter_decay, measure):
    return SimpleNamespace(niter=niter, niter_decay=niter_decay, measure=measure)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("niter,niter_decay", [(0, 40), (15, 15), (5, 11), (0, 3)])
def test_plan_over_the_window_edges(variant, niter, niter_decay):
    from multimodal_learning_amd import teacher_epoch_end_plan
    total = niter + niter_decay
    epochs = sorted(set(range(max(total - 16, 0), total + 1)) | {15, 16})
    for measure in (0, 1):
        opt = _opt(niter, niter_decay, measure)
        for epoch in epochs:
            plan = teacher_epoch_end_plan(opt, epoch, variant)
            # the reference's statements, literally
            measured = bool(opt.measure or epoch == (opt.niter + opt.niter_decay - 1))
            patches = measured and epoch > (opt.niter + opt.niter_decay - 15)
            save = measured and epoch > 15
            assert tuple(plan) == (measured, patches, save), (variant, total, measure, epoch, plan)
            assert plan._fields == ("measure", "use_patches", "may_save")


def test_plan_named_edges():
    from multimodal_learning_amd import teacher_epoch_end_plan as plan
    on, off = _opt(0, 40, 1), _opt(0, 40, 0)
    assert plan(on, 25, "mia2022") == (True, False, True) and plan(on, 26, "mia2022") == (True, True, True)     # total - 15 | - 14
    assert plan(on, 15, "mia2023") == (True, False, False) and plan(on, 16, "mia2023") == (True, False, True)
    assert plan(off, 38, "miccai2022") == (False, False, False) and plan(off, 40, "miccai2022") == (False, False, False)
    assert plan(off, 39, "miccai2022") == (True, True, True)          # the ONE measured epoch without opt.measure
    short = _opt(0, 3, 1)                                             # a run shorter than both windows: patches always, never saved
    assert [tuple(plan(short, e, "miccai2022")) for e in (1, 2, 3)] == [(True, True, False)] * 3
    with pytest.raises(ValueError):
        plan(on, 1, "stage2")

"""train_step.epoch_end_plan against a table written out from the three trainers' epoch ends:
  MICCAI-2022/train_test_path_multi_distill.py          measure :348, patches :360, average :368, checkpoint :387
  "MIA 2022/train_test_path_multi_distill_v2.py"         measure :527, patches :539, average :547, checkpoint :566
  "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py"   :478, :489, :497, :516
over a grid of (niter, niter_decay, epoch_count, measure).  The table below restates those lines one by one, epoch by epoch,
as the `if`s stand in the trainers; the function under test is a closed form."""
from types import SimpleNamespace

import pytest

VARIANTS = ("miccai2022", "mia2022", "mia2023")
GRID = [(niter, decay, first, measure) for niter in (0, 5) for decay in (2, 12, 30) for first in (0, 1) for measure in (0, 1)]


def _table(variant, niter, niter_decay, epoch_count, measure):
    """epoch -> (measure, use_patches, add_to_average, may_save), from the cited lines."""
    rows = {}
    for epoch in range(epoch_count, niter + niter_decay + 1):            # :228 | :373 | :286
        m = p = a = s = False
        if measure or epoch == (niter + niter_decay - 1):               # :348 | :527 | :478
            m = True
            if variant == "miccai2022":
                p = epoch > (niter + niter_decay - 10)                  # :360
            else:
                p = epoch > (niter + niter_decay - 20)                  # :539 | :489
            a = epoch > niter_decay - 3                                 # :368 | :547 | :497
            if variant == "miccai2022":
                s = epoch > niter_decay - 10                            # :387
            else:
                s = epoch > niter_decay - 20                            # :566 | :516
        rows[epoch] = (m, p, a, s)
    return rows


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("niter,niter_decay,epoch_count,measure", GRID)
def test_epoch_end_plan_matches_the_cited_lines(variant, niter, niter_decay, epoch_count, measure):
    from multimodal_learning_amd.train_step import EpochEndPlan, epoch_end_plan
    opt = SimpleNamespace(niter=niter, niter_decay=niter_decay, epoch_count=epoch_count, measure=measure)
    table = _table(variant, niter, niter_decay, epoch_count, measure)
    assert table, "the grid leaves no empty epoch range"
    for epoch, want in table.items():
        got = epoch_end_plan(opt, epoch, variant)
        assert isinstance(got, EpochEndPlan) and tuple(got) == want, (epoch, tuple(got), want)
        assert all(type(f) is bool for f in got)


def test_windows_differ_between_the_trainers_and_the_default_measures_one_epoch():
    from multimodal_learning_amd.train_step import EPOCH_AVERAGE_OVER, epoch_end_plan
    opt = SimpleNamespace(niter=0, niter_decay=30, epoch_count=1, measure=1)
    assert epoch_end_plan(opt, 15, "miccai2022").use_patches is False and epoch_end_plan(opt, 15, "mia2022").use_patches is True
    assert epoch_end_plan(opt, 15, "miccai2022").may_save is False and epoch_end_plan(opt, 15, "mia2023").may_save is True
    assert [e for e in range(1, 31) if epoch_end_plan(opt, e, "mia2023").add_to_average] == [28, 29, 30]
    assert EPOCH_AVERAGE_OVER == 3.0
    opt.measure = 0                     # without --measure the one measured epoch is the one BEFORE the loop's last (:228, :348)
    assert [e for e in range(1, 31) if epoch_end_plan(opt, e, "miccai2022").measure] == [29]
    # the checkpoint window hangs on niter_decay alone: with niter > 0 it opens earlier than the patch window
    opt = SimpleNamespace(niter=5, niter_decay=12, epoch_count=1, measure=1)
    assert epoch_end_plan(opt, 3, "miccai2022") == (True, False, False, True)


def test_unknown_variant_raises():
    from multimodal_learning_amd.train_step import epoch_end_plan
    with pytest.raises(ValueError):
        epoch_end_plan(SimpleNamespace(niter=0, niter_decay=3, measure=1), 1, "stage1")

"""train_step.distill_loss_plan: the one decision of DistillStep's generic loss path, over the whole option grid, without a
device.  The expectations are literal: read off the batch bodies of the three trainers as DistillStep ran them before the
plan existed (one inline tail and three `_*_tail` methods, each with its own copy of the condition)."""
import itertools
from types import SimpleNamespace

import pytest

VARIANTS = ("miccai2022", "mia2022", "mia2023")
BOTH, FUSE, EMA = ("fuse", "ema"), ("fuse",), ("ema",)
KD, KD_PATH = "criterion_kd", "criterion_kd_path"

# tests/test_gpu_step.py: BRANCH_NAMES / MIA_BRANCH_OPTS -> (num_teachers, which_teacher, distill, assign_weights)
BRANCH_OPTS = {"t1_fuse_crd": (1, "fuse", "crd", "False"), "t1_ema_crd": (1, "self_EMA", "crd", "False"),
               "t1_fuse_kd": (1, "fuse", "kd", "False"), "t1_ema_kd": (1, "self_EMA", "kd", "False"),
               "t2_kd_gk": (2, "fuse", "kd", "True"), "t2_kd_sum": (2, "fuse", "kd", "False"),
               "t2_crd_sum": (2, "fuse", "crd", "False"), "default": (2, "fuse", "crd", "True")}

# (variant, branch) -> (kl, feat, weighting, rank_draws, unused, crd_heads, report, kd_global)
EXPECT = {
    # the three default commands: two teachers, both CRD calls, GK-Refine; the MICCAI bank draws ranks once per CRD call
    ("miccai2022", "default"): (BOTH, "crd2", "gk", 2, (), True, "scaled", False),
    ("mia2022", "default"): (BOTH, "crd2", "gk", 0, (), True, "scaled", False),
    ("mia2023", "default"): (BOTH, "crd2", "gk", 0, (), True, "unscaled_rows", False),
    # the seven BRANCH_NAMES of the MICCAI-2022 body
    ("miccai2022", "t1_fuse_crd"): (FUSE, "crd1", "sum", 1, (KD_PATH,), True, "scaled", False),
    ("miccai2022", "t1_ema_crd"): (EMA, "crd1", "sum", 1, (KD_PATH,), True, "scaled", False),
    ("miccai2022", "t1_fuse_kd"): (FUSE, "none", "sum", 0, (KD, KD_PATH), True, "scaled", False),
    ("miccai2022", "t1_ema_kd"): (EMA, "none", "sum", 0, (KD, KD_PATH), True, "scaled", False),
    ("miccai2022", "t2_kd_gk"): (BOTH, "none", "gk", 0, (KD, KD_PATH), True, "scaled", False),
    ("miccai2022", "t2_kd_sum"): (BOTH, "none", "sum", 0, (KD, KD_PATH), True, "scaled", False),
    ("miccai2022", "t2_crd_sum"): (BOTH, "crd2", "sum", 2, (), True, "scaled", False),
    # the six MIA_BRANCHES
    ("mia2022", "t1_fuse_crd"): (FUSE, "crd1", "sum", 0, (KD_PATH,), True, "scaled", False),
    ("mia2022", "t1_ema_crd"): (EMA, "crd1", "sum", 0, (KD_PATH,), True, "scaled", False),
    ("mia2023", "t1_fuse_crd"): (FUSE, "crd1", "sum", 0, (KD_PATH,), True, "scaled", False),
    ("mia2023", "t1_ema_crd"): (EMA, "crd1", "sum", 0, (KD_PATH,), True, "scaled", False),
    ("mia2023", "t1_fuse_kd"): (FUSE, "none", "sum", 0, (KD, KD_PATH), True, "scaled", False),
    ("mia2023", "t2_kd_gk"): (BOTH, "none", "gk", 0, (KD, KD_PATH), True, "scaled", False),
    # the fixed-weight forms of the other two default bodies, and the MIA-2022 trainer's `--distill kd` (a baseline there)
    ("mia2022", "t2_crd_sum"): (BOTH, "crd2", "sum", 0, (), True, "scaled", False),
    ("mia2023", "t2_crd_sum"): (BOTH, "crd2", "sum", 0, (), True, "unscaled_rows", False),
    ("mia2022", "t2_kd_gk"): (BOTH, "none", "gk", 0, (), False, "baseline", False),
    ("mia2022", "t1_ema_kd"): (EMA, "none", "sum", 0, (), False, "baseline", False),
}


def _opt(nt=2, which="fuse", distill="crd", aw="True", **kw):
    return SimpleNamespace(num_teachers=nt, which_teacher=which, distill=distill, assign_weights=aw, batch_size=8, **kw)


def _plan(*a, **k):
    from multimodal_learning_amd.train_step import distill_loss_plan
    return distill_loss_plan(*a, **k)


@pytest.mark.parametrize("variant,name", list(EXPECT))
def test_named_configurations_map_to_the_expected_record(variant, name):
    from multimodal_learning_amd.train_step import LossPlan
    plan = _plan(_opt(*BRANCH_OPTS[name]), variant)
    assert isinstance(plan, LossPlan) and plan == LossPlan(*EXPECT[variant, name])


@pytest.mark.parametrize("distill", ["feats_KL", "rkd", "pkt", "similarity"])
def test_mia2022_baseline_criteria(distill):
    """One zoo criterion on the fused teacher's feature, fixed weights, no CRD heads in the optimiser, the baseline report."""
    from multimodal_learning_amd.train_step import LossPlan
    assert _plan(_opt(2, "fuse", distill, "False"), "mia2022") == LossPlan(BOTH, "zoo", "sum", 0, (), False, "baseline", False)
    assert _plan(_opt(1, "self_EMA", distill, "False"), "mia2022") == LossPlan(EMA, "zoo", "sum", 0, (), False, "baseline", False)
    assert _plan(_opt(1, "fuse", distill, "False"), "mia2022") == LossPlan(FUSE, "zoo", "sum", 0, (), False, "baseline", False)


def _parent_outcome(variant, nt, which, distill, aw):
    """None where the parent's DistillStep ran the combination, else the exception type it raised (at construction, or in
    its first step for the two checks that sat inside the tails)."""
    teachers_ok = nt == 2 or (nt == 1 and which in ("fuse", "self_EMA"))
    if variant == "mia2022" and distill != "crd":
        if distill not in ("kd", "feats_KL", "rkd", "pkt", "similarity"):
            return NotImplementedError                       # the zoo check of __init__
        if not teachers_ok:
            return NotImplementedError                       # the baseline tail's teacher selection
        if aw == "True" and not (distill == "kd" and nt == 2):
            return NotImplementedError                       # assign_weights with a baseline criterion
        return None
    if not teachers_ok:
        return UnboundLocalError                             # loss_div unbound (:263-271)
    if distill not in ("crd", "kd"):
        return NotImplementedError                           # :289-290
    if aw == "True" and nt != 2:
        return UnboundLocalError                             # KD_loss_list unbound (:293-304)
    return None


GRID = list(itertools.product(VARIANTS, (1, 2, 3), ("fuse", "self_EMA", "other"),
                              ("crd", "kd", "feats_KL", "rkd", "pkt", "similarity", "sp"), ("True", "False")))


def test_whole_option_grid_runs_or_raises_like_the_parent():
    ran = 0
    for variant, nt, which, distill, aw in GRID:
        opt, want = _opt(nt, which, distill, aw), _parent_outcome(variant, nt, which, distill, aw)
        if want is not None:
            with pytest.raises(want) as ei:
                _plan(opt, variant)
            assert type(ei.value) is want, (variant, nt, which, distill, aw)
            continue
        plan = _plan(opt, variant)
        ran += 1
        # the record's own consistency over the grid
        assert plan.kl == (BOTH if nt == 2 else FUSE if which == "fuse" else EMA)
        assert plan.weighting == ("gk" if aw == "True" else "sum")
        assert (plan.feat == "crd2") == (distill == "crd" and nt == 2) and (plan.feat == "crd1") == (distill == "crd" and nt == 1)
        assert plan.rank_draws == ({"crd2": 2, "crd1": 1}.get(plan.feat, 0) if variant == "miccai2022" else 0)
        assert plan.crd_heads == (plan.report != "baseline") and not plan.kd_global
        assert (plan.report == "unscaled_rows") == (variant == "mia2023" and plan.feat == "crd2")
    # 5 runnable teacher choices (two teachers x 3 names, one teacher x 2) with fixed weights, 3 with GK-Refine: 8 per variant
    # for crd and for kd; the four zoo criteria of mia2022 run with fixed weights only
    assert len(GRID) == 378 and ran == 3 * 8 + 3 * 8 + 4 * 5


def test_messages_of_the_reference_failures():
    with pytest.raises(UnboundLocalError, match="local variable 'KD_loss_list' referenced before assignment"):
        _plan(_opt(1, "fuse", "crd", "True"), "miccai2022")
    with pytest.raises(UnboundLocalError, match="local variable 'loss_div' referenced before assignment"):
        _plan(_opt(1, "nobody", "crd", "False"), "mia2023")
    with pytest.raises(NotImplementedError, match=r"--distill sp \(built: crd, kd, feats_KL, rkd, pkt, similarity\)"):
        _plan(_opt(2, "fuse", "sp", "False"), "mia2022")
    with pytest.raises(NotImplementedError, match="^sp$"):
        _plan(_opt(2, "fuse", "sp", "False"), "mia2023")
    with pytest.raises(NotImplementedError, match="assign_weights with --distill pkt"):
        _plan(_opt(2, "fuse", "pkt", "True"), "mia2022")
    with pytest.raises(NotImplementedError, match="num_teachers 3 / which_teacher 'fuse'"):
        _plan(_opt(3, "fuse", "kd", "False"), "mia2022")


def test_loss_weighting_other_than_gk_refine_fails_at_construction():
    """The MIA-2023 body with GK-Refine on: only `loss_weighting == GK_refine` is built (the parent raised in its first step)."""
    for name in ("default", "t2_kd_gk"):
        with pytest.raises(NotImplementedError, match="loss_weighting 'uniform'"):
            _plan(_opt(*BRANCH_OPTS[name], loss_weighting="uniform"), "mia2023")
        assert _plan(_opt(*BRANCH_OPTS[name], loss_weighting="GK_refine"), "mia2023").weighting == "gk"
    # fixed weights never read it; the other variants have no such option
    assert _plan(_opt(2, "fuse", "crd", "False", loss_weighting="uniform"), "mia2023").weighting == "sum"
    assert _plan(_opt(loss_weighting="uniform"), "miccai2022").weighting == "gk"


class _NoGather:
    world_size = 2

    def all_reduce_sum(self, t):
        return t


class _Sync(_NoGather):
    def all_gather_cat(self, t):
        return t


@pytest.mark.parametrize("distill", ["rkd", "pkt", "similarity"])
def test_global_batch_criteria_need_the_collectives(distill):
    with pytest.raises(NotImplementedError, match="must provide all_gather_cat"):
        _plan(_opt(2, "fuse", distill, "False"), "mia2022", sync=_NoGather())
    plan = _plan(_opt(2, "fuse", distill, "False"), "mia2022", sync=_Sync())
    # pkt / similarity hand every replica the global value (reported / world_size); rkd returns this replica's part
    assert plan.feat == "zoo" and plan.report == "baseline" and plan.kd_global == (distill != "rkd")


def test_rkd_needs_all_reduce_sum_and_bounds_the_global_batch():
    from multimodal_learning_amd.distiller_zoo import RKD_MAX_ROWS
    sync = SimpleNamespace(world_size=2, all_gather_cat=lambda t: t)
    with pytest.raises(NotImplementedError, match="must provide all_reduce_sum"):
        _plan(_opt(2, "fuse", "rkd", "False"), "mia2022", sync=sync)
    opt = _opt(2, "fuse", "rkd", "False")
    opt.batch_size = RKD_MAX_ROWS // 2 + 1
    with pytest.raises(ValueError, match="exceeds the %d rows" % RKD_MAX_ROWS):
        _plan(opt, "mia2022", sync=_Sync())
    opt.batch_size = RKD_MAX_ROWS // 2
    assert _plan(opt, "mia2022", sync=_Sync()).feat == "zoo"
    # feats_KL and kd are per-row: no collective needed, nothing global to report
    for distill in ("feats_KL", "kd"):
        assert not _plan(_opt(2, "fuse", distill, "False"), "mia2022", sync=_NoGather()).kd_global

"""Host-side survival metrics of the stage-1 evaluation (MICCAI-2022/utils.py:386-419): the log-rank p-value against an
independent implementation (scipy, test-only dependency) and the median-split accuracy.  No GPU."""
import numpy as np
import pytest


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_cox_log_rank_matches_scipy_logrank(seed):
    stats = pytest.importorskip("scipy.stats")
    from multimodal_learning_amd import utils as U
    rs = np.random.RandomState(seed)
    N = 150 + 40 * seed
    hazards = rs.randn(N)
    t = rs.randint(1, 40, N).astype(np.float64)             # ties in time
    t[hazards > 0.3] = np.maximum(1, t[hazards > 0.3] - 8)   # a real group effect on some draws
    e = (rs.rand(N) > 0.35).astype(np.float64)
    got = U.cox_log_rank(hazards, e, t)
    g = hazards > np.median(hazards)
    x = stats.CensoredData(uncensored=t[~g & (e > 0)], right=t[~g & (e == 0)])
    y = stats.CensoredData(uncensored=t[g & (e > 0)], right=t[g & (e == 0)])
    want = stats.logrank(x, y, alternative="two-sided").pvalue
    assert abs(got - want) <= 1e-10, (got, want)


def test_cox_log_rank_zero_variance_is_nan():
    """Every event at the last time: no event time with both groups at risk and a spread of outcomes - undefined, nan."""
    from multimodal_learning_amd import utils as U
    h = np.array([0.1, 0.2, 0.3, 0.4])
    t = np.array([1.0, 2.0, 3.0, 4.0])
    e = np.array([0.0, 0.0, 0.0, 1.0])
    assert np.isnan(U.cox_log_rank(h, e, t))


def test_accuracy_cox_vs_reference_golden(golden_dir):
    """The reference's own test() computed surv_acc_test from these risks and events (make_golden_eval_stage1.py)."""
    import os
    from multimodal_learning_amd import utils as U
    g = np.load(os.path.join(golden_dir, "eval_stage1_b6_h64.npz"))
    assert U.accuracy_cox(g["surv_risk_pred_all"], g["surv_censor_all"]) == float(g["surv_surv_acc_test"])


def test_accuracy_cox_median_split():
    from multimodal_learning_amd import utils as U
    h = np.array([0.1, 0.9, 0.5, 0.7, 0.3])       # median 0.5: > median -> group 1
    labels = np.array([0, 1, 1, 1, 0], dtype=np.float64)
    assert U.accuracy_cox(h, labels) == 0.8


def test_cindex_from_counts_rule():
    from multimodal_learning_amd import utils as U
    assert U.cindex_from_counts((5, 4, 1)) == 0.9
    with pytest.raises(ZeroDivisionError):
        U.cindex_from_counts((0, 0, 0))


def test_surv_option_pairings_on_the_host():
    """The task / head pairing check needs no GPU: surv is accepted by the stage-1 teacher only with Sigmoid and label_dim 1."""
    import multimodal_learning_amd as m
    from multimodal_learning_amd.train_step import _validate_task
    _validate_task(m.stage2_opt(task="surv", act_type="Sigmoid", label_dim=1), "T", surv_ok=True)
    for bad in (dict(task="surv"), dict(task="surv", act_type="Sigmoid"), dict(act_type="Sigmoid", label_dim=1)):
        with pytest.raises(NotImplementedError):
            _validate_task(m.stage2_opt(**bad), "T", surv_ok=True)
    with pytest.raises(NotImplementedError):
        _validate_task(m.stage2_opt(task="surv", act_type="Sigmoid", label_dim=1), "D")

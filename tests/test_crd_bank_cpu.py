"""The CRD bank base class and the per-call plan without a GPU: what the four criteria's memory modules
hold after construction - bit for bit a restatement of the constructors' RNG order -, what a checkpoint load does to the
first-call state, what CrdCall refuses, and that building a plan leaves the module as it was."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

N, K, P, S = 48, 12, 6, 24
CLASS_IDX = [np.arange(0, 20), np.arange(20, 48)]
CRITERIA = [("CRD_loss", "neighbors"), ("CRD_criterion_v3", "neighbors"), ("CRD_criterion", "neighbors"),
            ("CRD_criterion_v10", "neighbors"), ("CRD_criterion_v10", "centers")]


def _opt(D, pos_extra):
    return SimpleNamespace(s_dim=S, t_dim=S + 8, feat_dim=D, nce_p=P if pos_extra == "neighbors" else 2, nce_k=K, nce_p2=2, nce_k2=5,
                           nce_t=0.07, nce_m=0.5, n_data=N, select_pos_pairs=True, select_neg_pairs="True", sample_KD="False",
                           select_pos_mode="hard", pos_extra=pos_extra)


def _build(which, opt):
    from multimodal_learning_amd.CL_utils import CRD_criterion, CRD_criterion_v3, CRD_criterion_v10, CRD_loss
    if which == "CRD_loss":
        return CRD_loss.CRDLoss(opt, opt.n_data)
    if which == "CRD_criterion":
        return CRD_criterion.CRDLoss(opt)
    if which == "CRD_criterion_v3":
        return CRD_criterion_v3.CRDLoss(opt, opt.n_data)
    return CRD_criterion_v10.CRDLoss(opt, opt.n_data, CLASS_IDX)


def _embed(which, dim_in, D):
    """The criterion's projection head as torch builds it (the draws of its Linear layers, in order)."""
    if which == "CRD_criterion":
        return torch.nn.Sequential(torch.nn.Linear(dim_in, D), torch.nn.ReLU(), torch.nn.Linear(D, D))
    return torch.nn.Linear(dim_in, D)


@pytest.mark.parametrize("which,pos_extra", CRITERIA)
@pytest.mark.parametrize("D", [64, 128])
def test_constructed_banks_are_the_restated_draws(which, pos_extra, D):
    opt = _opt(D, pos_extra)
    torch.manual_seed(1234 + D)
    crd = _build(which, opt)
    # the restatement: the two Embed heads, then torch.rand(n, D) twice, each scaled into +-1 / sqrt(D / 3)
    torch.manual_seed(1234 + D)
    heads = [_embed(which, opt.s_dim, D), _embed(which, opt.t_dim, D)]
    stdv = 1.0 / math.sqrt(D / 3)
    banks = [torch.rand(N, D).mul_(2 * stdv).add_(-stdv) for _ in range(2)]
    sd = crd.state_dict()
    head_keys = (["linear.0.weight", "linear.0.bias", "linear.2.weight", "linear.2.bias"] if which == "CRD_criterion" else
                 ["linear.weight", "linear.bias"])
    expect = {"embed_%s.%s" % (h, k): None for h in "st" for k in head_keys}
    n_params = 6 if which == "CRD_loss" else 5
    expect.update({"contrast.params": (n_params,), "contrast.memory_v1": (N, D), "contrast.memory_v2": (N, D)})
    assert list(sd) == list(expect)                               # (all_sample_labels of v10 is not persistent)
    for k, shape in expect.items():
        assert shape is None or tuple(sd[k].shape) == shape, k
    for h, head in zip("st", heads):
        ref = head.state_dict()
        for k in head_keys:
            assert torch.equal(sd["embed_%s.%s" % (h, k)], ref[k.replace("linear.", "", 1)]), (h, k)
    want = [K, 0.07, -1, -1, 0.5] + ([opt.nce_p] if which == "CRD_loss" else [])
    assert torch.equal(sd["contrast.params"], torch.tensor(want, dtype=torch.float32))
    assert torch.equal(sd["contrast.memory_v1"], banks[0]) and torch.equal(sd["contrast.memory_v2"], banks[1])
    mem = crd.contrast
    assert mem._z_set is False and mem._draw_step is None and mem._draw_seed is None and mem.sample_KD is False
    assert mem.sync is None and mem.batch_norm_size is None and mem.last is None and mem.nLem == N and mem.K == K
    if which == "CRD_criterion_v10":
        assert "all_sample_labels" in dict(mem.named_buffers()) and mem.all_sample_labels.dtype == torch.int32
        assert mem.all_sample_labels.tolist() == [0] * 20 + [1] * 28


@pytest.mark.parametrize("which,pos_extra", CRITERIA)
def test_loading_a_state_with_positive_z_ends_the_first_call_state(which, pos_extra):
    opt = _opt(128, pos_extra)
    a, b = _build(which, opt), _build(which, opt)
    assert not b.contrast._z_set
    a.contrast.params[2:4] = torch.tensor([310.5, 295.25])
    b.load_state_dict(a.state_dict())
    assert b.contrast._z_set and torch.equal(b.contrast.params, a.contrast.params)
    a.contrast.params[3] = -1.0                                   # one constant still unset: the first call is still to come
    b.load_state_dict(a.state_dict())
    assert not b.contrast._z_set


def test_sample_kd_is_the_banks_own_flag():
    opt = _opt(128, "neighbors")
    opt.sample_KD = "True"
    assert _build("CRD_loss", opt).contrast.sample_KD is True


def test_a_plan_with_inconsistent_widths_is_refused_by_field_name():
    from multimodal_learning_amd.CL_utils.memory_new import CrdCall
    B = 3
    idx = torch.zeros(B, P + K, dtype=torch.int64)
    call = CrdCall(P, K, 2, 5, idx, select_pos=True, select_neg=True, ranks=None, per_sample=True)
    assert (call.P, call.K, call.P2, call.K2, call.select_pos, call.select_neg, call.per_sample) == (P, K, 2, 5, True, True, True)
    assert call.idx is idx and call.idx_bank2 is None and call.posw_s is None and call.posw_t is None and call.scan is None
    with pytest.raises(ValueError, match=r"CrdCall\.idx .*\[B, %d\]" % (P + K)):
        CrdCall(P, K, 2, 5, idx[:, :-1])
    with pytest.raises(ValueError, match=r"CrdCall\.idx "):
        CrdCall(P, K, 2, 5, idx.int())
    with pytest.raises(ValueError, match=r"CrdCall\.idx_bank2"):
        CrdCall(P, K, P, K, idx, idx_bank2=idx[:, 1:])
    w = torch.full((B, P), 1.0 / P)
    CrdCall(P, K, P, K, idx, idx_bank2=idx.clone(), posw_s=w, posw_t=w)
    with pytest.raises(ValueError, match=r"CrdCall\.posw_s"):
        CrdCall(P, K, P, K, idx, posw_s=w[:, :-1], posw_t=w)
    with pytest.raises(ValueError, match=r"CrdCall\.posw_t"):
        CrdCall(P, K, P, K, idx, posw_s=w, posw_t=torch.ones(B, P + K))
    # the bank-scan form: idx holds the P positives alone, the negatives are columns col0 .. col0 + K of scan["idx"]
    neg = torch.zeros(B, K + 1, dtype=torch.int64)
    scan = dict(idx=neg, col0=1, K=K)
    assert CrdCall(P, K, P, K, idx[:, :P], scan=scan).scan is scan
    with pytest.raises(ValueError, match=r"CrdCall\.idx .*\[B, %d\]" % P):
        CrdCall(P, K, P, K, idx, scan=scan)
    with pytest.raises(ValueError, match=r"CrdCall\.scan"):
        CrdCall(P, K, P, K, idx[:, :P], scan=dict(idx=neg[:, :-1], col0=1, K=K))
    with pytest.raises(ValueError, match=r"CrdCall\.scan"):
        CrdCall(P, K + 1, P, K + 1, idx[:, :P], scan=scan)
    with pytest.raises(NotImplementedError, match="ranked pair selection"):
        CrdCall(P, K, P, K, idx[:, :P], scan=scan, select_neg=True)
    with pytest.raises(AttributeError):
        call.stale = 1                                            # named fields only


@pytest.mark.parametrize("which,pos_extra", CRITERIA)
def test_building_a_plan_leaves_the_memory_module_as_it_was(which, pos_extra):
    from multimodal_learning_amd.CL_utils.memory_new import CrdCall
    opt = _opt(128, pos_extra)
    mem = _build(which, opt).contrast
    before = (set(vars(mem)), set(mem._buffers), {k: v for k, v in vars(mem).items() if not k.startswith("_") and k != "training"})
    B = 4
    if which == "CRD_criterion_v10":
        assert mem.P is None and mem.P2 is None and mem.K2 is None          # the widths are per call
        NP = opt.nce_p
        call = CrdCall(NP, K, NP, K, torch.zeros(B, NP + K, dtype=torch.int64), idx_bank2=torch.zeros(B, NP + K, dtype=torch.int64),
                       posw_s=torch.ones(B, NP), posw_t=torch.ones(B, NP), per_sample=True)
    else:
        Pm = opt.nce_p if which == "CRD_loss" else 1
        call = mem.plan(torch.zeros(B, Pm + K, dtype=torch.int64), ranks=None, per_sample=True)
        want = (Pm, K, 2, 5, True, True) if which == "CRD_loss" else (1, K, 1, K, False, False)
        assert (call.P, call.K, call.P2, call.K2, call.select_pos, call.select_neg) == want
        with pytest.raises(ValueError, match=r"CrdCall\.idx "):
            mem.plan(torch.zeros(B, Pm + K + 1, dtype=torch.int64))
    assert call.per_sample
    after = (set(vars(mem)), set(mem._buffers), {k: v for k, v in vars(mem).items() if not k.startswith("_") and k != "training"})
    assert before[0] == after[0] and before[1] == after[1]
    assert all(after[2][k] is before[2][k] or after[2][k] == before[2][k] for k in before[2])

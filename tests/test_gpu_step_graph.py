"""The graph input sets of the two training steps (step_graph.StepGraphs) on the device: a third resident input set and host
tensors are staged into a private set and never into the caller's adopted tensors, on DistillStep and TeacherStage1Step alike,
and a capture that fails leaves the owner launching eagerly."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _to_cuda(batch):
    return tuple(tuple(u.cuda() for u in t) if isinstance(t, tuple) else t.cuda() for t in batch)


def _tensors(batch):
    return [u for t in batch for u in (t if isinstance(t, tuple) else (t,))]


def _run_three_sets(step, host, resident, n_eager=2, n_graph=9, **kw):
    """`n_eager` eager steps, then `n_graph` graph steps that feed the input sets 0, 1, 2, 0, ... - the resident ones if
    `resident`, whose other two sets must come out of every step bit for bit as they went in."""
    step.enable_graph()
    feeds = [_to_cuda(b) for b in host] if resident else host
    for i in range(n_eager + n_graph):
        kwi = {k: v[i] for k, v in kw.items()}
        fed = (i - n_eager) % 3
        if resident and i >= n_eager:
            others = [t for j in range(3) if j != fed for t in _tensors(feeds[j])]
            before = [t.clone() for t in others]
        out = step.step(feeds[fed], epoch=1, **kwi)
        torch.cuda.synchronize()
        if resident and i >= n_eager:
            for j, (t, b) in enumerate(zip(others, before)):
                assert torch.equal(t, b), "step %d overwrote tensor %d of an input set it was not fed" % (i, j)
    return out, feeds


def test_distill_step_stages_a_third_resident_set_into_a_private_set():
    """Three resident input sets fed in turn for nine graph steps: two are adopted, the third is staged into a private set, no
    step touches the tensors of a set it was not fed, and the trajectory is bit-identical to feeding the same batches from
    the host.  (Before the shared input-set manager DistillStep copied the third set over the caller's first adopted
    tensors: this test failed on the overwrite and on the diverged trajectory.)"""
    import multimodal_learning_amd as m
    from oracle.step import default_opt, synthetic_batch
    from tests.test_gpu_step import _mk_step, _tuple
    m.set_precision("bf16")
    opt = default_opt()
    host = [_tuple(synthetic_batch(8, 64, seed=70 + i)) for i in range(3)]
    rng = np.random.RandomState(5)
    ranks = [[rng.choice(np.arange(30, 100), 20, replace=False) for _ in range(2)] for _ in range(11)]

    def run(resident):
        step = _mk_step(opt, 1024, seed=0)
        out, feeds = _run_three_sets(step, host, resident, ranks=ranks)
        sets = list(step._slots)
        if resident:
            assert sorted(q["adopted"] for q in sets) == [False, True, True] and all(len(q["graphs"]) == 1 for q in sets)
            for q, fed in zip([q for q in sets if q["adopted"]], feeds):
                assert q["x_path"].data_ptr() == fed[0][0].data_ptr(), "inputs were staged, not adopted"
            private = next(q for q in sets if not q["adopted"])
            assert not {t.data_ptr() for t in _tensors(feeds[0]) + _tensors(feeds[1]) + _tensors(feeds[2])} & set(private["ptrs"])
        else:
            assert [q["adopted"] for q in sets] == [False] and len(sets[0]["graphs"]) == 1
        return out["loss"].item(), step.model.state_dict()["fc_new2.weight"].clone(), \
            step.ema_model.state_dict()["conv1.weight"].clone(), step.criterion_kd.contrast.memory_v1.clone()

    b, a = run(True), run(False)
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


def test_stage1_step_stages_a_third_resident_set_into_a_private_set():
    """The same rule on TeacherStage1Step (grading task, no t-SVD, CRD off): two adopted sets and one private set with one
    graph each, untouched caller tensors, the host-fed trajectory bit for bit."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    from oracle.step import synthetic_batch
    from tests.test_gpu_step import _tuple
    m.set_precision("bf16")
    opt = m.stage2_opt(dropout_rate=0.0, batch_size=8, cut_fuse_grad=False, num_teachers=2)
    opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss, opt.tSVD_loss = 1, 1.0, 0, 0, "False", "False"
    host = [_tuple(synthetic_batch(8, 64, seed=80 + i)) for i in range(3)]

    def run(resident):
        model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
        model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3)); ema.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 4))
        st = m.TeacherStage1Step(copy.copy(opt), device="cuda", models=(model.cuda(), ema.cuda()))
        out, feeds = _run_three_sets(st, host, resident)
        sets = list(st._g_sets)
        assert st._want_graph and all(len(q["graphs"]) == 1 for q in sets)
        assert sorted(q["adopted"] for q in sets) == ([False, True, True] if resident else [False])
        return out["loss"].item(), [p.detach().clone() for p in st.model.parameters()], \
            [p.detach().clone() for p in st.ema_model.parameters()]

    a, b = run(False), run(True)
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(x, y)


def test_a_failed_capture_drops_the_sets_and_leaves_the_owner_eager():
    """The fallback of StepGraphs.graph, reached with a body that raises a Python exception before it launches anything: the
    warning names the step, the owner stops asking for graphs, every set is gone, the optimiser's flag is as it was and the
    device still takes eager work."""
    from types import SimpleNamespace
    from multimodal_learning_amd.step_graph import StepGraphs
    owner = SimpleNamespace(sync=None, optimizer=SimpleNamespace(_prepared=False), _want_graph=True)
    graphs = StepGraphs(torch.device("cuda"), "probe", ("x",), ())
    st = graphs.input_set(dict(x=torch.zeros(4, device="cuda")))
    assert len(graphs) == 1 and st["adopted"]

    def body():
        raise RuntimeError("raised before any launch")

    with pytest.warns(UserWarning, match="HIP graph capture of the probe step failed"):
        assert graphs.graph(owner, st, "step", body) is None
    assert owner._want_graph is False and len(graphs) == 0 and owner.optimizer._prepared is False
    assert torch.ones(1).cuda().item() == 1.0

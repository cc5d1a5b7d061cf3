"""The input-set policy of the captured training steps (step_graph.select_set) on made-up pointer and shape tuples: which set
serves a batch, when a set is adopted, and that an adopted set - the caller's own tensors - is never a copy target."""
import copy

SH = ((8, 3, 64, 64), (8, 80), (8,))
A, B, C, D = (0x1000, 0x2000, 0x3000), (0x4000, 0x5000, 0x6000), (0x7000, 0x8000, 0x9000), (0xa000, 0xb000, 0xc000)


def _select(sets, ptrs, shapes=SH, stage=True):
    """One call with a resident pointer tuple, or host tensors (`ptrs` None).  A new private set gets buffers of its own, as
    StepGraphs.input_set gives it."""
    from multimodal_learning_amd.step_graph import select_set
    st, new, copy_in = select_set(sets, ptrs is not None, ptrs, shapes, stage)
    if new and not st["adopted"]:
        assert st["ptrs"] is None
        st["ptrs"] = (0xf000, 0xf100, 0xf200)
    return st, new, copy_in


def test_first_call_with_host_tensors_makes_one_private_set_and_copies():
    sets = []
    st, new, copy_in = _select(sets, None)
    assert sets == [st] and new and copy_in and not st["adopted"] and st["shapes"] == SH and st["graphs"] == {}
    assert _select(sets, None) == (st, False, True) and len(sets) == 1


def test_first_call_with_resident_tensors_is_adopted_without_a_copy():
    sets = []
    st, new, copy_in = _select(sets, A)
    assert sets == [st] and new and not copy_in and st["adopted"] and st["ptrs"] == A


def test_two_resident_sets_are_adopted_and_further_inputs_share_one_private_set():
    sets = []
    a, b = _select(sets, A)[0], _select(sets, B)[0]
    assert b is not a and b["adopted"] and b["ptrs"] == B and len(sets) == 2
    before = copy.deepcopy([a, b])
    # a third resident tuple: the private set, created once, copy needed; the adopted records stay as they were
    p, new, copy_in = _select(sets, C)
    assert new and copy_in and not p["adopted"] and p is not a and p is not b and len(sets) == 3
    assert _select(sets, D) == (p, False, True)
    assert _select(sets, C) == (p, False, True)
    # host tensors after two adopted sets: the same private set
    assert _select(sets, None) == (p, False, True)
    assert [a, b] == before and sets == [a, b, p]
    # a repeated pointer tuple: its own adopted set, no copy
    assert _select(sets, A) == (a, False, False) and _select(sets, B) == (b, False, False)
    assert sum(q["adopted"] for q in sets) == 2 and [q for q in sets if not q["adopted"]] == [p]


def test_a_private_set_is_never_an_adopted_record():
    sets = []
    seen = []
    for ptrs in (None, A, None, B, C, A, None, D, B):
        st, _, copy_in = _select(sets, ptrs)
        seen.append((st, copy_in))
    adopted = [q for q in sets if q["adopted"]]
    assert [q["ptrs"] for q in adopted] == [A, B] and len(sets) == 3
    for st, copy_in in seen:
        assert copy_in == (not st["adopted"]), "inputs are copied into the private set and into nothing else"
        assert not (copy_in and any(st is q for q in adopted))


def test_the_private_sets_own_buffers_are_served_by_it_without_a_copy():
    """DistillStep.static_inputs() hands the private buffers out to be filled in place."""
    sets = []
    p = _select(sets, None)[0]
    assert _select(sets, p["ptrs"]) == (p, False, False) and len(sets) == 1


def test_a_shape_change_drops_every_set():
    sets = []
    for ptrs in (A, B, None):
        _select(sets, ptrs)
    assert len(sets) == 3
    other = ((4, 3, 64, 64),) + SH[1:]
    st, new, copy_in = _select(sets, A, shapes=other)
    assert sets == [st] and new and st["adopted"] and st["shapes"] == other and not copy_in


def test_without_staging_only_a_set_of_its_own_serves_a_resident_tuple():
    """DistillStep.precapture: no graph is captured for inputs that would have to be copied."""
    sets = []
    assert _select(sets, None, stage=False) == (None, False, False) and sets == []
    a = _select(sets, A, stage=False)[0]
    b = _select(sets, B, stage=False)[0]
    assert a["adopted"] and b["adopted"]
    assert _select(sets, C, stage=False) == (None, False, False) and len(sets) == 2
    assert _select(sets, A, stage=False) == (a, False, False)


def test_the_manager_does_not_keep_its_step_alive():
    """A step owns its StepGraphs; with a reference back the pair would be a cycle, and the captured graphs would be destroyed
    whenever the garbage collector runs - possibly inside a later capture - instead of with the step."""
    import gc
    import weakref
    from multimodal_learning_amd.step_graph import StepGraphs

    class Step:
        pass

    gc.disable()
    try:
        step = Step()
        step.graphs = StepGraphs("cpu", "probe", ("x",), ())
        _select(step.graphs.sets, A)
        graphs, gone = weakref.ref(step.graphs), weakref.ref(step)
        del step
        assert gone() is None and graphs() is None
    finally:
        gc.enable()

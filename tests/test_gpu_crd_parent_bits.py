"""Every CRD entry point, bit for bit what the commit before the bank refactor computed on the MI355X.

tests/golden/crd_parent_bits.npz was written there by tests/golden/make_crd_parent_bits.py on that commit - twice, and the
two files agreed in every array, so every recorded quantity is compared with exact equality.  The runs, their shapes and what
is recorded are that file's `RUNS` / `Run` / `record_step`: two calls per criterion object (first-call Z, momentum update),
the loss, the per-sample losses, d f_s, d W_embed_s, d W_embed_t, `params`, the updated rows of both banks; one eager
DistillStep iteration per fused loss head."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden_dir):
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import make_crd_parent_bits
    return make_crd_parent_bits


@pytest.fixture(scope="module")
def bits(golden_dir):
    return np.load(os.path.join(golden_dir, "crd_parent_bits.npz"))


def _same(bits, got, prefix=""):
    assert got, prefix
    bad = [k for k, v in got.items()
           if v.dtype != bits[prefix + k].dtype or v.shape != bits[prefix + k].shape
           or not np.array_equal(v.view(np.int32), bits[prefix + k].view(np.int32))]
    assert not bad, bad


def test_the_golden_file_holds_exactly_the_recorded_runs(G, bits):
    tags = {k.split(".")[0] for k in bits.files}
    assert tags == set(G.RUNS) | {"step_" + v for v in G.STEP_VARIANTS}
    assert all(np.isfinite(bits[k]).all() for k in bits.files)


@pytest.mark.parametrize("tag", ["c1_dcd_hard", "c2_dcd_ranks_kd", "c3_mem3_forward", "c4_dcd_long", "c5_v3_draw", "c5_mt_draw",
                                 "c6_v10_knn_d128", "c6_v10_knn_d256", "c7_v10_scan_n70", "c7_v10_scan_n1030", "c8_v10_means",
                                 "c8_v10_kmeans"])
def test_criterion_calls_are_bitwise_what_the_parent_commit_gives(G, bits, tag):
    assert tag in G.RUNS
    run = G.Run(**G.RUNS[tag])
    for it in range(2):
        _same(bits, run.call(), "%s.%d." % (tag, it))
        call = run.mem.last["call"]
        kw = G.RUNS[tag]
        assert (call.scan is not None) == (kw.get("scan") == "1")
        assert call.per_sample == (kw["kind"] != "mem3" and not (kw["kind"] == "dcd" and kw.get("sample_KD", "False") == "False"))


@pytest.mark.parametrize("first,second", [("c6_v10_knn_d128", "c8_v10_means"), ("c8_v10_kmeans", "c6_v10_knn_d128"),
                                          ("c8_v10_means", "c7_v10_scan_n70")])
def test_interleaved_criteria_of_other_forms_keep_their_stand_alone_bits(G, bits, first, second):
    """Two criterion objects of different forms called in turn - KNN positives with weights and a second column list, then
    centre columns without either, and the other way round; the bank-scan form after the gathered one: each call must give
    what its run gives alone (nothing of one call's plan may reach the next)."""
    a, b = G.Run(**G.RUNS[first]), G.Run(**G.RUNS[second])
    for it in range(2):
        _same(bits, a.call(), "%s.%d." % (first, it))
        _same(bits, b.call(), "%s.%d." % (second, it))
        assert a.mem.last["call"] is not b.mem.last["call"]
        assert (b.mem.last["call"].idx_bank2 is None) == second.startswith("c8")


@pytest.mark.parametrize("variant", ["miccai2022", "mia2022", "mia2023"])
def test_fused_head_steps_are_bitwise_what_the_parent_commit_gives(G, bits, variant):
    assert variant in G.STEP_VARIANTS
    _same(bits, G.record_step(variant))

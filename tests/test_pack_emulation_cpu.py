"""The restatement of the packed weight buffer (tests/pack_emulation.py) against the properties its documentation states, and
its named defects against the cases of tests/test_gpu_pack.py: each must change the bytes that test compares."""
import numpy as np
import pytest

from tests import pack_emulation as P


def test_fragment_order_is_a_bijection_with_the_documented_coordinates():
    r, k = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    idx = P.frag_index(r, k)
    assert sorted(idx.ravel().tolist()) == list(range(4096))
    # [k-step 2][N tile 4][lane 64][8]: row r = 4 li + n, k = 32 ks + 8 lg + j, lane = 16 lg + li
    for ks in range(2):
        for n in range(4):
            for lane in range(64):
                lg, li = lane >> 4, lane & 15
                for j in range(8):
                    assert idx[4 * li + n, 32 * ks + 8 * lg + j] == ((ks * 4 + n) * 64 + lane) * 8 + j


def test_split_planes_sum_to_the_weight_exactly():
    w = P.random_weights([(64, 64, 3, 3)], 1)[0]
    w.ravel()[:4] = [0.0, 1.0, -31.9, 2.0 ** -20]
    p0, p1, p2 = (P.bf16_val(p) for p in P.split3(w))
    assert np.array_equal((p0 + p1) + p2, w)
    assert np.array_equal(P.bf16_val(P.bf16_bits(w)), p0)
    # round to nearest even: a tie goes to the even mantissa
    assert P.bf16_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)).tolist() == [0x3F80, 0x3F82]


def test_half_pair_blocks_give_the_weight_back():
    w = P.random_weights([(64, 64, 3, 3)], 2)[0]
    hi2k, lo, hi = (b.view(np.float16).astype(np.float64) for b in P.hp_blocks(w))
    assert np.array_equal(hi2k, hi * 2048.0)
    err = np.abs(hi + lo / 2048.0 - w.astype(np.float64))
    assert (err <= 2.0 ** -22 * np.abs(w)).all()


def test_written_mask_and_sizes():
    w = P.random_weights([(128, 64, 3, 3)], 3)[0]
    n = w.size
    for arith, layout, written in (("bf16", "row", n), ("bf16", "copy", 2 * n), ("bf16x6", "row", 3 * n), ("fp16x3", "row", 3 * n),
                                   ("fp16x3", "tap6", 3 * n)):
        words, wr = P.pack_conv(w, arith, False, layout)
        assert words.size == P.NPLANES * n and int(wr.sum()) == written, (arith, layout)
        assert not words[~wr].any()
    assert not P.pack_conv(w, "bf16", False, "copy")[1][2 * n:].any()      # plane 2 is never written
    sw, swr = P.pack_stem(P.random_weights([(64, 3, 7, 7)], 4)[0], "bf16")
    assert sw.size == P.NPLANES * P.STEM_PLANE and swr.all()
    assert not sw.reshape(3, 7, 64, 8, 4)[..., 7, :].any() and not sw.reshape(3, 7, 64, 8, 4)[..., 3].any()      # the zero padding


def test_layout_rules():
    units = P.resnet_units((1, 1, 1, 1))
    assert len(units) == 11 and len(P.resnet_units((8, 1, 1, 1))) == 25
    bf = P.plan_layouts(units, "bf16")
    assert bf[0] == ("row", "row") and bf[2] == ("copy", "row") and bf[3] == ("copy", "copy") and bf[4] == ("row", "row")
    hp = P.plan_layouts(units, "fp16x3")
    assert hp[0] == ("tap5", "tap5") and hp[2] == ("tap6", "row") and hp[3] == ("row", "row")
    assert set(P.plan_layouts(units, "fp16x3", tap5=False, tap6=False)) == {("row", "row")}
    assert not P.copy_shape(128, 192, 3, True) and not P.copy_shape(640, 640, 3, True) and not P.copy_shape(128, 64, 1, True)


def _network_bytes(layers, arith, defect=None):
    units = P.resnet_units(layers)
    ws = P.random_weights([(64, 3, 7, 7)] + [(O, I, KS, KS) for (O, I, KS, S) in units], 11)
    return P.pack_network(ws[0], units, ws[1:], arith, P.plan_layouts(units, arith), defect)[0]


def _conv_bytes(defect=None):
    out = []
    for name, Cin, Cout, KS, S, pad, ariths in P.CONVS:
        w = P.random_weights([(Cout, Cin, KS, KS)], 5)[0]
        for arith in ariths:
            for dgrad in (False, True):
                lay = P.plan_layouts([(Cout, Cin, KS, S)], arith)[0][dgrad]
                if arith == "bf16" and defect == "stray_copy" and KS == 3:
                    lay = "copy"
                words, wr = P.pack_conv(w, arith, dgrad, lay, defect)
                out.append(np.where(wr, words, 0x5A5A))
    return out


@pytest.fixture(scope="module")
def sound():
    return {"nets": {(l, a): _network_bytes(l, a) for l, a in P.NETWORKS[:3]}, "convs": _conv_bytes()}


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_each_defect_changes_the_bytes_of_the_gpu_cases(sound, defect):
    """In the small network (all three arithmetics) and in the single convolutions."""
    changed_net = [(l, a) for (l, a), ref in sound["nets"].items() if not np.array_equal(ref, _network_bytes(l, a, defect))]
    changed_conv = sum(not np.array_equal(a, b) for a, b in zip(sound["convs"], _conv_bytes(defect)))
    assert changed_net and changed_conv, (defect, changed_net, changed_conv)

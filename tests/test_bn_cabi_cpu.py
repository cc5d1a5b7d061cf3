"""Host-side argument rule of the ph_debug_bn_* test entries (csrc/bn_act.hip, "test entry points") without a GPU: a NULL required
pointer, a channel count the kernels cannot take, a size below 1, a unit count outside 1 .. 20 and the other documented cases return
PH_EINVAL before anything is launched.  Every call here returns before a launch; the buffers are host memory that is never
dereferenced (the pointer tables of ph_debug_bn_eval_params are read on the host, as documented)."""
import ctypes

import pytest

from tests import bn_emulation as E

OK, EINVAL = 0, -22
BF16, F32, HP = E.BF16, E.BF16X6, E.FP16X3


@pytest.fixture(scope="module")
def L():
    import multimodal_learning_amd as m
    m.build()
    return E.bind(m.lib())


_BUF = (ctypes.c_float * 256)()                      # host memory: never dereferenced


@pytest.fixture(scope="module")
def p():
    a = ctypes.addressof(_BUF)
    return a + -a % 256


def _each_null(call, args, required):
    """call(*args) with each of the `required` positions set to NULL in turn returns PH_EINVAL."""
    for i in required:
        a = list(args)
        a[i] = None
        assert call(*a) == EINVAL, (call.__name__, i)


def _each(call, args, pos, values):
    for v in values:
        a = list(args)
        a[pos] = v
        assert call(*a) == EINVAL, (call.__name__, pos, v)


def test_abi_version_and_public_header_are_untouched(L):
    import os
    assert L.ph_abi_version() == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pathomic_hip.h")).read()
    assert "ph_debug_bn" not in header


def test_pack_input_finalize_and_eval_params(L, p):
    pk = (p, p, 2, 3, 5, BF16, None)
    _each_null(L.ph_debug_bn_pack_input, pk, (0, 1))
    for pos in (2, 3, 4):
        _each(L.ph_debug_bn_pack_input, pk, pos, (0, -1))
    _each(L.ph_debug_bn_pack_input, pk, 5, (-1, 4, 5))
    fin = (p, 4, 64, 16.0, 1e-5, 0.1, p, p, p, p, p, p, p, p, p, None)
    _each_null(L.ph_debug_bn_finalize, fin, (0, 6, 7, 8, 9, 10, 11))
    _each(L.ph_debug_bn_finalize, fin, 1, (0, -1))
    _each(L.ph_debug_bn_finalize, fin, 2, (0, -8))
    _each(L.ph_debug_bn_finalize, fin, 3, (0.0, -1.0, float("nan")))
    _each_null(L.ph_debug_bn_finalize, fin, (12, 13))                     # one running statistic without the other
    tab = (ctypes.c_void_p * 20)(*([p] * 20))
    widths = (ctypes.c_int * 20)(*([64] * 20))
    t, w = ctypes.addressof(tab), ctypes.addressof(widths)
    ev = (t, t, t, t, t, t, t, t, w, 20, 1e-5, None)
    _each_null(L.ph_debug_bn_eval_params, ev, range(9))
    _each(L.ph_debug_bn_eval_params, ev, 9, (0, -1, 21, 1000))
    hole = (ctypes.c_void_p * 20)(*([p] * 19 + [None]))                    # a NULL inside a table
    for pos in range(8):
        a = list(ev)
        a[pos] = ctypes.addressof(hole)
        assert L.ph_debug_bn_eval_params(*a) == EINVAL, pos
    zero = (ctypes.c_int * 20)(*([64] * 19 + [0]))                         # a unit without channels
    a = list(ev)
    a[8] = ctypes.addressof(zero)
    assert L.ph_debug_bn_eval_params(*a) == EINVAL


def test_apply_and_pooling_entries(L, p):
    ap = (p, p, p, None, None, None, None, p, None, 33, 64, 1, BF16, 0, None)
    _each_null(L.ph_debug_bn_apply, ap, (0, 1, 2, 7))
    _each(L.ph_debug_bn_apply, ap, 9, (0,))
    _each(L.ph_debug_bn_apply, ap, 10, (0, -64, 4, 60, 68, 24, 40, 192, 320, 4096, 2056))       # C % 8, 256 % (C / 8), C > 2048
    _each(L.ph_debug_bn_apply, ap, 11, (-1, 4, 2, 3))                       # relu & 2 without y_r
    _each(L.ph_debug_bn_apply, ap, 12, (-1, 4))
    _each(L.ph_debug_bn_apply, ap, 13, (-1, 2))
    yr = list(ap)
    yr[4], yr[5], yr[6], yr[11] = p, p, p, 3
    _each_null(L.ph_debug_bn_apply, yr, (5, 6))                             # y_r without scale_r / shift_r
    hp = list(ap)
    hp[12] = HP
    _each(L.ph_debug_bn_apply, hp, 10, (8, 32, 96))                         # a half-pair tensor: C % 64
    _each(L.ph_debug_bn_apply, hp, 7, (p + 16, p + 128))                    # .. and 256-byte aligned
    hp[3], hp[13] = p + 64, 1
    assert L.ph_debug_bn_apply(*hp) == EINVAL                               # res as a half-pair image
    mp = (p, p, p, p, p, p, None, 2, 5, 7, 64, BF16, None)
    _each_null(L.ph_debug_bn_relu_maxpool, mp, (0, 1, 2, 3, 4))             # (4: raw without idx)
    for pos in (7, 8, 9):
        _each(L.ph_debug_bn_relu_maxpool, mp, pos, (0, -3))
    _each(L.ph_debug_bn_relu_maxpool, mp, 10, (0, 4, 12, -8))
    _each(L.ph_debug_bn_relu_maxpool, mp, 11, (-1, 4))
    m2 = list(mp)
    m2[11] = HP
    _each(L.ph_debug_bn_relu_maxpool, m2, 10, (8, 72))
    _each(L.ph_debug_bn_relu_maxpool, m2, 3, (p + 32,))
    for fn in (L.ph_debug_bn_avgpool, L.ph_debug_bn_avgpool_t):
        av = (p, p, 3, 49, 64, BF16, None)
        _each_null(fn, av, (0, 1))
        _each(fn, av, 2, (0, -1))
        _each(fn, av, 3, (0, -1))
        _each(fn, av, 4, (0, 8, 32, 96, -64))                               # C % 64
        _each(fn, av, 5, (-1, 4))
    assert L.ph_debug_bn_avgpool_t(p + 64, p, 3, 49, 64, HP, None) == EINVAL
    ab = (p, p, 3, 49, 64, 1, BF16, None)
    _each_null(L.ph_debug_bn_avgpool_bwd, ab, (0, 1))
    _each(L.ph_debug_bn_avgpool_bwd, ab, 2, (0,))
    _each(L.ph_debug_bn_avgpool_bwd, ab, 3, (0,))
    _each(L.ph_debug_bn_avgpool_bwd, ab, 4, (0, 8, 100))
    _each(L.ph_debug_bn_avgpool_bwd, ab, 6, (-1, 5))


def test_backward_entries(L, p):
    assert L.ph_debug_bn_bwd_parts(0, 64) == EINVAL
    for C in (0, 4, 60, 24, 4096):
        assert L.ph_debug_bn_bwd_parts(100, C) == EINVAL
    for npix, C in ((1, 64), (5, 512), (33, 512), (300, 64), (1000, 256), (262144, 64), (262144 + 77, 64), (10 ** 7, 512)):
        assert L.ph_debug_bn_bwd_parts(npix, C) == E.bn_bwd_parts(npix, C) == max(1, min(1024, -(-npix * (C // 8) // 2048)))
    assert L.ph_debug_bn_stem_bwd_parts(0, 4) == L.ph_debug_bn_stem_bwd_parts(4, 0) == EINVAL
    for B, H in ((1, 1), (5, 6), (2, 16), (1, 7), (3, 5), (64, 256)):
        assert L.ph_debug_bn_stem_bwd_parts(B, H) == E.stem_blocks(B, H) == -(-B * H // 16)
    rd = (p, p, p, p, p, p, 300, 64, BF16, p, p, p, None)
    _each_null(L.ph_debug_bn_bwd_reduce, rd, (0, 2, 3, 4, 5, 9, 10))        # (9, 10: mscale without mshift and the reverse)
    _each(L.ph_debug_bn_bwd_reduce, rd, 6, (0,))
    _each(L.ph_debug_bn_bwd_reduce, rd, 7, (0, 4, 60, 24, 40, 192, 4096))
    _each(L.ph_debug_bn_bwd_reduce, rd, 8, (-1, 4))
    fi = (p, 4, 64, 300.0, p, p, p, p, p, 4, p, p, p, None)
    _each_null(L.ph_debug_bn_bwd_finalize, fi, (0, 6, 7, 8, 10, 11))        # (8, 10, 11: dzs without amax / gamma / invstd)
    _each(L.ph_debug_bn_bwd_finalize, fi, 1, (0, -1))
    _each(L.ph_debug_bn_bwd_finalize, fi, 2, (0, -1))
    _each(L.ph_debug_bn_bwd_finalize, fi, 3, (0.0, -2.0))
    _each(L.ph_debug_bn_bwd_finalize, fi, 9, (0, -1))
    fu = (p, 4, 64, 300.0, p, p, p, p, p, 1, None)
    _each_null(L.ph_debug_bn_bwd_finalize_fused, fu, (0, 6, 7, 8))
    _each(L.ph_debug_bn_bwd_finalize_fused, fu, 9, (0, 3, -1, 100))         # row2 is 1 or 2
    _each(L.ph_debug_bn_bwd_finalize_fused, fu, 1, (0,))
    _each(L.ph_debug_bn_bwd_finalize_fused, fu, 3, (0.0,))
    ba = (p, p, p, p, p, p, p, p, p, 300, 64, BF16, p, p, p, None)
    _each_null(L.ph_debug_bn_bwd_apply, ba, (0, 2, 3, 4, 5, 6, 7, 8, 12, 13))
    _each(L.ph_debug_bn_bwd_apply, ba, 9, (0,))
    _each(L.ph_debug_bn_bwd_apply, ba, 10, (0, 4, 60, 24, 4096))
    _each(L.ph_debug_bn_bwd_apply, ba, 11, (-1, 4))
    b2 = list(ba)
    b2[11] = HP
    _each(L.ph_debug_bn_bwd_apply, b2, 10, (8, 32))
    _each(L.ph_debug_bn_bwd_apply, b2, 8, (p + 64,))


def test_stem_entries(L, p):
    sr = (p, p, p, p, p, p, p, p, p, 5, 6, 10, 64, BF16, None, 0, None)
    _each_null(L.ph_debug_bn_stem_bwd_reduce, sr, (0, 1, 2, 4, 5, 6, 7, 8))
    for pos in (9, 10, 11):
        _each(L.ph_debug_bn_stem_bwd_reduce, sr, pos, (0, -2))
    _each(L.ph_debug_bn_stem_bwd_reduce, sr, 12, (0, 8, 32, 128, 512))       # the stem has 64 channels
    _each(L.ph_debug_bn_stem_bwd_reduce, sr, 13, (-1, 4))
    _each(L.ph_debug_bn_stem_bwd_reduce, sr, 15, (-1, 2))
    am = list(sr)
    am[14] = p
    for H, form in ((7, 0), (5, 0), (6, 1)):                                # amax with an odd H, or with the per-pixel form
        a = list(am)
        a[10], a[15] = H, form
        assert L.ph_debug_bn_stem_bwd_reduce(*a) == EINVAL, (H, form)
    sa = (p, p, p, p, p, p, p, p, p, p, p, 5, 6, 10, 64, BF16, None, None)
    _each_null(L.ph_debug_bn_stem_bwd_apply, sa, range(11))
    for pos in (11, 12, 13):
        _each(L.ph_debug_bn_stem_bwd_apply, sa, pos, (0, -2))
    _each(L.ph_debug_bn_stem_bwd_apply, sa, 14, (0, 8, 128))
    _each(L.ph_debug_bn_stem_bwd_apply, sa, 15, (-1, 4))
    s2 = list(sa)
    s2[15], s2[10] = HP, p + 128
    assert L.ph_debug_bn_stem_bwd_apply(*s2) == EINVAL

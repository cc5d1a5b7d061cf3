"""Host-side argument rule of the GK-Refine, mask and flat-buffer entries (include/pathomic_hip.h, "Argument rule of ...") without a
GPU: a NULL required pointer, a size outside the documented range and a misaligned Adam buffer return PH_EINVAL, and n == 0 on an
elementwise update returns PH_OK, each before anything is launched.  Every call here returns before a launch; the buffers are host
memory that is never dereferenced."""
import ctypes

import pytest

OK, EINVAL = 0, -22


@pytest.fixture(scope="module")
def L():
    import multimodal_learning_amd as m
    m.build()
    return m.lib()


_BUF = (ctypes.c_float * 64)()                       # host memory: never dereferenced


@pytest.fixture(scope="module")
def p():
    a = ctypes.addressof(_BUF)
    return a + -a % 16


def _each_null(call, args, required):
    """call(*args) with each of the `required` positions set to NULL in turn returns PH_EINVAL."""
    for i in required:
        a = list(args)
        a[i] = None
        assert call(*a) == EINVAL, (call.__name__, i)


def test_gk_entries_reject_null_and_bad_sizes(L, p):
    _each_null(L.ph_gram, (p, p, 3, 10, None), (0, 1))
    for ng in (1, 6, 0, -1):
        assert L.ph_gram(p, p, ng, 10, None) == EINVAL
    for n in (0, -1):
        assert L.ph_gram(p, p, 3, n, None) == EINVAL
    _each_null(L.ph_gk_scale, (p, p, 3, 2, 1.0, p, p, None), (0, 1, 5))          # losses is required once nl > 0
    for ng, nl in ((0, 0), (3, -1), (3, 4)):
        assert L.ph_gk_scale(p, p, ng, nl, 1.0, p, p, None) == EINVAL
    _each_null(L.ph_gk_finish, (p, p, p, p, p, 4.0, p, p, p, p, p, None), (0, 1, 2, 3, 4, 6, 7, 8, 9, 10))
    _each_null(L.ph_gk_scale_momentum, (p, 5, 0, 0.0, 0.9, p, p, None), (0, 5))
    assert L.ph_gk_scale_momentum(p, 0, 0, 0.0, 0.9, p, p, None) == EINVAL
    _each_null(L.ph_gk_finish_momentum, (p, p, 0.7, 1.3, p, 0.45, 4.0, 0, 0.0, 0.9, p, p, p, p, p, p, None), (0, 1, 10, 12, 13, 14, 15))


def test_mask_entries_reject_null_and_bad_sizes(L, p):
    sp = (p, p, p, p, 1, 1, 4, 4, 8, 2, None)
    _each_null(L.ph_superpixel_mask, sp, (0, 1, 2))
    for pos, v in ((4, 0), (5, 0), (8, 0), (8, 2049), (9, 0), (9, 9)):
        a = list(sp)
        a[pos] = v
        assert L.ph_superpixel_mask(*a) == EINVAL, (pos, v)
    _each_null(L.ph_topk_threshold_mask, (p, p, 1, 8, 2, None), (0, 1))
    for B, D, K in ((0, 8, 2), (1, 0, 1), (1, 16385, 2), (1, 8, 0), (1, 8, 9)):
        assert L.ph_topk_threshold_mask(p, p, B, D, K, None) == EINVAL
    _each_null(L.ph_apply_mask, (p, p, p, 1, 1, 4, None), (0, 1, 2))
    for B, C, n in ((0, 1, 4), (1, 0, 4), (1, 1, 0)):
        assert L.ph_apply_mask(p, p, p, B, C, n, None) == EINVAL


def test_updates_reject_null_and_accept_n_zero(L, p):
    adam = (p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.99, None)
    adam_dev = (p, p, p, p, p, 8, 0.9, 0.999, 1e-8, 0.0, p, None)
    adagrad = (p, p, p, p, 8, 1e-10, 0.0, p, None)
    _each_null(L.ph_adam_ema_step, adam, (0, 1, 2, 3))
    _each_null(L.ph_adam_ema_step_dev, adam_dev, (0, 1, 2, 3, 10))
    _each_null(L.ph_adagrad_ema_step_dev, adagrad, (0, 1, 2, 7))
    _each_null(L.ph_ema_update, (p, p, 8, 0.99, None), (0, 1))
    _each_null(L.ph_ema_update_dev, (p, p, 8, p, None), (0, 1, 3))
    _each_null(L.ph_scaled_diff, (p, p, p, 0.5, p, 8, None), (0, 1, 2, 4))
    _each_null(L.ph_l1_sign_axpy, (p, p, 8, p, 1.0, None), (0, 1))
    _each_null(L.ph_l1_sum, (p, 8, p, p, 0, None), (0, 2, 3))
    _each_null(L.ph_sqdiff_sum, (p, p, p, 8, 1.0, None), (0, 1, 2))
    _each_null(L.ph_maxnorm_mix, (p, p, p, 8, 0.5, 0.5, None), (0, 1, 2))
    assert L.ph_maxnorm_mix(p, p, p, 0, 0.5, 0.5, None) == EINVAL
    _each_null(L.ph_sigmoid_range_fwd, (p, p, p, p, p, 8, None), (0, 1, 2, 3, 4))
    _each_null(L.ph_sigmoid_range_bwd, (p, p, p, p, 8, None), (0, 1, 2, 3))
    assert L.ph_sigmoid_range_fwd(p, p, p, p, p, 0, None) == EINVAL and L.ph_sigmoid_range_bwd(p, p, p, p, 0, None) == EINVAL

    # n == 0: PH_OK without a launch, with or without the optional ema; a NULL required pointer still comes first
    def zero(args, pos):
        a = list(args)
        a[pos] = 0
        return a
    for ema in (p, None):
        a = zero(adam, 5); a[4] = ema
        assert L.ph_adam_ema_step(*a) == OK
        a = zero(adam_dev, 5); a[4] = ema
        assert L.ph_adam_ema_step_dev(*a) == OK
        a = zero(adagrad, 4); a[3] = ema
        assert L.ph_adagrad_ema_step_dev(*a) == OK
    assert L.ph_ema_update(p, p, 0, 0.99, None) == OK and L.ph_ema_update_dev(p, p, 0, p, None) == OK
    assert L.ph_scaled_diff(p, p, p, 0.5, p, 0, None) == OK
    for cd in (p, None):
        assert L.ph_l1_sign_axpy(p, p, 0, cd, 1.0, None) == OK
    a = zero(adam, 5); a[0] = None
    assert L.ph_adam_ema_step(*a) == EINVAL
    assert L.ph_ema_update(None, p, 0, 0.99, None) == EINVAL and L.ph_scaled_diff(p, p, None, 0.5, p, 0, None) == EINVAL


def test_adam_buffers_must_be_16_byte_aligned(L, p):
    for form, args in ((L.ph_adam_ema_step, (p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.99, None)),
                       (L.ph_adam_ema_step_dev, (p, p, p, p, p, 8, 0.9, 0.999, 1e-8, 0.0, p, None))):
        for pos in range(5):
            for off in (4, 8, 12):
                a = list(args)
                a[pos] = p + off
                assert form(*a) == EINVAL, (pos, off)

"""SLIC superpixels without a GPU: the numpy restatement of the all-integer definition
(tests/slic_emulation.py) on inputs whose answer is known, and the host side of the new C-ABI entries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_emulation as E  # noqa: E402


def test_lab_of_the_primaries():
    """8-bit CIELAB in the OpenCV convention (L * 255 / 100, a + 128, b + 128)."""
    want = {(255, 255, 255): (255, 128, 128), (0, 0, 0): (0, 128, 128), (255, 0, 0): (136, 208, 195),
            (0, 255, 0): (224, 42, 211), (0, 0, 255): (82, 207, 20), (128, 128, 128): (137, 128, 128)}
    for rgb, lab in want.items():
        assert tuple(int(v) for v in E.rgb_to_lab8(np.array(rgb, dtype=np.uint8))) == lab, rgb


@pytest.mark.parametrize("H,W,K", [(256, 256, 64), (192, 160, 30), (512, 512, 100), (160, 192, 30), (96, 64, 7)])
def test_grid_and_label_range(H, W, K):
    rng = np.random.default_rng(H + W + K)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    gy, gx = E.grid(H, W, K)
    labels, N = E.slic(img, K, iters=3)
    assert N == gy * gx <= K and gy * gy * W <= K * H < (gy + 1) * (gy + 1) * W and gx == K // gy
    assert labels.shape == (H, W) and labels.dtype == np.int16 and labels.min() >= 0 and labels.max() < N


def test_aligned_blocks_are_recovered_exactly():
    """Noise-free random coloured 32 x 32 blocks, grid = block grid: the label map is the block index map."""
    img, idx = E.blocks_image(256, 256, 32, seed=0)
    labels, N = E.slic(img, 64)
    assert N == 64 and np.array_equal(labels, idx)
    assert np.bincount(labels.reshape(-1)).tolist() == [1024] * 64


def test_boundary_adherence_where_grid_and_blocks_do_not_line_up():
    """512 x 512, 64 x 64 blocks with +-12 noise, K = 100 (grid 10 x 10 over 8 x 8 blocks): at most 1 % of the pixels lie
    outside the majority block of their superpixel (a condition; the restatement stays below 0.1 %)."""
    img, idx = E.blocks_image(512, 512, 64, seed=1, noise=12)
    labels, N = E.slic(img, 100)
    share = E.impure_share(labels, idx)
    area = np.bincount(labels.reshape(-1), minlength=N)
    print("impure share %.4f %%, areas %d .. %d" % (100 * share, area.min(), area.max()))
    assert N == 100 and share <= 0.01 and area.min() > 0


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_new_symbols_and_abi_version():
    from multimodal_learning_amd import _lib as B
    L = _lib()
    assert L.ph_abi_version() == 1
    for name in ("ph_slic", "ph_slic_lab", "ph_slic_workspace_bytes", "ph_slic_num_labels", "ph_augment_params_v",
                 "ph_augment_apply_v"):
        assert name in B.SIGNATURES and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is B.SIGNATURES[name][0] and list(fn.argtypes) == B.SIGNATURES[name][1], name


def test_workspace_and_label_count_on_the_host():
    L = _lib()
    prev = 0
    for n in (1, 2, 3, 9, 64, 256):
        b = L.ph_slic_workspace_bytes(n, 1024, 1024, 100)
        assert b > prev and b >= n * 1024 * 1024 * 4
        prev = b
    assert L.ph_slic_workspace_bytes(1, 1, 1, 1) > 0
    for H, W, K in ((256, 256, 64), (192, 160, 30), (512, 512, 100), (512, 512, 2048), (1024, 1024, 100)):
        gy, gx = E.grid(H, W, K)
        assert L.ph_slic_num_labels(H, W, K) == gy * gx
    for bad in ((0, 512, 512, 100), (1, 512, 512, 0), (1, 0, 512, 100), (1, 512, 0, 100), (1, 512, 512, 2100), (1, 4, 4, 100)):
        assert L.ph_slic_workspace_bytes(*bad) == 0, bad


def test_entry_points_reject_bad_arguments_before_any_launch():
    """Pointers are never dereferenced on the host and nothing is launched: the codes come back without a device."""
    L = _lib()
    EINVAL = -22
    p = C.c_void_p(4096)                       # a non-null placeholder
    assert L.ph_slic(p, p, 1, 512, 512, 2100, 10, 10, p, None) == EINVAL         # grid 45 x 46: N = 2070 > 2048
    assert L.ph_slic(p, p, 1, 512, 512, 0, 10, 10, p, None) == EINVAL            # K < 1
    assert L.ph_slic(p, p, 1, 0, 512, 100, 10, 10, p, None) == EINVAL            # zero-sized image
    assert L.ph_slic(p, p, 1, 512, 0, 100, 10, 10, p, None) == EINVAL
    assert L.ph_slic(p, p, 0, 512, 512, 100, 10, 10, p, None) == EINVAL
    assert L.ph_slic(p, p, 1, 512, 512, 100, 10, 0, p, None) == EINVAL           # no iteration
    assert L.ph_slic(p, p, 1, 512, 512, 100, -1, 10, p, None) == EINVAL
    assert L.ph_slic(None, p, 1, 512, 512, 100, 10, 10, p, None) == EINVAL
    assert L.ph_slic_lab(p, p, 0, p, None) == EINVAL
    assert L.ph_slic_num_labels(512, 512, 2100) == EINVAL and L.ph_slic_num_labels(512, 512, 0) == EINVAL
    outs = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    assert L.ph_augment_params_v(p, 4, 4, 0, None, 64, 64, 65, 0.1, 0.1, 0.05, 0.01, None) == EINVAL   # crop > tile
    assert L.ph_augment_params_v(p, 4, 5, 0, None, 64, 64, 32, 0.1, 0.1, 0.05, 0.01, None) == EINVAL   # too many views
    assert L.ph_augment_apply_v(p, p, None, p, outs, None, 4, 4, 64, 48, 49, None) == EINVAL           # crop > tile
    assert L.ph_augment_apply_v(p, p, None, p, outs, None, 4, 0, 64, 64, 32, None) == EINVAL
    assert L.ph_augment_apply_v(p, None, None, p, outs, outs, 4, 4, 64, 64, 32, None) == EINVAL        # label output without maps

"""Device SLIC (csrc/slic.hip) against its numpy restatement (tests/slic_emulation.py): the
definition is all-integer, so every comparison here is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_emulation as E  # noqa: E402

pytestmark = pytest.mark.gpu


def _sinusoid(H, W, seed, noise=10):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([128 + 100 * np.sin(y / 17.0 + x / 29.0), 128 + 90 * np.cos(x / 13.0), 128 + 80 * np.sin((x - y) / 23.0)], -1)
    return np.clip(np.rint(img) + rng.integers(-noise, noise + 1, img.shape), 0, 255).astype(np.uint8)


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


def _segment(img, K, **kw):
    import multimodal_learning_amd as m
    labels, N = m.superpixel.slic_segment(torch.from_numpy(img)[None].cuda(), K, **kw)
    return labels[0].cpu().numpy(), N


def test_lab_conversion_equals_the_restatement_on_all_colours():
    import multimodal_learning_amd as m
    v = torch.arange(1 << 24, dtype=torch.int32)
    rgb = torch.stack([v & 255, (v >> 8) & 255, v >> 16], 1).to(torch.uint8)
    got = m.superpixel.rgb_to_lab8(rgb.cuda()).cpu().numpy()
    want = E.rgb_to_lab8(rgb.numpy())
    bad = np.argwhere((got != want).any(1))
    assert bad.size == 0, (len(bad), rgb.numpy()[bad[:4, 0]], got[bad[:4, 0]], want[bad[:4, 0]])
    # a pixel count that is no multiple of four, from an odd address: the scalar path
    odd = m.superpixel.rgb_to_lab8(rgb.cuda()[5:5 + 1003]).cpu().numpy()
    assert np.array_equal(odd, want[5:5 + 1003])


CASES = {
    "blocks_aligned": lambda: (E.blocks_image(256, 256, 32, seed=0)[0], 64),
    "blocks_noisy": lambda: (E.blocks_image(512, 512, 64, seed=1, noise=12)[0], 100),
    "sinusoid": lambda: (_sinusoid(256, 320, 2), 50),
    "noise": lambda: (_noise(256, 256, 3), 64),
    "constant": lambda: (np.full((128, 128, 3), (90, 140, 200), dtype=np.uint8), 16),
    "192x160_k30": lambda: (_sinusoid(192, 160, 4), 30),
    "512x512_k100": lambda: (_sinusoid(512, 512, 5), 100),
    "1024x1024_k100": lambda: (_sinusoid(1024, 1024, 6), 100),
    "512x512_k2048": lambda: (_sinusoid(512, 512, 7), 2048),
    "97x75_k12": lambda: (_noise(97, 75, 8), 12),          # H W no multiple of four: the scalar loads and stores
    "one_row_of_cells": lambda: (_sinusoid(16, 400, 9), 9),
    "512x512_k4": lambda: (_sinusoid(512, 512, 12), 4),    # distances beyond 2^32: the 64-bit kernel
}


@pytest.mark.parametrize("case", list(CASES))
def test_segmentation_equals_the_restatement_on_every_pixel(case):
    img, K = CASES[case]()
    want, N = E.slic(img, K)
    got, n_dev = _segment(img, K)
    bad = np.argwhere(got != want)
    area = np.bincount(want.reshape(-1).astype(np.int64), minlength=N)
    print(f"{case}: N {N}, areas {area.min()} .. {area.max()}, differing pixels {len(bad)}")
    assert n_dev == N and got.dtype == np.int16 and got.shape == want.shape
    assert bad.size == 0, (len(bad), bad[:4])
    if case == "512x512_k2048":
        assert N == 2025 and area.min() > 0


def test_other_compactness_and_iteration_counts_equal_the_restatement():
    img = _sinusoid(160, 224, 10)
    for m_, it in ((0, 4), (40, 1), (3, 7), (1000, 3)):       # m = 1000: distances beyond 2^32
        want, _ = E.slic(img, 35, compactness=m_, iters=it)
        got, _ = _segment(img, 35, compactness=m_, iters=it)
        assert np.array_equal(got, want), (m_, it)


def test_aligned_blocks_are_recovered_on_the_device():
    img, idx = E.blocks_image(256, 256, 32, seed=0)
    got, N = _segment(img, 64)
    assert N == 64 and np.array_equal(got, idx)


def test_reproducible_and_independent_of_chunking():
    import multimodal_learning_amd as m
    tiles = torch.from_numpy(np.stack([_sinusoid(128, 160, 20 + i, noise=4 * i) for i in range(9)])).cuda()
    a, N = m.superpixel.slic_segment(tiles, 40)
    b, _ = m.superpixel.slic_segment(tiles, 40)
    assert torch.equal(a, b) and a.dtype == torch.int16 and tuple(a.shape) == (9, 128, 160)
    c, _ = m.superpixel.slic_segment(tiles, 40, chunk=4)
    assert torch.equal(a, c)
    for i in range(9):
        one, _ = m.superpixel.slic_segment(tiles[i:i + 1], 40)
        assert torch.equal(one[0], a[i]), i
    assert np.array_equal(a[3].cpu().numpy(), E.slic(tiles[3].cpu().numpy(), 40)[0])
    out = torch.full((9, 128, 160), -7, device="cuda", dtype=torch.int16)
    r, _ = m.superpixel.slic_segment(tiles, 40, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(out, a)
    with pytest.raises(RuntimeError):
        m.superpixel.slic_segment(tiles, 40, out=out.int())
    with pytest.raises(ValueError):
        m.superpixel.slic_segment(tiles, 5000)
    with pytest.raises(RuntimeError):
        m.superpixel.slic_segment(tiles.cpu(), 40)


def test_labels_drive_the_superpixel_mask_kernel():
    """superpixel_topk_mask on cropped device labels = numpy per-label mean / top-k on the same labels (tolerance of
    tests/test_gpu_losses.py for that kernel: 2e-5 of the largest |mean|; the mask where the cut is clear by more)."""
    import multimodal_learning_amd as m
    B, SH, S, K, path_k = 3, 160, 128, 40, 5
    tiles = torch.from_numpy(np.stack([_sinusoid(SH, SH, 30 + i) for i in range(B)])).cuda()
    labels, N = m.superpixel.slic_segment(tiles, K)
    crop = labels[:, 9:9 + S, 21:21 + S].long().contiguous()
    g = torch.Generator().manual_seed(0)
    grad = torch.randn(B, 3, S, S, generator=g) * 1e-3
    mask, mean = m.superpixel.superpixel_topk_mask(grad.cuda(), crop, path_k, num_superpixels=N, return_mean=True)
    lab = crop.cpu().numpy()
    gs = grad.double().sum(1).numpy()
    for b in range(B):
        area = np.bincount(lab[b].reshape(-1), minlength=N).astype(np.float64)
        ref = np.bincount(lab[b].reshape(-1), weights=gs[b].reshape(-1), minlength=N) / (area + 1e-9)
        tol = 2e-5 * np.abs(ref).max()
        assert np.abs(mean[b].cpu().numpy() - ref).max() <= tol
        order = np.argsort(-ref, kind="stable")
        if ref[order[path_k - 1]] - ref[order[path_k]] > tol:
            want = np.isin(lab[b], order[:path_k]).astype(np.float32)
            assert np.array_equal(mask[b].cpu().numpy(), want), b

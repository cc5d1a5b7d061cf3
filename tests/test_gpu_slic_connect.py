"""The device connectivity pass over SLIC label maps (csrc/slic.hip) against its restatement
(tests/slic_connect_emulation.py): the rule is all-integer and order-independent, so every comparison is an equality on
every pixel.  Shapes: the eight SLIC-derived maps of the literal table (tests/test_slic_connect_cpu.py), and hand-made
maps at the edges of the 64 x 16 block decomposition - one row, one column, one pixel, neither side a multiple of the
block, a component that crosses every seam."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_connect_emulation as CE  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(name):
    """Restated connected map of a table row, computed once."""
    if name not in _WANT:
        _, _, _, labels, N, min_size = CE.table_labels(name)
        _WANT[name] = CE.connect(labels, N, min_size)
        _WANT[name].setflags(write=False)
    return _WANT[name]


def _connect(lab, N, min_size, **kw):
    import multimodal_learning_amd as m
    t = torch.from_numpy(np.array(lab))
    t = (t[None] if t.dim() == 2 else t).cuda()
    return m.superpixel.slic_connect(t, N, min_size, **kw).cpu().numpy()


def _blobs(H, W, N, seed, salt=0.15):
    """Coarse random label blocks of 7 x 5 pixels with `salt` of the pixels redrawn: large components and many fragments."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, N, ((H + 6) // 7, (W + 4) // 5))
    lab = np.repeat(np.repeat(coarse, 7, 0), 5, 1)[:H, :W]
    redraw = rng.random((H, W)) < salt
    return np.where(redraw, rng.integers(0, N, (H, W)), lab).astype(np.int16)


@pytest.mark.parametrize("name", list(CE.TABLE))
def test_slic_segment_with_the_pass_equals_the_restatement(name):
    import multimodal_learning_amd as m
    img, K, comp, labels, N, min_size = CE.table_labels(name)
    tiles = torch.from_numpy(img)[None].cuda()
    got, n_dev = m.superpixel.slic_segment(tiles, K, compactness=comp, enforce_connectivity=True)
    plain, _ = m.superpixel.slic_segment(tiles, K, compactness=comp)
    assert n_dev == N and got.dtype == torch.int16
    assert np.array_equal(plain[0].cpu().numpy(), labels)                    # the default is the segmentation alone
    bad = np.argwhere(got[0].cpu().numpy() != _want(name))
    assert bad.size == 0, (len(bad), bad[:4])
    quarter, _ = m.superpixel.slic_segment(tiles, K, compactness=comp, enforce_connectivity=True, min_size_factor=0.25)
    assert torch.equal(quarter, got)
    tiny, _ = m.superpixel.slic_segment(tiles, K, compactness=comp, enforce_connectivity=True, min_size_factor=0.0)
    assert torch.equal(tiny, plain)                                           # min_size 1: the identity


@pytest.mark.parametrize("name", list(CE.TABLE))
def test_slic_connect_on_the_restated_maps_equals_the_restatement(name):
    _, _, _, labels, N, min_size = CE.table_labels(name)
    got = _connect(labels, N, min_size)[0]
    bad = np.argwhere(got != _want(name))
    assert bad.size == 0, (len(bad), bad[:4])


@pytest.mark.parametrize("min_size", [4096, 1])
def test_checkerboard(min_size):
    cb = CE.checkerboard()
    got = _connect(cb, 2, min_size)[0]
    assert np.array_equal(got, CE.connect(cb, 2, min_size))
    if min_size == 1:
        assert np.array_equal(got, cb)
    else:
        assert (got[:, 0] == 0).all() and (got[:, 1:] == 1).all()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 37), (41, 1)])
def test_degenerate_shapes(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for N, min_size in ((3, 2), (3, 5), (2, 100)):
        lab = rng.integers(0, N, (H, W)).astype(np.int16)
        assert np.array_equal(_connect(lab, N, min_size)[0], CE.connect(lab, N, min_size)), (N, min_size)


def test_serpentine_across_every_block_seam():
    lab = CE.serpentine(96, 160)
    for min_size in (200, 100, 1):                     # the gaps hold 159 pixels each: all but the first merged / kept / identity
        want = CE.connect(lab, 2, min_size)
        assert np.array_equal(_connect(lab, 2, min_size)[0], want), min_size
    assert (CE.connect(lab, 2, 200)[2:] == 0).all() and np.array_equal(CE.connect(lab, 2, 100), lab)
    inv = (1 - lab).astype(np.int16)                   # the labels swapped: the serpentine is label 1
    assert np.array_equal(_connect(inv, 2, 10 ** 6)[0], CE.connect(inv, 2, 10 ** 6))


@pytest.mark.parametrize("seed,N,min_size", [(0, 6, 20), (1, 2, 9), (2, 40, 3)])
def test_odd_dimensions(seed, N, min_size):
    lab = _blobs(70, 130, N, seed)
    assert np.array_equal(_connect(lab, N, min_size)[0], CE.connect(lab, N, min_size))


def test_several_tiles_in_one_call():
    tiles = np.stack([_blobs(70, 130, 6, 10 + i, salt=0.1 * (i + 1)) for i in range(3)])
    all3 = _connect(tiles, 6, 15)
    for i in range(3):
        assert np.array_equal(all3[i], CE.connect(tiles[i], 6, 15)), i
        assert np.array_equal(_connect(tiles[i], 6, 15)[0], all3[i]), i
    assert np.array_equal(_connect(tiles, 6, 15, chunk=1), all3)
    assert np.array_equal(_connect(tiles, 6, 15, chunk=2), all3)


def test_buffers_in_place_guard_bands_and_exact_workspace():
    import multimodal_learning_amd as m
    from multimodal_learning_amd._lib import lib, ptr, stream
    n, H, W, N, min_size, G = 2, 70, 130, 6, 15, 512
    tiles = np.stack([_blobs(H, W, N, 20 + i) for i in range(n)])
    want = np.stack([CE.connect(t, N, min_size) for t in tiles])
    src = torch.from_numpy(tiles).cuda()
    keep = src.clone()
    # out of place into the middle of a guarded buffer
    buf = torch.full((n * H * W + 2 * G,), -12345, dtype=torch.int16, device="cuda")
    out = buf[G:G + n * H * W].view(n, H, W)
    r = m.superpixel.slic_connect(src, N, min_size, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(src, keep)
    assert np.array_equal(out.cpu().numpy(), want)
    assert (buf[:G] == -12345).all() and (buf[G + n * H * W:] == -12345).all()
    # in place
    r = m.superpixel.slic_connect(src, N, min_size, out=src)
    assert r.data_ptr() == src.data_ptr() and np.array_equal(src.cpu().numpy(), want)
    # the C entry with a workspace of exactly the bytes it asks for, between guard bands
    nbytes = lib().ph_slic_connect_workspace_bytes(n, H, W, N)
    assert nbytes >= n * H * W * 8 + n * N * 8
    wbuf = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = wbuf[G:G + nbytes]
    out2 = torch.empty_like(keep)
    assert lib().ph_slic_connect(ptr(keep), ptr(out2), n, H, W, N, min_size, ptr(ws), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), want)
    assert (wbuf[:G] == 0xA5).all() and (wbuf[G + nbytes:] == 0xA5).all()
    with pytest.raises(RuntimeError):
        m.superpixel.slic_connect(keep.int(), N, min_size)
    with pytest.raises(RuntimeError):
        m.superpixel.slic_connect(keep.cpu(), N, min_size)
    with pytest.raises(RuntimeError):
        m.superpixel.slic_connect(keep, N, min_size, out=out2.int())
    with pytest.raises(ValueError):
        m.superpixel.slic_connect(keep, N, 0)
    with pytest.raises(ValueError):
        m.superpixel.slic_connect(keep, 5000, 3)


def test_labels_outside_the_table_complete_and_stay():
    from multimodal_learning_amd._lib import lib, ptr, stream
    H, W, N = 70, 130, 6
    lab = _blobs(H, W, N, 30)
    rng = np.random.default_rng(31)
    wrong = rng.random((H, W)) < 0.05
    lab[wrong] = np.where(rng.random(int(wrong.sum())) < 0.5, -1, N).astype(np.int16)
    src = torch.from_numpy(lab)[None].cuda()
    out = torch.empty_like(src)
    ws = torch.empty(lib().ph_slic_connect_workspace_bytes(1, H, W, N), dtype=torch.uint8, device="cuda")
    assert lib().ph_slic_connect(ptr(src), ptr(out), 1, H, W, N, 20, ptr(ws), stream()) == 0
    torch.cuda.synchronize()
    got = out[0].cpu().numpy()
    assert np.array_equal(got[wrong], lab[wrong])
    assert np.array_equal(got, CE.connect(lab, N, 20))


def test_two_runs_are_bitwise_equal():
    _, _, _, labels, N, min_size = CE.table_labels("noise97x75")
    stack = np.stack([labels, labels[::-1].copy(), labels])
    a, b = _connect(stack, N, min_size), _connect(stack, N, min_size)
    assert np.array_equal(a, b) and np.array_equal(a[0], a[2]) and np.array_equal(a[0], _want("noise97x75"))


def _src(B, SH, SW, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (B, SH // 8, SW // 8, 3), generator=g, dtype=torch.uint8)
    img = base.repeat_interleave(8, 1).repeat_interleave(8, 2).int() + torch.randint(-20, 21, (B, SH, SW, 3), generator=g)
    return img.clamp(0, 255).to(torch.uint8)


def test_loader_passes_the_two_arguments_on():
    import multimodal_learning_amd as m
    import slic_emulation as E
    n, SH, S, K = 12, 96, 64, 30
    tiles = _src(n, SH, SH, 5)
    opt = lambda: types.SimpleNamespace(input_size_path=S, nce_p=4, nce_k=10, pos_mode="multi_pos", label_dim=3, num_superpixels=K)
    args = (tiles.cuda(), torch.randn(n, 80), torch.arange(n) % 3)
    o = opt()
    ld = m.augment.ResidentSuperpixelLoader(o, *args, seed=3, enforce_connectivity=True)
    N = m.superpixel.slic_num_labels(SH, SH, K)
    assert ld.num_labels == N == o.num_superpixels_max and ld.sp_maps.dtype == torch.int16
    min_size = ((SH * SH) // N) // 4
    changed = 0
    for i in range(n):
        seg, _ = E.slic(tiles[i].numpy(), K)
        want = CE.connect(seg, N, min_size)
        changed += int((want != seg).sum())
        assert np.array_equal(ld.sp_maps[i].cpu().numpy(), want), i
    assert changed > 0                                                        # the pass had something to do
    half = m.augment.ResidentSuperpixelLoader(opt(), *args, seed=3, enforce_connectivity=True, min_size_factor=0.5)
    assert np.array_equal(half.sp_maps[0].cpu().numpy(), CE.connect(E.slic(tiles[0].numpy(), K)[0], N, ((SH * SH) // N) // 2))
    plain = m.augment.ResidentSuperpixelLoader(opt(), *args, seed=3)
    seg, _ = m.superpixel.slic_segment(tiles.cuda(), K)
    assert torch.equal(plain.sp_maps, seg) and plain.num_labels == N


def test_top_one_mask_on_a_connected_map_is_one_label():
    import multimodal_learning_amd as m
    name = "blocks96_n40"
    _, _, _, labels, N, _ = CE.table_labels(name)
    want = _want(name)
    dev = torch.from_numpy(np.array(want))[None].cuda()
    g = torch.Generator().manual_seed(0)
    grad = torch.randn(1, 3, *want.shape, generator=g)
    mask, mean = m.superpixel.superpixel_topk_mask(grad.cuda(), dev.long(), 1, num_superpixels=N, return_mean=True)
    top = int(mean[0].argmax())
    got = mask[0].cpu().numpy()
    assert np.array_equal(got, (want == top).astype(np.float32))
    assert set(np.unique(want[got == 1])) == {top}

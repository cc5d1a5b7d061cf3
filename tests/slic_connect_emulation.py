"""Numpy / scipy restatement of the connectivity pass over SLIC label maps, written from its definition in DESIGN.md
section 14 (not from the kernels).  Integers only, so the device has to agree on every pixel.

    out = connect(labels [H, W], N, min_size)                       # same dtype and shape as labels
    out, info = connect(labels, N, min_size, return_info=True)      # info: counts and the component map

The keyword arguments after `return_info` inject one defect each (tests/test_slic_connect_cpu.py shows that the cases
tell every one of them from the rule); all of them default to the rule.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def components(labels, eight=False):
    """Component map [H, W] int64: every pixel carries the first pixel (lowest raster index y W + x) of its maximal
    4-connected set of equal labels."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(idx[:, :-1], idx[:, 1:], lab[:, :-1] == lab[:, 1:]), (idx[:-1], idx[1:], lab[:-1] == lab[1:])]
    if eight:
        pairs += [(idx[:-1, :-1], idx[1:, 1:], lab[:-1, :-1] == lab[1:, 1:]), (idx[:-1, 1:], idx[1:, :-1], lab[:-1, 1:] == lab[1:, :-1])]
    a = np.concatenate([p[0][p[2]] for p in pairs])
    b = np.concatenate([p[1][p[2]] for p in pairs])
    graph = coo_matrix((np.ones(a.size, dtype=np.int8), (a, b)), shape=(H * W, H * W))
    _, cid = connected_components(graph, directed=False)
    first = np.full(cid.max() + 1, H * W, dtype=np.int64)
    np.minimum.at(first, cid, idx.reshape(-1))
    return first[cid].reshape(H, W)


def connect(labels, N, min_size, return_info=False, eight=False, le=False, tie_high=False, left_first=False, one_level=False,
            principal_by_first=False):
    labels = np.asarray(labels)
    lab = labels.astype(np.int64)
    H, W = lab.shape
    min_size = int(min_size)
    if min_size < 1 or N < 1:
        raise ValueError("min_size and N must be at least 1")
    comp = components(lab, eight=eight)
    flat_c, flat_l = comp.reshape(-1), lab.reshape(-1)
    roots, size = np.unique(flat_c, return_counts=True)           # ascending first pixels
    rlab = flat_l[roots]
    valid = (rlab >= 0) & (rlab < N)
    # principal component of a label: largest size, then lowest first pixel
    principal = np.zeros(roots.size, dtype=bool)
    for l in np.unique(rlab[valid]):
        k = np.flatnonzero(rlab == l)
        if principal_by_first:
            principal[k[0]] = True
        else:
            big = k[size[k] == size[k].max()]
            principal[big[-1] if tie_high else big[0]] = True
    small = size <= min_size if le else size < min_size
    merged = valid & ~principal & small & (roots != 0)
    # target: the component of the pixel above the first pixel, in row 0 the pixel to its left
    y, x = np.divmod(roots, W)
    if left_first:
        t = np.where(x > 0, roots - 1, roots - W)
    else:
        t = np.where(y > 0, roots - W, roots - 1)
    target = np.searchsorted(roots, flat_c[np.where(merged, t, 0)])   # index of the target component among the roots
    final = rlab.copy()
    for i in np.flatnonzero(merged):                               # ascending: a target's first pixel is lower, so it is final
        final[i] = rlab[target[i]] if one_level else final[target[i]]
    out = final[np.searchsorted(roots, flat_c)].reshape(H, W).astype(labels.dtype)
    if not return_info:
        return out
    kept = valid & ~principal & ~small
    info = dict(components=int(roots.size), merged=int(merged.sum()), kept=int(kept.sum()), changed=int((out != labels).sum()),
                components_after=int(np.unique(components(out)).size), comp=comp, roots=roots, size=size, principal=principal,
                merged_mask=merged, kept_mask=kept)
    return out, info


# ---- the inputs both test files share --------------------------------------------------------------------------------
def sinusoid(H, W, seed, noise=10):
    """`_sinusoid` of tests/test_gpu_slic.py."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([128 + 100 * np.sin(y / 17.0 + x / 29.0), 128 + 90 * np.cos(x / 13.0), 128 + 80 * np.sin((x - y) / 23.0)], -1)
    return np.clip(np.rint(img) + rng.integers(-noise, noise + 1, img.shape), 0, 255).astype(np.uint8)


def noise(H, W, seed):
    """`_noise` of tests/test_gpu_slic.py."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


def _draws():
    rng = np.random.default_rng(0)
    return [rng.integers(0, 256, (64, 64, 3)).astype(np.uint8) for _ in range(2)]


def _blocks(*a, **k):
    from slic_emulation import blocks_image
    return blocks_image(*a, **k)[0]


# name -> (image, K, compactness, (N, min_size, components, merged, kept, pixels changed, components after)); SLIC with
# 10 iterations, min_size = ((H W) // N) // 4
TABLE = {
    "blocks96_n40": (lambda: _blocks(96, 96, 12, 3, noise=40), 30, 10, (30, 76, 960, 917, 13, 2580, 40)),
    "blocks91_n25": (lambda: _blocks(96, 96, 7, 5, noise=25), 30, 10, (30, 69, 603, 565, 8, 4420, 35)),
    "draw_a": (lambda: _draws()[0], 16, 10, (16, 64, 2631, 2614, 0, 3512, 16)),
    "draw_b_m1": (lambda: _draws()[1], 16, 1, (16, 64, 2685, 2668, 0, 3612, 17)),      # the fragment at pixel (0, 0) survives
    "blocks126x153": (lambda: _blocks(128, 160, 9, 7, noise=30), 40, 10, (40, 120, 1847, 1802, 5, 11257, 43)),
    "noise97x75": (lambda: noise(97, 75, 8), 12, 10, (12, 151, 4478, 4465, 0, 6101, 12)),
    "sinusoid192x160": (lambda: sinusoid(192, 160, 4), 30, 10, (30, 256, 557, 522, 4, 1519, 34)),
    "sinusoid16x400": (lambda: sinusoid(16, 400, 9), 9, 10, (9, 177, 42, 30, 3, 40, 12)),
}

_SEGMENTED = {}


def table_labels(name):
    """(image, K, compactness, labels int16 [H, W], N, min_size) of a TABLE row; the restated SLIC runs once per process."""
    if name not in _SEGMENTED:
        from slic_emulation import slic
        make, K, m, _ = TABLE[name]
        img = make()
        labels, N = slic(img, K, compactness=m)
        labels.setflags(write=False)
        _SEGMENTED[name] = (img, K, m, labels, N, max(1, ((labels.shape[0] * labels.shape[1]) // N) // 4))
    return _SEGMENTED[name]


def checkerboard(H=64, W=64):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((y + x) & 1).astype(np.int16)


def serpentine(H=96, W=160):
    """Label 0: one component of width 1 winding over the whole map (even rows, joined alternately at the right and the
    left end); label 1 in the gaps."""
    lab = np.ones((H, W), dtype=np.int16)
    lab[0::2] = 0
    for k, y in enumerate(range(1, H, 2)):
        lab[y, W - 1 if k % 2 == 0 else 0] = 0
    return lab

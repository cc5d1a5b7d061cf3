"""Numpy restatement of the device SLIC segmentation, written from its definition in DESIGN.md section 14 (not from the
kernel).  Everything is integer arithmetic, so the kernel has to agree on every pixel.  Needs numpy only.

    labels, N = slic(image_u8 [H, W, 3], num_components, compactness=10, iters=10)     # int16 [H, W], labels in [0, N)
"""
import numpy as np

MAX_LABELS = 2048
# sRGB -> XYZ rows divided by the D65 white (0.950456, 1, 1.088754), times 4096, rounded; every row sums to 4096
XYZ12 = np.array([[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]], dtype=np.int64)


def tables():
    """(lin [256]: sRGB byte -> 12-bit linear, ft [4096]: t / 4095 -> f(t) of CIELAB in 15-bit fixed point), float64 once."""
    c = np.arange(256, dtype=np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    t = np.arange(4096, dtype=np.float64) / 4095.0
    f = np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)
    return np.floor(4095.0 * lin + 0.5).astype(np.int64), np.floor(32768.0 * f + 0.5).astype(np.int64)


_LIN, _FT = tables()


def rgb_to_lab8(rgb):
    """uint8 [..., 3] sRGB -> uint8 [..., 3] (L * 255 / 100, a + 128, b + 128)."""
    l = _LIN[np.asarray(rgb, dtype=np.uint8).astype(np.int64)]
    xyz = (l @ XYZ12.T + 2048) >> 12
    fx, fy, fz = _FT[xyz[..., 0]], _FT[xyz[..., 1]], _FT[xyz[..., 2]]
    L = (29580 * fy - 133693440 + 1638400) // 3276800          # (116 fy - 16 * 2^15) * 255 / (100 * 2^15), rounded
    a = (500 * (fx - fy) + (128 << 15) + (1 << 14)) >> 15       # floor
    b = (200 * (fy - fz) + (128 << 15) + (1 << 14)) >> 15
    return np.clip(np.stack([L, a, b], -1), 0, 255).astype(np.uint8)


def grid(H, W, K):
    """(gy, gx): gy = floor(sqrt(K H / W)) as the largest g with g g W <= K H, gx = K // gy."""
    if H < 1 or W < 1 or K < 1:
        raise ValueError("empty image or K < 1")
    gy = 1
    while (gy + 1) * (gy + 1) * W <= K * H:
        gy += 1
    gx = K // gy
    if gx < 1 or gy > H or gx > W or gy * gx > MAX_LABELS:
        raise ValueError("grid %d x %d does not fit" % (gy, gx))
    return gy, gx


def slic(image, num_components, compactness=10, iters=10):
    image = np.asarray(image, dtype=np.uint8)
    H, W, _ = image.shape
    gy, gx = grid(H, W, int(num_components))
    N = gy * gx
    lab = rgb_to_lab8(image).astype(np.int64)
    S2, m2 = (H * W) // N, int(compactness) ** 2
    cy, cx = np.divmod(np.arange(N), gx)
    ceny, cenx = ((2 * cy + 1) * H) // (2 * gy), ((2 * cx + 1) * W) // (2 * gx)
    cen = np.concatenate([lab[ceny, cenx], ceny[:, None], cenx[:, None]], 1)        # [N, 5]: L a b y x
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    hy, hx = (yy * gy) // H, (xx * gx) // W
    quant = np.concatenate([lab.reshape(-1, 3), yy.reshape(-1, 1), xx.reshape(-1, 1)], 1)
    labels = np.zeros((H, W), dtype=np.int64)
    for it in range(int(iters)):
        best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
        for oy in (-1, 0, 1):                # the 3 x 3 cells in increasing label order; strict <: lowest label on a tie
            for ox in (-1, 0, 1):
                qy, qx = hy + oy, hx + ox
                ok = (qy >= 0) & (qy < gy) & (qx >= 0) & (qx < gx)
                l = np.where(ok, qy * gx + qx, 0)
                c = cen[l]
                d = (((lab - c[..., :3]) ** 2).sum(-1)) * S2 + m2 * ((yy - c[..., 3]) ** 2 + (xx - c[..., 4]) ** 2)
                take = ok & (d < best)
                best = np.where(take, d, best)
                labels = np.where(take, l, labels)
        if it == int(iters) - 1:
            break                            # the result is the last assignment
        flat = labels.reshape(-1)
        n = np.bincount(flat, minlength=N).astype(np.int64)
        for k in range(5):                   # float64 bincount sums of integers below 2^53: exact
            s = np.bincount(flat, weights=quant[:, k].astype(np.float64), minlength=N).astype(np.int64)
            cen[:, k] = np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), cen[:, k])
    return labels.astype(np.int16), N


def blocks_image(H, W, block, seed, noise=0):
    """Uniformly random coloured block x block squares (+ uniform integer noise of +-noise): (image uint8, block index map)."""
    rng = np.random.default_rng(seed)
    by, bx = H // block, W // block
    col = rng.integers(0, 256, (by, bx, 3))
    img = np.repeat(np.repeat(col, block, 0), block, 1)
    if noise:
        img = img + rng.integers(-noise, noise + 1, img.shape)
    idx = np.repeat(np.repeat(np.arange(by * bx).reshape(by, bx), block, 0), block, 1)
    return np.clip(img, 0, 255).astype(np.uint8), idx


def impure_share(labels, truth):
    """Share of pixels outside the majority block of their superpixel."""
    labels, truth = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(truth).reshape(-1).astype(np.int64)
    nt = int(truth.max()) + 1
    joint = np.bincount(labels * nt + truth, minlength=(int(labels.max()) + 1) * nt).reshape(-1, nt)
    return 1.0 - joint.max(1).sum() / labels.size

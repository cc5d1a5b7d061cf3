"""numpy restatement of the packed weight buffer of a ResNet plan and of one convolution (csrc/pack_weights.hip), written from the
layout documentation (csrc/ph_kernels.h), not from the kernel text.  Everything is a 16-bit word (bf16 or fp16
bits, `uint16`); every function returns the words together with a mask of the words a pack WRITES.

The buffer of a plan: the stem region first, then per convolution unit the forward region and then the dgrad region, NPLANES planes
of `plane = KS * KS * Cout * Cin` words each (the stem: 7 * 64 * 32).

A region of an orientation, a [tap][rows][K] matrix set (forward: rows = Cout, K = Cin; dgrad: rows = Cin, K = Cout):
  bf16      plane 0 = the bf16 rounding, row-major.  Layout "copy": plane 1 also holds the same words fragment-major,
            [tap][rows / 64][K / 64] x 4096; plane 2, and plane 1 of a "row" unit, are never written.
  bf16x6    the three planes of the split w = p0 + p1 + p2 (exact in fp32), each row-major.
  fp16x3    the half-pair blocks b = [hi * 2^11 | lo | hi], w ~= hi + lo * 2^-11, over the whole region:
            "row"   [tap][rows][K / 64][b 3][64]
            "tap5"  [tap][b 3] x 4096, fragment-major (64 x 64 only)
            "tap6"  [tap][rows / 64][K / 64][b 3] x 4096, fragment-major
Fragment-major order of a 64 x 64 (r, k) block: [k-step 2][N tile 4][lane 64][8] with r = 4 li + n, k = 32 ks + 8 lg + j,
lane = 16 lg + li.

`defect` builds one named mistake into the restatement (tests/test_pack_emulation_cpu.py shows that each changes the bytes of the
GPU test's cases): DEFECTS."""
import numpy as np

NPLANES = 3
ARITHS = {"bf16": 0, "bf16x6": 1, "fp16x3": 3}      # PH_PREC_*
DEFECTS = ("orientation", "plane_order", "hp_block_order", "frag_rk", "block2_offset", "stray_copy")
STEM_PLANE = 7 * 64 * 32


def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """The three bf16 planes of split3_bf16: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1)."""
    x = np.asarray(x, dtype=np.float32)
    p0 = bf16_bits(x)
    r1 = x - bf16_val(p0)
    p1 = bf16_bits(r1)
    p2 = bf16_bits(r1 - bf16_val(p1))
    return p0, p1, p2


def hp_blocks(x):
    """The fp16 blocks [hi * 2^11, lo, hi] of the half-pair split (hp_split): hi = fp16(x), lo = fp16((x - hi) * 2^11); |x| < 32."""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    hi2k = (hi.astype(np.float32) * np.float32(2048.0)).astype(np.float16)
    return [b.view(np.uint16) for b in (hi2k, lo, hi)]


def frag_index(r, k):
    """Position of element (r, k) of a 64 x 64 block in fragment-major order."""
    li, n = r >> 2, r & 3
    ks, lg, j = k >> 5, (k >> 3) & 3, k & 7
    return ((ks * 4 + n) * 64 + 16 * lg + li) * 8 + j


def _matrices(w, dgrad):
    """OIHW -> [tap][rows][K] of the orientation."""
    O, I, KH, KW = w.shape
    m = np.asarray(w, dtype=np.float32).reshape(O, I, KH * KW)
    return np.ascontiguousarray(m.transpose(2, 1, 0) if dgrad else m.transpose(2, 0, 1))


def _tiled_frag(R, K, nb, defect):
    """Word offset of (r, k) inside one tap of a [R / 64][K / 64][nb] x 4096 fragment-major slab set (block 0 of the nb)."""
    r, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    blk = (r >> 6) * (K >> 6) + (k >> 6)
    if defect == "block2_offset":      # blocks counted down the rows first
        blk = (k >> 6) * (R >> 6) + (r >> 6)
    f = frag_index(k & 63, r & 63) if defect == "frag_rk" else frag_index(r & 63, k & 63)
    return blk * nb * 4096 + f


def pack_conv(w, arith, dgrad, layout="row", defect=None):
    """One orientation of one convolution: (words[NPLANES * plane], written[NPLANES * plane])."""
    if defect == "orientation":
        dgrad = not dgrad
    m = _matrices(w, dgrad)
    NT, R, K = m.shape
    n = m.size
    out = np.zeros(NPLANES * n, np.uint16)
    wr = np.zeros(NPLANES * n, bool)
    tap = np.arange(NT)[:, None, None]
    if arith in ("bf16", "bf16x6"):
        assert layout in ("row", "copy") and (arith == "bf16" or layout == "row")
        planes = list(split3(m))
        if defect == "plane_order":
            planes[0], planes[1] = planes[1], planes[0]
        if arith == "bf16x6":
            out[:] = np.concatenate([p.ravel() for p in planes])
            wr[:] = True
        else:
            out[:n] = bf16_bits(m).ravel()
            wr[:n] = True
            if layout == "copy":
                idx = (n + tap * (R * K) + _tiled_frag(R, K, 1, defect)[None]).ravel()
                out[idx] = bf16_bits(m).ravel()
                wr[idx] = True
        return out, wr
    assert arith == "fp16x3" and layout in ("row", "tap5", "tap6")
    blocks = hp_blocks(m)
    if defect == "hp_block_order":
        blocks = blocks[::-1]
    r, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    if layout == "row":
        base, step = tap * (R * 3 * K) + (r * 3 * K + (k >> 6) * 192 + (k & 63))[None], 64
    elif layout == "tap5":
        assert R == 64 and K == 64
        base, step = tap * 12288 + _tiled_frag(64, 64, 3, defect)[None], 4096
    else:
        base, step = tap * (R * 3 * K) + _tiled_frag(R, K, 3, defect)[None], 4096
    for b, words in enumerate(blocks):
        idx = (base + b * step).ravel()
        out[idx] = words.ravel()
        wr[idx] = True
    return out, wr


def pack_stem(w, arith):
    """w [64][3][7][7] -> three planes [kh 7][cout 64][kw 8 x ch 4], zero padded: the split planes (bf16 and bf16x6 alike) or the
    half-pair blocks.  Every word is written."""
    v = np.zeros((7, 64, 8, 4), np.float32)
    v[:, :, :7, :3] = np.asarray(w, dtype=np.float32).transpose(2, 0, 3, 1)      # [kh][co][kw][ch]
    planes = hp_blocks(v) if arith == "fp16x3" else split3(v)
    out = np.concatenate([p.ravel() for p in planes])
    return out, np.ones(out.size, bool)


def copy_shape(rows, K, KS, fwd):
    """Perf mode: the weight shapes whose orientation carries the plane-1 copy - 3x3 with rows = K a multiple of 128 up to 512
    (conv_tap7.hip, either orientation) or, forward only, Cout = 2 Cin (conv_tap6b.hip)."""
    return KS == 3 and ((rows == K and K % 128 == 0 and 128 <= K <= 512) or (fwd and rows == 2 * K))


def plan_layouts(units, arith, tap5=True, tap6=True):
    """(forward layout, dgrad layout) of every convolution unit (Cout, Cin, KS, stride) of a plan; 3x3 units are pad 1."""
    out = []
    for (O, I, KS, S) in units:
        if arith == "bf16":
            out.append(("copy" if copy_shape(O, I, KS, True) else "row", "copy" if copy_shape(I, O, KS, False) else "row"))
        elif arith == "fp16x3":
            l1 = tap5 and KS == 3 and S == 1 and O == 64 and I == 64
            out.append(("tap5" if l1 else ("tap6" if tap6 and KS == 3 and S == 2 and O == 2 * I else "row"), "tap5" if l1 else "row"))
        else:
            out.append(("row", "row"))
    return out


def pack_network(stem_w, units, weights, arith, layouts, defect=None):
    """The packed buffer of a plan: (words, written).  units / weights / layouts: the convolution units behind the stem."""
    parts = [pack_stem(stem_w, arith)]
    for (O, I, KS, S), w, (lf, ld) in zip(units, weights, layouts):
        assert w.shape == (O, I, KS, KS)
        if defect == "stray_copy" and arith == "bf16":
            lf, ld = "copy", "copy"
        parts.append(pack_conv(w, arith, False, lf, defect))
        parts.append(pack_conv(w, arith, True, ld, defect))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- the cases of tests/test_gpu_pack.py (shared with the CPU test of the defects)

NETWORKS = [((1, 1, 1, 1), "bf16"), ((1, 1, 1, 1), "bf16x6"), ((1, 1, 1, 1), "fp16x3"), ((8, 1, 1, 1), "bf16"), ((8, 1, 1, 1), "fp16x3")]
# (name, Cin, Cout, KS, stride, pad, arithmetics); all on 8 x 8 maps, B = 1
CONVS = [("c64_64", 64, 64, 3, 1, 1, ("bf16", "bf16x6", "fp16x3")),
         ("c128_128", 128, 128, 3, 1, 1, ("bf16",)),
         ("c64_128_s2", 64, 128, 3, 2, 1, ("bf16", "fp16x3")),
         ("c64_128_1x1_s2", 64, 128, 1, 2, 0, ("bf16", "bf16x6", "fp16x3")),
         ("c192_128", 192, 128, 3, 1, 1, ("bf16",))]


def resnet_units(layers):
    """(Cout, Cin, KS, stride) of the convolution units of a BasicBlock trunk, in plan order: conv1, conv2, (downsample) per block."""
    units, inpl = [], 64
    for li, (n, pl) in enumerate(zip(layers, (64, 128, 256, 512))):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            units += [(pl, inpl, 3, s), (pl, pl, 3, 1)]
            if s != 1 or inpl != pl:
                units.append((pl, inpl, 1, s))
            inpl = pl
    return units


def random_weights(shapes, seed):
    """|w| < 32 (the half-pair range), uniform."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-31.9, 31.9, size=s).astype(np.float32) for s in shapes]

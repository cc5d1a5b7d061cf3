"""The shapes of the convolution dispatch sweep (tests/test_gpu_conv_sweep.py) and the kernel family each call reaches.

Each case sits on or just outside an eligibility predicate of ph_tapconv_select (conv_select.hip; the ph_tapconv*_eligible
functions beside the kernels).  Every map is non-square; several are odd."""
from tests.conv_emulation import BF16, BF16X6, BF16X3, FP16X3, FP16X1

# name: (Cin, Cout, IH, IW, KS, stride, pad, B)
CASES = {
    "l1": (64, 64, 10, 14, 3, 1, 1, 2),
    "l1_p0": (64, 64, 10, 13, 3, 1, 0, 2),
    "l1_s2": (64, 64, 11, 14, 3, 2, 1, 2),
    "c64_128": (64, 128, 9, 12, 3, 1, 1, 2),
    "c128_256": (128, 256, 8, 11, 3, 1, 1, 2),
    "c128_128": (128, 128, 7, 12, 3, 1, 1, 2),
    "c192_192": (192, 192, 9, 10, 3, 1, 1, 2),
    "s2_128_256": (128, 256, 9, 13, 3, 2, 1, 2),
    "s2_192_384": (192, 384, 11, 7, 3, 2, 1, 1),
    "c128_64": (128, 64, 8, 9, 3, 1, 1, 2),
    "c128_640": (128, 640, 6, 7, 3, 1, 1, 1),
    "k1_s1": (128, 256, 7, 9, 1, 1, 0, 2),
    "k1_s2": (64, 128, 9, 12, 1, 2, 0, 2),
    "k1_s2_p1": (64, 128, 9, 12, 1, 2, 1, 2),
    "s2_p0": (128, 256, 9, 12, 3, 2, 0, 2),
    # persistent families walking several tiles per workgroup
    "l1_big": (64, 64, 16, 40, 3, 1, 1, 20),
    "c128_128_big": (128, 128, 12, 20, 3, 1, 1, 20),
    "s2_128_256_big": (128, 256, 24, 18, 3, 2, 1, 20),
}

# geometries every entry point rejects (PH_EINVAL, output untouched)
REJECTED = {"k1_s2_p1", "s2_p0"}

WGRAD = {BF16: "wgrad_bf16", BF16X6: "wgrad_f32", BF16X3: "wgrad_f32", FP16X3: "wgrad_hp16", FP16X1: "wgrad_hp16"}

# (case, op) -> kernel family per arithmetic; op "fwd" or "dgrad" (dgrad_res reaches the same kernels as dgrad).  Split-plane
# arithmetics always run the first-generation float kernel.  None: the call is rejected.
_PERF_HP = {
    ("l1", "fwd"): ("tap4", "tap5"), ("l1", "dgrad"): ("tap4", "tap5"),
    ("l1_p0", "fwd"): ("tap2_l1", "gen1_hp16"), ("l1_p0", "dgrad"): ("tap2_l1", "gen1_hp16"),
    ("l1_s2", "fwd"): (None, None), ("l1_s2", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("c64_128", "fwd"): ("tap2", "gen1_hp16"), ("c64_128", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("c128_256", "fwd"): ("tap3", "tap3_hp"), ("c128_256", "dgrad"): ("tap3", "tap3_hp"),
    ("c128_128", "fwd"): ("tap7", "tap3_hp"), ("c128_128", "dgrad"): ("tap7", "tap3_hp"),
    ("c192_192", "fwd"): ("gen1_bf16", "gen1_hp16"), ("c192_192", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("s2_128_256", "fwd"): ("tap6b", "tap6"), ("s2_128_256", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("s2_192_384", "fwd"): ("tap6b", "tap6"), ("s2_192_384", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("c128_64", "fwd"): ("gen1_bf16", "gen1_hp16"), ("c128_64", "dgrad"): ("tap2", "gen1_hp16"),
    ("c128_640", "fwd"): ("gen1_bf16", "gen1_hp16"), ("c128_640", "dgrad"): ("tap3", "tap3_hp"),
    ("k1_s1", "fwd"): ("gen1_bf16", "gen1_hp16"), ("k1_s1", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("k1_s2", "fwd"): ("gen1_bf16", "gen1_hp16"), ("k1_s2", "dgrad"): ("gen1_bf16", "gen1_hp16"),
    ("l1_big", "fwd"): ("tap4", "tap5"), ("l1_big", "dgrad"): ("tap4", "tap5"),
    ("c128_128_big", "fwd"): ("tap7", "tap3_hp"), ("c128_128_big", "dgrad"): ("tap7", "tap3_hp"),
    ("s2_128_256_big", "fwd"): ("tap6b", "tap6"), ("s2_128_256_big", "dgrad"): ("gen1_bf16", "gen1_hp16"),
}


def expected_family(case, op, prec):
    """The kernel family the call reaches, None if it is rejected."""
    if case in REJECTED or (op == "fwd" and prec == FP16X1):
        return None
    if op == "wgrad":
        return WGRAD[prec]
    perf, hp = _PERF_HP[(case, op)]
    if prec == BF16:
        return perf
    if prec in (FP16X3, FP16X1):
        return hp
    return None if perf is None else "gen1_f32"

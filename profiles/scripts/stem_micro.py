"""Kernel-alone A/B of the stem backward tail on random operands: the apply pass (bf16, fp32, half-pair tensors), the unfused
weight gradient and the fused one, per library variant (libpathomic_hip<tag>.so; `_parent` = a build of the parent commit, which
has no fused form).  The launchers are reached by their C++ names.  The first kernel timed in a process reads slow: alternate.
    python3 profiles/scripts/stem_micro.py _parent "" _parent ""
"""
import ctypes, sys, os, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
vp, i32 = ctypes.c_void_p, ctypes.c_int

class W(ctypes.Structure):
    _fields_ = [("x4", vp), ("dy", vp), ("slab", vp), ("B", i32), ("IH", i32), ("IW", i32), ("OH", i32), ("OW", i32),
                ("nchunks", i32), ("tpc", i32), ("prod6", i32), ("hp", i32), ("y0", vp), ("dpool", vp), ("idx", vp),
                ("mean", vp), ("invstd", vp), ("scale", vp), ("shift", vp), ("gamma", vp), ("c1", vp), ("c2", vp),
                ("PH", i32), ("PW", i32)]

def cdiv(a, b): return (a + b - 1) // b

def run(tag, B, IH, IW, reps):
    lib = ctypes.CDLL(os.path.join(ROOT, "multimodal-learning_amd", "libpathomic_hip%s.so" % tag))
    wl = getattr(lib, "_Z20ph_stem_wgrad_launchPK11PhStemWgradiP12ihipStream_t")
    wl.argtypes = [vp, i32, vp]; wl.restype = i32
    al = getattr(lib, "_Z24ph_stem_bwd_apply_launchPKvPKhS0_PKfS4_S4_S4_S4_S4_S4_PviiiiiS4_P12ihipStream_t")
    al.argtypes = [vp] * 11 + [i32] * 5 + [vp, vp]; al.restype = i32
    g = torch.Generator(device="cuda").manual_seed(3)
    OH, OW = IH // 2, IW // 2
    PH, PW = (OH + 1) // 2, (OW + 1) // 2
    dev = "cuda"
    x4 = torch.randn(B, IH, IW, 4, device=dev, generator=g).bfloat16()
    y0 = torch.randn(B, OH, OW, 64, device=dev, generator=g).bfloat16()
    dpool = torch.randn(B, PH, PW, 64, device=dev, generator=g).bfloat16()
    idx = torch.randint(0, 9, (B, PH, PW, 64), device=dev, generator=g, dtype=torch.uint8)
    f = lambda s=1.0, o=0.0: (torch.randn(64, device=dev, generator=g) * s + o).float().contiguous()
    mean, invstd, scale, shift, gamma, c1, c2 = f(0.1), f(0.1, 1.0).abs(), f(), f(0.3), f(), f(0.01), f(0.01)
    dz = torch.full((B, OH, OW, 64), float("nan"), device=dev, dtype=torch.bfloat16)
    ntiles = B * cdiv(OH, 8) * cdiv(OW, 16)
    want = min(ntiles, 1024); tpc = cdiv(ntiles, want); nch = cdiv(ntiles, tpc)
    slab_a = torch.zeros(nch * 7 * 64 * 32, device=dev); slab_b = torch.zeros_like(slab_a)
    st = torch.cuda.current_stream().cuda_stream
    w = W(); w.x4 = x4.data_ptr(); w.dy = dz.data_ptr(); w.slab = slab_a.data_ptr()
    w.B, w.IH, w.IW, w.OH, w.OW, w.nchunks, w.tpc = B, IH, IW, OH, OW, nch, tpc
    fused = tag != "_parent"
    wf = None
    if fused:
        wf = W(); ctypes.memmove(ctypes.byref(wf), ctypes.byref(w), ctypes.sizeof(W))
        wf.dy = None; wf.slab = slab_b.data_ptr(); wf.y0 = y0.data_ptr(); wf.dpool = dpool.data_ptr(); wf.idx = idx.data_ptr()
        wf.mean, wf.invstd, wf.scale, wf.shift = mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr()
        wf.gamma, wf.c1, wf.c2, wf.PH, wf.PW = gamma.data_ptr(), c1.data_ptr(), c2.data_ptr(), PH, PW
    def apply():
        rc = al(dpool.data_ptr(), idx.data_ptr(), y0.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                gamma.data_ptr(), c1.data_ptr(), c2.data_ptr(), dz.data_ptr(), B, OH, OW, 64, 0, None, st)
        assert rc == 0, rc
    def old():
        rc = wl(ctypes.addressof(w) if tag != "_parent" else ctypes.addressof(w), 0, st); assert rc == 0, rc
    def new():
        rc = wl(ctypes.addressof(wf), 0, st); assert rc == 0, rc
    def timeit(fn):
        for _ in range(2): fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3
    t_apply = timeit(apply); t_old = timeit(old)
    if B > 8:
        y32 = torch.rand(B, OH, OW, 64, device=dev) ; dp32 = torch.rand(B, PH, PW, 64, device=dev); dz32 = torch.empty(B, OH, OW, 64, device=dev)
        for prec in (1, 3):
            def ap():
                rc = al(dp32.data_ptr(), idx.data_ptr(), y32.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                        gamma.data_ptr(), c1.data_ptr(), c2.data_ptr(), dz32.data_ptr(), B, OH, OW, 64, prec, None, st)
                assert rc == 0, rc
            print("   apply prec %d: %.1f us" % (prec, timeit(ap)), flush=True)
        del y32, dp32, dz32
    line = "lib%-8s B=%d %dx%d  apply %.1f us  wgrad %.1f us" % (tag, B, IH, IW, t_apply, t_old)
    if fused:
        t_new = timeit(new)
        torch.cuda.synchronize()
        same = torch.equal(slab_a.view(torch.int32), slab_b.view(torch.int32))
        line += "  fused %.1f us  slab bitwise equal: %s  finite: %s" % (t_new, same, bool(torch.isfinite(slab_b).all()))
    print(line, flush=True)
    return slab_a.clone()

if __name__ == "__main__":
    tags = sys.argv[1:] or [""]
    ref = {}
    for shape in ((3, 104, 80, 3), (64, 512, 512, 20)):
        for tag in tags:
            s = run(tag, *shape)
            k = shape[:3]
            if k in ref: print("   slab equals first variant's:", torch.equal(ref[k].view(torch.int32), s.view(torch.int32)), flush=True)
            else: ref[k] = s

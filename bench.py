#!/usr/bin/env python3
"""Headline benchmark: ROI-tiles/sec of one full teacher+student distillation step
(reference MICCAI-2022/train_test_path_multi_distill.py:242-330: student fwd+bwd, EMA fwd, teacher fwd,
2x KL, 2x CRD with DC-Distill selection, GK-Refine, Adam, EMA) on N MI355X GPUs of one node.

    python bench.py --gpus N --steps K --warmup W
    N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), or plainly as `python bench.py --gpus N`: with no WORLD_SIZE
    in the environment the parent starts the N replica processes itself (one per GPU, 127.0.0.1 rendezvous) BEFORE it
    touches torch or the GPU, waits for them and exits with their code - the reference's multi-GPU start is one plain
    command too (MICCAI-2022/utils.py:257-260 wraps the net in DataParallel).  If the graph-replayed run fails or hangs
    with N > 1 (RCCL calls inside HIP-graph capture), the launcher re-runs the replicas eagerly and `config.launch` says so.

Workload (BASELINE.json configs[1]): per-GPU batch 64 synthetic 512x512 ROI tiles + 320-d genomic vectors,
bf16 perf mode, README stage-2 flags, dropout 0.1 (the reference default: teacher Dropout/AlphaDropout live),
n_data = 1024 CRD bank rows.  Weak scaling: 64 tiles per GPU at every N (the top-level `value`).  Inputs are resident
in HBM before the timed region.  Prints ONE JSON line on rank 0.

A plain run does only what the headline figure needs: set-up, warm-up, the timed steps, --dump-outputs and the line,
which beside the headline value carries
  roofline.step_frac    algorithmic FLOPs of the whole step / time / dense bf16 MFMA peak (the north-star's 70 % is a
                        whole-path number), from the timed steps alone
  comm                  N > 1: what the communicator saw, from the timed steps and one all-reduce of ones
Everything that takes runs of its own is measured with --full only, after the timed steps:
  roofline.*            the dominant kernel, `all_kernels`, `step_hbm` and `hbm` (the HBM-bound CRD / optimiser /
                        BatchNorm-apply kernels against 8 TB/s) from the in-library kernel timer in 3 one-stream eager
                        steps after the graph-replayed timed region (an --eager run times the timed region itself and
                        carries them without --full)
  north_star_b256       N = 1: batch 256 on one GPU, its dominant kernel and `trunk_fwd_bwd` (the student's trunk alone)
  parity_mode           the same step in the arithmetics that meet the 1e-3 logit tolerance (N = 1), with
                        `value_tolerance_compliant`
  variants              N = 1: the MIA-2022 / MIA-2023 / t-SVD stage-1 legs (BASELINE configs[3] / configs[4])
  cpu_baseline          the CPU oracle's step; `faithful`: the reference's 3 forward + 6 backward order
  north_star_global_256 N > 1: BASELINE configs[2] / the north-star's strong-scaling point - global batch 256 split over
                        the N GPUs (32 tiles per GPU at N = 8), measured after the weak-scaling run
The --no-* switches leave single blocks of a --full run out.
  --north-star          N = 1: batch 256 on one GPU (the north-star's single-GPU roofline point) as the headline
  --dump-outputs DIR    the outputs of the last timed step as DIR/<name>.npy (seeded inputs: two builds compare 1:1)
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
CLS_NAMES = ["tapconv_kernel<bf16,S=1,BNT=64> (first generation: Cout=64 dgrad parity classes)",
             "tapconv_kernel<bf16,S=1,BNT=128> (first generation: 1x1 and dgrad parity classes, Cout>=128)",
             "tapconv_kernel<bf16,S=2> (stride-2 fwd)", "wgrad_kernel<bf16>", "stem_fwd_kernel<bf16>",
             "stem_wgrad_kernel<bf16>",
             "tapconv7_kernel (conv_tap7.hip, round 6: 3x3 stride-1 fwd+dgrad, Cin=Cout>=128, weights through a register window; PH_TAP7=0: tapconv3_kernel, conv_tap3.hip - bitwise the same outputs)",
             "tapconv4_kernel (conv_tap4.hip: 3x3 stride-1 fwd+dgrad, Cin=Cout=64: layer 1; one wave per SIMD, 16x16x32 fragments, resident weights, epilogue inside the next tile; PH_TAP4=0: tapconv2_l1_kernel)"]
NCLS = len(CLS_NAMES)
# ... + class 12 of ph_kernels.h (behind the four HBM-bound classes 8-11)
MASKED_CLS, MASKED_NAME = 12, "tapconv2_kernel<2,2,4,false,masked> (3x3 stride-2 fwd as a masked grid over the 4 pixel-parity planes)"
FUSED_CLS = [(13, "tapconv3_kernel<fused input> + input BatchNorm/ReLU applied in LDS (conv2 of layer 2, forward-only networks)"),
             (14, "tapconv4_kernel<fused input> + input BatchNorm/ReLU applied in LDS (layer 1, forward-only networks)")]
HBM_NAMES = ["crd_score_kernel (2 banks x B x 1000 rows of 512 B)", "crd_loss_grad_kernel (2 banks x B x 532 rows of 512 B)",
             "adam_ema_dev_kernel (28 B / parameter + 8 B / EMA parameter)", "bn_apply_kernel (2-3 activation tensors)"]
TOPK_CLS = 15                    # ph_kernels.h PH_CLS_CRD_TOPK
NALL = 16                        # = PH_NCLS
HBM_PEAK_GBS = 8000.0            # HBM3E peak (6290 GB/s measured with a float4 copy), same guide
# algorithmic FLOPs of the step per 512x512 tile: 3 ResNet-18 forwards + 1 backward without the image gradient
# (SURVEY 8-d layer table: 93.52 GFLOP); convolutions scale with the tile area
STEP_GFLOP_PER_TILE_512 = 93.52
# one network's ResNet(+heads) forward + backward alone - the denominator of the north-star's ">= 70 % bf16 MFMA roofline on the
# ResNet+fusion forward/backward at batch 256" (27.81 GMAC = 55.62 GFLOP per 512x512 tile, 14.24 TFLOP at B = 256)
TRUNK_FWD_BWD_GFLOP_PER_TILE_512 = 55.62


def trunk_fwd_bwd(m, B, H, device, steps=5):
    """The literal north-star quantity: the student's ResNet-18 + heads forward and backward ALONE at batch
    B, graph-replayed (two eager passes, one capture, `steps` timed replays), bf16.  Returns a dict for the bench line."""
    import torch
    m.set_precision("bf16")
    opt = m.stage2_opt(dropout_rate=0.0, batch_size=B)
    torch.manual_seed(1)
    net = m.define_net(opt, 1, path_only=True).to(device)
    net.train()
    if os.environ.get("PH_TRUNK_NO_OVERLAP") == "1":      # A/B switch: the whole backward on one stream
        net._no_bwd_overlap = True
    x = torch.randn(B, 3, H, H, device=device).clamp_(-1, 1)
    w = torch.linspace(0.5, 1.5, 128, device=device)

    def body():
        _, feat, hazard, pred, _ = net(x_path=x)
        loss = (feat * w).sum() + hazard.sum()
        loss.backward()
        return loss
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for p_ in net.parameters():
                p_.grad = None
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p_ in net.parameters():
        p_.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = body()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    lv = float(loss.detach())
    gn = float(sum(p_.grad.float().abs().sum() for p_ in net.parameters() if p_.grad is not None))
    if not (lv == lv and gn == gn and gn > 0):
        raise RuntimeError("trunk_fwd_bwd: non-finite loss / gradients (%r, %r)" % (lv, gn))
    tfl = TRUNK_FWD_BWD_GFLOP_PER_TILE_512 * (H / 512.0) ** 2 * B / 1e3
    net.release_workspaces()
    del g, net, x
    torch.cuda.empty_cache()
    return {"workload": "student ResNet-18 + heads forward + backward alone, batch %d, %dx%d, bf16, one captured HIP graph "
                        "(BASELINE.json north_star: 'ResNet+fusion forward/backward at batch 256 on 1 MI355X')" % (B, H, H),
            "steps": steps, "ms": round(1000.0 * dt, 3), "tiles_per_s": round(B / dt, 1),
            "algorithmic_tflop": round(tfl, 3), "achieved": round(tfl / dt, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tfl / dt / MFMA_BF16_PEAK_TFLOPS, 4), "target_frac": 0.70,
            "profile": "profiles/r06_kernel_stats_trunk_b256.txt (rocprofv3 --kernel-trace --stats -- python3 bench.py --trunk-only)"}


def hbm_ledger(B, H, es=2):
    """Algorithmic HBM bytes of ONE distillation step in perf mode, tensor by tensor, as the data flow of csrc/resnet_plan.hip
    defines it (every tensor a launch must read or write counted once per launch; weights, BatchNorm vectors and the heads /
    losses / optimiser are listed separately).  `es` = bytes per activation element (2 in perf mode).  Train-mode BatchNorm
    needs the batch statistics of a whole conv output before any consumer can normalise it, so every conv output is written
    raw and read again - that, not the convolutions, is what makes the step HBM-heavy.  Returns {category: bytes}."""
    led = {}

    def add(k, v):
        led[k] = led.get(k, 0.0) + float(v)
    OH = H // 2
    P = OH // 2
    act = lambda c, h: B * c * h * h * es      # noqa: E731
    layers = [(64, 64, P, 1), (64, 128, P // 2, 2), (128, 256, P // 4, 2), (256, 512, P // 8, 2)]      # Cin, Cout, OH, stride of block 0
    wbytes = 0
    for net in ("student", "ema", "teacher"):
        train = net == "student"
        if net != "teacher":
            add("pack_input", B * 3 * H * H * 4 + B * H * H * 4 * es)      # the student and the teacher share one packed image
        x4 = B * H * H * 4 * es
        if train:
            add("stem conv", x4 + act(64, OH))
            add("stem bn+relu+maxpool", act(64, OH) + act(64, P) * 2 + B * 64 * P * P)      # + arg codes (1 B) + conv output at the arg-max
        else:
            add("stem conv with pooled epilogue", x4 + act(64, P))
        for li, (cin, cout, oh, stride) in enumerate(layers):
            ih = oh * stride
            for bi in range(2):
                c_in = cin if bi == 0 else cout
                h_in = ih if bi == 0 else oh
                add("conv forward (in + out)", act(c_in, h_in) + act(cout, oh))                    # conv1
                fused_a1 = (not train) and cout <= 128
                if not fused_a1:
                    add("bn_apply a1", 2 * act(cout, oh))
                add("conv forward (in + out)", 2 * act(cout, oh))                                 # conv2
                if bi == 0 and stride == 2:
                    add("conv forward (in + out)", act(c_in, h_in) / 4 + act(cout, oh))           # 1x1 / 2 downsample
                add("bn_apply block output", 3 * act(cout, oh))                                   # y2 + shortcut -> out
        add("avgpool", act(256, P // 4) + act(512, P // 8))
    # student backward
    for li, (cin, cout, oh, stride) in enumerate(layers):
        ih = oh * stride
        for bi in range(2):
            c_in = cin if bi == 0 else cout
            h_in = ih if bi == 0 else oh
            a, ai = act(cout, oh), act(c_in, h_in)
            add("bn backward (reduce + apply)", 3 * a + 4 * a)                                    # bn2: g, out, y2 | + dz
            add("conv wgrad (x + dz + slab)", 2 * a + 2 * 37.7e6)
            add("conv dgrad (dz + dx [+ residual])", 2 * a)
            add("bn backward (reduce + apply)", 2 * a + 3 * a)                                    # bn1: mask re-derived from y1
            add("conv wgrad (x + dz + slab)", ai + a + 2 * 37.7e6)
            add("conv dgrad (dz + dx [+ residual])", a + ai + (2 * ai if not (bi == 0 and stride == 2) else 0))
            if bi == 0 and stride == 2:
                add("bn backward (reduce + apply)", 3 * a + 4 * a)
                add("conv wgrad (x + dz + slab)", ai / 4 + a + 2 * 37.7e6 / 9)
                add("conv dgrad (dz + dx [+ residual])", a + 2 * ai)
    add("avgpool backward", act(512, P // 8) + 2 * act(256, P // 4))
    add("stem backward (pool scatter + bn + wgrad)", 2 * act(64, P) * 2 + B * 64 * P * P * 4 + 2 * act(64, OH) + act(64, OH) + B * H * H * 4 * es + 2 * 29e6)
    nparam = 11.18e6 + 0.05e6
    add("weights: packing (3 networks x fwd + student dgrad layouts)", 3 * nparam * 4 + (3 + 1) * nparam * 2 + 4 * nparam * 2 * 2)
    add("adam + ema (28 B + 8 B per parameter)", nparam * 36)
    add("heads, fusion, losses, CRD bank rows (n_data 1024)", 2 * 2 * B * 1000 * 512 + 2 * 2 * B * 532 * 512 + 30e6)
    return led


def _counter_step_gb():
    """HBM bytes of one whole step from the PMC counters (profiles/summarize.py writes `step_total_bytes` into the traffic file)."""
    for tname in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json"):
        tf = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tf):
            try:
                v = json.load(open(tf)).get("step_total_bytes")
                return None if v is None else round(v / 1e9, 2)
            except Exception:
                return None
    return None


def make_batch(B, H, n_data, opt, device, seed):
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(1234 + seed)
    x_path = torch.rand(B, 3, H, H, generator=g) * 2 - 1
    ema_x_path = x_path + 0.01 * torch.randn(B, 3, H, H, generator=g)
    x_omic = torch.randn(B, opt.input_size_omic, generator=g)
    grade = torch.randint(0, 3, (B,), generator=g)
    index = torch.randperm(n_data, generator=g)[:B]
    sample_idx = torch.randint(0, n_data, (B, opt.nce_p + opt.nce_k), generator=g)
    sample_idx[:, 0] = index
    z = torch.zeros(B)
    d = lambda t: t.to(device)
    return ((d(x_path), d(ema_x_path)), d(z), d(x_omic), d(z), d(z), d(grade), d(index), d(sample_idx))


def cpu_baseline(nsteps=10, faithful_steps=3, like_steps=2):
    """The CPU oracle (a port of the reference's algorithm, pinned to it by tests/test_oracle_golden.py) timed on
    this host for BASELINE config 1 (B=16, 224x224), 3 fwd + 1 bwd ("minimal") mode.  Threads are capped at 16:
    at B=16 torch's CPU kernels stop scaling there (with all 256 host threads of the GPU box the same step takes
    ~80x longer from oversubscription; the reference's own driver caps at 4, train_cv_path_multi_MT.py:2-4)."""
    import torch
    from oracle.step import DistillOracle, default_opt, synthetic_batch
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    orc = DistillOracle(default_opt(), seed=0, n_data=1024)
    bt = synthetic_batch(16, 224, seed=0)
    orc.step(bt)   # warm-up
    t0 = time.time()
    for i in range(nsteps):
        orc.step(synthetic_batch(16, 224, seed=1 + i))
    dt = (time.time() - t0) / nsteps
    res = {"value": round(16.0 / dt, 3), "unit": "tiles/s", "cores": cores, "kind": "port",
           "sample": f"{nsteps} distill steps of BASELINE config 1 (B=16, 224x224, 320-d omic, fp32, 3 fwd + 1 bwd), "
                     f"{dt:.2f} s/step after 1 warm-up; NOT comparable per tile with the GPU figure (224x224 fp32 tiles "
                     f"against 512x512 bf16 tiles: 5.2x the FLOPs each)"}
    if like_steps > 0:
        # the GPU workload's tile size on the CPU: B = 16 tiles of 512 x 512 (5.2x the FLOPs of a 224 x 224 tile), same step
        orc.step(synthetic_batch(16, 512, seed=70))
        t0 = time.time()
        for i in range(like_steps):
            orc.step(synthetic_batch(16, 512, seed=71 + i))
        dtl = (time.time() - t0) / like_steps
        res["like_for_like"] = {"value": round(16.0 / dtl, 3), "unit": "tiles/s", "cores": cores,
                                "sample": f"{like_steps} distill steps at the GPU workload's tile size (B=16, 512x512, fp32, 3 fwd + 1 bwd), "
                                          f"{dtl:.2f} s/step after 1 warm-up: comparable per tile with the headline value"}
    if faithful_steps > 0:
        # what the reference executes: AEKD_loss runs one FULL backward per loss (train_test_path_multi_distill.py:49-56),
        # 3 forwards + 6 backwards per step for the same numbers
        t0 = time.time()
        for i in range(faithful_steps):
            orc.step(synthetic_batch(16, 224, seed=50 + i), faithful=True)
        dtf = (time.time() - t0) / faithful_steps
        res["faithful"] = {"value": round(16.0 / dtf, 3), "unit": "tiles/s",
                           "sample": f"{faithful_steps} steps in the reference's own execution order (3 fwd + 6 bwd), {dtf:.2f} s/step"}
    return res


def variant_setup(name, B, H, device, rank=0, sync=None, generic_head=False):
    """The other stage-2 bodies / the stage-1 t-SVD trainer at BASELINE sizes (configs[3] / configs[4], single-GPU legs):
    "mia2022": MIA-2022 stage 2, vanilla K+1 CRD bank with nce_k 4096 (bank 16 384 rows), momentum GK-Refine;
    "mia2023": MIA-2023 stage 2 = configs[4]: n_data 65 536 bank rows, nce_k 4096, nce_p 6 class-aware KNN positives
               (the full-bank cosine scan of CRD_criterion_v10.py:45-176), per-sample GK-Refine;
    "tsvd":    MIA-2022 stage-1 trainer with the t-SVD low-rank term (train_test_tSVD.py:299-431) = configs[3].
    Returns (step object, [batch, batch], description)."""
    import numpy as np
    import torch
    import multimodal_learning_amd as m
    g = torch.Generator().manual_seed(4321 + rank)
    d = lambda t: t.to(device)      # noqa: E731

    def batch(n_data, K, labels=None):
        x = torch.rand(B, 3, H, H, generator=g) * 2 - 1
        index = torch.randperm(n_data, generator=g)[:B]
        sidx = torch.randint(0, n_data, (B, K + 1), generator=g); sidx[:, 0] = index
        grade = labels[index] if labels is not None else torch.randint(0, 3, (B,), generator=g)
        z = torch.zeros(B)
        return ((d(x), d(x + 0.01 * torch.randn(B, 3, H, H, generator=g))), d(z), d(torch.randn(B, 320, generator=g)), d(z), d(z),
                d(grade), d(index), d(sidx))
    if name == "mia2022":
        opt = m.stage2_opt(dropout_rate=0.1, batch_size=B)
        opt.nce_k, opt.grads_m, opt.grads_thresh, opt.thresh = 4096, 0.9, "False", 0.1
        opt.fused_loss_head = not generic_head
        n_data = 16384
        step = m.DistillStep(opt, n_data, device=device, variant="mia2022", sync=sync)
        desc = "MIA-2022 stage 2 (train_test_path_multi_distill_v2.py): CRD bank %d rows, nce_k 4096, momentum GK-Refine" % n_data
        bts = [batch(n_data, 4096) for _ in range(2)]
    elif name == "mia2023":
        n_data = 65536
        nce_k = int(os.environ.get("PH_BENCH_NCE_K", "4096"))      # 65536 = the other reading of configs[4] (SURVEY 8-e assumption (i))
        labels = torch.arange(n_data) % 3
        opt = m.stage2_opt(dropout_rate=0.1, batch_size=B)
        for k, v in dict(nce_k=nce_k, nce_p=6, pos_extra="neighbors", neg_mode="all_others", start_reweight=0, discrep_scale=1,
                         max_discrep=2.0, use_grads_thresh="True", grads_thresh=0.0, loss_weighting="GK_refine").items():
            setattr(opt, k, v)
        opt.fused_loss_head = not generic_head
        cls = [np.nonzero((labels == c).numpy())[0] for c in range(3)]
        step = m.DistillStep(opt, n_data, device=device, variant="mia2023", train_class_idx=cls, sync=sync)
        desc = ("BASELINE configs[4] single-GPU leg: MIA-2023 stage 2, CRD bank %d rows (full-bank class-masked cosine KNN, "
                "nce_p 6), nce_k %d, per-sample GK-Refine" % (n_data, nce_k))
        bts = [batch(n_data, nce_k, labels) for _ in range(2)]
    elif name == "tsvd":
        opt = m.stage2_opt(dropout_rate=0.1, batch_size=B, cut_fuse_grad=True, num_teachers=2)
        opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss = 1, 1.0, 0, 0, "False"
        # "MIA 2022/options.py":13-21 defaults (n_views 4, Lambda_global 0.05, pho 1.1, max_mu 1) with mu started at 1e-2 so that
        # the soft threshold Lambda / mu does not zero every singular value (a warm run's regime)
        opt.tSVD_loss, opt.n_views, opt.tSVD_mode, opt.mu, opt.pho, opt.max_mu = "True", 4, "pathomic", 1e-2, 1.1, 1.0
        opt.Lambda_global, opt.aux_iter = 0.05, 1
        step = m.TeacherStage1Step(opt, device=device, sync=sync)
        desc = ("BASELINE configs[3] single-GPU leg: MIA-2022 stage-1 trainer with the t-SVD term (train_test_tSVD.py), %d tiles, "
                "4 views, auxiliary update every batch" % B)
        bts = [make_batch(B, H, 1024, opt, device, seed=rank * 100 + 31 + i) for i in range(2)]
    else:
        raise SystemExit("unknown variant %r" % name)
    for c in (getattr(step, "criterion_kd", None), getattr(step, "criterion_kd_path", None)):
        if c is not None:
            c.contrast.verbose = False
    return step, bts, desc


def run_variant(name, B, H, device, L, steps=5, nce_k=None):
    """5 steps of one variant with resident inputs (graph replay for the stage-2 bodies), then 2 eager steps under the
    in-library event timer for the CRD kernels' achieved GB/s.  Returns the `variants[name]` object of the JSON line.
    nce_k (mia2023): the other reading of configs[4] - 65 536 NEGATIVES per query over the 65 536-row bank (SURVEY 8-e
    assumption (i)); CRDLoss then takes the negatives' terms in bank-scan form (CL_utils/memory_new.py: _crd_core_scan)."""
    import torch
    import multimodal_learning_amd as m
    saved = os.environ.get("PH_BENCH_NCE_K")
    if nce_k is not None:
        os.environ["PH_BENCH_NCE_K"] = str(nce_k)
    try:
        step, bts, desc = variant_setup(name, B, H, device)
    finally:
        if nce_k is not None:
            if saved is None:
                del os.environ["PH_BENCH_NCE_K"]
            else:
                os.environ["PH_BENCH_NCE_K"] = saved
    graph = hasattr(step, "enable_graph")
    if graph:
        step.enable_graph()
    for i in range(4):
        step.step(bts[i % 2], epoch=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step.step(bts[i % 2], epoch=5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    graph = graph and bool(getattr(step, "_want_graph", False))      # (a failed capture falls back to eager launches and says so)
    res = {"workload": desc, "tiles_per_gpu": B, "steps": steps, "ms_per_step": round(1000.0 * dt / steps, 3),
           "value": round(B * steps / dt, 2), "unit": "tiles/s", "final_loss": round(float(out["loss"]), 4),
           "launch": "one captured HIP graph per step" if graph else "eager"}
    if name == "tsvd":
        res["parity"] = ("adjacency / penalty / mu-schedule and the proximal operator pinned (reference goldens, float64 SVD at 2e-5); "
                         "`update_aux` itself UNPINNED: the reference imports it from my_utils/, which is absent from the repository "
                         "(MIA 2022/train_test_tSVD.py:31) - restated from its call site :382-391")
    if nce_k is not None:
        n_rows = 65536
        res["crd_form"] = ("bank-scan: scores = [B,128] x [128,%d] per bank (2 x %.1f MB of bank rows read once per GEMM), multiplicity "
                           "weights [B,%d] int32; the gathered kernels would read 2 banks x B x %d rows x 512 B = %.2f GB per pass (same-box "
                           "A/B PH_CRD_SCAN=0: 14.5 against 12.0 ms per step, profiles/EXPERIMENTS.md round 5)"
                           % (n_rows, n_rows * 512 / 1e6, n_rows, nce_k, 2.0 * B * nce_k * 512 / 1e9))
        graph = False      # (no per-kernel table for this leg)
    if graph:
        step._want_graph = False
        step._side_stream = None
        step.step(bts[0], epoch=5)
        L.ph_prof_reset(); L.ph_prof_enable(1)
        for i in range(2):
            step.step(bts[i % 2], epoch=5)
        torch.cuda.synchronize()
        L.ph_prof_enable(0)
        buf = (ctypes.c_double * (4 * NALL))()
        L.ph_prof_summary4(buf, NALL)
        traffic = {}
        for tname in ("r06_crd_traffic.json", "r05_crd_traffic.json", "r04_crd_traffic.json", "r03_crd_traffic.json"):      # (the newest committed counter pass)
            tf = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tf):
                traffic = json.load(open(tf)).get(name, {})
                break
        rows = []
        for cls, key, nm in ((8, "crd_score", "crd_score_kernel: 2 banks x B x (P+K) rows of 512 B"),
                             (TOPK_CLS, "crd_bank_topk", "ph_crd_bank_topk = 4 launches (sample pass, threshold, full pass, merge) under ONE event pair in eager steps, launch gaps included; kernel durations alone: profiles/r06_kernel_stats_mia2023.txt; 2 banks x n_data rows of 512 B, each once (+ 1/16 in the sample pass)"),
                             (9, "crd_loss_grad", "crd_loss_grad_kernel (+ reduce): 2 banks x B x (P2+K2) rows of 512 B")):
            n, ms, by = buf[4 * cls], buf[4 * cls + 1], buf[4 * cls + 2]
            if n == 0:
                continue
            gbs = by / (ms * 1e-3) / 1e9
            row = {"kernel": nm, "launches": int(n), "avg_launch_us": round(1000.0 * ms / n, 2),
                   "algorithmic_mb_per_launch": round(by / n / 1e6, 2), "achieved_gbs": round(gbs, 1), "peak_gbs": HBM_PEAK_GBS,
                   "frac": round(gbs / HBM_PEAK_GBS, 4)}
            t = traffic.get(key)
            if t:   # counter bytes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes) and the rate they give
                row["traffic"] = t["bytes_per_launch"]
                row["traffic_gbs"] = round(t["bytes_per_launch"] / (1000.0 * ms / n) / 1e3, 1)
                row["traffic_frac"] = round(row["traffic_gbs"] / HBM_PEAK_GBS, 4)
            rows.append(row)
        res["crd_hbm"] = rows
    for attr in ("model", "ema_model"):
        mod = getattr(step, attr, None)
        for sub in (mod.modules() if mod is not None else ()):
            if hasattr(sub, "release_workspaces"):
                sub.release_workspaces()
    fm = getattr(step, "fix_model", None)
    if fm is not None:
        fm.path_net.release_workspaces()
    del step, bts
    torch.cuda.empty_cache()
    return res


def measure(step, batches, steps, warmup, sync, device, graph=True, loader=False):
    """W untimed steps (>= 3 when the step is replayed from a HIP graph: two eager ones, one that captures), then
    exactly K timed steps between barrier + synchronize pairs; max over ranks.  Returns (seconds, last outputs)."""
    import torch
    if graph:
        step.enable_graph()          # steps 0-1 run eagerly, step 2 captures, later steps replay one HIP graph
    for i in range(max(warmup, 3 if graph else 0)):
        step.step(batches[i % 2], epoch=1)
    if graph and not loader:
        # the two resident batches are adopted in place as the graph's input sets (no staging copy); the second set's
        # graph is captured here - capture executes nothing - so that the timed region only replays
        step.precapture(batches[1], epoch=1)
    _flush_c_stdio()      # every rank: whatever native libraries printed while the communicators came up goes out NOW
    return step, batches


def _flush_c_stdio():
    """Flush the C library's stdio buffers (output of native libraries, e.g. RCCL's banner, is block-buffered when stdout is a
    pipe and would otherwise appear at process exit, after the JSON line)."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def timed(step, batches, steps, sync, device):
    import torch
    if sync is not None:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for i in range(steps):
        out = step.step(batches[i % 2], epoch=1)
    torch.cuda.synchronize()
    if sync is not None:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if sync is not None:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = t.item()
    return dt, out


DUMP_BUDGET_BYTES = 64 << 20
DUMP_MAX_ELEMENTS = 1 << 20      # larger arrays are dumped as a fixed seeded sample of this many elements


def snapshot_outputs(out):
    """The arrays the timed step handed its caller (`out` of its last timed step), copied to host memory NOW - a graph-replayed
    step returns its static output buffers, which later steps overwrite.  {name: float32 array, float64 for float64 and
    integer tensors}; a list / tuple entry becomes name_0, name_1, ...; None entries are left out."""
    import numpy as np
    import torch
    flat = {}

    def add(name, v):
        if isinstance(v, torch.Tensor):
            flat[name] = v
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                add("%s_%d" % (name, i), x)
        elif isinstance(v, (int, float)) and not isinstance(v, bool):
            flat[name] = torch.tensor(float(v), dtype=torch.float64)
    for k in sorted(out):
        add(k, out[k])
    res = {}
    for name, t in sorted(flat.items()):
        t = t.detach()
        t = t.to(torch.float64) if (t.dtype == torch.float64 or not t.is_floating_point()) else t.to(torch.float32)
        t = t.reshape(-1) if t.numel() > DUMP_MAX_ELEMENTS else t
        if t.numel() > DUMP_MAX_ELEMENTS:
            g = torch.Generator().manual_seed(0)
            idx = torch.randperm(t.numel(), generator=g)[:DUMP_MAX_ELEMENTS].sort().values
            t = t[idx.to(t.device)]
        res[name] = t.cpu().numpy().copy()
    total = sum(a.nbytes for a in res.values())
    if total > DUMP_BUDGET_BYTES:
        raise SystemExit("--dump-outputs: %d bytes of outputs exceed the %d-byte budget" % (total, DUMP_BUDGET_BYTES))
    return res


def write_outputs(arrays, d):
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)
    print("bench: wrote %d outputs of the last timed step (%d bytes) to %s" % (len(arrays), sum(a.nbytes for a in arrays.values()), d),
          file=sys.stderr, flush=True)


def launch_replicas(n, argv, timeout_s=None):
    """`python bench.py --gpus N` without a launcher: start N replica processes of this script (rank r on GPU r), wait,
    return their exit code.  Runs before torch is imported, so the parent never initialises the GPU.  Attempt 1 replays
    the step from a HIP graph (RCCL calls captured inside); if any replica fails or the attempt exceeds the time limit
    the replicas are killed by PID and attempt 2 runs eagerly (PH_BENCH_LAUNCH tells the children what to report)."""
    import socket
    import subprocess
    timeout_s = timeout_s or float(os.environ.get("PH_BENCH_LAUNCH_TIMEOUT", "300"))
    attempts = [("self-launched", [])]
    if "--eager" not in argv:
        attempts.append(("self-launched, eager fallback (the graph-replayed attempt failed or timed out)", ["--eager"]))
    rc = 1
    for note, extra in attempts:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PH_BENCH_LAUNCH=note)
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + extra, env=env))
        t0 = time.time()
        rc = None
        while rc is None:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes):
                rc = next(c for c in codes if c not in (None, 0))
            elif all(c == 0 for c in codes):
                rc = 0
            elif time.time() - t0 > timeout_s:
                rc = 124
                print("bench launcher: %d replicas exceeded %.0f s" % (n, timeout_s), file=sys.stderr, flush=True)
            else:
                time.sleep(0.2)
        for p in procs:                # exact PIDs this function started, nothing by pattern
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        if rc == 0:
            return 0
        print("bench launcher: attempt '%s' ended with code %s" % (note, rc), file=sys.stderr, flush=True)
    return rc


def stub_main(args):
    """Testing aid (tests/test_dist_gloo.py): the launcher + rendezvous + timing protocol of this file on CPU with
    the gloo backend and a stand-in step (one small matmul + an all-reduce).  Its JSON line says "stub"."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("PH_BENCH_STUB_FAIL_GRAPH") and not args.eager and rank == world - 1:
        raise SystemExit(7)            # stands for "RCCL inside graph capture failed on one replica"
    if world > 1:
        dist.init_process_group(backend="gloo")
    x = torch.ones(64, 64)

    def one():
        y = (x @ x).sum().reshape(1)
        if world > 1:
            dist.all_reduce(y)
        return y
    for _ in range(args.warmup):
        one()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = one()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    comm = None
    if world > 1:
        sys.path.insert(0, os.path.join(ROOT, "multimodal-learning_amd"))
        import importlib.util
        spec = importlib.util.spec_from_file_location("ph_dist", os.path.join(ROOT, "multimodal-learning_amd", "dist.py"))
        pd = importlib.util.module_from_spec(spec); spec.loader.exec_module(pd)
        comm = pd.comm_report(pd.ReplicaSync(), None, "gloo")      # every rank takes part
        comm["launch"] = os.environ.get("PH_BENCH_LAUNCH", "external launcher")
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": round(args.batch * world * args.steps / dt, 2), "unit": "tiles/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "data": "stub",
                          "sum": y.item(), "comm": comm,
                          "config": {"workload": "launcher self-test (CPU, gloo, stand-in step)",
                                     "launch": os.environ.get("PH_BENCH_LAUNCH", "external launcher")}}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="tiles per GPU")
    ap.add_argument("--device-loader", action="store_true",
                    help="also run the input pipeline inside the timed region: every step's batch is produced on the device "
                         "from resident uint8 source tiles (shuffle, flip/crop/colour jitter x 2 views, contrast indices), "
                         "captured in the same HIP graph as the step - NOT the default metric, whose inputs are resident "
                         "when the timed region starts")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--north-star", action="store_true",
                    help="N = 1: batch 256 on one GPU - the single-GPU roofline point of the north-star (BASELINE.json)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beside the headline figure: per-kernel rooflines, "
                         "north_star_b256, parity_mode, variants, cpu_baseline, north_star_global_256 (N > 1)")
    ap.add_argument("--no-parity-mode", action="store_true", help="--full: skip the extra parity-arithmetic measurements")
    ap.add_argument("--no-north-star-block", action="store_true", help="--full: skip the extra batch-256 single-GPU measurement (`north_star_b256`)")
    ap.add_argument("--no-strong", action="store_true", help="--full, N > 1: skip the extra global-batch-256 (configs[2]) measurement")
    ap.add_argument("--strong-batch", type=int, default=0,
                    help="testing aid (--full): run the extra strong-scaling measurement with this many tiles per GPU whatever N is")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-kernel-timer", action="store_true",
                    help="no in-library kernel timer (--full: the eager steps after the timed region; --eager: the timed region)")
    ap.add_argument("--eager", action="store_true", help="do not replay the step from a captured HIP graph")
    ap.add_argument("--generic-loss-head", action="store_true",
                    help="A/B: per-loss autograd graphs + GK-Refine by five small backward passes instead of loss_head.py")
    ap.add_argument("--no-masked", action="store_true",
                    help="A/B switch: first-generation kernel for the 3x3 stride-2 convolutions (not the masked tap grid)")
    ap.add_argument("--no-fuse", action="store_true",
                    help="A/B: separate bn_apply passes in the forward-only networks instead of the in-LDS BatchNorm + ReLU")
    ap.add_argument("--no-head-overlap", action="store_true",
                    help="A/B switch: the fused loss head on one stream (second CRD chain and head weight gradients not on a side stream)")
    ap.add_argument("--teacher-streams", type=int, default=2,
                    help="A/B switch: 1 = the fused teacher's forward behind the mean teacher's on one side stream (round 2)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "bf16x6/x3", "bf16x6", "fp16x3", "fp16x3/x1"],
                    help="arithmetic of the headline run (default: the perf mode BASELINE configs[1] names); the split-plane "
                         "modes are what `parity_mode` reports - this flag exists to profile them")
    ap.add_argument("--serial", action="store_true",
                    help="everything on ONE stream (no teacher streams, no side-stream weight gradients): the command "
                         "profiles/collect.sh traces for per-kernel durations - with the streams on, a launch's wall "
                         "duration includes time it shares the chip with other kernels")
    ap.add_argument("--no-bwd-overlap", action="store_true",
                    help="A/B switch: the student's backward on one stream (weight gradients not on the side stream)")
    ap.add_argument("--no-stem-pool", action="store_true",
                    help="A/B: separate stem conv + BatchNorm/ReLU/max-pool passes in the forward-only networks instead of "
                         "the stem kernel with the pooled epilogue")
    ap.add_argument("--force-dist", action="store_true", help="initialise RCCL and run the replica-sync code path even "
                    "with one rank (exercises the collectives inside graph capture on a 1-GPU box)")
    ap.add_argument("--variant", default="miccai2022", choices=["miccai2022", "mia2022", "mia2023", "tsvd"],
                    help="run another batch body as the measured step (profiling aid; the --full line carries "
                         "5-step figures of all three in `variants`)")
    ap.add_argument("--no-variants", action="store_true", help="--full: skip the `variants` block (configs[3] / configs[4] legs)")
    ap.add_argument("--stub-step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--grad-exchange", default="all_reduce", choices=["all_reduce", "reduce_scatter"],
                    help="N > 1: the gradient sum as bucketed all-reduce (default) or reduce-scatter + all-gather per bucket (A/B)")
    ap.add_argument("--trunk-only", action="store_true",
                    help="only the north-star's literal quantity: student ResNet forward + backward alone at batch 256 (profiling aid)")
    ap.add_argument("--no-trunk-block", action="store_true", help="skip `north_star_b256.trunk_fwd_bwd`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (losses, logits, features, GK-Refine "
                         "weights) as DIR/<name>.npy, float32 / float64, rank 0's; the inputs are seeded, so two builds can be "
                         "compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.trunk_only:
        ap.error("--dump-outputs covers the distillation step; --trunk-only has no step outputs to write")
    if args.north_star:
        args.batch = 256
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher in the command line: be the launcher (nothing has touched torch or the GPU yet)
        raise SystemExit(launch_replicas(args.gpus, sys.argv[1:]))
    if args.stub_step:
        raise SystemExit(stub_main(args))

    import numpy as np
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d does not match WORLD_SIZE=%d of the launcher" % (args.gpus, world))
    ext_eager = False
    if world > 1 and "PH_BENCH_LAUNCH" not in os.environ and not args.eager and not os.environ.get("PH_BENCH_DDP_GRAPH"):
        # Replicas started by an EXTERNAL launcher (torch.distributed.run): eager launches.  A graph capture that fails (an
        # RCCL call that cannot be captured on this stack) leaves the HIP streams in capture state for the rest of the process
        # (tests/probe_capture_fallback_gpu.py) - `python bench.py --gpus N` recovers by restarting its replicas eagerly, a rank
        # of someone else's launcher cannot.  Eager costs ~2 % at N = 1 (11.97 against 11.73 ms); PH_BENCH_DDP_GRAPH=1 opts in.
        args.eager = True
        ext_eager = True
    if os.environ.get("PH_BENCH_ONE_GPU"):
        local_rank = 0     # testing aid: every replica on GPU 0 (with PH_BENCH_BACKEND=gloo: RCCL refuses two ranks on one device)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    import multimodal_learning_amd as m
    sync = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        backend = os.environ.get("PH_BENCH_BACKEND", "nccl")
        # collectives inside captured graphs: the watchdog's asynchronous error handling must not touch the streams (torch's own
        # recipe for whole-network capture with a process group)
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
        if world == 1 and "RANK" not in os.environ:      # --force-dist straight from a shell: a one-rank group of its own
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device)
        else:
            dist.init_process_group(backend=backend)
        sync = m.dist.ReplicaSync(grad_exchange=args.grad_exchange)
    if args.trunk_only:
        r = trunk_fwd_bwd(m, 256 if args.batch == 64 else args.batch, args.size, device, steps=max(args.steps, 5))
        print(json.dumps({"metric": "student ResNet forward+backward alone", "value": r["tiles_per_s"], "unit": "tiles/s", "n_gpus": 1,
                          "steps": r["steps"], "warmup": 3, "ms_per_step": r["ms"], "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "bf16", "data": "synthetic", "config": {"workload": r["workload"]},
                          "roofline": {"bound": "mfma", "achieved": r["achieved"], "peak": r["peak"], "unit": "TFLOP/s", "frac": r["frac"],
                                       "traffic": None}}), flush=True)
        return
    m.set_precision(args.precision)
    if args.variant != "miccai2022":
        # profiling aid: another batch body through the same timing protocol (rocprofv3 -- python3 bench.py --variant ...)
        torch.manual_seed(0)
        np.random.seed(2019 + rank)
        L = m.lib()
        step, batches, desc = variant_setup(args.variant, 128 if (args.variant == "tsvd" and args.batch == 64) else args.batch,
                                            args.size, device, rank, sync, generic_head=args.generic_loss_head)
        graph = hasattr(step, "enable_graph") and not args.eager
        if graph:
            step.enable_graph()
        for i in range(max(args.warmup, 4)):
            step.step(batches[i % 2], epoch=5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out = step.step(batches[i % 2], epoch=5)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:
            write_outputs(snapshot_outputs(out), args.dump_outputs)
        graph = graph and bool(getattr(step, "_want_graph", False))      # (a failed capture falls back to eager launches)
        Bv = batches[0][0][0].shape[0]
        if rank == 0:
            print(json.dumps({"metric": "ROI-tiles/sec (variant step)", "value": round(Bv * world * args.steps / dt, 2), "unit": "tiles/s",
                              "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": round(1000.0 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
                              "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
                              "config": {"workload": desc, "tiles_per_gpu": Bv, "final_loss": round(float(out["loss"]), 4),
                                         "launch": "one captured HIP graph per step" if graph else "eager"}}), flush=True)
        if sync is not None:
            torch.distributed.destroy_process_group()
        return
    opt = m.stage2_opt(dropout_rate=0.1, batch_size=args.batch)
    opt.fused_loss_head = not args.generic_loss_head
    opt.teacher_streams = args.teacher_streams
    opt.overlap_head = not (args.no_head_overlap or args.serial)
    n_data = 1024
    torch.manual_seed(0)
    np.random.seed(2019 + rank)
    step = m.DistillStep(opt, n_data, device=device, sync=sync)
    for crd in (step.criterion_kd, step.criterion_kd_path):
        crd.contrast.verbose = False
    if sync is not None:
        # phase markers inside the step (ph_prof_stamp, also inside the replayed graph): 5 = the trunk backward is done and
        # the remaining gradient all-reduce is waited for, 10 = all gradients reduced (the `comm` object below)
        step._stamps = torch.zeros(16, dtype=torch.int64, device=device)
    if args.no_fuse:
        step.ema_model._no_fuse = True
        step.fix_model.path_net._no_fuse = True
    if args.no_masked:
        for net in (step.model, step.ema_model, step.fix_model.path_net):
            net._no_masked = True
    if args.no_bwd_overlap or args.serial:
        step.model._no_bwd_overlap = True
    if args.serial:
        step._side_stream = None
    if args.no_stem_pool:
        step.ema_model._no_stem_pool = True
        step.fix_model.path_net._no_stem_pool = True
    batches = [make_batch(args.batch, args.size, n_data, opt, device, seed=rank * 100 + i) for i in range(2)]
    if sync is not None:
        np.random.seed(2019)   # the 'mid' rank draw is host RNG state shared by all replicas

    if args.device_loader:
        import types
        g = torch.Generator().manual_seed(5 + rank)
        nt = 256                                   # source tiles of twice the crop edge (the reference crops 512 out of 1024)
        tiles = torch.randint(0, 256, (nt, 2 * args.size, 2 * args.size, 3), generator=g, dtype=torch.uint8).to(device)
        lopt = types.SimpleNamespace(input_size_path=args.size, nce_p=opt.nce_p, nce_k=opt.nce_k, pos_mode="multi_pos", label_dim=3)
        loader = m.augment.ResidentTileLoader(lopt, tiles, torch.randn(n_data, opt.input_size_omic, generator=g),
                                              torch.arange(n_data) % 3, device=device, seed=rank)
        loader.row_to_tile = torch.arange(n_data, device=device) % nt
        step.loader = loader
        batches = [None, None]
    L = m.lib()
    # the kernel timer times an eager run's own timed region; after a graph-replayed one it needs eager steps of its own (--full)
    kernel_timer = not args.no_kernel_timer and (args.eager or args.full)
    measure(step, batches, args.steps, args.warmup, sync, device, graph=not args.eager, loader=args.device_loader)
    if args.eager and kernel_timer:
        L.ph_prof_reset(); L.ph_prof_enable(1)
    dt, out = timed(step, batches, args.steps, sync, device)
    if args.dump_outputs and rank == 0:
        write_outputs(snapshot_outputs(out), args.dump_outputs)
    replayed = bool(getattr(step, "_want_graph", False))      # (False after a capture that failed and fell back to eager launches)
    L.ph_prof_enable(0)
    timer_region = "the timed region (eager)"
    if not args.eager and kernel_timer:
        # the in-library HIP-event timer brackets individual launches, which a graph replay does not expose:
        # time the same kernels in 3 eager steps right after the timed region (same data, same shapes)
        step._want_graph = False
        step._side_stream = None         # one stream, forward and backward: un-overlapped per-kernel durations
        step._head_side = None
        step.model._no_bwd_overlap = True
        step.step(batches[0], epoch=1)
        L.ph_prof_reset(); L.ph_prof_enable(1)
        for i in range(3):
            out2 = step.step(batches[i % 2], epoch=1)
        torch.cuda.synchronize()
        L.ph_prof_enable(0)
        timer_region = "3 eager steps right after the graph-replayed timed region"
        prof_steps = 3
    else:
        prof_steps = args.steps
    main_prof = None
    if kernel_timer:
        # read the headline step's per-class timings NOW: the extra runs below reset and reuse the in-library timer
        main_prof = (ctypes.c_double * (4 * NALL))()
        L.ph_prof_summary4(main_prof, NALL)
    loss = out["loss"].item()
    if not np.isfinite(loss):
        raise SystemExit("non-finite loss in benchmark: %r" % loss)
    comm = None
    if sync is not None:
        # what the communicator saw (every rank takes part): ranks that joined an all-reduce, one PCI device per rank, and
        # from the step's own markers the exposed part of the gradient all-reduce in the last timed step (max over ranks)
        comm = m.dist.comm_report(sync, device, os.environ.get("PH_BENCH_BACKEND", "nccl"))
        st_ = step._stamps.cpu().numpy() if step._stamps is not None else None
        if st_ is not None and st_[10] > st_[5] > 0:
            t = torch.tensor([(int(st_[10]) - int(st_[5])) * 1e-5, (int(st_[6]) - int(st_[0])) * 1e-5], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            comm["exposed_grad_allreduce_ms"] = round(t[0].item(), 4)      # 100 MHz device wall clock
            comm["step_span_ms"] = round(t[1].item(), 3)
            if st_[11] > 0 and st_[5] > st_[11]:
                # phase 1 (layers 3-4 + heads, 93 % of the bytes) starts at stamp 11 and has until the end of the trunk backward
                # (stamp 5) to hide; phase 2 (the rest) and whatever of phase 1 is left are the exposed part above
                t2 = torch.tensor([(int(st_[5]) - int(st_[11])) * 1e-5], device=device, dtype=torch.float64)
                torch.distributed.all_reduce(t2, op=torch.distributed.ReduceOp.MIN)
                comm["phase1_overlap_window_ms"] = round(t2[0].item(), 4)
        nparam = step.optimizer.flat.numel
        comm["grad_allreduce_bytes"] = int(nparam) * 4
        comm["exchanges_per_step"] = ("bucketed all-reduce of the flat gradient buffer in two phases (layers 3-4 + heads start "
                                      "when the backward has passed layer 3), all-gather of (index, embed_s, embed_t) rows x 2 "
                                      "criteria, all-reduce of the 5 x 5 GK-Refine Gram, one-off all-reduce of the CRD Z sums")
        comm["launch"] = ("eager" if args.eager else "collectives captured inside the step's HIP graph") + \
            ("; " + os.environ["PH_BENCH_LAUNCH"] if "PH_BENCH_LAUNCH" in os.environ else "")

    def extra_run(batch, prec, steps, profile=False):
        """One more measurement on a fresh step object (another per-GPU batch or another arithmetic), same protocol.
        profile: also 2 one-stream eager steps under the in-library kernel timer -> (seconds, loss, per-class summary)."""
        m.set_precision(prec)
        try:
            o2 = m.stage2_opt(dropout_rate=0.1, batch_size=batch)
            np.random.seed(2019 if sync is not None else 2019 + rank)
            st2 = m.DistillStep(o2, n_data, device=device, sync=sync)
            for crd in (st2.criterion_kd, st2.criterion_kd_path):
                crd.contrast.verbose = False
            b2 = [make_batch(batch, args.size, n_data, o2, device, seed=rank * 100 + 7 + i) for i in range(2)]
            measure(st2, b2, steps, 3, sync, device, graph=not args.eager)
            d2, o = timed(st2, b2, steps, sync, device)
            l2 = o["loss"].item()
            if not np.isfinite(l2):
                raise SystemExit("non-finite loss in the extra benchmark run: %r" % l2)
            prof = None
            if profile:
                st2._want_graph = False
                st2._side_stream = None; st2._head_side = None
                st2.model._no_bwd_overlap = True
                st2.step(b2[0], epoch=1)
                L.ph_prof_reset(); L.ph_prof_enable(1)
                for i in range(2):
                    st2.step(b2[i % 2], epoch=1)
                torch.cuda.synchronize()
                L.ph_prof_enable(0)
                prof = (ctypes.c_double * (4 * NALL))()
                L.ph_prof_summary4(prof, NALL)
            for mod in (st2.model, st2.ema_model, st2.fix_model.path_net):
                mod.release_workspaces()
            del st2, b2
            torch.cuda.empty_cache()
            return (d2, l2, prof) if profile else (d2, l2)
        finally:
            m.set_precision("bf16")

    # ---- --full: the measurements beside the headline figure, each on a fresh step object after the timed steps
    strong = None
    if args.full and (args.strong_batch > 0 or (world > 1 and not args.no_strong and 256 % world == 0 and (256 // world) != args.batch)):
        # BASELINE configs[2] ("Batch 256 DDP across 8 x MI355X") and the north-star's ">= 6x at 8 GPUs": the GLOBAL batch
        # of the single-GPU north-star point split over the N GPUs - strong scaling against `bench.py --north-star`
        per = args.strong_batch if args.strong_batch > 0 else 256 // world
        d2, l2 = extra_run(per, "bf16", args.steps)
        strong = {"workload": "BASELINE configs[2] / north-star strong scaling: global batch 256 = %d tiles per GPU x %d GPUs, "
                              "512x512, bf16, RCCL gradient / bank / Gram exchanges" % (per, world),
                  "value": round(per * world * args.steps / d2, 2), "unit": "tiles/s",
                  "ms_per_step": round(1000.0 * d2 / args.steps, 3), "tiles_per_gpu": per, "global_batch": per * world,
                  "scaling": "strong", "final_loss": round(l2, 4)}
    ns256 = None
    if args.full and world == 1 and not args.no_north_star_block and not args.device_loader and (args.batch, args.size) == (64, 512):
        # the north-star's own single-GPU point in the driver-timed line: batch 256 on one MI355X, 5 graph-replayed steps,
        # the dominant kernel's roofline from this run's own launches and its own counter traffic (profiles/r04_b256_traffic.json)
        for mod in (step.model, step.ema_model, step.fix_model.path_net):
            mod.release_workspaces()
        step._slots = None; step._static = None
        torch.cuda.empty_cache()
        nss = 5
        d2, l2, pr = extra_run(256, "bf16", nss, profile=True)
        ms256 = 1000.0 * d2 / nss
        cls_ms = {c: pr[4 * c + 1] for c in range(NALL)}
        domc = max(list(range(NCLS)) + [MASKED_CLS] + [c for c, _ in FUSED_CLS], key=lambda c: cls_ms[c])
        n_, ms_, fl_ = pr[4 * domc], pr[4 * domc + 1], pr[4 * domc + 2]
        ach_ = fl_ / (ms_ * 1e-3) / 1e12 if ms_ > 0 else 0.0
        tr_ = None
        tf = next((f for f in (os.path.join(ROOT, "profiles", n) for n in ("r06_b256_traffic.json", "r05_b256_traffic.json", "r04_b256_traffic.json"))
                   if os.path.exists(f)), "")
        if os.path.exists(tf):
            try:
                tr_ = json.load(open(tf)).get(str(domc), {}).get("bytes_per_launch")
            except Exception:
                tr_ = None
        ns256 = {"workload": "north-star single-GPU point: batch 256 on 1 MI355X, 512x512, bf16, same step (BASELINE.json north_star)",
                 "steps": nss, "ms_per_step": round(ms256, 3), "value": round(256 * nss / d2, 2), "unit": "tiles/s",
                 "final_loss": round(l2, 4),
                 "step_frac": round(STEP_GFLOP_PER_TILE_512 * 256 / ms256 / MFMA_BF16_PEAK_TFLOPS, 4),
                 "roofline": {"bound": "mfma", "kernel": dict([(c, n) for c, n in [(i, CLS_NAMES[i]) for i in range(NCLS)] + [(MASKED_CLS, MASKED_NAME)] + FUSED_CLS])[domc],
                              "launches": int(n_), "avg_launch_ms": round(ms_ / max(n_, 1), 4),
                              "algorithmic_gflop_per_launch": round(fl_ / max(n_, 1) / 1e9, 3), "achieved": round(ach_, 2),
                              "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach_ / MFMA_BF16_PEAK_TFLOPS, 4),
                              "traffic": tr_,
                              "traffic_note": "HBM bytes per launch at B = 256 from profiles/" + os.path.basename(tf) + " (rocprofv3 --pmc, "
                                              "separate FETCH_SIZE / WRITE_SIZE passes of `bench.py --north-star --serial`)"}}
    parity = None
    if args.full and world == 1 and not args.no_parity_mode and not args.device_loader:
        # the arithmetics that meet the north-star's 1e-3 tolerance (tests/test_gpu_step.py::
        # test_two_steps_from_mid_training_state_vs_reference_golden runs the same assertions against the reference's golden
        # in each of them), same step, same sizes:
        #   bf16x6/x3  fp32 activations; six bf16 MFMA products per k-step in every forward, the three leading ones in the
        #              backward's dgrad / wgrad kernels: every assertion of the parity mode holds (logits 4e-5, six loss terms
        #              1e-5, GK-Refine weights 3e-5, gradients 2e-3 relative, Adam moments, updated weights)
        #   bf16x3     three products everywhere: logits 5.3e-4 and the six loss terms 5.4e-4 (within 1e-3); the GK-Refine
        #              weights - cosines of DIFFERENCES of student and teacher probabilities - only to 5e-3 relative, and the
        #              total loss they multiply to 3e-3 relative
        #   bf16x6     six products everywhere (the parity mode of the golden tests)
        psteps = max(2, min(args.steps, 5))
        parity = {}
        for pm, what in (("fp16x3/x1", "half-pair forward as `fp16x3` (identical logits, losses, GK-Refine weights); the backward's dgrad / wgrad multiply "
                                       "the hi planes alone (one fp16 product, 11-bit operands, fp32 accumulation): every 1e-3 assertion of the "
                                       "parity mode holds, gradients included, at the bf16x6 tolerances (tests/test_gpu_step.py)"),
                         ("fp16x3", "half-pair mode: every tensor a convolution reads is stored as two fp16 planes (x = hi + lo 2^-11, 22 "
                                    "significant bits; BatchNorm-backward dz under a per-tensor power-of-two scale), conv outputs / "
                                    "gradients fp32, 3 fp16 MFMA products per k-step: every 1e-3 assertion of the parity mode holds"),
                         ("bf16x6/x3", "fp32 activations, 6 bf16 MFMA products per k-step forward / 3 backward: every 1e-3 assertion of the "
                                       "parity mode holds (logits, six loss terms, GK-Refine weights, gradients 2e-3)"),
                         ("bf16x3", "fp32 activations, 3 products everywhere: logits and the six loss terms within 1e-3 (5.4e-4), "
                                    "GK-Refine weights / total loss 5e-3 / 3e-3 relative"),
                         ("bf16x6", "fp32 activations, 6 products everywhere (fp32-equivalent; the mode of the golden tests)")):
            d2, l2 = extra_run(args.batch, pm, psteps)
            parity[pm] = {"arithmetic": what, "value": round(args.batch * psteps / d2, 2), "unit": "tiles/s",
                          "ms_per_step": round(1000.0 * d2 / psteps, 3), "steps": psteps, "final_loss": round(l2, 4)}
        parity["tolerance_compliant"] = "fp16x3/x1"      # the cheapest arithmetic that passes every 1e-3 assertion (also: fp16x3, bf16x6/x3, bf16x6)

    variants = None
    if args.full and world == 1 and not args.no_variants and not args.device_loader and (args.batch, args.size) == (64, 512):
        # driver-timed legs of BASELINE configs[3] / configs[4] (VERDICT r02 missing 2) and the CRD kernels against the
        # HBM roofline at the bank size of configs[4]; the headline step's buffers are released first
        for mod in (step.model, step.ema_model, step.fix_model.path_net):
            mod.release_workspaces()
        step._slots = None; step._static = None
        torch.cuda.empty_cache()
        variants = {"mia2022": run_variant("mia2022", 64, args.size, device, L),
                    "mia2023": run_variant("mia2023", 64, args.size, device, L),
                    "mia2023_nce_k_65536": run_variant("mia2023", 64, args.size, device, L, nce_k=65536),
                    "tsvd_stage1": run_variant("tsvd", 128, args.size, device, L)}

    trunk = None
    if ns256 is not None and not args.no_trunk_block:
        # the literal north-star quantity, measured last (a capture that fails cannot disturb the numbers above)
        for mod in (step.model, step.ema_model, step.fix_model.path_net):
            mod.release_workspaces()
        step._slots = None; step._static = None
        torch.cuda.empty_cache()
        try:
            trunk = trunk_fwd_bwd(m, 256, args.size, device)
        except Exception as exc:      # noqa: BLE001
            trunk = {"error": repr(exc)}
        ns256["trunk_fwd_bwd"] = trunk
    _flush_c_stdio()
    if sync is not None:
        torch.distributed.barrier()      # every rank's native output is out before rank 0 prints the line
    if rank == 0:
        tiles = args.batch * world * args.steps
        res = {"metric": "ROI-tiles/sec (teacher+student distill step)", "value": round(tiles / dt, 2),
               "unit": "tiles/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(1000.0 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": "%s: teacher+student distill step, bf16, batch %d per GPU, "
                                      "%dx%d tiles, 320-d omic, CRD P=300/K=700->P2=20/K2=512, n_data=1024, "
                                      "GK-Refine on, Adam+EMA, dropout 0.1"
                                      % (("BASELINE configs[1]" + (" per GPU, weak scaling (global batch %d)" % (64 * world)
                                                                  if world > 1 else ""))
                                         if (args.batch, args.size) == (64, 512) else
                                         "north-star single-GPU point (batch 256)" if (args.batch, args.size, world) == (256, 512, 1) else
                                         "BASELINE configs[0] shape" if (args.batch, args.size) == (16, 224) else "custom",
                                         args.batch, args.size, args.size),
                          "tiles_per_gpu": args.batch, "tile": args.size, "global_batch": args.batch * world,
                          "parallelism": f"dp{world}" if world > 1 else "single", "final_loss": round(loss, 4),
                          "launch": (("eager (external launcher: a failed graph capture cannot be recovered in-process; "
                                      "PH_BENCH_DDP_GRAPH=1 opts in)" if ext_eager else "eager") if args.eager
                                     else ("one captured HIP graph per step" if replayed
                                           else "eager (the graph capture failed: see the warning on stderr)"))
                                    + ("; replicas: " + os.environ["PH_BENCH_LAUNCH"] if "PH_BENCH_LAUNCH" in os.environ else ""),
                          "input_pipeline": ("on-device from resident uint8 tiles, inside the timed region and the graph"
                                             if args.device_loader else "inputs resident in HBM when the timed region starts")}}
        # ---- roofline of the dominant kernel (live HIP-event timing inside the timed region)
        if kernel_timer:
            buf4 = main_prof
            buf = [0.0] * (3 * NALL)
            byt = [0.0] * NALL
            for c in range(NALL):
                buf[3 * c], buf[3 * c + 1], buf[3 * c + 2], byt[c] = buf4[4 * c], buf4[4 * c + 1], buf4[4 * c + 2], buf4[4 * c + 3]
            mfma_cls = [(c, CLS_NAMES[c]) for c in range(NCLS)] + [(MASKED_CLS, MASKED_NAME)] + FUSED_CLS
            rows = [(nm, buf[3 * c], buf[3 * c + 1], buf[3 * c + 2]) for c, nm in mfma_cls]
            dom, dom_name = max(mfma_cls, key=lambda cn: buf[3 * cn[0] + 1])
            n, ms, fl = buf[3 * dom], buf[3 * dom + 1], buf[3 * dom + 2]
            ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            traffic = None
            tname = None
            for tname in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
                tf = os.path.join(ROOT, "profiles", tname)
                if os.path.exists(tf):
                    try:
                        traffic = json.load(open(tf)).get(str(dom), {}).get("bytes_per_launch")
                    except Exception:
                        traffic = None
                    break
            step_gflop = STEP_GFLOP_PER_TILE_512 * (args.size / 512.0) ** 2 * args.batch * world
            step_tflops = step_gflop / (1000.0 * dt / args.steps)          # GFLOP / ms = TFLOP/s, whole job

            def per_kernel(name, launches, ms_, flops, nbytes):
                """One MFMA kernel class against BOTH rooflines; `bound` = the one its algorithmic intensity puts it under
                (machine balance 2500 TFLOP/s / 8 TB/s = 312 FLOP/B), `frac` = achieved / peak of that roofline."""
                tf = flops / (ms_ * 1e-3) / 1e12 if ms_ > 0 else 0.0
                gb = nbytes / (ms_ * 1e-3) / 1e9 if ms_ > 0 else 0.0
                inten = flops / nbytes if nbytes > 0 else float("inf")
                bound = "mfma" if inten >= MFMA_BF16_PEAK_TFLOPS * 1e3 / HBM_PEAK_GBS else "hbm"
                fm, fh = tf / MFMA_BF16_PEAK_TFLOPS, gb / HBM_PEAK_GBS
                return {"kernel": name, "launches": int(launches), "total_ms": round(ms_, 3), "tflops": round(tf, 2),
                        "frac_mfma": round(fm, 4), "algorithmic_gbs": round(gb, 1), "frac_hbm": round(fh, 4),
                        "flop_per_byte": round(inten, 1) if nbytes > 0 else None, "bound": bound,
                        "frac": round(fm if bound == "mfma" else fh, 4)}
            hbm = []
            for j, name in enumerate(HBM_NAMES):
                a, b, c = buf[3 * (NCLS + j)], buf[3 * (NCLS + j) + 1], buf[3 * (NCLS + j) + 2]
                gbs = c / (b * 1e-3) / 1e9 if b > 0 else 0.0
                hbm.append({"kernel": name, "launches": int(a), "total_ms": round(b, 3), "avg_launch_us": round(1000.0 * b / max(a, 1), 2),
                            "algorithmic_mb_per_launch": round(c / max(a, 1) / 1e6, 2), "achieved_gbs": round(gbs, 1),
                            "peak_gbs": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4)})
            res["roofline"] = {"bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_BF16_PEAK_TFLOPS,
                               "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                               "traffic_note": "HBM bytes per launch from profiles/%s (rocprofv3 --pmc FETCH_SIZE / "
                                               "WRITE_SIZE in separate passes, FETCH_SIZE x2 gfx950 correction)" % tname,
                               "kernel": dom_name, "launches": int(n), "avg_launch_ms": round(ms / max(n, 1), 4),
                               "algorithmic_gflop_per_launch": round(fl / max(n, 1) / 1e9, 3),
                               "step_frac": round(step_tflops / world / MFMA_BF16_PEAK_TFLOPS, 4),
                               "step_tflops_per_gpu": round(step_tflops / world, 1),
                               "step_hbm": (lambda led: {"algorithmic_gb_per_step": round(sum(led.values()) / 1e9, 2),
                                                         "achieved_gbs": round(sum(led.values()) / (dt / args.steps) / 1e9, 1),
                                                         "peak_gbs": HBM_PEAK_GBS,
                                                         "frac": round(sum(led.values()) / (dt / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                                                         "counter_gb_per_step": _counter_step_gb(),
                                                         "ledger_gb": {k: round(v / 1e9, 3) for k, v in sorted(led.items(), key=lambda kv: -kv[1])},
                                                         "note": "per-tensor algorithmic HBM bytes of one step (bench.py: hbm_ledger) / ms_per_step / 8 TB/s - "
                                                                 "the step's real bound: train-mode BatchNorm makes every conv output travel "
                                                                 "to HBM and back; counter_gb_per_step: FETCH_SIZE x 2 + WRITE_SIZE over all "
                                                                 "kernels of one step (profiles/r06_traffic.json, null until collected)"})(
                                   hbm_ledger(args.batch, args.size)) if args.precision == "bf16" else None,
                               "step_note": "whole step: %.2f GFLOP per tile (3 ResNet-18 forwards + 1 backward, SURVEY 8-d) x tiles / "
                                            "ms_per_step / 2500 TFLOP/s; the reference executes 276.8 GFLOP per tile for the same "
                                            "numbers (6 backward passes)" % (STEP_GFLOP_PER_TILE_512 * (args.size / 512.0) ** 2),
                               "all_kernels": [per_kernel(nm, buf[3 * c], buf[3 * c + 1], buf[3 * c + 2], byt[c])
                                               for c, nm in mfma_cls if buf[3 * c] > 0],
                               "hbm": hbm,
                               "mfma_kernel_ms_per_step": round(sum(r[2] for r in rows) / prof_steps, 3),
                               "timer_region": timer_region + " (HIP events around single launches: includes ~4 us of launch "
                                                              "gap per launch over the rocprofv3 durations in profiles/)"}
        else:
            step_gflop = STEP_GFLOP_PER_TILE_512 * (args.size / 512.0) ** 2 * args.batch * world
            res["roofline"] = {"bound": "mfma", "step_frac": round(step_gflop / (1000.0 * dt / args.steps) / world / MFMA_BF16_PEAK_TFLOPS, 4),
                               "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s"}
        if comm is not None:
            res["comm"] = comm
        if ns256 is not None:
            res["north_star_b256"] = ns256
        if strong is not None:
            res["north_star_global_256"] = strong
        if parity is not None:
            res["parity_mode"] = parity
            # the headline `value` is the bf16 arithmetic of BASELINE configs[1] (logits at the bf16 noise floor, ~5e-2); the
            # cheapest arithmetic that meets the north-star's 1e-3 on logits AND loss is quoted beside it
            tc = parity[parity["tolerance_compliant"]]
            res["value_tolerance_compliant"] = {"value": tc["value"], "unit": "tiles/s", "ms_per_step": tc["ms_per_step"],
                                                "dtype": parity["tolerance_compliant"],
                                                "note": "same step, same sizes, in the cheapest arithmetic whose logits / losses are within "
                                                        "1e-3 of the fp32 reference (parity_mode block)"}
        if variants is not None:
            res["variants"] = variants
        if args.full and world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline()
        _flush_c_stdio()      # (RCCL prints its version banner through C stdio: without this it lands AFTER the JSON line)
        print(json.dumps(res), flush=True)
    if sync is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

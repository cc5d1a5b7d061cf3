"""Time of the connectivity pass of the device SLIC next to the segmentation it follows (not a test):

    python tests/bench_slic_connect_gpu.py [--tiles 64] [--size 1024] [--k 100] [--json PATH]

Over a resident store of textured tiles (the store of tests/bench_slic_gpu.py): slic_segment without and with the pass
and slic_connect alone (device events around the whole call, warmed up, repeated until a second is filled, the three
alternating in one process), the bytes the pass must move computed from the shapes, the component counts of tile 0 -
and one tile compared with the restatement (tests/slic_connect_emulation.py) on every pixel; that comparison is
asserted, the times are reported as they are."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import multimodal_learning_amd as m  # noqa: E402
import slic_connect_emulation as CE  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, the HBM3E specification of the MI355X


def connect_bytes(n, H, W, N):
    """Bytes the seven launches must move per call, from the shapes: local 2 (label) + 4 + 4 (parent, count written);
    flatten 4 + 4 (parent read, count read; roots' words rewritten where they moved - counted whole) + 4; principal,
    target and chain each re-read the 4-B parent; relabel reads the parent, gathers link and label (4 + 2) and writes 2.
    The seam pairs (one pixel in 13) and the per-label words are left out."""
    px = n * H * W
    return px * ((2 + 4 + 4) + (4 + 4 + 4) + 3 * 4 + (4 + 4 + 2 + 2)) + n * N * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    n, H, K = a.tiles, a.size, a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randint(0, 256, (n, H // 16, H // 16, 3), generator=g, dtype=torch.uint8, device="cuda")
    tiles = base.repeat_interleave(16, 1).repeat_interleave(16, 2)
    tiles = (tiles.short() + torch.randint(-12, 13, tiles.shape, generator=g, dtype=torch.int16, device="cuda")).clamp_(0, 255).to(torch.uint8)
    N = m.superpixel.slic_num_labels(H, H, K)
    min_size = m.superpixel.slic_min_size(H, H, N)
    out = torch.empty(n, H, H, device="cuda", dtype=torch.int16)
    seg, _ = m.superpixel.slic_segment(tiles, K, iters=a.iters)
    con = torch.empty_like(seg)

    # one tile against the restatement, every pixel
    lab0 = seg[0].cpu().numpy()
    want, info = CE.connect(lab0, N, min_size, return_info=True)
    got = m.superpixel.slic_connect(seg[:1], N, min_size)[0].cpu().numpy()
    differing = int((got != want).sum())
    print(f"tile 0 ({H} x {H}, N {N}, min_size {min_size}): {info['components']} components, {info['merged']} merged, "
          f"{info['kept']} kept, {info['changed']} pixels changed, {info['components_after']} components after; "
          f"device against the restatement: {differing} differing pixels")
    assert differing == 0

    fns = dict(segment=lambda: m.superpixel.slic_segment(tiles, K, iters=a.iters, out=out, chunk=n),
               segment_connect=lambda: m.superpixel.slic_segment(tiles, K, iters=a.iters, out=out, chunk=n, enforce_connectivity=True),
               connect=lambda: m.superpixel.slic_connect(seg, N, min_size, out=con, chunk=n))
    for f in fns.values():
        f(); f()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in fns}
    reps = 0
    while min(total.values()) < a.seconds * 1e3:
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            total[k] += e0.elapsed_time(e1)
        reps += 1
    ms = {k: v / reps for k, v in total.items()}
    nbytes = connect_bytes(n, H, H, N)
    rate = nbytes / (ms["connect"] * 1e-3)
    print(f"{n} tiles {H} x {H}, K = {K}, {a.iters} iterations, {reps} alternating calls each:")
    print(f"  slic_segment                          {ms['segment']:.2f} ms  ({ms['segment'] / n * 1e3:.1f} us per tile)")
    print(f"  slic_segment(enforce_connectivity)    {ms['segment_connect']:.2f} ms  ({ms['segment_connect'] / n * 1e3:.1f} us per tile)")
    print(f"  slic_connect alone                    {ms['connect']:.2f} ms  ({ms['connect'] / n * 1e3:.1f} us per tile), "
          f"{100 * ms['connect'] / ms['segment']:.0f} % of the segmentation")
    print(f"  bytes the pass must move {nbytes / 1e9:.2f} GB ({nbytes / n / H / H:.0f} B per pixel) -> {rate / 1e12:.2f} TB/s whole-call, "
          f"{100 * rate / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    res = dict(tiles=n, size=H, K=K, N=N, iters=a.iters, min_size=min_size, reps=reps, segment_ms=ms["segment"],
               segment_connect_ms=ms["segment_connect"], connect_ms=ms["connect"], connect_bytes=nbytes, connect_hbm_share=rate / HBM_PEAK,
               tile0={k: info[k] for k in ("components", "merged", "kept", "changed", "components_after")}, differing=differing)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()

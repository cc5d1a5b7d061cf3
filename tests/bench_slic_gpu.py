"""Time of the device SLIC segmentation and of the four-view augmenter (not a test):

    python tests/bench_slic_gpu.py [--tiles 256] [--size 1024] [--k 100] [--json PATH]

slic_segment over a resident store (device events around the whole call, warmed up, repeated until a second is filled),
the bytes one iteration has to move computed from the shapes, the resulting share of the HBM peak; then one four-view
batch (B = 64, 1024 -> 512) next to the two-view call, alternating in the same process.  Nothing is asserted: there is
no earlier implementation to compare with.  The numbers are what they are called - a whole-call rate, not a kernel's."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_learning_amd as m  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, the HBM3E specification of the MI355X


def slic_bytes(n, H, W, N, iters):
    """Bytes the launch sequence must move: the conversion reads 3 B and writes one 4-B Lab word per pixel; an iteration
    re-reads that word and writes a 2-B label; centres and sums (N records per tile) are noise next to it."""
    px = n * H * W
    per_iter = px * (4 + 2) + n * N * (8 + 6 * 8)
    return px * (3 + 4) + iters * per_iter, per_iter


def timed(fn, min_seconds=1.0, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1); reps += 1
    return total / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    n, H, K = a.tiles, a.size, a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randint(0, 256, (n, H // 16, H // 16, 3), generator=g, dtype=torch.uint8, device="cuda")
    tiles = base.repeat_interleave(16, 1).repeat_interleave(16, 2)
    tiles = (tiles.short() + torch.randint(-12, 13, tiles.shape, generator=g, dtype=torch.int16, device="cuda")).clamp_(0, 255).to(torch.uint8)
    N = m.superpixel.slic_num_labels(H, H, K)
    out = torch.empty(n, H, H, device="cuda", dtype=torch.int16)
    res = dict(tiles=n, size=H, K=K, N=N, iters=a.iters)
    for chunk in (64, n):
        ms, reps = timed(lambda: m.superpixel.slic_segment(tiles, K, iters=a.iters, out=out, chunk=chunk))
        total, per_iter = slic_bytes(n, H, H, N, a.iters)
        share = total / (ms * 1e-3) / HBM_PEAK
        print(f"slic_segment chunk {chunk}: {ms:.2f} ms per call of {n} tiles {H} x {H} at K = {K} ({reps} calls), "
              f"{ms / n * 1e3:.1f} us per tile; bytes to move {total / 1e9:.2f} GB ({per_iter / n / 1e6:.2f} MB per tile and "
              f"iteration) -> {total / (ms * 1e-3) / 1e12:.2f} TB/s whole-call, {100 * share:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
        res[f"slic_ms_chunk{chunk}"] = ms
        res[f"slic_us_per_tile_chunk{chunk}"] = ms / n * 1e3
        res[f"slic_hbm_share_chunk{chunk}"] = share
    res["slic_bytes"] = total

    B, S = 64, 512
    opt = types.SimpleNamespace(input_size_path=S)
    a2, a4 = m.augment.DeviceAugment(opt), m.augment.DeviceAugmentSP(opt)
    src, sp = tiles[:B].contiguous(), out[:B].contiguous()
    if H < S:
        print("tiles smaller than the crop: augmenter not timed")
    else:
        o2 = a2(src)
        o4 = a4(src, sp)
        t2 = t4 = 0.0
        R = 0
        torch.cuda.synchronize()
        while t2 + t4 < 2e3:                       # alternating, a second each
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(); a2(src, out=o2); ev[1].record(); a4(src, sp, out=o4); ev[2].record()
            torch.cuda.synchronize()
            t2 += ev[0].elapsed_time(ev[1]); t4 += ev[1].elapsed_time(ev[2]); R += 1
        b2 = B * 2 * (2 * S * S * 3 + 3 * S * S * 4)
        b4 = B * 4 * (2 * S * S * 3 + 3 * S * S * 4) + B * 2 * S * S * (2 + 8)
        print(f"two views:  {t2 / R * 1e3:.0f} us per batch of {B} ({H} -> {S}), {b2 / (t2 / R) / 1e9:.2f} TB/s algorithmic ({R} alternating calls)")
        print(f"four views + 2 label maps: {t4 / R * 1e3:.0f} us per batch of {B}, {b4 / (t4 / R) / 1e9:.2f} TB/s algorithmic")
        res.update(aug2_us=t2 / R * 1e3, aug4_us=t4 / R * 1e3, aug2_bytes=b2, aug4_bytes=b4)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings of the masked pixel draw and of the mask pack (records, not gates).

  * snerf_sample_pixels_masked at R rays against snerf_sample_pixels_uniform on the same uint8 image cache [M,H,W,3], both with the fused gather:
    device events around `--iters` back-to-back calls through ops (so a figure holds the launch and the two small allocations of a call as well
    as the kernel), after a warm-up;
  * snerf_mask_pack over the cache's byte mask [M,H,W]: time per call and the rate against the bytes it streams (n_pixels read, n_pixels / 8 +
    n_pixels / 256 written), and the whole MaskIndex.from_mask (pack + cumsum + the one read of the total).

    python tools/bench_masks.py --out masks_timing.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import ops  # noqa: E402


def timed(fn, iters, warmup=20):
    """Mean milliseconds of one fn() over `iters` back-to-back calls between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="masks_timing.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M, H, W, R = args.images, args.height, args.width, args.rays
    gen = torch.Generator(dev).manual_seed(1)
    images = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    mask = torch.ones(M, H, W, 1, dtype=torch.bool, device=dev)
    mask[:, : H // 8, : W // 3] = False  # a banner in the top left corner of every image
    n = M * H * W
    index = ops.MaskIndex.from_mask(mask)
    u2, u3 = torch.rand(R, 2, device=dev, generator=gen), torch.rand(R, 3, device=dev, generator=gen)
    idx, target = ops.sample_pixels_masked(u2, index, M, H, W, images)
    assert bool(mask[idx[:, 0], idx[:, 1], idx[:, 2], 0].all()) and torch.equal(target.cpu(), images[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().float() / 255.0)
    flat = ops._mask_bytes(mask, "mask")
    bits, counts = torch.empty_like(index.bits), torch.empty_like(index.block_counts)
    rows = []
    for _ in range(args.repeats):  # alternating, so that a drift of the machine shows in both
        rows.append({
            "masked_ms": timed(lambda: ops.sample_pixels_masked(u2, index, M, H, W, images), args.iters),
            "uniform_ms": timed(lambda: ops.sample_pixels_uniform(u3, M, H, W, images), args.iters),
            "pack_ms": timed(lambda: ops.mask_pack(flat, n, 0, bits, counts), max(args.iters // 10, 10), warmup=3),
            "from_mask_ms": timed(lambda: ops.MaskIndex.from_mask(mask), 10, warmup=2),
        })
    assert torch.equal(bits, index.bits) and torch.equal(counts, index.block_counts)
    best = {k: min(r[k] for r in rows) for k in rows[0]}
    streamed = n + 4 * index.bits.numel() + 4 * index.block_counts.numel()
    out = {"device": torch.cuda.get_device_name(0), "cache": [M, H, W], "pixels": n, "valid_pixels": index.total, "rays": R, "iters": args.iters,
           "method": "device events around back-to-back calls through ops (launch + allocations of a call included); best of the repeats below",
           "draw_masked_us": best["masked_ms"] * 1e3, "draw_uniform_us": best["uniform_ms"] * 1e3,
           "pack_us": best["pack_ms"] * 1e3, "pack_bytes_streamed": streamed, "pack_GB_per_s": streamed / (best["pack_ms"] * 1e-3) / 1e9,
           "mask_index_from_mask_us": best["from_mask_ms"] * 1e3,
           "index_bytes": 4 * index.bits.numel() + 4 * index.block_counts.numel() + 8 * index.block_prefix.numel(), "repeats": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "repeats"}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Step time of the K-Planes preset with bounded=True and with bounded=False (contracted coordinates inside the kernels, near / far collider,
piecewise spacing: DESIGN.md 4.15), and snerf_kplanes_gather_bwd_coords alone with and without snerf_coords.contract, in ONE process: the two
trainers alternate, `--rounds` rounds of `--steps` steps each on random rays, the median round is reported.  A record, no gate.

    python tools/bench_unbounded.py --out unbounded_step.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import ops  # noqa: E402
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--far-plane", type=float, default=1000.0)
    ap.add_argument("--out", default="unbounded_step.json")
    args = ap.parse_args()
    dev, R = torch.device("cuda:0"), args.rays
    gen = torch.Generator().manual_seed(0)
    g = lambda z: z.to(dev).contiguous()
    rays = {"origins": g((torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2),
            "directions": g(torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)), "times": g(torch.rand(R, 1, generator=gen))}
    target = g(torch.rand(R, 3, generator=gen))
    trs = {"bounded": KPlanesTrainer(KPlanesTrainConfig(), R, dev),
           "unbounded": KPlanesTrainer(KPlanesTrainConfig(bounded=False, near_plane=0.05, far_plane=args.far_plane), R, dev)}
    for tr in trs.values():
        assert tr.fused_field and tr.fused_proposal and tr.fused_proposal_backward and tr.quotient_scatter and tr.quotient_epilogue
    assert trs["unbounded"].contract and not trs["bounded"].contract
    ms = {k: [] for k in trs}
    for tr in trs.values():  # warm-up: first launches, workspaces
        for _ in range(10):
            tr.train_step(rays, target)
        tr.synchronize()
    for _ in range(args.rounds):
        for k, tr in trs.items():
            tr.restart()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.train_step(rays, target)
            tr.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = {"rays_per_step": R, "steps_per_round": args.steps, "rounds": args.rounds, "far_plane": args.far_plane,
           "schedule": "early training (every step updates the proposal networks)",
           "step_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "step_median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()}}
    out["unbounded_over_bounded"] = round(out["step_median_ms"]["unbounded"] / out["step_median_ms"]["bounded"], 4)
    # the coordinate gradient alone, at the nerf level's shape, on the unbounded trainer's own rays and bin edges
    tr = trs["unbounded"]
    S2, N = tr.S[2], R * tr.S[2]
    eb = tr.buf["eb"][2]
    gfeat = torch.randn(N, tr.field_planes.out_dim, device=dev)
    go, gd = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
    t = rays["times"].reshape(-1)
    coords = {"contract": ops.coords_from_rays(rays["origins"], rays["directions"], t, eb, None, True, contract=True),
              "box": ops.coords_from_rays(rays["origins"], rays["directions"], t, eb, [[-args.far_plane] * 3, [args.far_plane] * 3], True)}
    alone = {}
    for name, co in coords.items():
        for _ in range(5):
            ops.kplanes_gather_bwd_coords(tr._desc_field, tr.field_planes.planes, co, N, gfeat, want_pts=False, grad_origins=go, grad_dirs=gd)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            ops.kplanes_gather_bwd_coords(tr._desc_field, tr.field_planes.planes, co, N, gfeat, want_pts=False, grad_origins=go, grad_dirs=gd)
        b.record()
        torch.cuda.synchronize()
        alone[name] = round(a.elapsed_time(b) / 50 * 1e3, 2)
    out["gather_bwd_coords_us"] = {"samples": N, **alone}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

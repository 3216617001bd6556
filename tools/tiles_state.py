"""Same records and same sums before and after a change to the tiled (owner-computes) table backwards (csrc/tgrid_tiles.hip, csrc/hashgrid_tiles.hip): on
the seeded inputs of tests/test_gpu_tgrid_tiles.py (all CASES, rays and points) and of the tiled test in tests/test_gpu_hashgrid.py (its five
configurations) it saves the plan, tile_base[0 .. n_tiles], the records sorted within each tile (their order inside a tile depends on LDS atomic ranks), the
MODE 0 gradient and p, m, v after three fused steps.  Dev tool.

    python tools/tiles_state.py run TREE OUTDIR       # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/tiles_state.py cmp A B [A2]          # plan / tile_base / records array_equal; sums: max |B - A| per tensor, which may not exceed
                                                      # max |A2 - A| of a second run of A's tree (bit-equal where that is bit-equal); exit 1 otherwise
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

EXACT = ("plan", "tile_base", "records")


def compare(a, b, a2):
    bad = 0
    for f in sorted(os.listdir(a)):
        x, y = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
        x2 = torch.load(os.path.join(a2, f)) if a2 else x
        for k in x:
            if k in EXACT:
                ok = bool(torch.equal(x[k], y[k]))
                print(f"{f:34s} {k:10s} n = {x[k].numel():9d}  {'equal' if ok else 'DIFFERENT'}")
            else:
                d, d0 = float((y[k] - x[k]).abs().max()), float((x2[k] - x[k]).abs().max())
                ok = d <= d0
                print(f"{f:34s} {k:10s} n = {x[k].numel():9d}  max|B - A| = {d:.3e}  max|A2 - A| = {d0:.3e}  {'ok' if ok else 'EXCEEDS'}")
            bad += not ok
    print("VERDICT", "records equal, sums within the first tree's own run-to-run difference" if bad == 0 else f"{bad} differ")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
from soccernerfs_amd import _lib, ops
from soccernerfs_amd.tcnn_compat import Encoding, TiledHashTableBackward
from soccernerfs_amd.temporal_grid import TemporalGridEncoder, TiledTableBackward

os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
L = _lib.lib()


def binned(tb):
    """plan fields, prefix sums and the records sorted within each tile"""
    torch.cuda.synchronize()
    n = tb.plan.n_tiles
    plan = torch.tensor([tb.plan.tile_rows_log2, n, tb.plan.n_chunks, tb.plan.chunk, tb.plan.first_tiled_level, tb.plan.lds_bytes, tb.plan.count_ints,
                         tb.plan.record_capacity] + list(tb.plan.tile_start), dtype=torch.int64)
    base = tb.tile_base[: n + 1].cpu().numpy()
    rec = tb.records[: base[n]].cpu().numpy().view(np.uint32)
    tile = np.repeat(np.arange(n), np.diff(base))
    rec = rec[np.lexsort((rec, tile))]
    return {"plan": plan, "tile_base": torch.from_numpy(base.copy()), "records": torch.from_numpy(rec.astype(np.int64))}


# ---- temporal grid: CASES and _batch of tests/test_gpu_tgrid_tiles.py ----
CASES = [
    (dict(input_dim=3, temporal_dim=64, num_levels=16, level_dim=2, log2_hashmap_size=17, desired_resolution=2048), 0, -1),
    (dict(input_dim=3, temporal_dim=64, num_levels=16, level_dim=2, log2_hashmap_size=15, desired_resolution=2048), 5, 0),
    (dict(input_dim=3, temporal_dim=32, num_levels=5, level_dim=2, log2_hashmap_size=17, base_resolution=16, per_level_scale=1.4142135), 0, -1),
    (dict(input_dim=3, temporal_dim=12, num_levels=4, level_dim=4, log2_hashmap_size=12, base_resolution=5, per_level_scale=1.7), 4, 0),
    (dict(input_dim=3, temporal_dim=24, num_levels=3, level_dim=8, log2_hashmap_size=11, base_resolution=4, per_level_scale=2.0), 3, 1),
    (dict(input_dim=3, temporal_dim=7, num_levels=3, level_dim=1, log2_hashmap_size=10, base_resolution=6, per_level_scale=1.5, gridtype="tiled"), 6, 0),
]


def batch(gen, R, S, mode):
    o = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.9).to(DEV)
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    edges = torch.sort(torch.rand(R, S + 1, generator=gen) ** 3 * 1.6, dim=-1).values.to(DEV).contiguous()
    times = torch.rand(R, generator=gen).to(DEV)
    times[0], times[1] = 0.0, 1.0
    if mode == "rays":
        return ops.coords_from_rays(o, d, times, edges, [[-1.0] * 3, [1.0] * 3], False), times, (o, d, edges)
    mid = (edges[:, :-1] + edges[:, 1:]) / 2
    pts = (((o[:, None, :] + d[:, None, :] * mid[..., None]) + 1.0) / 2.0).reshape(R * S, 3).contiguous()
    return ops.coords_from_points(pts), times, (pts,)


for ci, (kw, sh, lc) in enumerate(CASES):
    for mode in ("rays", "points"):
        gen = torch.Generator().manual_seed(5)
        enc = TemporalGridEncoder(**kw).to(DEV)
        with torch.no_grad():
            enc.embeddings.copy_(((torch.rand(enc.embeddings.shape, generator=gen) - 0.5) * 0.2).to(DEV))
        rows, gc = enc.embeddings.shape
        R, S = 257, 48
        B = R * S
        tb = TiledTableBackward(enc, B, tile_rows_log2=sh, first_tiled_level=lc)
        p = enc.embeddings.detach().clone()
        m, v, gtab, grad0 = (torch.zeros(rows, gc, device=DEV) for _ in range(4))
        srow, part = torch.zeros(rows, device=DEV), torch.zeros(64, 16, device=DEV)
        for step in range(1, 4):
            co, times, keep = batch(gen, R, S, mode)
            gout = (torch.randn(B, enc.output_dim, generator=gen) * 1e-3).to(DEV)
            gout[5:9] = 0.0
            gout[11, : enc.level_dim] = 0.0
            ca, cb = enc._index_list_host[step * 7 % len(enc._index_list_host)]
            _lib.check(L.snerf_tgrid_tv_sign(ops._ptr(p), C.c_int64(rows), gc, ca, cb, 0.1, ops._ptr(part), 64, ops._ptr(srow), ops._stream()))
            tb.bin(co, times, S, gout)
            if step == 1:
                res = binned(tb)
                tb.coarse_levels(co, times, S, gout, grad0)
                tb.scatter(gout, grad0)
                res["grad_mode0"] = grad0.cpu()
            tb.coarse_levels(co, times, S, gout, gtab)
            tb.scatter_adam(gout, gtab, p, m, v, 1e-2, step, 1e-12, tv_cols=(ca, cb), srow=srow)
        torch.cuda.synchronize()
        res.update(p=p.cpu(), m=m.cpu(), v=v.cpu())
        torch.save(res, os.path.join(out, f"tgrid_case{ci}_{mode}.pt"))
        print("tgrid", ci, mode, "records", int(res["tile_base"][-1]), flush=True)

# ---- static hash grid: the configurations and inputs of the tiled test in tests/test_gpu_hashgrid.py ----
NP = dict(n_levels=16, n_features_per_level=2, base_resolution=16, per_level_scale=1.4472692012786865, log2_hashmap_size=15)
HASH = [(NP, 0, 0), (NP, 6, 3), (dict(n_levels=3, n_features_per_level=4, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=12), 4, 0),
        (dict(n_levels=5, n_features_per_level=8, base_resolution=5, per_level_scale=1.5, log2_hashmap_size=9), 3, 1),
        (dict(n_levels=4, n_features_per_level=1, base_resolution=7, per_level_scale=1.6, log2_hashmap_size=11), 5, 2)]
for ci, (cfg, sh, lc) in enumerate(HASH):
    gen = torch.Generator().manual_seed(8)
    enc = Encoding(3, {"otype": "HashGrid", **cfg}).to(DEV)
    F, B = cfg["n_features_per_level"], 5000
    tb = TiledHashTableBackward(enc, B, tile_rows_log2=sh, first_tiled_level=lc)
    p = enc.params.detach().clone()
    m, v, gtab, grad0 = (torch.zeros_like(p) for _ in range(4))
    for step in range(1, 4):
        x = torch.rand(B, 3, generator=gen)
        x[0, 0], x[1, 2], x[2], x[3] = 1.0, 0.0, -0.13, 1.21
        x = x.to(DEV)
        gout = ((torch.rand(B, cfg["n_levels"] * F, generator=gen) - 0.5) * 1e-3).to(DEV)
        gout[7:11] = 0.0
        tb.bin(x, gout)
        if step == 1:
            res = binned(tb)
            tb.coarse_levels(x, gout, grad0)
            tb.scatter(x, gout, grad0)
            res["grad_mode0"] = grad0.cpu()
        tb.coarse_levels(x, gout, gtab)
        tb.scatter_adam(x, gout, gtab if lc > 0 else None, p, m, v, 1e-2, step, 1e-6)
    torch.cuda.synchronize()
    res.update(p=p.cpu(), m=m.cpu(), v=v.cpu())
    torch.save(res, os.path.join(out, f"hash_case{ci}.pt"))
    print("hash", ci, "records", int(res["tile_base"][-1]), flush=True)

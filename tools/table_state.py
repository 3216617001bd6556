"""Same bits before and after a change to the table encoders' scatter / gather kernels (csrc/tgrid.hip, csrc/hashgrid.hip and the headers they share with
the tiled backwards): on seeded inputs it saves the forward output of every entry point (snerf_tgrid_encode_fwd in rays and points mode with the
run-length form on and off, snerf_tgrid_encode_fwd_dydx, snerf_hashgrid_encode_fwd) and the fixed-point gradient cells of snerf_tgrid_encode_bwd_fx
(run-length form on and off) and snerf_hashgrid_encode_bwd_fx (table and coordinates).  All of these are deterministic (the cells are integer sums), so
two trees that compute the same thing agree in every bit.  Sizes: the grids of bench.py's config-4 leg (main grid L = 16, C = 2, log2T = 19, temporal_dim
64 at 4096 x 48 samples; a proposal grid L = 5, log2T = 17 at 4096 x 256), the full NeRFPlayer's hash grid, and the small cases of
tests/test_gpu_tgrid.py / tests/test_gpu_hashgrid.py (level_dim 1..8, D = 2, tiled gridtype, F = 1..8).  tools/tiles_state.py does the same for the tiled
backwards.  Dev tool.

    python tools/table_state.py run TREE OUTDIR       # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/table_state.py cmp A B               # every tensor of every file torch.equal, no tolerance; exit 1 otherwise
"""
import ctypes as C
import os
import sys

import torch


def compare(a, b):
    bad = 0
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("file lists differ:", sorted(set(fa) ^ set(fb)))
        bad += 1
    for f in sorted(set(fa) & set(fb)):
        x, y = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
        if sorted(x) != sorted(y):
            print(f"{f}: tensor names differ")
            bad += 1
        for k in sorted(set(x) & set(y)):
            ok = x[k].shape == y[k].shape and x[k].dtype == y[k].dtype and bool(torch.equal(x[k], y[k]))
            nz = int((x[k] != 0).sum())
            print(f"{f:34s} {k:22s} n = {x[k].numel():10d} non-zero = {nz:10d}  {'equal' if ok else 'DIFFERENT'}")
            bad += not ok
    print("VERDICT", "every tensor equal" if bad == 0 else f"{bad} differ")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
from soccernerfs_amd import _lib, ops
from soccernerfs_amd.tcnn_compat import Encoding
from soccernerfs_amd.temporal_grid import TemporalGridEncoder

os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def cells(res, name, fx):
    """fixed-point cells of a table: a large table (config 4's main grid: 4 x 10^8 cells, a few percent touched) is saved as the indices and values of its
    non-zero cells, which determine it"""
    if fx.numel() <= 1 << 24:
        res[name] = fx.cpu()
    else:
        idx = fx.nonzero()[:, 0]
        res[name + ".index"], res[name + ".value"] = idx.to(torch.int32).cpu(), fx[idx].cpu()


def with_runs(runs, fn):
    os.environ["SNERF_TGRID_RUNS"] = runs
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("SNERF_TGRID_RUNS", None)


def tgrid_case(name, kw, R, S, seed):
    gen = torch.Generator().manual_seed(seed)
    enc = TemporalGridEncoder(**kw).to(DEV)
    D = enc.input_dim
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=gen) - 0.5).to(DEV))
    B = R * S
    o = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.9).to(DEV)
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    edges = torch.sort(torch.rand(R, S + 1, generator=gen) ** 3 * 1.6, dim=-1).values.to(DEV).contiguous()  # clustered, and rays leave the box
    times = torch.rand(R, generator=gen).to(DEV)
    times[0], times[1] = 0.0, 1.0
    mid = (edges[:, :-1] + edges[:, 1:]) / 2
    pts = (((o[:, None, :] + d[:, None, :] * mid[..., None]) + 1.0) / 2.0).reshape(B, 3)[:, :D].contiguous()
    gout = (torch.rand(B, enc.output_dim, generator=gen) - 0.5).to(DEV)
    gout[5:9] = 0.0
    modes = {"points": ops.coords_from_points(pts)}
    if D == 3:
        modes["rays"] = ops.coords_from_rays(o, d, times, edges, [[-1.0] * 3, [1.0] * 3], False)
    res = {}
    for mode, co in modes.items():
        for runs in ("1", "0"):
            fwd = torch.full((B, enc.output_dim), 7.0, device=DEV)
            with_runs(runs, lambda: _lib.check(L.snerf_tgrid_encode_fwd(C.byref(enc.desc), P(enc.embeddings), C.byref(co), None, P(times), S, C.c_int64(B), P(fwd),
                                                                        ops._stream()), "tgrid_encode_fwd"))
            fx = torch.zeros(enc.embeddings.numel(), dtype=torch.int64, device=DEV)
            with_runs(runs, lambda: _lib.check(L.snerf_tgrid_encode_bwd_fx(C.byref(enc.desc), C.byref(co), None, P(times), S, C.c_int64(B), P(gout), P(fx),
                                                                           ops._stream()), "tgrid_encode_bwd_fx"))
            res[f"{mode}_runs{runs}_fwd"] = fwd.cpu()
            cells(res, f"{mode}_runs{runs}_bwd_fx", fx)
        fwd = torch.full((B, enc.output_dim), 7.0, device=DEV)
        dydx = torch.full((B, enc.num_levels, D, enc.level_dim), 7.0, device=DEV)
        _lib.check(L.snerf_tgrid_encode_fwd_dydx(C.byref(enc.desc), P(enc.embeddings), C.byref(co), None, P(times), S, C.c_int64(B), P(fwd), P(dydx),
                                                 ops._stream()), "tgrid_encode_fwd_dydx")
        torch.cuda.synchronize()
        res[f"{mode}_dydx_fwd"], res[f"{mode}_dydx"] = fwd.cpu(), dydx.cpu()
    # explicit temporal rows (the reference-shaped API: always the per-sample kernel), points mode
    trow = enc.get_temporal_index(times.repeat_interleave(S)).contiguous()
    fwd = torch.full((B, enc.output_dim), 7.0, device=DEV)
    fx = torch.zeros(enc.embeddings.numel(), dtype=torch.int64, device=DEV)
    _lib.check(L.snerf_tgrid_encode_fwd(C.byref(enc.desc), P(enc.embeddings), C.byref(modes["points"]), P(trow), None, 1, C.c_int64(B), P(fwd), ops._stream()), "fwd rows")
    _lib.check(L.snerf_tgrid_encode_bwd_fx(C.byref(enc.desc), C.byref(modes["points"]), P(trow), None, 1, C.c_int64(B), P(gout), P(fx), ops._stream()), "bwd_fx rows")
    torch.cuda.synchronize()
    res["rows_fwd"] = fwd.cpu()
    cells(res, "rows_bwd_fx", fx)
    torch.save(res, os.path.join(out, f"tgrid_{name}.pt"))
    print("tgrid", name, "B", B, "tensors", len(res), flush=True)


def hash_case(name, D, cfg, B, seed):
    gen = torch.Generator().manual_seed(seed)
    enc = Encoding(D, {"otype": "HashGrid", **cfg}).to(DEV)
    with torch.no_grad():
        enc.params.copy_((torch.rand(enc.params.shape, generator=gen) - 0.5).to(DEV))
    F, nl = cfg["n_features_per_level"], cfg["n_levels"]
    x = torch.rand(B, D, generator=gen)
    x[0, 0], x[1, -1], x[2], x[3] = 1.0, 0.0, -0.13, 1.21  # borders and 'deformed' points outside the box (no bounds check, as tcnn)
    x = x.to(DEV)
    gout = ((torch.rand(B, nl * F, generator=gen) - 0.5) * 0.02).to(DEV)
    gout[7:11] = 0.0
    fwd = torch.full((B, nl * F), 7.0, device=DEV)
    _lib.check(L.snerf_hashgrid_encode_fwd(C.byref(enc.desc), P(enc.params), P(x), C.c_int64(B), P(fwd), ops._stream()), "hashgrid_encode_fwd")
    gt_fx = torch.zeros(enc.params.numel(), dtype=torch.int64, device=DEV)
    gx_fx = torch.zeros(B * D, dtype=torch.int64, device=DEV)
    _lib.check(L.snerf_hashgrid_encode_bwd_fx(C.byref(enc.desc), P(enc.params), P(x), C.c_int64(B), P(gout), P(gt_fx), P(gx_fx), ops._stream()), "hashgrid_encode_bwd_fx")
    torch.cuda.synchronize()
    res = {"fwd": fwd.cpu(), "bwd_x_fx": gx_fx.cpu()}
    cells(res, "bwd_table_fx", gt_fx)
    torch.save(res, os.path.join(out, f"hash_{name}.pt"))
    print("hash", name, "B", B, flush=True)


# ---- the sizes of bench.py's config-4 leg (NerfplayerNerfactoModelConfig: 4096 rays, 256 / 96 / 48 samples) ----
tgrid_case("config4_main", dict(input_dim=3, temporal_dim=64, num_levels=16, level_dim=2, log2_hashmap_size=19, desired_resolution=2048), 4096, 48, 31)
tgrid_case("config4_prop", dict(input_dim=3, temporal_dim=32, num_levels=5, level_dim=2, log2_hashmap_size=17, base_resolution=16, per_level_scale=2.0), 4096, 256, 32)
hash_case("full_nerfplayer", 3, dict(n_levels=16, n_features_per_level=2, base_resolution=16, per_level_scale=1.4472692012786865, log2_hashmap_size=18), 4096 * 48, 33)
# ---- the small cases of the tests ----
SMALL = [
    dict(input_dim=3, temporal_dim=64, num_levels=16, level_dim=2, log2_hashmap_size=15, desired_resolution=2048),  # the run-length tests' encoder
    dict(temporal_dim=8, level_dim=2, num_levels=4, log2_hashmap_size=10, base_resolution=4, per_level_scale=1.7),
    dict(temporal_dim=6, level_dim=4, num_levels=3, log2_hashmap_size=12, base_resolution=3, per_level_scale=2.0),
    dict(temporal_dim=5, level_dim=1, num_levels=2, log2_hashmap_size=8, base_resolution=4, per_level_scale=2.0, gridtype="tiled"),
    dict(temporal_dim=16, level_dim=8, num_levels=2, log2_hashmap_size=9, base_resolution=5, per_level_scale=1.5),
    dict(temporal_dim=4, level_dim=2, num_levels=2, log2_hashmap_size=8, base_resolution=4, per_level_scale=2.0, input_dim=2),
    dict(temporal_dim=4, level_dim=2, num_levels=3, log2_hashmap_size=8, base_resolution=4, per_level_scale=2.0, input_dim=1),
    dict(temporal_dim=7, level_dim=1, num_levels=3, log2_hashmap_size=10, base_resolution=6, per_level_scale=1.5, gridtype="tiled", align_corners=True),
]
for i, kw in enumerate(SMALL):
    tgrid_case(f"small{i}", kw, 129, 37, 40 + i)
HASH = [(3, dict(n_levels=16, n_features_per_level=2, base_resolution=16, per_level_scale=1.4472692012786865, log2_hashmap_size=15)),
        (3, dict(n_levels=3, n_features_per_level=4, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=12)),
        (3, dict(n_levels=5, n_features_per_level=8, base_resolution=5, per_level_scale=1.5, log2_hashmap_size=9)),
        (3, dict(n_levels=4, n_features_per_level=1, base_resolution=7, per_level_scale=1.6, log2_hashmap_size=11)),
        (2, dict(n_levels=6, n_features_per_level=2, base_resolution=8, per_level_scale=1.8, log2_hashmap_size=10)),
        (1, dict(n_levels=4, n_features_per_level=4, base_resolution=8, per_level_scale=2.0, log2_hashmap_size=8))]
for i, (D, cfg) in enumerate(HASH):
    hash_case(f"small{i}", D, cfg, 5000, 60 + i)

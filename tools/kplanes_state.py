"""Same results before and after a change to the K-Planes gradient kernels (csrc/kplanes.hip, csrc/kplanes_sorted.hip, csrc/kplanes_coords.hip,
csrc/proposal_bwd.hip and the header they share).  On seeded inputs it saves, per case,

  state_*.pt   what is determined bit for bit: the forward gather in points and rays mode, pass A's gvec (fp32 and bf16), G and the fix list of
               quotient_prepare (the list sorted by element: its append order is not fixed), grad_pts / grad_origins / grad_dirs of the coordinate
               backward (no atomics), the fixed-point cells of snerf_kplanes_gather_bwd_fx, and -- on two lattices of inputs on which every product
               and sum is exact in fp32 (tests/test_gpu_kplanes.py) -- the plane gradients of every float-atomic route;
  atomic_*.pt  what depends on the order of float atomics: the plane gradients of the direct, sorted, quotient and quotient-fallback
               (SNERF_PASSB_GROUPED=1) scatters and of snerf_kplanes_density_bwd.

Sizes: a nerf level (4096 rays x 48 samples, C = 32, scales 1, 2, 4, 8 of the preset's 64 x 64 x 64 x 100), a proposal level (C = 8, 128 x 128 x 128 x
100, 4096 x 128 samples), and small plane sets of the tests' sizes.  A tensor of more than 2^24 elements is saved as two 64-bit integer checksums of
its bits (plain and index-weighted sums): equal tensors give equal checksums.  Dev tool.

    python tools/kplanes_state.py run TREE OUTDIR       # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/kplanes_state.py cmp A B               # every tensor of every state_* file torch.equal, no tolerance; exit 1 otherwise
    python tools/kplanes_state.py noise P1 P2 P3 HEAD   # atomic_* files: per tensor the largest max|a - b| among three runs of one tree (its own order
                                                        # noise) and the largest max|head - p_i|; exit 1 where the second exceeds twice the first
"""
import ctypes as C
import itertools
import os
import sys

import torch


def compare(a, b):
    bad = n = 0
    fa, fb = (sorted(f for f in os.listdir(d) if f.startswith("state_")) for d in (a, b))
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
            print(f"{f:28s} {k:28s} n = {x[k].numel():10d} non-zero = {int((x[k] != 0).sum()):10d}  {'equal' if ok else 'DIFFERENT'}")
            bad += not ok
            n += 1
    print("VERDICT", f"{n} of {n} tensors equal" if bad == 0 else f"{bad} differ")
    return bad


def noise(parents, head):
    bad = 0
    for f in sorted(f for f in os.listdir(head) if f.startswith("atomic_")):
        ps = [torch.load(os.path.join(p, f)) for p in parents]
        h = torch.load(os.path.join(head, f))
        for k in sorted(h):
            own = max(float((a[k] - b[k]).abs().max()) for a, b in itertools.combinations(ps, 2))
            new = max(float((h[k] - p[k]).abs().max()) for p in ps)
            ok = new <= 2 * own
            print(f"{f:24s} {k:20s} max|grad| {float(ps[0][k].abs().max()):10.4g}  parent's own noise {own:10.4g}  head against parent {new:10.4g}  {'ok' if ok else 'ABOVE TWICE'}")
            bad += not ok
    print("VERDICT", "head within twice the parent's own order noise everywhere" if bad == 0 else f"{bad} above")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
if sys.argv[1] == "noise":
    sys.exit(1 if noise(sys.argv[2:5], sys.argv[5]) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
from soccernerfs_amd import _lib, ops
from soccernerfs_amd.plane_set import PlaneSet
from soccernerfs_amd.tcnn_compat import Network

os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def keep(res, name, t):
    t = t.detach().contiguous()
    if t.numel() <= 1 << 24:
        res[name] = t.cpu()
        return
    bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64).reshape(-1).to(torch.int64)
    idx = torch.arange(bits.numel(), device=bits.device) % 65521 + 1
    res[name + ".checksums"] = torch.stack([bits.sum(), (bits * idx).sum()]).cpu()


def grouped(on, fn):
    if on:
        os.environ["SNERF_PASSB_GROUPED"] = "1"
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("SNERF_PASSB_GROUPED", None)


def scatter_routes(ps, co, N, gout, feat, prefix, res):
    """plane gradients of every float-atomic route the plane set supports"""
    desc = ps.desc()
    g = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(C.byref(desc), P(ps.planes), C.byref(co), C.c_int64(N), P(gout), P(g), ops._stream()), "gather_bwd")
    res[prefix + "direct"] = g.cpu()
    for on in (False, True) if ps.C == 32 else (False,):
        tag = "_grouped" if on else ""
        ss = ops.SortedScatter(ps, N, DEV)
        ss.sort(co)
        g = torch.zeros_like(ps.planes)
        grouped(on, lambda: ss.scatter(ps.planes, co, gout, g))
        res[prefix + "sorted" + tag] = g.cpu()
        del ss
        if ps.concat and ps.C == 32:
            sq = ops.SortedScatter(ps, N, DEV, quotient=True)
            sq.sort(co)
            g = torch.zeros_like(ps.planes)
            grouped(on, lambda: sq.scatter_quotient(ps.planes, co, gout, feat, g))
            res[prefix + "quotient" + tag] = g.cpu()
            del sq


def case(name, C_, reso, concat, R, S, seed, density_bwd=False):
    gen = torch.Generator().manual_seed(seed)
    ps = PlaneSet(C_, reso, concat=concat, generator=gen)
    nc = ps.n_coords
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 1.1 - 0.2)
        ps.planes[torch.rand(ps.numel, generator=gen) < 0.002] = 0.0  # features vanish: the fix list is not empty
    ps = ps.to(DEV)
    desc = ps.desc()
    N = R * S
    o = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.9).to(DEV)
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    edges = torch.sort(torch.rand(R, S + 1, generator=gen) ** 2 * 1.6, dim=-1).values.to(DEV).contiguous()  # rays leave the box
    times = torch.rand(R, generator=gen).to(DEV)
    times[0], times[1] = 0.0, 1.0
    mid = (edges[:, :-1] + edges[:, 1:]) / 2
    pts = torch.cat([o[:, None, :] + d[:, None, :] * mid[..., None], (times * 2 - 1)[:, None, None].expand(R, S, 1)], dim=-1).reshape(N, 4)[:, :nc].contiguous()
    gout = (torch.rand(N, ps.out_dim, generator=gen) - 0.5).to(DEV)
    gout[5:9] = 0.0
    modes = {"points": ops.coords_from_points(pts)}
    if nc == 4:
        modes["rays"] = ops.coords_from_rays(o, d, times, edges, [[-1.0] * 3, [1.0] * 3], True)
    main = modes["rays" if nc == 4 else "points"]
    st, at = {}, {}
    feat = None
    for mode, co in modes.items():
        fwd = torch.full((N, ps.out_dim), 7.0, device=DEV)
        _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), P(ps.planes), C.byref(co), C.c_int64(N), P(fwd), ops._stream()), "gather_fwd")
        keep(st, f"fwd_{mode}", fwd)
        feat = fwd
    for bf16 in (0, 1):
        gvec = torch.zeros(len(reso) * len(ps.combs) * N * C_, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
        _lib.check(L.snerf_kplanes_gradvec(C.byref(desc), P(ps.planes), C.byref(main), C.c_int64(N), P(gout), P(gvec), bf16, ops._stream()), "gradvec")
        keep(st, "gvec_bf16" if bf16 else "gvec_fp32", gvec)
        del gvec
    if concat and C_ == 32:
        sq = ops.SortedScatter(ps, N, DEV, quotient=True)
        sq.quotient_prepare(gout, feat)
        n = int(sq.fix_count.item())
        lst = sq.fix_list[: 2 * n].view(n, 2)
        keep(st, "G", sq.G)
        keep(st, "fix_list_sorted", lst[torch.argsort(lst[:, 0])])
        del sq
    want = dict(grad_origins=torch.zeros(R, 3, device=DEV), grad_dirs=torch.zeros(R, 3, device=DEV)) if nc == 4 else {}
    keep(st, "grad_pts", ops.kplanes_gather_bwd_coords(desc, ps.planes, main, N, gout, **want)["grad_pts"])
    for k, t in want.items():
        keep(st, k, t)
    fx = torch.zeros(ps.numel, dtype=torch.int64, device=DEV)
    _lib.check(L.snerf_kplanes_gather_bwd_fx(C.byref(desc), P(ps.planes), C.byref(main), C.c_int64(N), P(gout), P(fx), ops._stream()), "gather_bwd_fx")
    keep(st, "bwd_fx", fx)
    del fx
    scatter_routes(ps, main, N, gout, feat, "", at)
    if density_bwd:
        net = Network(8, 1, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}, seed=seed + 3,
                      operands="bf16").to(DEV)
        assert L.snerf_kplanes_density_bwd_supported(C.byref(desc), C.byref(net.desc)) == 1
        gdens = (torch.rand(N, generator=gen) - 0.5).to(DEV)
        ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), device=DEV)
        gX, gp = torch.full((N, 8), -7.0, device=DEV), torch.zeros_like(ps.planes)
        a = (_lib.DensityBwdLevel * 1)()
        a[0].desc, a[0].planes, a[0].coords, a[0].N = C.addressof(desc), ps.planes.data_ptr(), C.addressof(main), N
        a[0].net, a[0].W, a[0].gdens = C.addressof(net.desc), net.params.data_ptr(), gdens.data_ptr()
        a[0].grad_planes, a[0].workspace, a[0].gX = gp.data_ptr(), ws.data_ptr(), gX.data_ptr()
        _lib.check(L.snerf_kplanes_density_bwd(a, 1, ops._stream()), "kplanes_density_bwd")
        torch.cuda.synchronize()
        keep(st, "density_bwd_gX", gX)
        at["density_bwd_planes"] = gp.cpu()
    torch.cuda.synchronize()
    torch.save(st, os.path.join(out, f"state_{name}.pt"))
    torch.save(at, os.path.join(out, f"atomic_{name}.pt"))
    print(name, "N", N, "state tensors", len(st), "atomic tensors", len(at), flush=True)


def lattice(kind, C_, concat, nc):
    """the two exact lattices of tests/test_gpu_kplanes.py: every float-atomic route is determined bit for bit"""
    gen = torch.Generator().manual_seed(77 if kind == "weights" else 78)
    ps = PlaneSet(C_, [r[:nc] for r in ([5, 5, 5, 3], [9, 9, 9, 3])], concat=concat, generator=gen)
    if kind == "weights":
        N = 3001
        choices = torch.tensor([-1.25] + [-1.0 + k / 8.0 for k in range(17)] + [1.25])
        pts = choices[torch.randint(0, len(choices), (N, nc), generator=gen)]
        with torch.no_grad():
            ps.planes.fill_(1.0)
    else:
        N = 1500
        pts = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, (N, nc), generator=gen)]
        if nc == 4:
            pts[:, 3] = torch.tensor([-1.0, 0.0, 1.0])[torch.randint(0, 3, (N,), generator=gen)]
        with torch.no_grad():
            ps.planes.copy_(torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (ps.numel,), generator=gen)])
            ps.planes[torch.rand(ps.numel, generator=gen) < 0.03] = 0.0
    gout = torch.randint(-8, 9, (N, ps.out_dim), generator=gen).to(torch.float32).to(DEV)
    ps, pts = ps.to(DEV), pts.contiguous().to(DEV)
    co = ops.coords_from_points(pts)
    desc = ps.desc()
    feat = torch.empty(N, ps.out_dim, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), P(ps.planes), C.byref(co), C.c_int64(N), P(feat), ops._stream()), "gather_fwd")
    res = {}
    scatter_routes(ps, co, N, gout, feat, "", res)
    torch.cuda.synchronize()
    torch.save(res, os.path.join(out, f"state_lattice_{kind}_C{C_}_nc{nc}.pt"))
    print("lattice", kind, C_, nc, "tensors", len(res), flush=True)


PRESET = [64, 64, 64, 100]
case("nerf_level", 32, [[r * m for r in PRESET[:3]] + PRESET[3:] for m in (1, 2, 4, 8)], True, 4096, 48, 51)
case("proposal_level", 8, [[128, 128, 128, 100]], False, 4096, 128, 52, density_bwd=True)
# ---- the small cases of tests/test_gpu_kplanes.py ----
for i, (C_, ms, concat, nc) in enumerate([(32, (1, 2, 4), True, 4), (8, (1,), False, 4), (16, (1, 3), False, 4), (32, (1, 2), True, 3), (8, (1, 2), True, 3)]):
    case(f"small{i}", C_, [[r * m for r in (11, 9, 7)] + [5][: nc - 3] for m in ms], concat, 47, 64, 60 + i)
for kind in ("weights", "values"):
    for C_, concat, nc in ((32, True, 4), (32, True, 3), (8, False, 4)):
        lattice(kind, C_, concat, nc)

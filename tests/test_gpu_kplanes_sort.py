"""GPU: the contract of snerf_kplanes_sort_samples (SortedScatter.sort), pinned directly.

For every plane segment q the sorted records must (1) hold every sample exactly once, (2) follow the FULL key order -- Morton code of the finest-scale
cell for spatial planes, time row * width + x cell for planes whose row axis is time -- and (3) carry the sample's two coordinates of that plane bit for
bit, with a zero fourth word.  The reference keys are formed on the host in float32 with the kernel's own expression, ((x + 1) / 2) * (res - 1) clamped
to [0, res - 1] and floored: no multiply-add to contract, so the integers are the same.

The lattice is where a binned sort can go wrong: sample counts around every chunk and wave boundary, grids that are neither square nor powers of two,
grids with one and with many coarse bins per plane, and batches that fall into one fine cell, one coarse bin, the clamped borders, or a few time rows."""
import ctypes as Ct
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

RESOLUTIONS = [
    [[8, 8, 8, 4]],
    [[11, 9, 7, 5], [22, 18, 14, 5]],
    [[64, 64, 64, 25], [128, 128, 128, 25]],
]
DISTRIBUTIONS = ("uniform", "identical", "one_bin", "corners", "raylike")
CASES = [(nc, ri, N) for nc in (4, 3) for ri in range(len(RESOLUTIONS)) for N in (1, 63, 257, 4097, 20000) if N < 20000 or ri == len(RESOLUTIONS) - 1]
RAY_SHAPES = {1: (1, 1), 63: (9, 7), 257: (1, 257), 4097: (17, 241), 20000: (625, 32)}  # N = rays x samples per ray


def _dev():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch.device("cuda:0")


def _resolutions(ri, n_coords):
    return [r[:n_coords] for r in RESOLUTIONS[ri]]


def _fine(reso):
    return [max(r[k] for r in reso) for k in range(len(reso[0]))]


def _cell(x, res):
    """floor of the clipped pixel coordinate, float32 throughout (csrc: axis_pix)"""
    assert x.dtype == torch.float32
    fx = ((x + 1.0) / 2.0) * float(res - 1)
    return fx.clamp(0.0, float(res - 1)).floor().to(torch.int64)


def _part1by1(v):
    v = v & 0xFFFF
    v = (v | (v << 8)) & 0x00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F
    v = (v | (v << 2)) & 0x33333333
    v = (v | (v << 1)) & 0x55555555
    return v


def _reference_keys(pts, reso):
    """[n_planes, N] int64: the full sort key of every sample on every plane"""
    nc = pts.shape[1]
    fine = _fine(reso)
    keys = []
    for a, b in itertools.combinations(range(nc), 2):
        ia, ib = _cell(pts[:, a], fine[a]), _cell(pts[:, b], fine[b])
        if nc == 4 and b == 3:
            keys.append(ib * fine[a] + ia)
        else:
            keys.append(_part1by1(ia) | (_part1by1(ib) << 1))
    return torch.stack(keys)


def _points(dist, N, reso, gen):
    nc = len(reso[0])
    fine = _fine(reso)
    if dist == "uniform":  # clamped borders included
        return torch.rand(N, nc, generator=gen) * 2.2 - 1.1
    if dist == "identical":  # one fine cell holds all N
        return (torch.rand(1, nc, generator=gen) * 2 - 1).expand(N, nc).contiguous()
    if dist == "one_bin":
        # an aligned 2 x 2 block of fine cells per spatial plane, one time row: consecutive keys inside one coarse bin of any sort that bins by
        # at least two low key bits, spread over the bin's cells
        cols = []
        for k in range(nc):
            r = fine[k]
            c0 = 2 * ((r - 1) // 4)
            width = 1.0 if k == 3 else 2.0
            pix = (c0 + 0.02 + torch.rand(N, generator=gen) * (width - 0.04)).clamp(max=float(r - 1))
            cols.append(pix / float(max(r - 1, 1)) * 2 - 1)
        return torch.stack(cols, -1).to(torch.float32).contiguous()
    if dist == "corners":  # exactly -1 and +1
        return (torch.randint(0, 2, (N, nc), generator=gen) * 2 - 1).to(torch.float32)
    assert dist == "raylike"  # 64 samples per ray, each ray at one of 3 times
    R = (N + 63) // 64
    o = torch.rand(R, 1, 3, generator=gen) * 2 - 1
    d = torch.nn.functional.normalize(torch.rand(R, 1, 3, generator=gen) * 2 - 1, dim=-1)
    t = torch.sort(torch.rand(R, 64, 1, generator=gen), dim=1).values
    p = o * 0.5 + d * t
    tm = torch.tensor([-0.7, 0.1, 0.55])[torch.randint(0, 3, (R,), generator=gen)].view(R, 1, 1).expand(R, 64, 1)
    return torch.cat([p, tm], -1).reshape(-1, 4)[:N, :nc].contiguous()


def _check_sorted(sorted_rec, pts, reso, what):
    """the three assertions of the contract, on the host"""
    N, nc = pts.shape
    pairs = list(itertools.combinations(range(nc), 2))
    rec = sorted_rec.cpu().view(torch.int32).view(len(pairs), N, 4)
    keys = _reference_keys(pts, reso)
    bits = pts.contiguous().view(torch.int32)
    for q, (a, b) in enumerate(pairs):
        ids = rec[q, :, 0].to(torch.int64)
        assert torch.equal(torch.sort(ids).values, torch.arange(N)), f"{what}: plane {q}: the sample ids are not a permutation of 0..N-1"
        seq = keys[q][ids]
        bad = (seq[1:] < seq[:-1]).nonzero()
        assert bad.numel() == 0, f"{what}: plane {q}: the key order descends at position {int(bad[0]) if bad.numel() else -1} ({bad.numel()} places)"
        assert torch.equal(rec[q, :, 1], bits[ids, a]) and torch.equal(rec[q, :, 2], bits[ids, b]), f"{what}: plane {q}: coordinates differ"
        assert int(rec[q, :, 3].abs().max()) == 0, f"{what}: plane {q}: the fourth word is not zero"


def _plane_set(reso, C=8, concat=False, gen=None):
    from soccernerfs_amd.plane_set import PlaneSet

    return PlaneSet(C, reso, concat=concat, generator=gen)


@pytest.mark.parametrize("n_coords,ri,N", CASES)
def test_sort_order_from_points(n_coords, ri, N):
    from soccernerfs_amd import ops

    dev = _dev()
    reso = _resolutions(ri, n_coords)
    ps = _plane_set(reso).to(dev)
    ss = ops.SortedScatter(ps, N, dev)
    gen = torch.Generator().manual_seed(1000 * ri + N + n_coords)
    for dist in DISTRIBUTIONS:
        pts = _points(dist, N, reso, gen)
        assert pts.shape == (N, n_coords) and pts.dtype == torch.float32
        ptsd = pts.to(dev)
        ss.sorted_rec.fill_(float("nan"))  # nothing of an earlier distribution may pass for this one's records
        ss.sort(ops.coords_from_points(ptsd))
        torch.cuda.synchronize()
        _check_sorted(ss.sorted_rec, pts, reso, f"{dist}, N={N}")


@pytest.mark.parametrize("n_coords,ri,N", CASES)
def test_sort_order_from_rays(n_coords, ri, N):
    """snerf_coords mode 1: positions from rays + bin edges, every ray at one of 3 times.  The box is [-2, 2]^3, so that the normalisation divides by a
    power of two and the host repeats the kernel's float32 arithmetic exactly."""
    from soccernerfs_amd import ops

    dev = _dev()
    reso = _resolutions(ri, n_coords)
    ps = _plane_set(reso).to(dev)
    R, S = RAY_SHAPES[N]
    gen = torch.Generator().manual_seed(2000 * ri + N + n_coords)
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.5
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    times = torch.tensor([0.15, 0.5, 0.8])[torch.randint(0, 3, (R,), generator=gen)].view(R, 1)
    eb = torch.cumsum(torch.rand(R, S + 1, generator=gen) * (3.0 / (S + 1)), -1)
    aabb = torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]])
    # kplanes_common.hpp: load_coords_ray, operation by operation in float32
    mid = eb[:, :-1] + eb[:, 1:]
    pos = o[:, None, :] + (d[:, None, :] * mid[..., None]) / 2.0
    p = ((pos - aabb[0]) / (aabb[1] - aabb[0])) * 2.0 - 1.0
    tt = (times * 2.0 - 1.0)[:, None, :].expand(R, S, 1)
    pts = torch.cat([p, tt], -1).reshape(N, 4)[:, :n_coords].contiguous()
    od, dd, td, ebd = o.to(dev), d.to(dev), times.to(dev), eb.to(dev)
    ss = ops.SortedScatter(ps, N, dev)
    ss.sorted_rec.fill_(float("nan"))
    ss.sort(ops.coords_from_rays(od, dd, td, ebd, aabb, True))
    torch.cuda.synchronize()
    _check_sorted(ss.sorted_rec, pts, reso, f"rays {R} x {S}")


@pytest.mark.parametrize("n_coords", [4, 3])
def test_sort_order_at_the_preset_resolution(n_coords):
    """The finest grid of the k-planes preset (1024^2, 100 time rows): the second level orders a bin by hundreds of counters -- more than one per
    thread, with carries between the waves of the workgroup -- where the small grids of the lattice leave it a handful.  Full key order, as above."""
    from soccernerfs_amd import ops

    dev = _dev()
    N = 20000
    reso = [r[:n_coords] for r in ([64, 64, 64, 100], [1024, 1024, 1024, 100])]
    ps = _plane_set(reso).to(dev)
    ss = ops.SortedScatter(ps, N, dev)
    gen = torch.Generator().manual_seed(4242 + n_coords)
    for dist in ("uniform", "raylike", "one_bin", "identical"):
        pts = _points(dist, N, reso, gen)
        if dist == "one_bin":  # a 64 x 64 block of fine cells instead of 2 x 2: many cells of few coarse bins
            centre = torch.rand(1, n_coords, generator=gen) * 1.8 - 0.9
            pts = (centre + (torch.rand(N, n_coords, generator=gen) - 0.5) * (128.0 / 1023.0)).contiguous()
            if n_coords == 4:
                pts[:, 3] = pts[0, 3]
        ptsd = pts.to(dev)
        ss.sorted_rec.fill_(float("nan"))
        ss.sort(ops.coords_from_points(ptsd))
        torch.cuda.synchronize()
        _check_sorted(ss.sorted_rec, pts, reso, f"preset grid, {dist}, N={N}")


@pytest.mark.parametrize("dist", ["identical", "one_bin"])
def test_scatter_downstream_of_a_skewed_sort(dist):
    """Pass B (product form and quotient form) behind the sort of a batch that sits in one fine cell / one coarse bin, against the sample-major
    scatter, at the tolerances tests/test_gpu_kplanes.py uses for the same comparisons.  Positive gradients: nothing cancels, so a sample that the
    sort lost or doubled moves a texel's sum by 1 / 4097 of itself, above the relative tolerance."""
    from soccernerfs_amd import _lib, ops

    dev = _dev()
    N, reso = 4097, RESOLUTIONS[2]
    gen = torch.Generator().manual_seed(77)
    ps = _plane_set(reso, C=32, concat=True, gen=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.8 + 0.2)
    ps = ps.to(dev)
    pts = _points(dist, N, reso, gen)
    gout = torch.rand(N, ps.out_dim, generator=gen) + 0.1
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    desc, L = ps.desc(), _lib.lib()
    direct = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(direct), ops._stream()))
    ss = ops.SortedScatter(ps, N, dev)
    ss.sort(co)
    got = torch.zeros_like(ps.planes)
    ss.scatter(ps.planes, co, goutd, got)
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=1e-5)
    feat = torch.empty(N, ps.out_dim, device=dev)
    _lib.check(L.snerf_kplanes_gather_fwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(feat), ops._stream()))
    sq = ops.SortedScatter(ps, N, dev, quotient=True)
    sq.sort(co)
    gotq = torch.zeros_like(ps.planes)
    sq.scatter_quotient(ps.planes, co, goutd, feat, gotq)
    torch.testing.assert_close(gotq, direct, rtol=1e-4, atol=2e-6 * float(direct.abs().max()))

"""GPU parity: K-Planes gather fwd/bwd (HIP, through the C ABI) vs the CPU oracle and the golden vectors.
Tolerances: features rtol 1e-5 / atol 1e-6; plane gradients (atomic order) rtol 1e-4."""
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    return torch.device("cuda:0")


def _plane_set_from_reference(grids, C, concat):
    from soccernerfs_amd.plane_set import PlaneSet

    reso = []
    for g in grids:
        # plane 0 = XY: [1,C,Y,X]; plane 1 = XZ: [1,C,Z,X]; plane 2 = XT: [1,C,T,X]
        reso.append([g[0].shape[3], g[0].shape[2], g[1].shape[2], g[2].shape[2]])
    ps = PlaneSet(C, reso, concat=concat)
    ps.load_reference(grids)
    return ps.to(_dev())


@pytest.mark.parametrize("tag", ["single", "multi", "prop"])
def test_gather_matches_golden(tag):
    from soccernerfs_amd import ops

    g = load_golden("g5_interp")
    C, n_scales, concat = [int(v) for v in g[f"{tag}_meta"]]
    grids = [[g[f"{tag}_plane_{s}_{p}"] for p in range(6)] for s in range(n_scales)]
    ps = _plane_set_from_reference(grids, C, bool(concat))
    pts = g[f"{tag}_pts"].to(_dev())
    feats = ops.interpolate_kplanes(pts, ps)
    torch.testing.assert_close(feats.cpu(), g[f"{tag}_feats"], rtol=1e-5, atol=1e-6)
    feats.backward(g[f"{tag}_gout"].to(_dev()))
    got = ps.to_reference(ps.planes.grad.cpu())
    for s in range(n_scales):
        for p in range(6):
            torch.testing.assert_close(got[s][p], g[f"{tag}_grad_{s}_{p}"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("C,ms,concat,lo,hi", [(32, (1, 2, 4), True, -1.2, 1.2), (8, (1,), False, -0.1, 1.1), (16, (1, 3), False, -1.0, 1.0)])
def test_gather_matches_oracle_random(C, ms, concat, lo, hi):
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd import ops

    gen = torch.Generator().manual_seed(7)
    base = (11, 9, 7, 5)
    grids = []
    for m in ms:
        reso = [r * m for r in base[:3]] + [base[3]]
        grids.append([torch.rand(1, C, reso[b], reso[a], generator=gen) + 0.2 for (a, b) in KO.COO_COMBS])
    N = 3001  # ragged: not a multiple of the block size
    pts = torch.rand(N, 4, generator=gen) * (hi - lo) + lo
    leaves = [[t.clone().requires_grad_(True) for t in sc] for sc in grids]
    ref = KO.interpolate_kplanes(pts, leaves, concat)
    gout = torch.rand(ref.shape, generator=gen) - 0.5
    ref.backward(gout)
    ps = _plane_set_from_reference(grids, C, concat)
    out = ops.interpolate_kplanes(pts.to(_dev()), ps)
    torch.testing.assert_close(out.cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    out.backward(gout.to(_dev()))
    got = ps.to_reference(ps.planes.grad.cpu())
    for s in range(len(ms)):
        for p in range(6):
            torch.testing.assert_close(got[s][p], leaves[s][p].grad, rtol=1e-4, atol=2e-6)


def test_gather_from_rays_matches_oracle():
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd import ops

    gen = torch.Generator().manual_seed(11)
    R, S, C = 37, 48, 8
    grids = [torch.rand(1, C, r2, r1, generator=gen) + 0.1 for (r1, r2) in [(12, 10), (12, 8), (12, 4), (10, 8), (10, 4), (8, 4)]]
    aabb = torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]])
    o = torch.rand(R, 3, generator=gen) * 2 - 1
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    times = torch.rand(R, 1, generator=gen)
    eb = torch.cumsum(torch.rand(R, S + 1, generator=gen) * 0.06, -1)
    pos = KO.sample_positions(o, d, eb[:, :-1], eb[:, 1:])
    for rescale in (True, False):
        p = KO.normalize_positions(pos, aabb)
        p = p * 2 - 1 if rescale else p
        pts = torch.cat([p, (times * 2 - 1)[:, None, :].expand(R, S, 1)], -1).reshape(-1, 4)
        ref = KO.interpolate_kplanes(pts, [grids], False)
        ps = _plane_set_from_reference([grids], C, False)
        dev = _dev()
        out = ops.interpolate_kplanes_rays(ps, o.to(dev), d.to(dev), times.to(dev), eb.to(dev), aabb, rescale)
        torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-6)


def test_gather_full_size_properties():
    """BASELINE config-2 sizes (5 scales x 6 planes, C=32, 64*4096 samples): size-independent properties.
    Constant planes k => every feature equals k^6 and every plane's gradient sums to k^5 * sum(gout)."""
    from soccernerfs_amd import ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    reso = [[64 * m, 64 * m, 64 * m, 100] for m in (1, 2, 4, 8, 16)]
    ps = PlaneSet(32, reso, concat=True, device=dev)
    k = 1.25
    with torch.no_grad():
        ps.planes.fill_(k)
    N = 64 * 4096
    pts = torch.rand(N, 4, device=dev) * 2.2 - 1.1
    out = ops.interpolate_kplanes(pts, ps)
    assert out.shape == (N, 160)
    torch.testing.assert_close(out, torch.full_like(out, k**6), rtol=2e-6, atol=0)
    gout = torch.rand_like(out) - 0.25
    out.backward(gout)
    g = ps.planes.grad
    for s in range(5):
        expect = (gout[:, s * 32:(s + 1) * 32].double().sum(0) * k**5).cpu()
        for p in range(6):
            got = ps.plane_view(s, p, g).double().sum((0, 1)).cpu()
            torch.testing.assert_close(got, expect, rtol=2e-4, atol=1e-3)
    # linearity of the backward in grad_out
    ps.planes.grad = None
    out2 = ops.interpolate_kplanes(pts, ps)
    out2.backward(2.0 * gout)
    torch.testing.assert_close(ps.planes.grad, 2.0 * g, rtol=1e-3, atol=1e-3)


def test_gather_empty_and_errors():
    from soccernerfs_amd import ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    ps = PlaneSet(8, [[4, 4, 4, 2]], concat=False, device=dev)
    out = ops.interpolate_kplanes(torch.zeros(0, 4, device=dev), ps)
    assert out.shape == (0, 8)
    bad = PlaneSet(8, [[4, 4, 4, 2]], concat=False, device=dev)
    bad.C = 12
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.interpolate_kplanes(torch.zeros(4, 4, device=dev), bad)


@pytest.mark.parametrize("C,ms,concat,N", [(32, (1, 2, 4), True, 3001), (8, (1,), False, 5000), (32, (1, 2, 4, 8, 16), True, 64 * 512)])
def test_sorted_scatter_equals_direct_scatter_and_oracle(C, ms, concat, N):
    """The sorted variant (counting sort by texel key + run-length combining) gives the same plane gradients as the
    sample-major scatter (and, for the small cases, as the oracle's autograd)."""
    import ctypes as Ct
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    gen = torch.Generator().manual_seed(21)
    base = (11, 9, 7, 5) if N < 20000 else (64, 64, 64, 100)
    ps = PlaneSet(C, [[r * m for r in base[:3]] + [base[3]] for m in ms], concat=concat, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) + 0.2)
    ref_grids = [[t.clone().requires_grad_(True) for t in sc] for sc in ps.to_reference()]
    ps = ps.to(dev)
    pts = torch.rand(N, 4, generator=gen) * 2.2 - 1.1
    pts[: N // 3, 3] = 0.25  # many samples share a time row, as rays of one image do
    pts[: N // 8] = pts[0]   # heavy duplicates: long equal-key runs
    gout = torch.rand(N, ps.out_dim, generator=gen) - 0.5
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    direct = torch.zeros_like(ps.planes)
    desc = ps.desc()
    _lib.check(_lib.lib().snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(direct),
                                                   ops._stream()))
    ss = ops.SortedScatter(ps, N, dev)
    ss.sort(co)
    # the order of every plane is a permutation of 0..N-1
    sn = ss.sorted_rec[:, 0].contiguous().view(torch.int32).view(-1, N)
    assert torch.equal(torch.sort(sn, dim=1).values, torch.arange(N, device=dev, dtype=torch.int32).expand_as(sn))
    got = torch.zeros_like(ps.planes)
    ss.scatter(ps.planes, co, goutd, got)
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=1e-5)
    # bf16 gradient vectors between pass A and pass B (the production path with 16-bit MLP operands): every contribution is rounded to 8
    # significant bits before the fp32 accumulation -> relative L2 error ~2^-9 / sqrt(#contributions), no bias
    ss16 = ops.SortedScatter(ps, N, dev, gvec_dtype=torch.bfloat16)
    ss16.sort(co)
    got16 = torch.zeros_like(ps.planes)
    ss16.scatter(ps.planes, co, goutd, got16)
    assert float((got16 - direct).norm() / direct.norm()) < 3e-3
    assert abs(float((got16 - direct).sum() / direct.abs().sum())) < 1e-4
    if N < 20000:
        ref = KO.interpolate_kplanes(pts, ref_grids, concat)
        ref.backward(gout)
        g = ps.to_reference(got.cpu())
        for s in range(len(ms)):
            for p in range(6):
                torch.testing.assert_close(g[s][p], ref_grids[s][p].grad, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("ms,N,zeros", [((1, 2, 4), 3000, False), ((1, 2), 1500, True), ((1, 2, 4, 8, 16), 100000, False), ((1,), 257, True)])
def test_quotient_scatter_equals_direct_scatter(ms, N, zeros):
    """Quotient form of the sorted scatter -- g_q = (gfeat .* feat) ./ v_q with v_q re-interpolated in pass B -- against the sample-major
    scatter and the product-form sorted scatter.  `zeros`: exact zeros planted in the planes, so that features vanish and the listed rows go
    through the exact fix-up (where the quotient alone would lose a plane's gradient)."""
    _quotient_against_direct(ms, N, zeros, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("ms,N,zeros,n_coords", [((1, 2), 1500, True, 4), ((1,), 257, True, 4), ((1,), 257, True, 3)])
def test_quotient_fallback_kernel_equals_direct_scatter(ms, N, zeros, n_coords, monkeypatch):
    """The same comparison, same bounds, with pass B forced onto scatter_grouped_kernel<NP, float, QUOT> -- the quotient form's kernel for
    2^30 <= N * C * n_scales < 2^31, which no batch of a test's size reaches by itself.  The two smallest cases: a partial chunk (1500 = 5 * 256 +
    220 entries per segment; 257 = one full chunk and a chunk of one entry and 255 null records) and zero texels; one of them on three planes."""
    monkeypatch.setenv("SNERF_PASSB_GROUPED", "1")  # read by the library at every launch
    _quotient_against_direct(ms, N, zeros, n_coords)


def _quotient_against_direct(ms, N, zeros, n_coords):
    import ctypes as Ct
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    gen = torch.Generator().manual_seed(33)
    base = (11, 9, 7, 5) if N < 20000 else (64, 64, 64, 100)
    ps = PlaneSet(32, [[r * m for r in base[:3]] + [base[3]][: n_coords - 3] for m in ms], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 1.2 - 0.3)  # both signs, values near zero included
        if zeros:
            # whole texels of scale 0 / plane 0 and a sprinkle everywhere: interpolated values that are exactly 0.0f
            ps.planes[: 32 * 40] = 0.0
            ps.planes[torch.rand(ps.numel, generator=gen) < 0.02] = 0.0
        if zeros:
            ps.plane_view(0, 2)[-1, -1, :] = 3e-39  # a SUBNORMAL texel: counts as zero in the quotient form (v_rcp_f32 may flush it)
    ps = ps.to(dev)
    pts = torch.rand(N, 4, generator=gen) * 2.2 - 1.1
    pts[: N // 3, 3] = 0.25
    pts[: N // 8] = pts[0]
    pts = pts[:, :n_coords].contiguous()
    if zeros:
        pts[N // 2: N // 2 + 64] = -1.0  # the all-zero corner texel of plane 0 exactly (weights 1, 0, 0, 0)
        pts[N // 2 + 64: N // 2 + 96] = 1.0  # the subnormal last texel of plane 2 exactly
    gout = torch.rand(N, ps.out_dim, generator=gen) - 0.5
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    desc = ps.desc()
    L = _lib.lib()
    direct = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(direct), ops._stream()))
    feat = torch.empty(N, ps.out_dim, device=dev)
    _lib.check(L.snerf_kplanes_gather_fwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(feat), ops._stream()))
    # planted zeros make thousands of features vanish at once.  (r06, ADVICE) The DEFAULT list holds the worst case (every feature of every sample),
    # so no input -- imported all-zero planes included -- can overflow it; a smaller list is the caller's explicit choice
    ss = ops.SortedScatter(ps, N, dev, quotient=True)
    assert ss.gvec is None and ss.fix_capacity == N * ps.out_dim
    assert ops.SortedScatter(ps, N, dev, quotient=True, fix_capacity=7).fix_capacity == 7
    ss.sort(co)
    got = torch.zeros_like(ps.planes)
    ss.scatter_quotient(ps.planes, co, goutd, feat, got)
    n_fix = int(ss.fix_count.item())
    assert (n_fix > 0) == zeros
    ss.check_fix_overflow()  # nothing was dropped
    if zeros:
        # the same scatter with a list that is too short must not lose gradient terms SILENTLY: the fix-up records the demanded count
        # and check_fix_overflow raises
        small = ops.SortedScatter(ps, N, dev, quotient=True, fix_capacity=max(n_fix // 2, 1))
        small.sort(co)
        small.scatter_quotient(ps.planes, co, goutd, feat, torch.zeros_like(ps.planes))
        assert int(small.fix_peak.item()) == n_fix
        with pytest.raises(RuntimeError, match="fix list holds"):
            small.check_fix_overflow()
    scale = float(direct.abs().max())
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=2e-6 * scale)
    assert float((got - direct).norm() / direct.norm()) < 2e-6
    # scale ranges (the multi-GPU exchange scatters the finest scale first) add up to the whole
    if len(ms) > 1:
        parts = torch.zeros_like(ps.planes)
        ss.quotient_prepare(goutd, feat)
        ss.quotient_scatter_scales(ps.planes, co, goutd, parts, len(ms) - 1, len(ms))
        ss.quotient_scatter_scales(ps.planes, co, goutd, parts, 0, len(ms) - 1)
        torch.testing.assert_close(parts, got, rtol=1e-4, atol=2e-6 * scale)


@pytest.mark.gpu
def test_quotient_scatter_when_the_product_of_six_normal_values_underflows():
    """A feature can vanish although no plane value does: six values of 2e-7 multiply to 6.4e-41, below the smallest normal float.  The
    quotient G / v_q has lost (almost) all bits there; quotient_prepare zeroes G for the channel, lists the row, and the fix-up adds the exact
    product-form term to EVERY plane (these gradients used to be dropped or mangled)."""
    import ctypes as Ct
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    gen = torch.Generator().manual_seed(4)
    ps = PlaneSet(32, [[11, 9, 7, 5], [22, 18, 14, 5]], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.8 + 0.2)
        for q in range(6):
            ps.plane_view(0, q)[0:2, 0:2, :] = 2e-7  # the first cell of every plane of scale 0
    ps = ps.to(dev)
    N = 600
    pts = torch.rand(N, 4, generator=gen) * 2 - 1
    pts[:64] = -1.0 + 0.04 + 0.1 * torch.rand(64, 4, generator=gen)  # inside the first cell of every axis (cell widths 0.2 .. 0.5)
    gout = torch.rand(N, ps.out_dim, generator=gen) + 0.5
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    desc = ps.desc()
    L = _lib.lib()
    direct = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(direct), ops._stream()))
    feat = torch.empty(N, ps.out_dim, device=dev)
    _lib.check(L.snerf_kplanes_gather_fwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(feat), ops._stream()))
    assert float(feat[:64, :32].abs().max()) < 1.2e-38  # the features of scale 0 underflowed ...
    ss = ops.SortedScatter(ps, N, dev, quotient=True, fix_capacity=N * ps.out_dim)  # 64 samples x 32 channels vanish at once
    ss.sort(co)
    got = torch.zeros_like(ps.planes)
    ss.scatter_quotient(ps.planes, co, goutd, feat, got)
    assert int(ss.fix_count.item()) >= 64
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=2e-6 * float(direct.abs().max()))
    for q in range(6):  # ... but every plane's gradient there (g * (2e-7)^5 ~ 3e-34 per sample) arrives, to fp32 accuracy
        a, b = ps.plane_view(0, q, got)[0:2, 0:2, :], ps.plane_view(0, q, direct)[0:2, 0:2, :]
        assert float(b.abs().min()) > 1e-36
        torch.testing.assert_close(a, b, rtol=2e-4, atol=0)


@pytest.mark.gpu
def test_quotient_scatter_with_one_subnormal_plane_value_beside_a_normal_feature():
    """ONE plane value is subnormal (not zero) while the other five multiply to more than 1, so the feature is a normal number and
    G = gfeat * feat is usable -- but v_rcp_f32 may flush the subnormal divisor.  Pass B divides by it in IEEE arithmetic there; that plane's
    gradient (gfeat * the others' product) used to be dropped silently."""
    import ctypes as Ct
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.plane_set import PlaneSet

    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    ps = PlaneSet(32, [[11, 9, 7, 5], [22, 18, 14, 5]], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 2.0 + 2.0)  # every value in [2, 4): five of them multiply to >= 32
        ps.plane_view(1, 4)[0:2, 0:2, :] = 3e-39                           # the first cell of plane YT of scale 1: subnormal
    ps = ps.to(dev)
    N = 500
    pts = torch.rand(N, 4, generator=gen) * 2 - 1
    pts[:80, 1] = -1.0 + 0.05 * torch.rand(80, generator=gen)  # y and t inside the first cell of scale 1 (cell widths 2 / 17 and 0.5)
    pts[:80, 3] = -1.0 + 0.3 * torch.rand(80, generator=gen)
    gout = torch.rand(N, ps.out_dim, generator=gen) + 0.5
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    desc = ps.desc()
    L = _lib.lib()
    direct = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(direct), ops._stream()))
    feat = torch.empty(N, ps.out_dim, device=dev)
    _lib.check(L.snerf_kplanes_gather_fwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(feat), ops._stream()))
    f1 = feat[:80, 32:64].abs()
    assert float(f1.min()) >= 1.17549435e-38 and float(f1.max()) < 1e-35  # normal numbers, carried by a subnormal factor
    ss = ops.SortedScatter(ps, N, dev, quotient=True)
    ss.sort(co)
    got = torch.zeros_like(ps.planes)
    ss.scatter_quotient(ps.planes, co, goutd, feat, got)
    assert int(ss.fix_count.item()) == 0  # nothing vanished: no fix-up involved
    a, b = ps.plane_view(1, 4, got)[0:2, 0:2, :], ps.plane_view(1, 4, direct)[0:2, 0:2, :]
    assert float(b.abs().min()) > 1.0  # gfeat * (>= 32) summed over the cell's samples
    torch.testing.assert_close(a, b, rtol=2e-4, atol=0)
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=2e-6 * float(direct.abs().max()))


# ---- an exact lattice: every product and every sum is exact in fp32, so no route may differ from another in a single bit ----
_LATTICE_RES = [[5, 5, 5, 3], [9, 9, 9, 3]]


def _lattice_inputs(kind, C, concat, n_coords):
    """kind "weights": planes all 1.0; coordinates from {-1.25, -1 + k/8 (k = 0..16), 1.25}, so every tap weight is a multiple of 1/8 (1/4 at
    resolution 5, 1/2 at 9), every plane value is exactly 1 (and v_rcp_f32(1) = 1); N = 3001, |sum| <= 3001 * 8 units of 2^-9.
    kind "values": coordinates on texel centres of both scales (space {-1, -0.5, 0, 0.5, 1}, time {-1, 0, 1}: weights 1 and 0), texels from
    {0.5, 1, 2} with ~3 % exactly 0.0 (features vanish: the fix list and its one-zero / several-zeros branches run); N = 1500, a term is at most
    8 * 2^5 in units of 2^-5: sums below 2^24 units.  grad_out: integers in [-8, 8]."""
    from soccernerfs_amd.plane_set import PlaneSet

    gen = torch.Generator().manual_seed(77 if kind == "weights" else 78)
    ps = PlaneSet(C, [r[:n_coords] for r in _LATTICE_RES], concat=concat, generator=gen)
    if kind == "weights":
        N = 3001
        choices = torch.tensor([-1.25] + [-1.0 + k / 8.0 for k in range(17)] + [1.25])
        pts = choices[torch.randint(0, len(choices), (N, n_coords), generator=gen)]
        with torch.no_grad():
            ps.planes.fill_(1.0)
    else:
        N = 1500
        pts = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])[torch.randint(0, 5, (N, n_coords), generator=gen)]
        if n_coords == 4:
            pts[:, 3] = torch.tensor([-1.0, 0.0, 1.0])[torch.randint(0, 3, (N,), generator=gen)]
        with torch.no_grad():
            ps.planes.copy_(torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (ps.numel,), generator=gen)])
            ps.planes[torch.rand(ps.numel, generator=gen) < 0.03] = 0.0
    gout = torch.randint(-8, 9, (N, ps.out_dim), generator=gen).to(torch.float32)
    return ps, pts.contiguous(), gout


def _lattice_oracle(ps, pts, gout):
    """Plane gradients in float64 (autograd through the oracle's bilinear restatement, over this plane set's axis pairs), rounded to fp32."""
    from oracle import kplanes_oracle as KO

    grids = [[t.double().requires_grad_(True) for t in sc] for sc in ps.to_reference()]
    p64 = pts.double()
    outs = []
    for sc in grids:
        prod = 1.0
        for plane, comb in zip(sc, ps.combs):
            prod = prod * KO.bilinear_plane(plane, p64[:, list(comb)])
        outs.append(prod)
    feat = torch.cat(outs, dim=-1) if ps.concat else sum(outs)
    feat.backward(gout.double())
    flat = torch.zeros(ps.numel, dtype=torch.float64)
    for s, sc in enumerate(grids):
        for p, plane in enumerate(sc):
            ps.plane_view(s, p, flat).copy_(plane.grad[0].permute(1, 2, 0))
    return flat.to(torch.float32)


def _lattice_routes(ps, pts, gout, monkeypatch):
    """name -> plane gradients of every scatter route that supports the plane set, on the device."""
    import ctypes as Ct
    from soccernerfs_amd import _lib, ops

    dev = _dev()
    N = pts.shape[0]
    ps = ps.to(dev)
    ptsd, goutd = pts.to(dev), gout.to(dev)
    co = ops.coords_from_points(ptsd)
    desc = ps.desc()
    L = _lib.lib()
    out = {}
    out["direct"] = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(out["direct"]), ops._stream()))
    fx = torch.zeros(ps.numel, dtype=torch.int64, device=dev)
    _lib.check(L.snerf_kplanes_gather_bwd_fx(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(goutd), ops._ptr(fx), ops._stream()))
    out["fixed_point"] = torch.zeros_like(ps.planes)
    ops.fx_to_float(fx, out["fixed_point"])
    quot = ps.C == 32 and ps.concat
    feat = torch.empty(N, ps.out_dim, device=dev)
    _lib.check(L.snerf_kplanes_gather_fwd(Ct.byref(desc), ops._ptr(ps.planes), Ct.byref(co), Ct.c_int64(N), ops._ptr(feat), ops._stream()))
    n_fix = None
    for grouped in (False, True):  # pass B: scatter_halfwave_kernel, then (C = 32) scatter_grouped_kernel through the library's switch
        if grouped:
            if ps.C != 32:
                break
            monkeypatch.setenv("SNERF_PASSB_GROUPED", "1")
        tag = "_grouped" if grouped else ""
        ss = ops.SortedScatter(ps, N, dev)
        ss.sort(co)
        out["sorted" + tag] = torch.zeros_like(ps.planes)
        ss.scatter(ps.planes, co, goutd, out["sorted" + tag])
        if quot:
            sq = ops.SortedScatter(ps, N, dev, quotient=True)
            sq.sort(co)
            out["quotient" + tag] = torch.zeros_like(ps.planes)
            sq.scatter_quotient(ps.planes, co, goutd, feat, out["quotient" + tag])
            n_fix = int(sq.fix_count.item())
    monkeypatch.delenv("SNERF_PASSB_GROUPED", raising=False)
    return {k: v.detach().cpu() for k, v in out.items()}, n_fix


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["weights", "values"])
@pytest.mark.parametrize("C,concat,n_coords", [(32, True, 4), (32, True, 3), (8, False, 4)])
def test_every_scatter_route_is_exact_on_a_lattice(kind, C, concat, n_coords, monkeypatch):
    """On these inputs every product and sum of the plane-gradient scatter is exact in fp32, so neither the order of the atomics nor the form
    (product, quotient, fixed point) can change a bit: the direct scatter, its fixed-point form, the sorted product form (fp32 vectors) and, for
    C = 32 with concatenated scales, the quotient form -- each sorted route through both pass-B kernels -- must all equal the float64 oracle
    rounded to fp32."""
    ps, pts, gout = _lattice_inputs(kind, C, concat, n_coords)
    want = _lattice_oracle(ps, pts, gout)
    assert float(want.abs().max()) > 0
    got, n_fix = _lattice_routes(ps, pts, gout, monkeypatch)
    expected = {"direct", "fixed_point", "sorted"} | ({"sorted_grouped"} if C == 32 else set()) | ({"quotient", "quotient_grouped"} if C == 32 and concat else set())
    assert set(got) == expected
    if C == 32 and concat:
        assert (n_fix > 0) == (kind == "values")  # the planted zero texels reach the fix list
    for name, g in got.items():
        bad = int((g != want).sum())
        print(f"{kind} C={C} n_coords={n_coords} {name}: {bad} of {g.numel()} cells differ from the oracle, max |diff| {float((g - want).abs().max()):.3g}")
    for name, g in got.items():
        assert torch.equal(g, want), name

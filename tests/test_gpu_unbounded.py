"""GPU: unbounded scenes on the fused path -- snerf_coords.contract = 1, the L-inf scene contraction evaluated where the kernels derive a
sample's coordinate from its ray.

1  Coordinates, by EQUALITY: every kernel that derives coordinates from rays is run in mode 1 with contract = 1 and in mode 0 on points that
   the CPU computed in float32 as SceneContraction(order=inf)(o + (d * mid) / 2) / 2 (tests/unbounded_reference.expected_points, through the
   package's torch module); outputs are compared with torch.equal.  The rays are dyadic and hold, per case, samples inside the unit cube, on its
   face (m == 1: the second branch), outside with each axis and sign largest, two-axis ties and m = 2^k up to 1024.  The mode-0 side is what the
   existing lattices pin to float64, so the chain closes.  Plane and weight gradients of snerf_kplanes_density_bwd are sums of float atomics
   (no fixed-point route exists for that kernel): its gX is compared by equality, its plane gradients by the fixed-point route of the plane
   gather on the same gX.
2  The quotient scatter with far samples crowded against p -> 1, against the product form at the tolerance of tests/test_gpu_kplanes.py.
3  The coordinate gradient (grad_pts, grad_origins, grad_dirs) against the float64 restatement, bound = 5 x the float32 restatement's deviation
   (profiles/r27_unbounded_deviations.json).
4  KPlanesTrainer(bounded=False) against KPlanesModel(bounded=False) + torch.optim.Adam; the default bf16 path with the fused kernels asserted;
   frozen time planes and a 3-coordinate model; deterministic mode.
5  KPlanesRenderer from an unbounded trainer: both tails against the trainer's eval forward, rays that point away, a checkpoint round trip."""
import ctypes as C

import pytest
import torch

from tests import pose_reference as PR
from tests import unbounded_reference as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _net(d_in, hidden, n_hidden, d_out, out_act, operands=1):
    from soccernerfs_amd import _lib

    d = _lib.MlpDesc()
    d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d_in, hidden, n_hidden, d_out, 1, out_act, operands
    return d


def _plane_set(Cn, view, seed):
    """C = 8: one summed scale (a proposal level's shape); C = 32: two concatenated scales (the field's).  view "4" / "3" / "frozen"."""
    from soccernerfs_amd.plane_set import PlaneSet

    gen = torch.Generator().manual_seed(seed)
    base = [12, 10, 9, 3] if view != "3" else [12, 10, 9]
    ms = (1,) if Cn == 8 else (1, 2)
    ps = PlaneSet(Cn, [[r * m for r in base[:3]] + base[3:] for m in ms], concat=Cn == 32, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.8 + 0.2)
    ps = ps.to(DEV)
    return ps, (ps.space_desc() if view == "frozen" else ps.desc())


class _Pair:
    """One ray set on the device, as mode-1 contracted coordinates and as mode-0 points from the CPU's float32 expression."""

    def __init__(self, rs, nc):
        from soccernerfs_amd import ops

        g = lambda t: t.to(DEV).contiguous()
        self.o, self.d, self.eb, self.t = g(rs["origins"]), g(rs["dirs"]), g(rs["ebins"]), g(rs["times"])
        self.pts_cpu = U.expected_points(rs, nc)
        self.pts = g(self.pts_cpu)
        self.N = self.pts.shape[0]
        self.rays = ops.coords_from_rays(self.o, self.d, self.t if nc == 4 else None, self.eb, None, True, contract=True)
        self.points = ops.coords_from_points(self.pts)
        assert self.rays.contract == 1 and self.rays.mode == 1 and self.points.contract == 0


def _both(pair, fn):
    a, b = fn(pair.rays), fn(pair.points)
    torch.cuda.synchronize()
    return a, b


def _equal(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        same = torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert same, f"{what}: {k} differs in {int((x != y).sum())} of {x.numel()} cells"


@pytest.mark.parametrize("Cn", [8, 32])
@pytest.mark.parametrize("view", ["4", "3", "frozen"])
@pytest.mark.parametrize("shape", U.RAY_SHAPES, ids=lambda s: f"R{s[0]}-S{s[1]}")
def test_contracted_coordinates_equal_the_cpu_expression(shape, view, Cn):
    from soccernerfs_amd import _lib, ops
    from tests.test_gpu_kplanes_sort import _check_sorted

    L = _lib.lib()
    R, S = shape
    nc = 4 if view == "4" else 3
    ps, desc = _plane_set(Cn, view, 17)
    gen = torch.Generator().manual_seed(5)
    W = ps.out_dim
    reso = [r[:nc] for r in ps.resolutions]
    rounds = U.coordinate_rounds(R, S)
    if Cn == 8:
        net = _net(8, 64, 1, 1, 0)
        Wp = ((torch.rand(8 * 64 + 64, generator=gen) * 2 - 1) * 0.4).to(DEV)
        n_ws = int(L.snerf_mlp_gw_workspace_floats(C.byref(net)))
        assert L.snerf_kplanes_density_fwd_supported(C.byref(desc), C.byref(net)) == 1
        dbwd = bool(L.snerf_kplanes_density_bwd_supported(C.byref(desc), C.byref(net)))
        assert dbwd == (view == "4")
    else:
        sig, col = _net(W, 128, 1, 16, 0), _net(15, 64, 2, 3, 1)
        Ws = ((torch.rand(W * 128 + 128 * 16, generator=gen) * 2 - 1) * 0.2).to(DEV)
        Wc = ((torch.rand(15 * 64 + 64 * 64 + 64 * 3, generator=gen) * 2 - 1) * 0.3).to(DEV)
        assert L.snerf_kplanes_field_fwd_supported(C.byref(desc), C.byref(sig), C.byref(col)) == 1
    for k, rs in enumerate(rounds):
        pr = _Pair(rs, nc)
        N, what = pr.N, f"R{R} S{S} {view} C{Cn} round {k}"
        gout = (torch.rand(N, W, generator=gen) - 0.5).to(DEV)

        def gather(co):
            out = torch.empty(N, W, device=DEV)
            _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(out), _st()), "gather_fwd")
            fx = torch.zeros(ps.numel, dtype=torch.int64, device=DEV)
            _lib.check(L.snerf_kplanes_gather_bwd_fx(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(gout), _p(fx), _st()), "gather_bwd_fx")
            return {"features": out, "plane gradients (fixed point)": fx}

        a, b = _both(pr, gather)
        _equal(a, b, what)
        assert int(a["plane gradients (fixed point)"].abs().max()) > 0
        # the sort: ids a permutation, keys of the expected points non-descending, the records' coordinate words the expected points' bits
        ss = ops.SortedScatter(ps, N, DEV, desc=desc)
        ss.sorted_rec.fill_(float("nan"))
        ss.sort(pr.rays)
        torch.cuda.synchronize()
        _check_sorted(ss.sorted_rec, pr.pts_cpu, reso, what)
        if Cn == 8:
            gd = (torch.rand(N, generator=gen) - 0.5).to(DEV)

            def density(co):
                dens, feat = torch.empty(N, device=DEV), torch.empty(N, 8, device=DEV)
                _lib.check(L.snerf_kplanes_density_fwd(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), C.byref(net), _p(Wp), _p(dens), _p(feat), _st()),
                           "density_fwd")
                out = {"density": dens, "proposal features": feat}
                if dbwd:
                    lv = (_lib.DensityBwdLevel * 2)()
                    gX, gp, ws = torch.empty(N, 8, device=DEV), torch.zeros(ps.numel, device=DEV), torch.zeros(n_ws, device=DEV)
                    lv[0].desc, lv[0].planes, lv[0].coords, lv[0].N = C.addressof(desc), ps.planes.data_ptr(), C.addressof(co), N
                    lv[0].net, lv[0].W, lv[0].gdens = C.addressof(net), Wp.data_ptr(), gd.data_ptr()
                    lv[0].grad_planes, lv[0].workspace, lv[0].gX = gp.data_ptr(), ws.data_ptr(), gX.data_ptr()
                    _lib.check(L.snerf_kplanes_density_bwd(lv, 1, _st()), "density_bwd")
                    fx = torch.zeros(ps.numel, dtype=torch.int64, device=DEV)
                    _lib.check(L.snerf_kplanes_gather_bwd_fx(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(gX), _p(fx), _st()), "gather_bwd_fx")
                    out.update({"gX": gX, "plane gradients of gX (fixed point)": fx})
                    out["_gp"] = gp
                return out

            a, b = _both(pr, density)
            gpa, gpb = a.pop("_gp", None), b.pop("_gp", None)
            _equal(a, b, what)
            if gpa is not None:  # float atomics: the same terms in any order
                scale = float(gpb.abs().max())
                torch.testing.assert_close(gpa, gpb, rtol=1e-5, atol=1e-6 * max(scale, 1e-30))
        else:
            orders = [None]
            if view == "4" and S % 32 == 0:
                orders.append(torch.arange(R - 1, -1, -1, dtype=torch.int32, device=DEV))

            def field(co, order=None):
                out = {"density": torch.empty(N, device=DEV), "rgb": torch.empty(N, 3, device=DEV), "feat16": torch.empty(N, W, dtype=torch.bfloat16, device=DEV),
                       "h": torch.empty(N, 16, device=DEV), "feat32": torch.empty(N, W, device=DEV)}
                head = (C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), C.byref(sig), _p(Ws), C.byref(col), _p(Wc), _p(out["density"]), _p(out["rgb"]),
                        _p(out["feat16"]), _p(out["h"]), _p(out["feat32"]))
                rc = L.snerf_kplanes_field_fwd(*head, _st()) if order is None else L.snerf_kplanes_field_fwd_ordered(*head, _p(order), _st())
                _lib.check(rc, "field_fwd")
                out["feat16"] = out["feat16"].view(torch.int16)
                return out

            a, b = _both(pr, field)
            _equal(a, b, what)
            assert torch.equal(a["feat32"], _both(pr, gather)[1]["features"])
            for order in orders[1:]:
                w = field(pr.rays, order)
                torch.cuda.synchronize()
                _equal(w, b, what + " ordered walk")


def test_quotient_scatter_with_samples_crowded_against_the_face():
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    ps, desc = _plane_set(32, "4", 23)
    gen = torch.Generator().manual_seed(8)
    R, S = 96, 32
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 0.8
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    nears, fars = torch.full((R,), 0.05, device=DEV), torch.full((R,), 1000.0, device=DEV)
    _, eb = ops.spaced_bins(nears, fars, S, torch.rand(R, S + 1, generator=gen).to(DEV), kind="piecewise")
    g = lambda t: t.to(DEV).contiguous()
    o, d, t = g(o), g(d), g(torch.rand(R, generator=gen))
    co = ops.coords_from_rays(o, d, t, eb, None, True, contract=True)
    N = R * S
    pts = U.points(o.cpu(), d.cpu(), eb.cpu(), t.cpu())
    # the piecewise spacing puts a tenth of a ray's samples beyond distance 5 (p > 0.9) and its last ones beyond 50 (p > 0.99): crowded cells
    far = pts[:, :3].abs().amax(-1)
    assert float((far > 0.9).float().mean()) > 0.05 and float(far.max()) > 0.99 and float(far.max()) <= 1.0
    gout = g(torch.rand(N, ps.out_dim, generator=gen) - 0.5)
    direct = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(gout), _p(direct), _st()), "gather_bwd")
    feat = torch.empty(N, ps.out_dim, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(feat), _st()), "gather_fwd")
    ss = ops.SortedScatter(ps, N, DEV, quotient=True, fix_capacity=64)
    ss.sort(co)
    got = torch.zeros_like(ps.planes)
    ss.scatter_quotient(ps.planes, co, gout, feat, got)
    torch.cuda.synchronize()
    assert int(ss.fix_peak.item()) == 0  # the overflow word
    ss.check_fix_overflow()
    scale = float(direct.abs().max())
    torch.testing.assert_close(got, direct, rtol=1e-4, atol=2e-6 * scale)  # the existing comparison of the two forms (tests/test_gpu_kplanes.py)
    assert float((got - direct).norm() / direct.norm()) < 2e-6


@pytest.mark.parametrize("c", U.GRAD_CASES, ids=U.grad_case_id)
def test_coordinate_gradient_through_the_contraction(c):
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.plane_set import PlaneSet

    rec = U.load_bounds()["coords_gradient"][U.grad_case_id(c)]
    d = U.make_gradient_case(c)
    ps = PlaneSet(c["C"], d["reso"], concat=bool(c["concat"]), device=DEV)
    ps.load_reference([[p.to(DEV) for p in g] for g in d["planes"]])
    nc, R, N = len(c["base"]), c["R"], c["N"]
    keep = [d[k].to(DEV).contiguous() for k in ("origins", "dirs", "times", "ebins")]
    co = ops.coords_from_rays(keep[0], keep[1], keep[2] if nc == 4 else None, keep[3], None, True, contract=True)
    gout = d["gout"].to(DEV).contiguous()
    desc = ps.desc()
    pad = 4

    def run():
        gp = torch.full((N + pad, nc), 1234.5, device=DEV)
        go, gd = torch.zeros(R + pad, 3, device=DEV), torch.zeros(R + pad, 3, device=DEV)
        _lib.check(_lib.lib().snerf_kplanes_gather_bwd_coords(C.byref(desc), _p(ps.planes), C.byref(co), C.c_int64(N), _p(gout), _p(gp), _p(go), _p(gd), _st()),
                   "kplanes_gather_bwd_coords")
        torch.cuda.synchronize()
        return gp, go, gd

    gp, go, gd = run()
    assert bool((gp[N:] == 1234.5).all()) and float(go[R:].abs().max()) == 0 and float(gd[R:].abs().max()) == 0
    ok, okr = U.grad_comparable(c, d), U.grad_rays_comparable(c, d)
    assert float(ok.double().mean()) >= U.KEEP_SHARE and bool(okr.all())
    gp64, go64, gd64 = U.grad_reference(c, d, torch.float64)
    for name, got, want, key in (("grad_pts", gp[:N].cpu()[ok], gp64[ok], "dev32_grad_pts"), ("grad_origins", go[:R].cpu()[okr], go64[okr], "dev32_grad_origins"),
                                 ("grad_dirs", gd[:R].cpu()[okr], gd64[okr], "dev32_grad_dirs")):
        dev = PR.rel_dev(got, want)
        print(f"{U.grad_case_id(c)}: {name} deviation {dev:.3e} (float32 restatement {rec[key]:.3e}, bound {U.FACTOR * rec[key]:.3e})")
    for name, got, want, key in (("grad_pts", gp[:N].cpu()[ok], gp64[ok], "dev32_grad_pts"), ("grad_origins", go[:R].cpu()[okr], go64[okr], "dev32_grad_origins"),
                                 ("grad_dirs", gd[:R].cpu()[okr], gd64[okr], "dev32_grad_dirs")):
        assert PR.rel_dev(got, want) <= U.FACTOR * rec[key], name
    gp2, go2, gd2 = run()  # fixed order, no atomics: the same bits
    assert torch.equal(gp2, gp) and torch.equal(go2, go) and torch.equal(gd2, gd)
    # contract = 0 on the same buffers is a different answer: the switch is read
    co0 = ops.coords_from_rays(keep[0], keep[1], keep[2] if nc == 4 else None, keep[3], [[-40.0] * 3, [40.0] * 3], True)
    gp0 = torch.empty(N, nc, device=DEV)
    _lib.check(_lib.lib().snerf_kplanes_gather_bwd_coords(C.byref(desc), _p(ps.planes), C.byref(co0), C.c_int64(N), _p(gout), _p(gp0), None, None, _st()), "bwd_coords")
    torch.cuda.synchronize()
    assert not torch.equal(gp0, gp[:N])


@pytest.mark.parametrize("which", ["field", "density_field"])
def test_fields_in_kernel_route_equals_the_torch_route(which):
    """KPlanesField._features / KPlanesDensityField.get_density with SceneContraction(order=inf) and compact ray samples (the in-kernel route)
    against the torch route on the same samples: _pts_from_positions(get_positions(), times, distortion) + a mode-0 gather, with the points
    evaluated by torch on the CPU and on the device.  Equality.  Another distortion (order 2) keeps the torch route."""
    from soccernerfs_amd import ops
    from soccernerfs_amd.kplanes_field import KPlanesDensityField, KPlanesField, _pts_from_positions
    from soccernerfs_amd.ray_samplers import _make_samples
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.spatial_distortions import SceneContraction

    rs = U.coordinate_rounds(129, 33)[0]
    g = lambda t: t.to(DEV).contiguous()
    R = rs["origins"].shape[0]
    rb = RayBundle(origins=g(rs["origins"]), directions=g(rs["dirs"]), pixel_area=torch.ones(R, 1, device=DEV), times=g(rs["times"])[:, None],
                   nears=torch.zeros(R, 1, device=DEV), fars=torch.ones(R, 1, device=DEV))
    eb = g(rs["ebins"])
    samples = _make_samples(rb, eb, eb, "uniform")
    aabb = torch.tensor([[-1.5] * 3, [1.5] * 3])
    torch.manual_seed(3)
    for order, in_kernel in ((float("inf"), True), (2, False)):
        dist = SceneContraction(order=order)
        if which == "field":
            f = KPlanesField(aabb, spacetime_resolution=(12, 10, 9, 3), feat_dim=32, multiscale_res=(1, 2), concat_features_across_scales=True,
                             spatial_distortion=dist).to(DEV)
            run = lambda s: f._features(s)
        else:
            f = KPlanesDensityField(aabb, resolution=(12, 10, 9, 3), feature_dim=8, spatial_distortion=dist).to(DEV)
            run = lambda s: f.get_density(s)[0]
        with torch.no_grad():
            f.grids.planes.copy_(torch.rand(f.grids.numel, device=DEV) * 0.8 + 0.2)
            got = run(samples)
            plain = rb.get_ray_samples(bin_starts=eb[..., :-1, None], bin_ends=eb[..., 1:, None])  # no compact form: the torch route
            dev_route = run(plain)
            pts_dev = _pts_from_positions(plain.frustums.get_positions(), plain.times, f.aabb, True, dist)
            pts_cpu = _pts_from_positions(plain.frustums.get_positions().cpu(), plain.times.cpu(), None, True, dist)
        torch.cuda.synchronize()
        if in_kernel:
            assert torch.equal(pts_cpu, U.expected_points(rs)) and torch.equal(pts_dev.cpu(), pts_cpu), "torch evaluates the contraction differently on the device"
            if which == "field":
                assert torch.equal(got, ops.interpolate_kplanes(g(pts_cpu), f.grids))
        assert torch.equal(got.reshape(dev_route.shape), dev_route), (which, order)
        assert bool(torch.isfinite(got).all()) and float(got.std()) > 0


def test_unbounded_step_fed_by_the_masked_pixel_draw():
    """Masks and bounded = False: PixelSampler draws inside batch["mask"] (snerf_sample_pixels_masked), ops.generate_rays(collider="near_far")
    forms the rays, an unbounded trainer (deterministic mode) takes two steps on them.  The drawn pixels lie inside the mask, the targets are
    the images' pixels, and the steps equal, bit for bit, those of a second trainer fed the same origins / directions / times directly (its own
    constant nears / fars: the collider's are the same constants)."""
    from soccernerfs_amd import ops, synthetic
    from soccernerfs_amd.pixel_samplers import PixelSampler
    from soccernerfs_amd.trainer import KPlanesTrainer

    R, M, H, W = 256, 3, 33, 47
    gen = torch.Generator().manual_seed(8)
    images = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, generator=gen).to(DEV)
    mask = torch.rand(M, H, W, 1, generator=gen) < 0.5
    mask[:, :6, :20] = False  # a banner
    mask[1] = False           # one image fully masked out
    mask = mask.to(DEV)
    c = synthetic.make_cameras(M, W, H)
    cam = {k: c[k].to(DEV).contiguous() for k in ("fx", "fy", "cx", "cy", "c2w")}
    times = torch.tensor([0.2, 0.5, 0.8], device=DEV)
    batch = {"image": images, "image_idx": torch.arange(M, device=DEV), "mask": mask}
    trs = [KPlanesTrainer(_cfg(deterministic=True), R, DEV) for _ in range(2)]
    trs[1].params.copy_(trs[0].params)
    trs[1]._params_alt.copy_(trs[0]._params_alt)
    sampler = PixelSampler(R)
    torch.manual_seed(5)
    for step in range(2):
        out = sampler.sample(batch)
        idx = out["indices"]
        ci, y, x = idx[:, 0], idx[:, 1], idx[:, 2]
        assert bool(mask[ci, y, x, 0].all()) and not bool((ci == 1).any()) and isinstance(batch["mask_index"], ops.MaskIndex)
        assert torch.equal(out["image"], images[ci, y, x].float() / 255.0)
        rays = ops.generate_rays(idx.contiguous(), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["c2w"], times, near_plane=NEAR, training=True,
                                 collider="near_far", far_plane=FAR)
        assert float(rays["nears"].min()) == float(rays["nears"].max()) == pytest.approx(NEAR) and float(rays["fars"].min()) == FAR
        _, _, rng = _rays(R, 90 + step)
        target = out["image"].contiguous()
        a = trs[0].train_step(rays, target, rng).clone()
        direct = {k: rays[k].clone() for k in ("origins", "directions", "times")}
        b = trs[1].train_step(direct, target, rng).clone()
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    for tr in trs:
        tr.synchronize()
    assert torch.equal(trs[0].params, trs[1].params) and torch.equal(trs[0].exp_avg, trs[1].exp_avg)
    assert all(co.contract == 1 for co in trs[0]._coords)


# ------------------------------------------------------------------------------------------------------------------------------------ 4
E, SAMPLES, NEAR, FAR = U.STEP_E, U.STEP_SAMPLES, U.STEP_NEAR, U.STEP_FAR


def _cfg(**kw):
    from soccernerfs_amd.trainer import KPlanesTrainConfig

    base = dict(aabb_scale=E["aabb_scale"], spacetime_resolution=E["base_res"], multiscale_res=E["multiscale"], feature_dim=32,
                proposal_resolutions=E["prop_res"], proposal_feature_dim=8, num_proposal_samples_per_ray=SAMPLES[0],
                num_nerf_samples_per_ray=SAMPLES[1], warm_up_end=1, max_steps=1000, bounded=False, near_plane=NEAR, far_plane=FAR)
    base.update(kw)
    return KPlanesTrainConfig(**base)


def _rays(R, seed, S=SAMPLES):
    """unbounded_reference.step_rays on the device: half of the rays never meet the unit cube."""
    g = lambda z: z.to(DEV).contiguous()
    rays, target, rng = U.step_rays(R, seed, S)
    return {k: g(v) for k, v in rays.items()}, g(target), {"t_rand": g(rng["t_rand"]), "u": [g(u) for u in rng["u"]], "bg": g(rng["bg"])}


def _params(seed=5):
    from oracle import kplanes_oracle as KO

    return KO.make_kplanes_params(**dict(E, seed=seed))


def _model(P):
    from soccernerfs_amd.kplanes import KPlanesModel, KPlanesModelConfig
    from soccernerfs_amd.scene_colliders import SceneBox

    cfg = KPlanesModelConfig(multiscale_res=tuple(E["multiscale"]), spacetime_resolution=tuple(E["base_res"]), feature_dim=E["feat_dim"],
                             proposal_net_args_list=[{"feature_dim": E["prop_feat"], "resolution": list(r)} for r in E["prop_res"]],
                             num_proposal_samples_per_ray=SAMPLES[0], num_nerf_samples_per_ray=SAMPLES[1], sigma_net_hidden_dim=E["sigma_hidden"],
                             rgb_net_hidden_dim=E["color_hidden"], disable_viewing_dependent=True, bounded=False, near_plane=NEAR, far_plane=FAR)
    a = E["aabb_scale"]
    model = KPlanesModel(cfg, SceneBox(aabb=torch.tensor([[-a] * 3, [a] * 3])), num_train_data=4)
    from soccernerfs_amd.spatial_distortions import SceneContraction

    assert isinstance(model.field.spatial_distortion, SceneContraction) and model.field.spatial_distortion.order == float("inf")
    model.field.grids.load_reference(P["field_grids"])
    model.field.sigma_net.load_linear_weights(P["field_sigma"])
    model.field.color_net.load_linear_weights(P["field_color"])
    for i, pn in enumerate(model.proposal_networks):
        pn.grids.load_reference([P["prop_grids"][i]])
        pn.sigma_net.load_linear_weights(P["prop_sigma"][i])
    model = model.to(DEV)
    model.scene_box.aabb = model.scene_box.aabb.to(DEV)
    return model


def _state(module):
    from soccernerfs_amd import checkpoint as CK

    return {k: v for k, v in CK.reference_state_dict(module).items() if not k.endswith("aabb") and "device_indicator" not in k}


def _compare_steps(tr, P, steps, rgb_atol, loss_rtol, param_rel):
    """tests/test_gpu_view_dependent.py::_compare_steps for the unbounded model: the trainer against KPlanesModel(bounded=False) +
    torch.optim.Adam on the same parameters, rays and draws."""
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.trainer import cosine_lr_factor

    R = tr.R
    model = _model(P).train()
    opts = {k: torch.optim.Adam([p for p in v if p.requires_grad], lr=tr.cfg.lr, eps=tr.cfg.adam_eps) for k, v in model.get_param_groups().items()}
    cbs = model.get_training_callbacks()
    worst = {"rgb": 0.0, "loss": 0.0, "param": 0.0}
    for step in range(steps):
        rays, target, rng = _rays(R, 20 + step)
        draws = [rng["t_rand"], rng["u"][0], rng["u"][1], rng["bg"]]
        model.set_rand_fn(lambda shape, device: draws.pop(0))
        for where, fn in cbs:
            if where == "before":
                fn(step)
        rb = RayBundle(origins=rays["origins"], directions=rays["directions"], pixel_area=torch.ones(R, 1, device=DEV), times=rays["times"])
        out = model(rb)
        assert float(rb.nears.max()) == float(rb.nears.min()) == pytest.approx(NEAR) and float(rb.fars.min()) == FAR
        ld = model.get_loss_dict(out, {"image": target})
        lr = tr.cfg.lr * cosine_lr_factor(step, tr.cfg.warm_up_end, tr.cfg.max_steps, tr.cfg.lr_alpha)
        for o in opts.values():
            o.zero_grad(set_to_none=True)
            for pg in o.param_groups:
                pg["lr"] = lr
        sum(ld.values()).backward()
        for o in opts.values():
            o.step()
        for where, fn in cbs:
            if where == "after":
                fn(step)
        rgb = tr.train_step(rays, target, rng).clone()
        lt = {k: float(v) for k, v in tr.loss_dict().items()}
        assert set(lt) == set(ld), (set(lt) ^ set(ld))
        worst["rgb"] = max(worst["rgb"], float((rgb - out["rgb"].detach()).abs().max()))
        print(f"step {step}: rgb deviation {worst['rgb']:.3e}")
        for k, v in ld.items():
            want = float(v.detach())
            if abs(want) > 1e-9:
                worst["loss"] = max(worst["loss"], abs(lt[k] - want) / abs(want))
            print(f"step {step}: {k} trainer {lt[k]:.9e} model {want:.9e}")
        assert worst["rgb"] <= (rgb_atol[step] if isinstance(rgb_atol, (list, tuple)) else rgb_atol), (step, worst)
        for k, v in ld.items():
            want = float(v.detach())
            assert abs(lt[k] - want) <= loss_rtol * abs(want) + 1e-9, (step, k, lt[k], want)
    tr.synchronize()
    got, want = _state(tr._named_module()), _state(model)
    assert set(got) == set(want)
    rel = {k: float((got[k].double() - want[k].double()).norm() / (want[k].double().norm() + 1e-30)) for k in want}
    worst["param"] = max(rel.values())
    print("worst deviations", worst)
    for k in want:
        assert rel[k] <= param_rel, (k, rel[k])
    return worst


def test_three_steps_fp32_match_the_unbounded_model_with_torch_adam():
    """fp32 operands.  Floor: the tolerances of the bounded comparison (tests/test_gpu_view_dependent.py: rgb 1e-6, loss terms 1e-6 relative,
    parameters 3e-7 relative L2).  The far samples exceed them -- Adam's normalised update (eps 1e-12) amplifies the relative error of the tiny
    gradients that texels seen only by far, nearly weightless samples receive -- so the float32-against-float64 restatement of the same three
    steps decides: bound = max(floor, 5 x its deviation), from profiles/r27_unbounded_deviations.json (three_steps; measured on the CPU by
    tools/measure_unbounded_deviations.py: rgb 2.1e-6, loss 1.2e-5, parameters 1.2e-3).  Measured on the GPU with these rays, two runs: rgb 8.9e-8 / 1.2e-7,
    loss 2.3e-7 / 1.0e-7, parameters 5.2e-6 / 4.6e-5 (the float-atomic gradient sums differ from run to run)."""
    from soccernerfs_amd.trainer import KPlanesTrainer

    rec = U.load_bounds()["three_steps"]
    bound = {k: max(rec["floor"][k], U.FACTOR * rec["dev32"][k]) for k in ("rgb", "loss", "param")}
    assert rec["floor"] == U.STEP_TOLERANCES and rec["rays"] == 256
    P = _params()
    tr = KPlanesTrainer(_cfg(mlp_operands="fp32"), 256, DEV)
    assert tr.contract and tr.SPACING == 1 and not tr.fused_field
    tr.load_oracle_params(P)
    _compare_steps(tr, P, 3, rgb_atol=bound["rgb"], loss_rtol=bound["loss"], param_rel=bound["param"])
    assert all(c.contract == 1 for c in tr._coords)


def test_three_steps_default_bf16_path_is_fused_and_agrees_with_the_unfused_kernels():
    """The default path (bf16 operands; fused field forward, fused proposal density and backward, quotient scatter and epilogue) against the
    same trainer on the unfused kernels, at the shape and within the 16-bit budget of tests/test_gpu_static_planes.py
    (test_frozen_default_path_is_fused_and_agrees_with_the_unfused_kernels): rgb equal at step 0 and within 2e-3 after, parameters within
    2e-5 in the mean, loss terms within 2e-2.  The launch names are asserted: a silent fall-back would pass the comparison."""
    from soccernerfs_amd.trainer import KPlanesTrainer

    R = 256
    # 32 nerf samples per ray (that file's renderer shape): a multiple of the 32-sample tile, so the forward is the walk in frame-time order
    trs = [KPlanesTrainer(_cfg(warm_up_end=2, num_nerf_samples_per_ray=32, fused_field=f, fused_proposal=f), R, DEV) for f in (True, False)]
    a, u = trs
    assert a.contract and a.fused_field and a.fused_proposal and a.fused_proposal_backward and a.quotient_scatter and a.quotient_epilogue
    assert a.cfg.mlp_operands == "bf16" and a.field_fwd_time_order and u.contract and not u.fused_field and not u.fused_proposal
    u.params.copy_(a.params)
    u._params_alt.copy_(a._params_alt)
    a.enable_kernel_timing(["kplanes_density_fwd", "kplanes_field_fwd", "kplanes_density_bwd", "kplanes_scatter_sorted.field", "kplanes_sort"])
    for step in range(3):
        rays, target, rng = _rays(R, 20 + step, ((64, 32), 32))
        outs = [tr.train_step(rays, target, rng).clone() for tr in trs]
        assert a._fwd_fused and not u._fwd_fused and a._qg_step
        if step == 0:
            assert torch.equal(outs[0], outs[1])
        else:
            torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=2e-3)
    for tr in trs:
        tr.synchronize()
    times = a.kernel_times_ms()
    assert times["kplanes_density_fwd"][1] == 6 and times["kplanes_field_fwd"][1] == 3 and times["kplanes_density_bwd"][1] == 3, times
    assert times["kplanes_scatter_sorted.field"][1] == 3 and times["kplanes_sort"][1] == 3, times
    assert all(c.contract == 1 for c in a._coords) and int(a._ss.fix_peak.item()) == 0
    print("fused against unfused: mean |parameter difference|", float((a.params - u.params).abs().mean()))
    assert float((a.params - u.params).abs().mean()) < 2e-5
    ld0, ld1 = a.loss_dict(), u.loss_dict()
    assert set(ld0) == set(ld1)
    for k in ld0:
        torch.testing.assert_close(ld0[k], ld1[k], rtol=2e-2, atol=1e-7)
    rgb = [tr.forward(rays, None, 1.0, training=False).clone() for tr in trs]
    assert bool(torch.isfinite(rgb[0]).all())
    torch.testing.assert_close(rgb[0], rgb[1], rtol=0, atol=2e-3)


@pytest.mark.parametrize("model", ["frozen", "three_coords"])
def test_static_unbounded_step_fused_forward_equals_unfused(model):
    from soccernerfs_amd.trainer import KPlanesTrainer

    kw = dict(freeze_time_planes=True) if model == "frozen" else dict(spacetime_resolution=(16, 16, 16), proposal_resolutions=((24, 24, 24), (32, 32, 32)))
    trs = [KPlanesTrainer(_cfg(**kw, fused_field=f, fused_proposal=f), 256, DEV) for f in (True, False)]
    a, u = trs
    assert a.contract and a._static and a.fused_field and a.fused_proposal and not u.fused_field and not u.fused_proposal
    u.params.copy_(a.params)
    u._params_alt.copy_(a._params_alt)
    rays, target, rng = _rays(256, 3)
    if model == "three_coords":
        del rays["times"]
    outs = [tr.train_step(rays, target, rng).clone() for tr in trs]
    for tr in trs:
        tr.synchronize()
    assert a._fwd_fused and not u._fwd_fused
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].std()) > 0
    for k in ("rgb",):
        assert torch.equal(a.buf[k], u.buf[k])
    for lvl in range(3):
        assert torch.equal(a.buf["dens"][lvl], u.buf["dens"][lvl]) and torch.equal(a.buf["eb"][lvl], u.buf["eb"][lvl])


@pytest.mark.parametrize("option", ["view_dependent", "depth_loss"])
def test_unbounded_composes_with_field_options(option):
    """disable_viewing_dependent=False and the depth losses on an unbounded trainer: two steps of the default path against the unfused
    kernels (rgb equal at step 0, within the 16-bit budget of tests/test_gpu_static_planes.py after), the option's own term or net in use."""
    from soccernerfs_amd.trainer import KPlanesTrainer

    R = 256
    kw = dict(disable_viewing_dependent=False) if option == "view_dependent" else {}
    trs = [KPlanesTrainer(_cfg(warm_up_end=2, fused_field=f, fused_proposal=f, **kw), R, DEV) for f in (True, False)]
    a, u = trs
    assert a.contract and a.fused_field and not u.fused_field and a.view_dependent == (option == "view_dependent")
    u.params.copy_(a.params)
    u._params_alt.copy_(a._params_alt)
    gen = torch.Generator().manual_seed(12)
    for step in range(2):
        rays, target, rng = _rays(R, 80 + step)
        depth = (torch.rand(R, generator=gen) * 4 + 0.5).to(DEV) if option == "depth_loss" else None
        outs = [tr.train_step(rays, target, rng, depth=depth).clone() for tr in trs]
        assert a._fwd_fused and not u._fwd_fused
        if step == 0:
            assert torch.equal(outs[0], outs[1])
        else:
            torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=2e-3)
    for tr in trs:
        tr.synchronize()
    ld0, ld1 = a.loss_dict(), u.loss_dict()
    assert set(ld0) == set(ld1) and ("depth_loss" in ld0) == (option == "depth_loss")
    for k in ld0:
        assert bool(torch.isfinite(ld0[k]).all())
        torch.testing.assert_close(ld0[k], ld1[k], rtol=2e-2, atol=1e-7)
    assert float((a.params - u.params).abs().mean()) < 2e-5


def test_deterministic_unbounded_runs_are_bit_identical():
    from soccernerfs_amd.trainer import KPlanesTrainer

    runs = []
    for _ in range(2):
        tr = KPlanesTrainer(_cfg(deterministic=True), 256, DEV)
        assert tr.contract
        tr.load_oracle_params(_params())
        for step in range(3):
            rays, target, rng = _rays(256, 40 + step)
            tr.train_step(rays, target, rng)
        tr.synchronize()
        runs.append((tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all())


def test_ray_gradients_of_the_first_unbounded_step():
    """trainer.ray_grads after step 1 (learning rate 0 under the linear warm-up: the planes are still the ones the step differentiated), all
    three levels.  (a) The three snerf_kplanes_gather_bwd_coords launches, repeated through the C ABI on the trainer's coordinates and feature
    gradients in the trainer's order, give the same bits: every level passes contract = 1 and nothing else adds to the buffers.  (b) Against
    the float64 restatement fed the same feature gradients (bin edges constant), at 3 x the float32 restatement's deviation,
    which is evaluated here on the same inputs."""
    from soccernerfs_amd import _lib
    from soccernerfs_amd.trainer import KPlanesTrainer

    R = 64
    tr = KPlanesTrainer(_cfg(mlp_operands="fp32", ray_gradients=True, warm_up_end=512), R, DEV)
    tr.load_oracle_params(_params())
    before = tr.params.clone()
    rays, target, rng = _rays(R, 70)
    tr.train_step(rays, target, rng)
    tr.synchronize()
    assert torch.equal(tr.params, before) and all(c.contract == 1 for c in tr._coords)
    b = tr.buf
    levels = [(tr._desc_prop[0], tr.prop_planes[0], b["gpfeat"][0]), (tr._desc_prop[1], tr.prop_planes[1], b["gpfeat"][1]),
              (tr._desc_field, tr.field_planes, b["gfeat"])]
    go, gd = torch.zeros(R, 3, device=DEV), torch.zeros(R, 3, device=DEV)
    want = {dt: [torch.zeros(R, 3, dtype=dt), torch.zeros(R, 3, dtype=dt)] for dt in (torch.float64, torch.float32)}
    o, d, t = (rays[k].cpu() for k in ("origins", "directions", "times"))
    for lvl, (desc, ps, gfeat) in enumerate(levels):
        N = R * tr.S[lvl]
        _lib.check(_lib.lib().snerf_kplanes_gather_bwd_coords(C.byref(desc), _p(ps.planes), C.byref(tr._coords[lvl]), C.c_int64(N), _p(gfeat), None, _p(go), _p(gd),
                                                              _st()), "kplanes_gather_bwd_coords")
        planes = [[p.detach().cpu() for p in g] for g in ps.to_reference()]
        for dt in want:
            a, c = U.level_ray_gradient(o, d, b["eb"][lvl][:R].cpu(), t.reshape(-1), planes, ps.combs, ps.concat, gfeat[:N].cpu(), dt)
            want[dt][0] += a
            want[dt][1] += c
    torch.cuda.synchronize()
    assert torch.equal(go, tr.ray_grads["origins"]) and torch.equal(gd, tr.ray_grads["directions"])
    assert float(go.abs().max()) > 0 and float(gd.abs().max()) > 0 and bool(torch.isfinite(go).all()) and bool(torch.isfinite(gd).all())
    for name, got, i in (("origins", go, 0), ("directions", gd, 1)):
        dev32 = PR.rel_dev(want[torch.float32][i], want[torch.float64][i])
        dev = PR.rel_dev(got.cpu(), want[torch.float64][i])
        print(f"ray_grads[{name}]: deviation {dev:.3e}, float32 restatement {dev32:.3e}, bound {3 * dev32:.3e}")
        assert dev <= 3 * dev32, name


def test_unbounded_trainer_honours_its_rays_own_nears_and_fars():
    from soccernerfs_amd.trainer import KPlanesTrainer

    tr = KPlanesTrainer(_cfg(mlp_operands="fp32"), 64, DEV)
    rays, _, _ = _rays(64, 1)
    with torch.no_grad():
        tr.forward(rays, None, 1.0, training=False)
        torch.cuda.synchronize()
        assert float(tr.buf["eb"][0][:, 0].abs().max()) == 0.0 and float(tr.buf["eb"][0][:, -1].min()) == pytest.approx(FAR)  # eval: near 0
        own = dict(rays, nears=torch.full((64, 1), 0.5, device=DEV), fars=torch.full((64, 1), 3.0, device=DEV))
        tr.forward(own, None, 1.0, training=False)
        torch.cuda.synchronize()
        assert float(tr.buf["eb"][0][:, 0].min()) == pytest.approx(0.5) and float(tr.buf["eb"][0][:, -1].max()) == pytest.approx(3.0)


# ------------------------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("model", ["dynamic", "frozen", "three_coords"])
def test_renderer_from_an_unbounded_trainer(model, tmp_path):
    """Six planes, the space planes of frozen time planes, and a 3-coordinate model (the static kinds render from cameras without times, as
    tests/test_gpu_static_planes.py does): the fused tail (field_render_kernel at contract = 1, six and three planes) equals the unfused chain
    (field forward + weights + compositing) bit for bit, and both equal the trainer's eval forward."""
    from soccernerfs_amd import ops, synthetic
    from soccernerfs_amd.cameras import Cameras
    from soccernerfs_amd.render import KPlanesRenderer
    from soccernerfs_amd.trainer import KPlanesTrainer

    R, W, H = 256, 16, 12
    S = ((64, 32), 32)
    kw = {"dynamic": {}, "frozen": dict(freeze_time_planes=True),
          "three_coords": dict(spacetime_resolution=(16, 16, 16), proposal_resolutions=((24, 24, 24), (32, 32, 32)))}[model]
    static = model != "dynamic"
    tr = KPlanesTrainer(_cfg(num_nerf_samples_per_ray=32, **kw), R, DEV)
    assert tr.contract and tr._static == static and tr.fused_field
    for step in range(2):
        rays, target, rng = _rays(R, 60 + step, S)
        if model == "three_coords":
            del rays["times"]
        tr.train_step(rays, target, rng)
    c = synthetic.make_cameras(3, W, H)
    c2w = c["c2w"].clone()
    c2w[2, :, 2] = -c2w[2, :, 2]  # camera 2 looks AWAY from the origin (the camera looks along -z): its rays never come back
    c2w[2, :, 0] = -c2w[2, :, 0]
    cams = Cameras(c2w, c["fx"], c["fy"], c["cx"], c["cy"], W, H, times=None if static else torch.tensor([0.25, 0.5, 0.75])).to(DEV)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    for k in (1, 2):
        frames = {}
        for fused in (False, True):
            rn = KPlanesRenderer(tr, rays_per_chunk=100, fused_tail=fused)  # chunk boundaries inside rows
            assert rn.fused_tail == fused and rn.contract and rn.SPACING == 1
            frames[fused] = rn.render_frame(cams, k)
            anneal = rn.default_anneal()
        idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
        rays = ops.generate_rays(idx.contiguous(), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, cams.times, near_plane=NEAR, training=False,
                                 collider="near_far", far_plane=FAR)
        assert float(rays["nears"].abs().max()) == 0.0 and float(rays["fars"].min()) == float(rays["fars"].max()) == FAR
        if k == 2:
            assert bool(((rays["origins"] * rays["directions"]).sum(-1) > 0).all())  # every ray points away from the origin
        rays.pop("nears"), rays.pop("fars")  # the trainer's own eval-mode constants
        if model == "three_coords":
            del rays["times"]
        rgb = tr.forward(rays, None, anneal, training=False).clone()
        acc, depth = tr.buf["acc"][:H * W].clone(), tr.buf["depth"][:H * W].clone()
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all()) and float(rgb.std()) > 0
        assert torch.equal(frames[False]["rgb"], rgb.view(H, W, 3))
        assert torch.equal(frames[False]["accumulation"], acc.view(H, W, 1)) and torch.equal(frames[False]["depth"], depth.view(H, W, 1))
        for key in ("rgb", "accumulation", "depth"):
            assert torch.equal(frames[True][key], frames[False][key]), (k, key)
    # early termination runs and stays within its cutoff
    rn = KPlanesRenderer(tr, rays_per_chunk=100, transmittance_cutoff=1e-3)
    early = rn.render_frame(cams, 1)
    assert bool(torch.isfinite(early["rgb"]).all())
    torch.testing.assert_close(early["rgb"], KPlanesRenderer(tr, rays_per_chunk=100, fused_tail=True).render_frame(cams, 1)["rgb"], rtol=0, atol=2e-3)
    # checkpoint -> a new unbounded trainer -> the same frame
    tr.save_checkpoint(str(tmp_path))
    tr2 = KPlanesTrainer(_cfg(num_nerf_samples_per_ray=32, **kw), R, DEV)
    tr2.load_checkpoint(str(tmp_path))
    again = KPlanesRenderer(tr2, rays_per_chunk=100).render_frame(cams, 1, anneal=anneal)
    assert torch.equal(again["rgb"], KPlanesRenderer(tr, rays_per_chunk=100).render_frame(cams, 1, anneal=anneal)["rgb"])

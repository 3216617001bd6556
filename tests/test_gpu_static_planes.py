"""GPU tests of static scenes on the fused path: the three-plane forms of the fused field forward, the fused proposal density and the render
tail against the unfused kernels on the same descriptor (bit for bit) and the CPU oracle; KPlanesTrainer(freeze_time_planes=True) and a
3-coordinate KPlanesTrainer against a restated reference, against each other and against the unfused path; the hand-over between the two
stages through a checkpoint; KPlanesRenderer from both.

"Three planes" comes in two forms everywhere: a PlaneSet with three coordinates, and PlaneSet.space_desc() of a 4-coordinate set, whose time
planes are filled with NaN here so that any read of them shows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]
VIEWS = ["three_coords", "space_view"]


def _planes(C_, base3, ms, view, gen, lo=0.3, hi=1.2):
    """-> (plane set on the device, its three-plane descriptor, [scale][XY, XZ, YZ] reference tensors on the host)."""
    from soccernerfs_amd.plane_set import PlaneSet

    reso = [[r * m for r in base3] + ([6] if view == "space_view" else []) for m in ms]
    ps = PlaneSet(C_, reso, concat=C_ == 32, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * (hi - lo) + lo)
        if view == "space_view":
            for s in range(len(ms)):
                for p in (2, 4, 5):
                    ps.plane_view(s, p).fill_(float("nan"))
    space = (0, 1, 3) if view == "space_view" else (0, 1, 2)
    ref = [[sc[p].clone() for p in space] for sc in ps.to_reference()]
    ps = ps.to(DEV)
    desc = ps.space_desc()
    assert desc.n_coords == 3
    return ps, desc, ref


def _nets(n_scales, operands, seed=0):
    from soccernerfs_amd.tcnn_compat import Network

    mk = lambda i, o, h, nh, act: Network(i, o, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h,
                                                   "n_hidden_layers": nh}, seed=seed + 7 * i, operands=operands)
    return mk(32 * n_scales, 16, 128, 1, "None").to(DEV), mk(15, 3, 64, 2, "Sigmoid").to(DEV)


def _field_fwd(desc, ps, sigma, color, co, N, keep):
    from soccernerfs_amd import _lib, ops

    L, p, F = _lib.lib(), ops._ptr, ps.out_dim
    dt = torch.bfloat16 if sigma.desc.operands == 1 else torch.float16
    out = {"dens": torch.full((N,), -1.0, device=DEV), "rgb": torch.full((N, 3), -1.0, device=DEV)}
    if keep:
        out.update(feat16=torch.full((N, F), -1.0, device=DEV, dtype=dt), h=torch.full((N, 16), -1.0, device=DEV), feat32=torch.full((N, F), -1.0, device=DEV))
    _lib.check(L.snerf_kplanes_field_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(N), C.byref(sigma.desc), p(sigma.params), C.byref(color.desc),
                                         p(color.params), p(out["dens"]), p(out["rgb"]), p(out["feat16"]) if keep else None, p(out["h"]) if keep else None,
                                         p(out["feat32"]) if keep else None, ops._stream()), "field_fwd")
    return out


def _field_unfused(desc, ps, sigma, color, co, N):
    from soccernerfs_amd import _lib, ops

    L, p, F = _lib.lib(), ops._ptr, ps.out_dim
    feat, h, dens, rgb = torch.empty(N, F, device=DEV), torch.empty(N, 16, device=DEV), torch.empty(N, device=DEV), torch.empty(N, 3, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(N), p(feat), ops._stream()), "gather")
    _lib.check(L.snerf_mlp_fwd(C.byref(sigma.desc), p(sigma.params), p(feat), F, C.c_int64(N), p(h), 16, 15, p(dens), ops._stream()), "sigma")
    _lib.check(L.snerf_mlp_fwd(C.byref(color.desc), p(color.params), p(h), 16, C.c_int64(N), p(rgb), 3, -1, None, ops._stream()), "color")
    return {"feat32": feat, "h": h, "dens": dens, "rgb": rgb}


def _six(ref_scale):
    """[XY, XZ, YZ] -> the six-entry list oracle.interpolate_kplanes indexes (the time planes are never touched with freeze_time_planes)."""
    return [ref_scale[0], ref_scale[1], None, ref_scale[2], None, None]


# ---- a. fused field forward, three planes ----
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("ms,N", [((1,), 1), ((1, 2), 33), ((1, 2, 4), 1031), ((1, 2, 4, 8, 16), 2100), ((1, 2, 3, 4, 6, 8), 64)])
def test_fused_field_forward_three_planes(ms, N, operands, view):
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd import _lib, ops

    gen = torch.Generator().manual_seed(len(ms) * 1000 + N)
    ps, desc, ref = _planes(32, (12, 10, 9), ms, view, gen)
    sigma, color = _nets(len(ms), operands)
    assert _lib.lib().snerf_kplanes_field_fwd_supported(C.byref(desc), C.byref(sigma.desc), C.byref(color.desc)) == 1
    pts = (torch.rand(N, 3, generator=gen) * 2 - 1) * 1.145  # 0.874^3 = 2/3 of the points inside the box, the rest clamp to the border
    dpts = pts.to(DEV).contiguous()
    co = ops.coords_from_points(dpts)
    want = _field_unfused(desc, ps, sigma, color, co, N)
    plain = _field_fwd(desc, ps, sigma, color, co, N, keep=False)
    assert torch.equal(plain["dens"], want["dens"]) and torch.equal(plain["rgb"], want["rgb"])
    got = _field_fwd(desc, ps, sigma, color, co, N, keep=True)
    for k in ("dens", "rgb", "h", "feat32"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["feat16"], want["feat32"].to(got["feat16"].dtype))
    assert bool(torch.isfinite(got["dens"]).all()) and bool(torch.isfinite(got["rgb"]).all())  # no NaN time plane was read
    # the oracle's frozen gather + its nets, at SURVEY 8d's 16-bit tolerance (as tests/test_gpu_field_fused.py)
    feat = KO.interpolate_kplanes(torch.cat([pts, torch.zeros(N, 1)], -1), [_six(r) for r in ref], True, freeze_time_planes=True)
    hh = KO.mlp(feat, [w.cpu() for w in sigma.linear_weights()])
    torch.testing.assert_close(got["dens"].cpu(), torch.exp(hh[:, 15]), rtol=2e-2, atol=1e-3)
    torch.testing.assert_close(got["rgb"].cpu(), KO.mlp(hh[:, :15], [w.cpu() for w in color.linear_weights()], out_act="Sigmoid"), rtol=0, atol=4e-3)


def _rays(R, S, gen):
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    near = torch.rand(R, 1, generator=gen) * 0.2
    steps = torch.cumsum(torch.rand(R, S + 1, generator=gen) * 0.8 + 0.6, dim=1)
    eb = near + (torch.rand(R, 1, generator=gen) * 2.5 + 0.5) * (steps - steps[:, :1]) / (steps[:, -1:] - steps[:, :1])
    return tuple(x.to(DEV).contiguous() for x in (o, d, eb))


# ---- b. ray coordinates without a time ----
@pytest.mark.parametrize("R,S", [(5, 7), (37, 32), (1, 1)])
def test_ray_coordinates_without_times(R, S):
    from soccernerfs_amd import _lib, ops

    gen = torch.Generator().manual_seed(R)
    ps, desc, _ = _planes(32, (12, 10, 9), (1, 2), "three_coords", gen)
    pp, pdesc, _ = _planes(8, (24, 20, 18), (1,), "three_coords", gen)
    sigma, color = _nets(2, "bf16")
    o, d, eb = _rays(R, S, gen)
    nan_times = torch.full((R,), float("nan"), device=DEV)
    N, L, p = R * S, _lib.lib(), ops._ptr
    outs = []
    for times in (None, nan_times):
        co = ops.coords_from_rays(o, d, times, eb, AABB, True)
        assert (co.times is None) == (times is None)
        res = _field_fwd(desc, ps, sigma, color, co, N, keep=True)
        res["gather"] = torch.full((N, ps.out_dim), -1.0, device=DEV)
        _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(N), p(res["gather"]), ops._stream()), "gather")
        cp = ops.coords_from_rays(o, d, times, eb, AABB, False)
        res["pfeat"] = torch.full((N, 8), -1.0, device=DEV)
        _lib.check(L.snerf_kplanes_gather_fwd(C.byref(pdesc), p(pp.planes), C.byref(cp), C.c_int64(N), p(res["pfeat"]), ops._stream()), "gather prop")
        outs.append(res)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and bool(torch.isfinite(outs[0][k].float()).all()), k
    assert torch.equal(outs[0]["feat32"], outs[0]["gather"])


# ---- c. fused proposal density, three planes ----
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["ReLU", "None"])
@pytest.mark.parametrize("R,S", [(37, 50), (5, 7), (1, 1)])
def test_fused_proposal_density_three_planes(R, S, act, operands, view):
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.tcnn_compat import Network

    gen = torch.Generator().manual_seed(R + S)
    ps, desc, _ = _planes(8, (24, 20, 18), (1,), view, gen, lo=0.1, hi=0.9)
    with torch.no_grad():  # every fifth texel exactly zero: vanishing features, signed zeros in the product
        for q in ((0, 1, 3) if view == "space_view" else (0, 1, 2)):
            v = ps.plane_view(0, q)
            v.view(-1, 8)[::5] = 0.0
    net = Network(8, 1, {"otype": "FullyFusedMLP", "activation": act, "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}, seed=3,
                  operands=operands).to(DEV)
    L, p, N = _lib.lib(), ops._ptr, R * S
    assert L.snerf_kplanes_density_fwd_supported(C.byref(desc), C.byref(net.desc)) == 1
    o, d, eb = _rays(R, S, gen)
    co = ops.coords_from_rays(o, d, None, eb, AABB, False)
    feat_u, out_u, dens_u = torch.empty(N, 8, device=DEV), torch.empty(N, 1, device=DEV), torch.empty(N, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(N), p(feat_u), ops._stream()), "gather")
    _lib.check(L.snerf_mlp_fwd(C.byref(net.desc), p(net.params), p(feat_u), 8, C.c_int64(N), p(out_u), 1, 0, p(dens_u), ops._stream()), "mlp")
    for keep in (True, False):
        feat, dens = torch.full((N, 8), -7.0, device=DEV), torch.full((N,), -7.0, device=DEV)
        _lib.check(L.snerf_kplanes_density_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(N), C.byref(net.desc), p(net.params), p(dens),
                                               p(feat) if keep else None, ops._stream()), "density_fwd")
        assert torch.equal(dens, dens_u) and bool(torch.isfinite(dens).all())
        assert torch.equal(feat, feat_u) if keep else bool((feat == -7.0).all())
    assert torch.equal(dens_u, torch.exp(out_u[:, 0]))


# ---- d. render tail, three planes ----
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("R", [1, 70])
@pytest.mark.parametrize("S", [32, 64])
def test_field_render_three_planes(S, R, view):
    from soccernerfs_amd import _lib, ops

    gen = torch.Generator().manual_seed(S + R)
    ps, desc, _ = _planes(32, (12, 10, 9), (1, 2, 4), view, gen)
    sigma, color = _nets(3, "bf16")
    L, p = _lib.lib(), ops._ptr
    assert L.snerf_kplanes_field_render_supported(C.byref(desc), C.byref(sigma.desc), C.byref(color.desc), S) == 1
    o, d, eb = _rays(R, S, gen)
    co = ops.coords_from_rays(o, d, None, eb, AABB, True)
    f = _field_fwd(desc, ps, sigma, color, co, R * S, keep=False)
    w = torch.empty(R, S, device=DEV)
    _lib.check(L.snerf_weights_fwd(p(f["dens"]), p(eb), R, S, p(w), ops._stream()), "weights")
    keys = ("rgb", "acc", "depth_median", "depth_expected", "median_index")
    mk = lambda fill: {"rgb": torch.full((R, 3), fill, device=DEV), "acc": torch.full((R,), fill, device=DEV), "depth_median": torch.full((R,), fill, device=DEV),
                       "depth_expected": torch.full((R,), fill, device=DEV), "median_index": torch.full((R,), -1, dtype=torch.int64, device=DEV)}
    want, got = mk(-1.0), mk(-2.0)
    a = _lib.RenderArgs()
    a.weights, a.rgb, a.ebins, a.R, a.S, a.bg_mode, a.training = w.data_ptr(), f["rgb"].data_ptr(), eb.data_ptr(), R, S, 1, 0
    a.rgb_out, a.acc_out, a.depth_median, a.depth_expected, a.median_index = (want[k].data_ptr() for k in keys)
    _lib.check(L.snerf_render_fwd(C.byref(a), ops._stream()), "render_fwd")
    _lib.check(L.snerf_kplanes_field_render(C.byref(desc), p(ps.planes), C.byref(co), R, C.byref(sigma.desc), p(sigma.params), C.byref(color.desc),
                                            p(color.params), 0.0, p(got["rgb"]), p(got["acc"]), p(got["depth_median"]), p(got["depth_expected"]),
                                            p(got["median_index"]), None, ops._stream()), "field_render")
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["rgb"]).all()) and float(want["acc"].min()) > 0.0


# ---- trainers ----
def _dev_batch(b):
    g = lambda z: z.to(DEV).contiguous()
    return ({k: g(v) for k, v in b["rays"].items()}, g(b["target"]),
            {"t_rand": g(b["rng"]["t_rand"]), "u": [g(u) for u in b["rng"]["u"]], "bg": g(b["rng"]["bg"])})


def _time_ranges(tr):
    """(lo, hi) float ranges of the flat buffer that hold planes with the time axis."""
    out = []
    for name, ps in [(f"prop{i}.planes", p) for i, p in enumerate(tr.prop_planes)] + [("field.planes", tr.field_planes)]:
        o = tr.off[name][0]
        for s in range(len(ps.resolutions)):
            for q in (2, 4, 5):
                H, W = ps.shapes[s][q]
                out.append((o + ps.offsets[s][q], o + ps.offsets[s][q] + H * W * ps.C))
    return out


def _cat(t, ranges):
    return torch.cat([t[a:b] for a, b in ranges]).clone()


# ---- e. three training steps, exact fp32 operands, against the restated reference ----
@pytest.mark.parametrize("sweep", ["train_step", "caller_driven"])
def test_three_frozen_training_steps_match_the_restated_reference(sweep):
    """The shape and draws of tests/test_gpu_trainer.py::test_three_training_steps_match_oracle with freeze_time_planes, at that test's bounds
    (the frozen step is a subset of its arithmetic).  The time planes' Adam moments are given sentinel values first: nothing may touch them.
    sweep "train_step": the regularisers inside the optimiser sweep over the three-plane view; "caller_driven": forward / backward /
    optimizer_step() issued by the caller, i.e. the regulariser sweep of its own and the plain Adam kernel over the runs between the time planes.
    Measured on an MI355X ("train_step"): rgb 1.2e-7 abs, summed loss 7.6e-8 rel, field planes 2.9e-6, nets 1.1e-6, proposal planes 2.8e-6."""
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer, anneal_value, cosine_lr_factor
    from tests import static_reference as SR

    E, R, (S01, S2) = SR.THREE_STEPS, SR.THREE_STEPS_RAYS, SR.THREE_STEPS_SAMPLES
    P = KO.make_kplanes_params(**E)
    leaves = KO.all_param_tensors(P)
    for x in leaves:
        x.requires_grad_(True)
    cfg = KPlanesTrainConfig(aabb_scale=E["aabb_scale"], spacetime_resolution=E["base_res"], multiscale_res=E["multiscale"], feature_dim=E["feat_dim"],
                             proposal_resolutions=E["prop_res"], proposal_feature_dim=E["prop_feat"], sigma_net_hidden_dim=E["sigma_hidden"],
                             rgb_net_hidden_dim=E["color_hidden"], mlp_operands="fp32", num_proposal_samples_per_ray=S01, num_nerf_samples_per_ray=S2,
                             warm_up_end=SR.THREE_STEPS_WARM_UP, freeze_time_planes=True)
    tr = KPlanesTrainer(cfg, R, DEV)
    assert not tr.fused_field and not tr.fused_proposal and not tr.field_fwd_time_order
    tr.load_oracle_params(P)
    tranges = _time_ranges(tr)
    for a, b in tranges:
        tr.exp_avg[a:b] = 0.25
        tr.exp_avg_sq[a:b] = 0.5
    before = [_cat(t, tranges) for t in (tr.params, tr._params_alt, tr.exp_avg, tr.exp_avg_sq)]
    assert bool((before[0] == 1).all()) and torch.equal(before[0], before[1])  # both ping-pong halves hold the frozen planes from the start
    gen = torch.Generator().manual_seed(SR.THREE_STEPS_SEED)
    ms, vs = [torch.zeros_like(x) for x in leaves], [torch.zeros_like(x) for x in leaves]
    for step in range(3):
        b = SR.draw_batch(gen, R)
        out = SR.forward(P, b["rays"], b["rng"], S01, S2, anneal_value(step, 1000, 10.0), freeze_time_planes=True)
        ld = SR.loss_dict(P, out, b["target"], freeze_time_planes=True)
        loss = sum(ld.values())
        for x in leaves:
            x.grad = None
        loss.backward()
        SR.adam_on_touched(leaves, ms, vs, step + 1, 1e-2 * cosine_lr_factor(step, SR.THREE_STEPS_WARM_UP, 30000, 0.0))
        rays, target, rng = _dev_batch(b)
        if sweep == "train_step":
            rgb = tr.train_step(rays, target, rng)
            got_ld = tr.loss_dict()
        else:
            rgb = tr.forward(rays, rng, anneal_value(step, 1000, 10.0), training=True)
            tr.backward(target, rng, proposal_grads=True, include_reg=True)
            got_ld = tr.loss_dict()
            tr.optimizer_step()
        assert set(got_ld) == set(ld) and not set(got_ld) & set(SR.TIME_TERMS)
        print(f"step {step}: rgb max abs dev {float((rgb.cpu() - out['rgb'].detach()).abs().max()):.3e}, "
              f"loss rel dev {abs(float(sum(got_ld.values()).cpu()) - float(loss.detach())) / float(loss.detach()):.3e}")
        torch.testing.assert_close(rgb.cpu(), out["rgb"].detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(sum(got_ld.values()).cpu(), loss.detach(), rtol=1e-6, atol=1e-9)
    tr.synchronize()
    got = tr.field_planes.to_reference()
    dev = lambda a, b: float((a.cpu() - b.detach()).abs().max())
    worst = {"field": max(dev(got[s][p], P["field_grids"][s][p]) for s in range(2) for p in (0, 1, 3)),
             "sigma": max(dev(a, b) for a, b in zip(tr.sigma_net.linear_weights(), P["field_sigma"])),
             "color": max(dev(a, b) for a, b in zip(tr.color_net.linear_weights(), P["field_color"])),
             "prop": max(dev(tr.prop_planes[i].to_reference()[0][p], P["prop_grids"][i][p]) for i in range(2) for p in (0, 1, 3))}
    print("max abs parameter deviations after three steps:", worst)
    for s in range(2):
        for p in (0, 1, 3):
            torch.testing.assert_close(got[s][p].cpu(), P["field_grids"][s][p].detach(), rtol=0, atol=1.5e-5)
    for a, b in zip(tr.sigma_net.linear_weights(), P["field_sigma"]):
        torch.testing.assert_close(a.cpu(), b.detach(), rtol=0, atol=1.5e-6)
    for a, b in zip(tr.color_net.linear_weights(), P["field_color"]):
        torch.testing.assert_close(a.cpu(), b.detach(), rtol=0, atol=1.5e-6)
    for i in range(2):
        gp = tr.prop_planes[i].to_reference()[0]
        for p in (0, 1, 3):
            torch.testing.assert_close(gp[p].cpu(), P["prop_grids"][i][p].detach(), rtol=0, atol=1e-5)
        for a, b in zip(tr.prop_nets[i].linear_weights(), P["prop_sigma"][i]):
            torch.testing.assert_close(a.cpu(), b.detach(), rtol=0, atol=1.5e-6)
    # something moved, and the frozen planes did not: value, exp_avg, exp_avg_sq, in BOTH ping-pong halves, bit for bit
    assert float((got[1][0].cpu() - KO.make_kplanes_params(**E)["field_grids"][1][0]).abs().max()) > 1e-4
    after = [_cat(t, tranges) for t in (tr.params, tr._params_alt, tr.exp_avg, tr.exp_avg_sq)]
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert tr.step == 3 and float(tr.grads.abs().max()) == 0.0


# ---- f. the default path ----
SMALL = dict(aabb_scale=1.5, spacetime_resolution=(16, 16, 16, 4), multiscale_res=(1, 2), feature_dim=32,
             proposal_resolutions=((24, 24, 24, 4), (32, 32, 32, 4)), proposal_feature_dim=8, num_proposal_samples_per_ray=(64, 32),
             num_nerf_samples_per_ray=16, warm_up_end=2, mlp_operands="bf16")
SMALL3 = dict(SMALL, spacetime_resolution=(16, 16, 16), proposal_resolutions=((24, 24, 24), (32, 32, 32)))


def _draws(R, gen, S=(64, 32, 16), times=True):
    g = lambda z: z.to(DEV).contiguous()
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    rays = {"origins": g(o), "directions": g(d), "times": g(torch.rand(R, 1, generator=gen))}
    target = g(torch.rand(R, 3, generator=gen))
    rng = {"t_rand": g(torch.rand(R, S[0] + 1, generator=gen)), "u": [g(torch.rand(R, S[1] + 1, generator=gen)), g(torch.rand(R, S[2] + 1, generator=gen))],
           "bg": g(torch.rand(R, 3, generator=gen))}
    return rays, target, rng


def test_frozen_default_path_is_fused_and_agrees_with_the_unfused_kernels():
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 256
    trs = [KPlanesTrainer(KPlanesTrainConfig(**SMALL, freeze_time_planes=True, fused_field=f, fused_proposal=f), R, DEV) for f in (True, False)]
    a, u = trs
    assert a.fused_field and a.fused_proposal and a.quotient_scatter and a.quotient_epilogue and not a.fused_proposal_backward
    assert not a.field_fwd_time_order and not u.fused_field and not u.fused_proposal
    a.enable_kernel_timing(["kplanes_density_bwd", "kplanes_density_fwd", "kplanes_field_fwd", "kplanes_gather_bwd.prop"])
    nets0 = [n.params.detach().clone() for n in a.prop_nets]
    tranges = _time_ranges(a)
    gen = torch.Generator().manual_seed(2)
    for step in range(3):
        rays, target, rng = _draws(R, gen)
        outs = [tr.train_step(rays, target, rng).clone() for tr in trs]
        if step == 0:
            assert torch.equal(outs[0], outs[1])
        else:
            torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=2e-3)
    for tr in trs:
        tr.synchronize()
    times = a.kernel_times_ms()
    assert "kplanes_density_bwd" not in times  # the fused proposal backward is not built for three planes: its launch is not taken
    assert times["kplanes_density_fwd"][1] == 6 and times["kplanes_field_fwd"][1] == 3 and times["kplanes_gather_bwd.prop"][1] == 6
    assert all(float((n.params.detach() - n0).abs().max()) > 0 for n, n0 in zip(a.prop_nets, nets0))  # the proposal networks were updated
    assert float((a.params - u.params).abs().mean()) < 2e-5
    ld0, ld1 = a.loss_dict(), u.loss_dict()
    assert set(ld0) == set(ld1) == {"rgb_loss", "distortion_loss", "interlevel_loss", "space_tv_loss", "space_tv_proposal_loss"}
    for k in ld0:
        torch.testing.assert_close(ld0[k], ld1[k], rtol=2e-2, atol=1e-7)
    for tr in trs:
        for t in (tr.params, tr._params_alt):
            assert bool((_cat(t, tranges) == 1).all())
        assert float(_cat(tr.exp_avg, tranges).abs().max()) == 0.0 and float(_cat(tr.exp_avg_sq, tranges).abs().max()) == 0.0
    rgb = [tr.forward(rays, None, 1.0, training=False).clone() for tr in trs]
    torch.testing.assert_close(rgb[0], rgb[1], rtol=0, atol=2e-3)


# ---- g. a 3-coordinate model against the frozen 4-coordinate one ----
def test_three_coordinate_model_equals_the_frozen_model():
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 128
    fr = KPlanesTrainer(KPlanesTrainConfig(**SMALL, freeze_time_planes=True, deterministic=True), R, DEV)
    st = KPlanesTrainer(KPlanesTrainConfig(**SMALL3, deterministic=True), R, DEV)
    assert st.fused_field and st.fused_proposal and fr.fused_field and fr.fused_proposal and st.field_planes.n_coords == 3

    def space_planes(tr):
        q = (0, 1, 3) if tr.field_planes.n_coords == 4 else (0, 1, 2)
        sets = [tr.field_planes] + list(tr.prop_planes)
        return [ps.plane_view(s, p).detach().clone() for ps in sets for s in range(len(ps.resolutions)) for p in q]

    nets = lambda tr: [n.params.detach().clone() for n in (tr.sigma_net, tr.color_net, *tr.prop_nets)]
    # one seed: the time planes are filled with ones, not drawn, so both models start from the same space planes and nets
    assert all(torch.equal(x, y) for x, y in zip(space_planes(fr), space_planes(st))) and all(torch.equal(x, y) for x, y in zip(nets(fr), nets(st)))
    start = space_planes(st)
    gen = torch.Generator().manual_seed(4)
    for step in range(3):
        rays, target, rng = _draws(R, gen)
        rgb_f = fr.train_step(rays, target, rng).clone()
        rgb_s = st.train_step({k: v for k, v in rays.items() if k != "times"}, target, rng).clone()  # a static scene's rays carry no times
        assert torch.equal(rgb_f, rgb_s), step
        lf, ls = fr.loss_dict(), st.loss_dict()
        assert set(lf) == set(ls)
        for k in ("rgb_loss", "distortion_loss", "interlevel_loss"):
            assert torch.equal(lf[k], ls[k]), (step, k)
        for k in ("space_tv_loss", "space_tv_proposal_loss"):  # float partial sums in arrival order
            torch.testing.assert_close(lf[k], ls[k], rtol=1e-6, atol=0)
    fr.synchronize()
    st.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(space_planes(fr), space_planes(st)))
    assert all(torch.equal(x, y) for x, y in zip(nets(fr), nets(st)))
    assert float((space_planes(st)[0] - start[0]).abs().max()) > 0  # and they trained


# ---- h. hand-over between the stages ----
def test_frozen_checkpoint_hands_over_to_the_dynamic_stage(tmp_path):
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 128
    s1 = KPlanesTrainer(KPlanesTrainConfig(**SMALL, freeze_time_planes=True), R, DEV)
    gen = torch.Generator().manual_seed(6)
    for _ in range(2):
        s1.train_step(*_draws(R, gen))
    s1.save_checkpoint(str(tmp_path))
    s1.synchronize()
    s2 = KPlanesTrainer(KPlanesTrainConfig(**dict(SMALL, warm_up_end=0), seed=9), R, DEV)  # no warm-up: its first step already moves parameters
    assert not torch.equal(s2.params, s1.params)
    assert s2.load_checkpoint(str(tmp_path), params_only=True) == 0
    assert torch.equal(s2.params, s1.params) and torch.equal(s2._params_alt, s1.params)
    assert s2.step == 0 and float(s2.exp_avg.abs().max()) == 0.0 and float(s2.exp_avg_sq.abs().max()) == 0.0
    tranges = _time_ranges(s2)
    assert bool((_cat(s2.params, tranges) == 1).all())
    s2.train_step(*_draws(R, gen))
    s2.synchronize()
    assert s2.step == 1 and "time_smoothness_loss" in s2.loss_dict()
    assert float((_cat(s2.params, tranges) - 1).abs().max()) > 0  # stage 2 learns the dynamics: the time planes move
    # the plain load restores step and moments as before, into a trainer with the flag and into one without
    for kw in (dict(freeze_time_planes=True), dict()):
        s3 = KPlanesTrainer(KPlanesTrainConfig(**SMALL, seed=11, **kw), R, DEV)
        assert s3.load_checkpoint(str(tmp_path)) == 2 and s3.step == 2
        for x, y in ((s3.params, s1.params), (s3._params_alt, s1.params), (s3.exp_avg, s1.exp_avg), (s3.exp_avg_sq, s1.exp_avg_sq)):
            assert torch.equal(x, y)
        assert float(s3.exp_avg.abs().max()) > 0


# ---- i. the renderer ----
@pytest.mark.parametrize("model", ["frozen", "three_coords"])
def test_renderer_from_static_trainers(model):
    from soccernerfs_amd import ops, synthetic
    from soccernerfs_amd.cameras import Cameras
    from soccernerfs_amd.render import KPlanesRenderer
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R, W, H = 256, 40, 24
    cfg = dict(SMALL if model == "frozen" else SMALL3, num_nerf_samples_per_ray=32)
    if model == "frozen":
        cfg["freeze_time_planes"] = True
    tr = KPlanesTrainer(KPlanesTrainConfig(**cfg), R, DEV)
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):
        rays, target, rng = _draws(R, gen, S=(64, 32, 32))
        if model == "three_coords":
            del rays["times"]
        tr.train_step(rays, target, rng)
    c = synthetic.make_cameras(3, W, H)
    cams = Cameras(c["c2w"], c["fx"], c["fy"], c["cx"], c["cy"], W, H, times=None).to(DEV)  # no times: a static model needs none
    k = 1
    frames = {}
    for fused in (False, True):
        rn = KPlanesRenderer(tr, rays_per_chunk=256, fused_tail=fused)  # 256 = 6.4 rows of 40 pixels: chunk boundaries fall inside rows
        assert rn.fused_tail == fused
        frames[fused] = rn.render_frame(cams, k)
        anneal = rn.default_anneal()
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
    rgb, acc, depth = torch.empty(H * W, 3, device=DEV), torch.empty(H * W, device=DEV), torch.empty(H * W, device=DEV)
    for i in range(0, H * W, R):
        rays = ops.generate_rays(idx[i:i + R].contiguous(), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, None, aabb=tr.aabb,
                                 near_plane=tr.cfg.near_plane, training=False)
        if model == "three_coords":
            del rays["times"]
        n = rays["origins"].shape[0]
        rgb[i:i + n] = tr.forward(rays, None, anneal, training=False)
        acc[i:i + n], depth[i:i + n] = tr.buf["acc"][:n], tr.buf["depth"][:n]
    assert float(rgb.std()) > 0 and bool(torch.isfinite(rgb).all())
    for fused in (False, True):
        assert torch.equal(frames[fused]["rgb"], rgb.view(H, W, 3)), fused
        assert torch.equal(frames[fused]["accumulation"], acc.view(H, W, 1)), fused
        assert torch.equal(frames[fused]["depth"], depth.view(H, W, 1)), fused

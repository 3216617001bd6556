"""GPU parity of the fused proposal density backward (csrc/proposal_bwd.hip: snerf_kplanes_density_bwd) against the unfused kernels it replaces,
snerf_mlp_bwd_ws (the 8 -> 64 -> 1 net's backward from gdens) + snerf_kplanes_gather_bwd (the plane scatter of the feature gradient):

* gX bit for bit (the same operand images and MFMA sequence);
* plane gradients and the net's weight gradients within 1e-6 relative L2 (the same terms, run-length combined along longer runs), or within 4x
  the relative L2 between two unfused runs where their float atomics alone differ by more (tiny planes with thousands of terms per texel);
* both levels in one launch at the preset's sizes on ray samples, ragged N, S not a multiple of the 32-sample tile, taps clamped at the plane
  border, texels that are exactly zero, both operand types, with and without the hidden ReLU;
* the trainer with the switch on and off (non-deterministic mode): every gradient segment of an updating step under the same bound; the forward
  of a step bit for bit; parameters after update and non-update steps within 4x the distance between two unfused runs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPS = 16  # replicas of a snerf_mlp_bwd_ws workspace


def _level(res, operands, act="ReLU", seed=0, zero_rows=False):
    from soccernerfs_amd.plane_set import PlaneSet
    from soccernerfs_amd.tcnn_compat import Network

    gen = torch.Generator().manual_seed(seed)
    ps = PlaneSet(8, [list(res)], concat=False, a=0.1, b=0.9, generator=gen)
    if zero_rows:  # exactly-zero texels: every 5th texel of the flat buffer
        with torch.no_grad():
            ps.planes.view(-1, 8)[::5] = 0.0
    net = Network(8, 1, {"otype": "FullyFusedMLP", "activation": act, "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}, seed=seed + 3,
                  operands=operands)
    return ps.to(DEV), net.to(DEV), gen


def _unfused(ps, net, co, N, gdens):
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    desc = ps.desc()
    feat = torch.empty(N, 8, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(desc), ops._ptr(ps.planes), C.byref(co), C.c_int64(N), ops._ptr(feat), ops._stream()))
    ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), device=DEV)
    gX = torch.full((N, 8), -7.0, device=DEV)
    _lib.check(L.snerf_mlp_bwd_ws(C.byref(net.desc), ops._ptr(net.params), ops._ptr(feat), 8, C.c_int64(N), None, 1, 0, ops._ptr(gdens), ops._ptr(gX), 8,
                                  ops._ptr(ws), ops._stream()))
    gp = torch.zeros_like(ps.planes)
    _lib.check(L.snerf_kplanes_gather_bwd(C.byref(desc), ops._ptr(ps.planes), C.byref(co), C.c_int64(N), ops._ptr(gX), ops._ptr(gp), ops._stream()))
    torch.cuda.synchronize()
    return gX, gp, ws.view(REPS, -1).sum(0)


def _fused(levels):
    """levels: list of (ps, net, co, N, gdens); one launch for all of them."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    arr = (_lib.DensityBwdLevel * len(levels))()
    keep, outs = [], []
    for i, (ps, net, co, N, gdens) in enumerate(levels):
        desc = ps.desc()
        assert L.snerf_kplanes_density_bwd_supported(C.byref(desc), C.byref(net.desc)) == 1
        ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), device=DEV)
        gX = torch.full((N, 8), -7.0, device=DEV)
        gp = torch.zeros_like(ps.planes)
        a = arr[i]
        a.desc, a.planes, a.coords, a.N = C.addressof(desc), ps.planes.data_ptr(), C.addressof(co), N
        a.net, a.W, a.gdens = C.addressof(net.desc), net.params.data_ptr(), gdens.data_ptr()
        a.grad_planes, a.workspace, a.gX = gp.data_ptr(), ws.data_ptr(), gX.data_ptr()
        keep.append(desc)
        outs.append((gX, gp, ws))
    _lib.check(L.snerf_kplanes_density_bwd(arr, len(levels), ops._stream()), "kplanes_density_bwd")
    torch.cuda.synchronize()
    return [(gX, gp, ws.view(REPS, -1).sum(0)) for gX, gp, ws in outs]


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _check(fused, args):
    """gX bit for bit; plane and weight gradients within 1e-6 relative L2, or within 4x the spread of two unfused runs where the unfused float
    atomics alone differ by more (tiny planes that collect thousands of contributions per texel)."""
    gX_f, gp_f, gw_f = fused
    gX_u, gp_u, gw_u = _unfused(*args)
    _, gp_u2, gw_u2 = _unfused(*args)
    assert torch.equal(gX_f, gX_u)
    assert float(gp_u.abs().sum()) > 0 and float(gw_u.abs().sum()) > 0
    for f, u, u2 in ((gp_f, gp_u, gp_u2), (gw_f, gw_u, gw_u2)):
        assert _rel_l2(f, u) <= max(1e-6, 4.0 * _rel_l2(u2, u)), (_rel_l2(f, u), _rel_l2(u2, u))


def _rays(gen, R, S):
    o = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2).to(DEV)
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    t = torch.rand(R, generator=gen).to(DEV)
    eb = torch.sort(torch.rand(R, S + 1, generator=gen) * 3.0, dim=-1).values.to(DEV)
    return o, d, t, eb


def _gdens(gen, N):
    g = (torch.randn(N, generator=gen) * 1e-3)
    g[3::7] = 0.0  # samples whose weights carry no gradient
    return g.to(DEV)


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_both_levels_at_preset_size_on_ray_samples(operands):
    """The preset's two proposal levels (128^3 x 100 and 256^3 x 100 planes, 256 and 128 samples per ray), 4096 rays, one launch."""
    from soccernerfs_amd import ops

    lv, alive = [], []
    for i, (res, S) in enumerate((((128, 128, 128, 100), 256), ((256, 256, 256, 100), 128))):
        ps, net, gen = _level(res, operands, seed=i)
        R = 4096
        rays = _rays(gen, R, S)
        alive.append(rays)  # the Coords hold raw pointers into these
        co = ops.coords_from_rays(*rays, [[-1.5] * 3, [1.5] * 3], False)
        lv.append((ps, net, co, R * S, _gdens(gen, R * S)))
    fused = _fused(lv)
    for args, f in zip(lv, fused):
        _check(f, args)


@pytest.mark.parametrize("act", ["ReLU", "None"])
@pytest.mark.parametrize("R,S", [(37, 50), (5, 7), (1, 1)])
def test_ragged_rays_and_zero_texels(R, S, act):
    """S not a multiple of the 32-sample tile, a last tile that is not full, exactly-zero texels, no hidden activation."""
    from soccernerfs_amd import ops

    ps, net, gen = _level((24, 20, 18, 5), "bf16", act, seed=4, zero_rows=True)
    o, d, t, eb = _rays(gen, R, S)
    co = ops.coords_from_rays(o, d, t, eb, [[-1.5] * 3, [1.5] * 3], True)
    N = R * S
    gd = _gdens(gen, N)
    _check(_fused([(ps, net, co, N, gd)])[0], (ps, net, co, N, gd))


@pytest.mark.parametrize("N", [70000, 1031, 33, 1])
def test_points_clamped_at_the_border(N):
    """Explicit points, a third of them outside [-1, 1] (taps clamped at the plane border: the x0 + 1 corner carries weight 0)."""
    from soccernerfs_amd import ops

    ps, net, gen = _level((16, 12, 9, 4), "bf16", seed=7)
    ps2, net2, _ = _level((9, 7, 5, 3), "bf16", seed=8)
    pts = (torch.rand(N, 4, generator=gen) * 3.0 - 1.5).to(DEV)
    pts[::11] = 1.0  # exactly on the last texel
    co = ops.coords_from_points(pts)
    gd = _gdens(gen, N)
    fused = _fused([(ps, net, co, N, gd), (ps2, net2, co, N, gd)])
    _check(fused[0], (ps, net, co, N, gd))
    _check(fused[1], (ps2, net2, co, N, gd))


def test_other_shapes_are_refused():
    from soccernerfs_amd import _lib
    from soccernerfs_amd.plane_set import PlaneSet
    from soccernerfs_amd.tcnn_compat import Network

    L = _lib.lib()
    ps, net, _ = _level((16, 16, 16, 4), "bf16")
    net32 = Network(8, 1, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}).to(DEV)
    ps32 = PlaneSet(32, [[8, 8, 8, 4]], concat=True).to(DEV)
    d8, d32 = ps.desc(), ps32.desc()
    assert L.snerf_kplanes_density_bwd_supported(C.byref(d8), C.byref(net32.desc)) == 0
    assert L.snerf_kplanes_density_bwd_supported(C.byref(d32), C.byref(net.desc)) == 0
    assert L.snerf_kplanes_density_bwd(None, 1, None) != 0


SMALL = dict(aabb_scale=1.5, spacetime_resolution=(16, 16, 16, 4), multiscale_res=(1, 2), proposal_resolutions=((24, 24, 24, 4), (32, 32, 32, 4)),
             num_proposal_samples_per_ray=(64, 48), num_nerf_samples_per_ray=16)


def _batch(gen, R):
    o = (torch.rand(R, 3, device=DEV, generator=gen) * 2 - 1) * 0.8
    d = torch.nn.functional.normalize(torch.rand(R, 3, device=DEV, generator=gen) * 2 - 1, dim=-1)
    rays = {"origins": o.contiguous(), "directions": d.contiguous(), "times": torch.rand(R, 1, device=DEV, generator=gen)}
    target = torch.rand(R, 3, device=DEV, generator=gen)
    rng = {"t_rand": torch.rand(R, 65, device=DEV, generator=gen), "u": [torch.rand(R, 49, device=DEV, generator=gen),
           torch.rand(R, 17, device=DEV, generator=gen)], "bg": torch.rand(R, 3, device=DEV, generator=gen)}
    return rays, target, rng


def test_trainer_gradients_with_and_without_the_fused_proposal_backward():
    """One forward + backward that updates the proposal networks (non-deterministic mode): every gradient segment of the fused trainer within
    1e-6 relative L2 of the unfused one (or 4x the spread of two unfused runs, where their float atomics alone differ by more)."""
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 256
    grads = []
    for fused in (True, False, False):
        tr = KPlanesTrainer(KPlanesTrainConfig(fused_proposal_backward=fused, **SMALL), R, DEV)
        assert tr.fused_proposal_backward == fused
        rays, target, rng = _batch(torch.Generator(device=DEV).manual_seed(5), R)
        tr.forward(rays, rng, 1.0, training=True)
        tr.backward(target, rng, proposal_grads=True)
        tr.synchronize()
        grads.append({k: v.clone() for k, v in tr.gviews.items()})
    g_f, g_u, g_u2 = grads
    assert set(g_f) >= {"prop0.planes", "prop1.planes", "prop0.mlp", "prop1.mlp"}
    for k in g_f:
        assert float(g_u[k].abs().sum()) > 0, k
        assert _rel_l2(g_f[k], g_u[k]) <= max(1e-6, 4.0 * _rel_l2(g_u2[k], g_u[k])), (k, _rel_l2(g_f[k], g_u[k]), _rel_l2(g_u2[k], g_u[k]))


def test_train_step_with_and_without_the_fused_proposal_backward():
    """Update step, step without update, update step (early schedule), fused against unfused from the same initial state: the first step's
    forward bit for bit, the parameters after the three steps within 4x the distance between two unfused runs (their float atomics already
    differ, and Adam's eps of 1e-15 turns the sign of a near-zero gradient into a full step)."""
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 256
    runs = []
    for fused in (True, False, False):
        tr = KPlanesTrainer(KPlanesTrainConfig(fused_proposal_backward=fused, **SMALL), R, DEV)
        assert tr.fused_proposal_backward == fused
        tr.step, tr._steps_since_update = 20, 2
        gen = torch.Generator(device=DEV).manual_seed(3)
        fwd, updated = [], []
        for _ in range(3):
            rays, target, rng = _batch(gen, R)
            before = tr._steps_since_update
            rgb = tr.train_step(rays, target, rng).clone()
            tr.synchronize()
            updated.append(tr._steps_since_update <= before)
            fwd.append((rgb, [w.clone() for w in tr.buf["w"]], [s.clone() for s in tr.buf["sb"]]))
        runs.append((fwd, tr.params.clone(), updated))
    (fwd_f, p_f, upd_f), (fwd_u, p_u, upd_u), (_, p_u2, _) = runs
    assert upd_f == upd_u == [True, False, True]
    # the first step's forward runs on the same parameters: bit-identical
    assert torch.equal(fwd_f[0][0], fwd_u[0][0])
    for a, b in zip(fwd_f[0][1] + fwd_f[0][2], fwd_u[0][1] + fwd_u[0][2]):
        assert torch.equal(a, b)
    err, spread = float((p_f - p_u).norm()), float((p_u2 - p_u).norm())
    assert spread > 0 and err <= 4.0 * spread, (err, spread)

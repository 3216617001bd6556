"""GPU: the view-dependent K-Planes colour net in the fused trainer (KPlanesTrainConfig.disable_viewing_dependent = False: the reference class's
default, NS/models/kplanes.py:145; colour net on [SH degree 4 of the direction | 15 geometry features], NS/fields/kplanes_field.py:206-216,
:260-262, :314-323; csrc/color_vd.hip, the VD variants of csrc/field_fused.hip and csrc/mlp_rows.hip).

* the fused forward against the unfused 16-bit kernels fed the same planes (bit for bit), its SH columns against soccernerfs_amd/sh.py, and the
  colour input at G6b (the reference's own class) on the exact and the bf16 path;
* the colour backward that forms its input on chip against the workgroup-tile kernel and a float64 emulation of what it rounds;
* whole training steps against KPlanesModel(disable_viewing_dependent=False) + torch.optim.Adam (fp32 and the default bf16 path), deterministic
  mode, and a checkpoint round trip into the model."""
import ctypes as C

import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = dict(base_res=(16, 16, 16, 4), multiscale=(1, 2), feat_dim=32, prop_res=((24, 24, 24, 4), (32, 32, 32, 4)), prop_feat=8, sigma_hidden=128,
         color_hidden=64, aabb_scale=1.5, seed=5)
SAMPLES = ((64, 32), 16)


def _desc(d_in, hidden, n_hidden, d_out, out_act, operands):
    from soccernerfs_amd import _lib

    d = _lib.MlpDesc()
    d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d_in, hidden, n_hidden, d_out, 1, out_act, operands
    return d


def _rays(R, seed, dev=DEV):
    gen = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    t, target = torch.rand(R, 1, generator=gen), torch.rand(R, 3, generator=gen)
    (S0, S1), S2 = SAMPLES
    rng = {"t_rand": torch.rand(R, S0 + 1, generator=gen), "u": [torch.rand(R, S1 + 1, generator=gen), torch.rand(R, S2 + 1, generator=gen)],
           "bg": torch.rand(R, 3, generator=gen)}
    g = lambda z: z.to(dev).contiguous()
    return {"origins": g(o), "directions": g(d), "times": g(t)}, g(target), {"t_rand": g(rng["t_rand"]), "u": [g(u) for u in rng["u"]], "bg": g(rng["bg"])}


def _sh_ref(dirs):
    from soccernerfs_amd.sh import sh4_from_unit_dirs

    return sh4_from_unit_dirs(((dirs + 1.0) / 2.0) * 2.0 - 1.0)  # get_normalized_directions, then tcnn's 2x - 1 (tcnn_compat.Encoding)


def _params(seed=5):
    from oracle import kplanes_oracle as KO

    P = KO.make_kplanes_params(**dict(E, seed=seed))
    gen = torch.Generator().manual_seed(seed + 100)
    P["field_color"][0] = (torch.rand(64, 31, generator=gen) * 2 - 1) * (6.0 / 95) ** 0.5  # xavier-uniform [64, 31]
    return P


def _cfg(**kw):
    from soccernerfs_amd.trainer import KPlanesTrainConfig

    return KPlanesTrainConfig(aabb_scale=E["aabb_scale"], spacetime_resolution=E["base_res"], multiscale_res=E["multiscale"], feature_dim=32,
                              proposal_resolutions=E["prop_res"], proposal_feature_dim=8, num_proposal_samples_per_ray=SAMPLES[0],
                              num_nerf_samples_per_ray=SAMPLES[1], disable_viewing_dependent=False, warm_up_end=1, max_steps=1000, **kw)


def test_fused_forward_equals_unfused_16bit_kernels_and_sh_columns_are_sh_py():
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.trainer import KPlanesTrainer

    R = 300  # ragged: 4800 samples, not a multiple of the 32-sample tile of every workgroup's last tile
    tr = KPlanesTrainer(_cfg(), R, DEV)
    assert tr.view_dependent and tr.fused_field and tr.color_bwd_vd and tr.color_net.dims == [31, 64, 64, 3] and tr.cfg.mlp_operands == "bf16"
    tr.load_oracle_params(_params())
    rays, _, _ = _rays(R, 3)
    L, b, N = _lib.lib(), tr.buf, R * SAMPLES[1]
    with torch.no_grad():
        tr.forward(rays, None, 1.0, training=False)  # bins of the nerf level; the eval forward is the fused kernel
    torch.cuda.synchronize()
    eb = b["eb"][2][:R].clone()
    co = ops.coords_from_rays(rays["origins"], rays["directions"], rays["times"].reshape(-1), eb, tr.aabb, True)
    dens_f, rgb_f = torch.empty(N, device=DEV), torch.empty(N, 3, device=DEV)
    feat16 = torch.empty(N, 64, dtype=torch.bfloat16, device=DEV)
    h_f = torch.empty(N, 16, device=DEV)
    _lib.check(L.snerf_kplanes_field_fwd(C.byref(tr._desc_field), ops._ptr(tr.field_planes.planes), C.byref(co), C.c_int64(N), C.byref(tr.sigma_net.desc),
                                         ops._ptr(tr.sigma_net.params), C.byref(tr.color_net.desc), ops._ptr(tr.color_net.params), ops._ptr(dens_f),
                                         ops._ptr(rgb_f), ops._ptr(feat16), ops._ptr(h_f), None, ops._stream()), "field_fwd")
    # unfused: gather -> sigma_net -> colour input -> colour net, the same bf16 operands
    feat = torch.empty(N, 64, device=DEV)
    _lib.check(L.snerf_kplanes_gather_fwd(C.byref(tr._desc_field), ops._ptr(tr.field_planes.planes), C.byref(co), C.c_int64(N), ops._ptr(feat), ops._stream()), "gather")
    h_u, dens_u = torch.empty(N, 16, device=DEV), torch.empty(N, device=DEV)
    _lib.check(L.snerf_mlp_fwd(C.byref(tr.sigma_net.desc), ops._ptr(tr.sigma_net.params), ops._ptr(feat), 64, C.c_int64(N), ops._ptr(h_u), 16, 15,
                               ops._ptr(dens_u), ops._stream()), "sigma")
    cx = torch.full((N, 32), 7.0, device=DEV)
    _lib.check(L.snerf_kplanes_color_input_fwd(ops._ptr(rays["directions"]), SAMPLES[1], ops._ptr(h_u), C.c_int64(N), ops._ptr(cx), ops._stream()), "cx")
    rgb_u = torch.empty(N, 3, device=DEV)
    _lib.check(L.snerf_mlp_fwd(C.byref(tr.color_net.desc), ops._ptr(tr.color_net.params), ops._ptr(cx), 32, C.c_int64(N), ops._ptr(rgb_u), 3, -1, None,
                               ops._stream()), "color")
    torch.cuda.synchronize()
    assert torch.equal(dens_f, dens_u) and torch.equal(h_f, h_u) and torch.equal(feat16, feat.to(torch.bfloat16))
    assert torch.equal(rgb_f, rgb_u), float((rgb_f - rgb_u).abs().max())
    assert torch.equal(rgb_f, b["rgb"][:N])  # the trainer's eval forward
    dirs = rays["directions"].repeat_interleave(SAMPLES[1], 0)
    assert torch.equal(cx[:, :16], _sh_ref(dirs)), "SH columns differ from soccernerfs_amd/sh.py"
    assert torch.equal(cx[:, 16:31], h_u[:, :15]) and float(cx[:, 31].abs().max()) == 0.0


def test_colour_input_at_g6b_exact_and_bf16():
    """G6b (the reference's KPlanesField, view-dependent): the colour input built by the kernel + the generic colour-net kernels reproduce its rgb
    at test_view_dependent_field_matches_reference_golden's tolerances (fp32 operands) and within the default path's bf16 budget."""
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.kplanes_field import KPlanesField
    from soccernerfs_amd.rays import Frustums, RaySamples
    from soccernerfs_amd.tcnn_compat import Network

    g = load_golden("g6b_field_options")
    f = KPlanesField(g["aabb"], spacetime_resolution=[6, 5, 4, 3], feat_dim=32, multiscale_res=[1, 2], concat_features_across_scales=True,
                     disable_viewing_dependent=False, sigma_net_layers=1, sigma_net_hidden_dim=128, rgb_net_layers=2, rgb_net_hidden_dim=64).to(DEV)
    f.grids.load_reference([[g[f"vd_plane_{s}_{q}"] for q in range(6)] for s in range(2)])
    f.sigma_net.load_linear_weights([g[f"vd_sigma_{i}"].to(DEV) for i in range(2)])
    f.color_net.load_linear_weights([g[f"vd_color_{i}"].to(DEV) for i in range(3)])
    pos, dirs, tms = g["vd_positions"].to(DEV), g["vd_directions"].to(DEV), g["vd_times"].to(DEV)
    R, S = pos.shape[:2]
    rs = RaySamples(frustums=Frustums(origins=pos, directions=dirs, starts=torch.zeros(R, S, 1, device=DEV), ends=torch.zeros(R, S, 1, device=DEV),
                                      pixel_area=torch.ones(R, S, 1, device=DEV)), times=tms[:, None])
    f.train(True)
    with torch.no_grad():
        _, geo = f.get_density(rs)
        h = torch.zeros(R * S, 16, device=DEV)
        h[:, :15] = geo
        d = dirs.expand(R, S, 3).reshape(-1, 3).contiguous()  # one "ray" per sample: S = 1
        cx = torch.empty(R * S, 32, device=DEV)
        _lib.check(_lib.lib().snerf_kplanes_color_input_fwd(ops._ptr(d), 1, ops._ptr(h), C.c_int64(R * S), ops._ptr(cx), ops._stream()), "cx")
        assert torch.equal(cx[:, :16], _sh_ref(d))
        rgb = f.color_net(cx[:, :31].contiguous()).view(R, S, 3)
        torch.testing.assert_close(rgb.cpu(), g["vd_train_rgb"], rtol=2e-5, atol=2e-6)
        net16 = Network(31, 3, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 64, "n_hidden_layers": 2},
                        operands="bf16").to(DEV)
        net16.params.data.copy_(f.color_net.params.data)
        rgb16 = torch.empty(R * S, 3, device=DEV)
        _lib.check(_lib.lib().snerf_mlp_fwd(C.byref(net16.desc), ops._ptr(net16.params), ops._ptr(cx), 32, C.c_int64(R * S), ops._ptr(rgb16), 3, -1, None,
                                            ops._stream()), "color16")
        torch.testing.assert_close(rgb16.view(R, S, 3).cpu(), g["vd_train_rgb"], rtol=0, atol=4e-3)


@pytest.mark.parametrize("operands", [1, 2])
@pytest.mark.parametrize("R,S,ldgy", [(139, 8, 3), (37, 16, 4), (4096, 64, 3)])
def test_colour_backward_vd_matches_tile_kernel_and_emulation(R, S, ldgy, operands):
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    d = _desc(31, 64, 2, 3, 1, operands)
    N = R * S
    gen = torch.Generator().manual_seed(R + S)
    dims = [31, 64, 64, 3]
    Ws = [((torch.rand(dims[i], dims[i + 1], generator=gen) * 2 - 1) * (6.0 / (dims[i] + dims[i + 1])) ** 0.5) for i in range(3)]
    W = torch.cat([w.reshape(-1) for w in Ws]).to(DEV)
    dirs = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    h = (torch.rand(N, 16, generator=gen) - 0.3).to(DEV)
    gY = (torch.rand(N, ldgy, generator=gen) - 0.5).to(DEV)
    cx = torch.empty(N, 32, device=DEV)
    _lib.check(L.snerf_kplanes_color_input_fwd(ops._ptr(dirs), S, ops._ptr(h), C.c_int64(N), ops._ptr(cx), ops._stream()), "cx")
    gh = torch.full((N, 16), 7.0, device=DEV)  # sentinel: column 15 must stay untouched
    gW = torch.zeros_like(W)
    _lib.check(L.snerf_kplanes_color_bwd_vd(C.byref(d), ops._ptr(W), ops._ptr(dirs), S, ops._ptr(h), C.c_int64(N), ops._ptr(gY), ldgy, ops._ptr(gh),
                                            ops._ptr(gW), ops._stream()), "color_bwd_vd")
    gX_t, gW_t = torch.zeros(N, 32, device=DEV), torch.zeros_like(W)
    _lib.check(L.snerf_mlp_bwd_tile(C.byref(d), ops._ptr(W), ops._ptr(cx), 32, C.c_int64(N), ops._ptr(gY), ldgy, -1, None, ops._ptr(gX_t), 32,
                                    ops._ptr(gW_t), ops._stream()), "tile")
    # the replica workspace form folds to the same weight gradient
    ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(d))), device=DEV)
    gh2, gW2 = torch.zeros(N, 16, device=DEV), torch.zeros_like(W)
    _lib.check(L.snerf_kplanes_color_bwd_vd_ws(C.byref(d), ops._ptr(W), ops._ptr(dirs), S, ops._ptr(h), C.c_int64(N), ops._ptr(gY), ldgy, ops._ptr(gh2),
                                               ops._ptr(ws), ops._stream()), "color_bwd_vd_ws")
    _lib.check(L.snerf_mlp_gw_reduce(C.byref(d), ops._ptr(ws), ops._ptr(gW2), ops._stream()), "reduce")
    torch.cuda.synchronize()
    assert float((gh[:, 15] - 7.0).abs().max()) == 0.0 and bool(torch.isfinite(gh).all()) and bool(torch.isfinite(gW).all())
    assert torch.equal(gh[:, :15], gh2[:, :15]) and float(ws.abs().max()) == 0.0
    torch.testing.assert_close(gW2, gW, rtol=1e-4, atol=1e-5 * float(gW.abs().max()))
    # ---- against the workgroup-tile kernel on the materialised input (test_gpu_mlp_rows.py's bounds) ----
    a, b = gh[:, :15], gX_t[:, 16:31]
    scale = float(b.abs().max())
    bad = (a - b).abs() > 1e-5 * scale + 1e-4 * b.abs()
    assert float(bad.float().mean()) < 2e-3, float(bad.float().mean())
    torch.testing.assert_close(gW, gW_t, rtol=2e-3, atol=2e-4 * float(gW_t.abs().max()))
    # ---- against a float64 emulation of what the kernel rounds (operands to bf16 / fp16, everything else exact) ----
    dt, GS = (torch.bfloat16, 1.0) if operands == 1 else (torch.float16, 8192.0)
    rd = lambda t: t.float().to(dt).double()
    rg = lambda t: ((t * GS).float().clamp(-65504.0, 65504.0) if operands == 2 else t.float()).to(dt).double() / GS
    x = rd(cx[:, :31].double())
    Wd = [rd(w.to(DEV).double()) for w in Ws]
    acts = [x]
    for l in range(2):
        acts.append(rd(torch.relu(acts[-1] @ Wd[l])))
    z = acts[-1] @ Wd[2]
    gq = rg(gY[:, :3].double() * torch.sigmoid(z) * (1 - torch.sigmoid(z)))
    gWs = [None, None, acts[2].t() @ gq]
    for l in (2, 1):
        gq = rg((gq @ Wd[l].t()) * (acts[l] > 0))
        gWs[l - 1] = acts[l - 1].t() @ gq
    gx = (gq @ Wd[0].t())[:, 16:31]
    gw = torch.cat([w.reshape(-1) for w in gWs])
    bad = (a.double() - gx).abs() > 2e-3 * float(gx.abs().max()) + 1e-2 * gx.abs()
    assert float(bad.float().mean()) < 5e-3, float(bad.float().mean())
    assert float((a.double() - gx).abs().mean()) < 2e-3 * float(gx.abs().mean() + 1e-20)
    assert float((gW.double() - gw).norm() / gw.norm()) < 5e-3


def test_deterministic_weight_gradient_of_the_vd_shape_is_reproducible():
    """Deterministic mode runs the view-dependent colour net through the fixed-point kernel on the materialised input: the same bits twice."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    d = _desc(31, 64, 2, 3, 1, 1)
    N = 4096 * 4
    gen = torch.Generator().manual_seed(7)
    W = ((torch.rand(31 * 64 + 64 * 64 + 64 * 3, generator=gen) * 2 - 1) * 0.2).to(DEV)
    X = torch.zeros(N, 32, device=DEV)
    X[:, :31] = (torch.rand(N, 31, generator=gen) - 0.3).to(DEV)
    gY = (torch.rand(N, 3, generator=gen) - 0.5).to(DEV)
    outs = []
    for _ in range(2):
        fx = torch.zeros(W.numel(), dtype=torch.int64, device=DEV)
        gX = torch.zeros(N, 32, device=DEV)
        _lib.check(L.snerf_mlp_bwd_fx(C.byref(d), ops._ptr(W), ops._ptr(X), 32, C.c_int64(N), ops._ptr(gY), 3, -1, None, ops._ptr(gX), 32, ops._ptr(fx),
                                      ops._stream()), "bwd_fx")
        outs.append((fx.clone(), gX.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and int(outs[0][0].abs().max()) > 0


def _model(P):
    from soccernerfs_amd.kplanes import KPlanesModel, KPlanesModelConfig
    from soccernerfs_amd.scene_colliders import SceneBox

    cfg = KPlanesModelConfig(multiscale_res=tuple(E["multiscale"]), spacetime_resolution=tuple(E["base_res"]), feature_dim=E["feat_dim"],
                             proposal_net_args_list=[{"feature_dim": E["prop_feat"], "resolution": list(r)} for r in E["prop_res"]],
                             num_proposal_samples_per_ray=SAMPLES[0], num_nerf_samples_per_ray=SAMPLES[1], sigma_net_hidden_dim=E["sigma_hidden"],
                             rgb_net_hidden_dim=E["color_hidden"], disable_viewing_dependent=False)
    a = E["aabb_scale"]
    model = KPlanesModel(cfg, SceneBox(aabb=torch.tensor([[-a] * 3, [a] * 3])), num_train_data=4)
    assert model.field.color_net.dims == [31, 64, 64, 3]
    if P is not None:
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
    """`steps` training steps of the trainer and of KPlanesModel + torch.optim.Adam (one optimiser per parameter group, the trainer's
    learning-rate schedule) on the same parameters, batch and draws; returns the largest deviations seen.  rgb_atol: per step (a list) or
    for all; param_rel = None: the default path's 16-bit budget for the parameters (tests/test_gpu_default_path.py) instead of a relative L2 bound."""
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.trainer import cosine_lr_factor

    R = tr.R
    model = _model(P).train()
    groups = model.get_param_groups()
    opts = {k: torch.optim.Adam([p for p in v if p.requires_grad], lr=tr.cfg.lr, eps=tr.cfg.adam_eps) for k, v in groups.items()}
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
        assert worst["rgb"] <= (rgb_atol[step] if isinstance(rgb_atol, (list, tuple)) else rgb_atol), (step, worst)
        for k, v in ld.items():
            want = float(v.detach())
            dev_ = abs(lt[k] - want) / (abs(want) + 1e-12)
            if abs(want) > 1e-9:
                worst["loss"] = max(worst["loss"], dev_)
            assert abs(lt[k] - want) <= loss_rtol * abs(want) + 1e-9, (step, k, lt[k], want)
    tr.synchronize()
    got, want = _state(tr._named_module()), _state(model)
    assert set(got) == set(want)
    for k in want:
        if param_rel is not None:
            rel = float((got[k].double() - want[k].double()).norm() / (want[k].double().norm() + 1e-30))
            worst["param"] = max(worst["param"], rel)
            assert rel <= param_rel, (k, rel)
        else:  # Adam moves a parameter by ~lr sign(g) this early: bound the mean and the outliers, as the view-independent default-path test does
            diff = (got[k] - want[k]).abs()
            worst["param"] = max(worst["param"], float(diff.mean()))
            assert float(diff.mean()) < 1.2e-3, (k, float(diff.mean()))
            assert float((diff > 2e-3).float().mean()) < 0.12, (k, float((diff > 2e-3).float().mean()))
            assert float(diff.max()) <= 3.1e-2, (k, float(diff.max()))
    print("worst deviations", worst)
    return worst


def test_three_steps_fp32_match_kplanes_model_with_torch_adam():
    from soccernerfs_amd.trainer import KPlanesTrainer

    P = _params()
    tr = KPlanesTrainer(_cfg(mlp_operands="fp32"), 256, DEV)
    assert tr.view_dependent and not tr.fused_field and not tr.color_bwd_vd and tr.color_net.desc.operands == 0
    tr.load_oracle_params(P)
    # measured (one run): rgb 1.2e-7, loss terms 2.1e-7 relative, parameters 4.6e-8 relative L2 -> bounds at ~5x
    _compare_steps(tr, P, 3, rgb_atol=1e-6, loss_rtol=1e-6, param_rel=3e-7)


def test_three_steps_default_bf16_path_match_kplanes_model():
    from soccernerfs_amd.trainer import KPlanesTrainer

    P = _params()
    tr = KPlanesTrainer(_cfg(), 256, DEV)
    assert tr.view_dependent and tr.fused_field and tr.color_bwd_vd and tr.quotient_scatter and tr.cfg.mlp_operands == "bf16"
    tr.load_oracle_params(P)
    # the view-independent default-path budget (tests/test_gpu_default_path.py): rgb 4e-3 at step 0 and twice that once the parameters carry
    # the 16-bit path's own Adam updates, loss terms 3e-2, parameters by mean / outlier fraction / 2 lr per step
    _compare_steps(tr, P, 3, rgb_atol=[4e-3, 8e-3, 8e-3], loss_rtol=3e-2, param_rel=None)


def test_deterministic_view_dependent_runs_are_bit_identical():
    from soccernerfs_amd.trainer import KPlanesTrainer

    runs = []
    for _ in range(2):
        tr = KPlanesTrainer(_cfg(deterministic=True), 256, DEV)
        assert tr.view_dependent and not tr.color_bwd_vd and "cx" in tr.buf
        tr.load_oracle_params(_params())
        for step in range(3):
            rays, target, rng = _rays(256, 40 + step)
            tr.train_step(rays, target, rng)
        tr.synchronize()
        runs.append(tr.params.clone())
    assert torch.equal(runs[0], runs[1])


def test_checkpoint_roundtrip_into_the_view_dependent_model(tmp_path):
    from soccernerfs_amd import checkpoint as CK
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.trainer import KPlanesTrainer

    R = 256
    tr = KPlanesTrainer(_cfg(mlp_operands="fp32"), R, DEV)
    tr.load_oracle_params(_params())
    for step in range(2):
        rays, target, rng = _rays(R, 60 + step)
        tr.train_step(rays, target, rng)
    path = tr.save_checkpoint(str(tmp_path))
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert tuple(saved["pipeline"]["_model.field.color_net.layers.0.weight"].shape) == (64, 31)
    model = _model(None)
    start, moments = CK.load_checkpoint(str(tmp_path), model)
    assert start == 2 and len(moments) == 7
    model = model.to(DEV).eval()
    rays, _, _ = _rays(R, 99)
    with torch.no_grad():
        want = tr.forward(rays, None, 1.0, training=False).clone()
        out = model(RayBundle(origins=rays["origins"], directions=rays["directions"], pixel_area=torch.ones(R, 1, device=DEV), times=rays["times"]))
    print("checkpoint round trip: max |rgb diff|", float((out["rgb"] - want).abs().max()))
    torch.testing.assert_close(out["rgb"], want, rtol=0, atol=1e-5)

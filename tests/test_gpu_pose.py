"""GPU: the camera optimiser's kernels and its path through the fused K-Planes trainer -- snerf_pose_apply, snerf_raygen_pose_bwd,
KPlanesTrainConfig(ray_gradients=True) + CameraOptimizer over three joint training steps -- against the float64 restatement of
tests/pose_reference.py (the reference's chain with nears / fars detached: the kernels hold the bin edges constant).

Bounds: 5 x the deviation of the float32 restatement from the float64 one on the same inputs, relative to the output's largest magnitude, from
profiles/r15_pose_deviations.json (tools/measure_pose_deviations.py)."""
import pytest
import torch

from tests import pose_reference as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def bounds():
    return PR.load_bounds()


def _cameras(t):
    from soccernerfs_amd.cameras import Cameras

    f = lambda a: torch.from_numpy(a).float().to(DEV)
    return Cameras(f(t["c2w"]), f(t["fx"]), f(t["fy"]), f(t["cx"]), f(t["cy"]), 64, 48,
                   distortion_params=None if t["distortion"] is None else f(t["distortion"]), camera_type=torch.from_numpy(t["types"]))


def _optimizer(M, groups, adj=None):
    from soccernerfs_amd.camera_optimizers import CameraOptimizer, CameraOptimizerConfig

    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), M, DEV, groups=None if groups is None else torch.tensor(groups))
    if adj is not None:
        opt.pose_adjustment.data.copy_(adj.to(DEV))
    return opt


@pytest.mark.parametrize("kind", PR.POSE_TABLES)
def test_zero_adjustments_leave_table_and_rays_bit_identical(kind):
    from soccernerfs_amd.cameras import RayGenerator

    t = PR.make_pose_table(kind)
    cams = _cameras(t)
    cams.camera_to_worlds[0, 1, 2] = -0.0  # a composition with the identity would turn this into +0.0
    cams.camera_to_worlds[1, 2, 3] = -0.0
    idx = torch.from_numpy(t["indices"]).to(DEV)
    for groups in PR.POSE_GROUPS.values():
        opt = _optimizer(PR.POSE_M, groups)
        adj = opt.adjusted_camera_to_worlds(cams)
        assert adj.data_ptr() != cams.camera_to_worlds.data_ptr()
        assert torch.equal(adj.view(torch.int32), cams.camera_to_worlds.view(torch.int32))
        a, b = RayGenerator(cams)(idx), RayGenerator(cams, opt)(idx)
        for name in ("origins", "directions", "pixel_area"):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
        assert torch.equal(a.metadata["directions_norm"], b.metadata["directions_norm"])
        eye = opt(torch.arange(PR.POSE_M, device=DEV))
        assert torch.equal(eye, torch.eye(4, device=DEV)[None, :3, :4].expand(PR.POSE_M, 3, 4))


@pytest.mark.parametrize("above", [False, True], ids=["below_clamp", "above_clamp"])
@pytest.mark.parametrize("gname", list(PR.POSE_GROUPS))
@pytest.mark.parametrize("kind", PR.POSE_TABLES)
def test_pose_apply_and_backward(kind, gname, above, bounds):
    t = PR.make_pose_table(kind)
    groups = PR.POSE_GROUPS[gname]
    G = PR.POSE_M if groups is None else max(groups) + 1
    adj = PR.pose_adjustments(G, 1, above)
    assert bool(((adj[:, 3:] ** 2).sum(1) >= 1e-4).all()) == above and bool(((adj[:, 3:] ** 2).sum(1) < 1e-4).all()) == (not above)
    key = f"{kind}-{gname}-{'above' if above else 'below'}_clamp"
    cams = _cameras(t)
    opt = _optimizer(PR.POSE_M, groups, adj)
    g = None if groups is None else torch.as_tensor(groups)
    # forward: the composed table
    want = PR.adjusted_c2w(torch.from_numpy(t["c2w"]), adj.double(), g)
    got = opt.adjusted_camera_to_worlds(cams)
    dev = PR.rel_dev(got, want)
    print(f"{key}: c2w_adj deviation {dev:.3e} (bound {PR.FACTOR * bounds['pose_apply'][key]['dev32_c2w']:.3e})")
    assert dev <= PR.FACTOR * bounds["pose_apply"][key]["dev32_c2w"]
    # CameraOptimizer.forward: the same transforms applied to identities
    e = opt(torch.arange(PR.POSE_M, device=DEV))
    we = PR.pose_delta_transform(adj.double() if g is None else adj.double()[g])
    assert PR.rel_dev(e, we) <= PR.FACTOR * bounds["pose_apply"][key]["dev32_c2w"]
    # backward
    idx = torch.from_numpy(t["indices"]).to(DEV)
    rg = {"origins": torch.from_numpy(t["g_o"]).float().to(DEV), "directions": torch.from_numpy(t["g_d"]).float().to(DEV)}
    grad = opt.backward(idx, rg).clone()
    ref = PR.pose_gradient(t, adj, groups, torch.float64)
    dev = PR.rel_dev(grad, ref)
    print(f"{key}: grad_pose deviation {dev:.3e} (bound {PR.FACTOR * bounds['pose_bwd'][key]['dev32_grad_pose']:.3e})")
    assert dev <= PR.FACTOR * bounds["pose_bwd"][key]["dev32_grad_pose"]
    # it accumulates; and a second run from zero gives the same bits
    twice = opt.backward(idx, rg).clone()
    torch.testing.assert_close(twice, 2 * grad, rtol=1e-6, atol=0)
    opt.grad.zero_()
    assert torch.equal(opt.backward(idx, rg), grad)
    assert opt.skipped_steps() == {"camera_opt": 0}


def test_nonfinite_pose_gradient_skips_the_step():
    t = PR.make_pose_table("perspective")
    cams = _cameras(t)
    opt = _optimizer(PR.POSE_M, None, PR.pose_adjustments(PR.POSE_M, 2, False))
    opt.adjusted_camera_to_worlds(cams)
    before = opt.pose_adjustment.detach().clone()
    idx = torch.from_numpy(t["indices"]).to(DEV)
    g_o = torch.from_numpy(t["g_o"]).float().to(DEV)
    g_o[7, 1] = float("inf")
    opt.backward(idx, {"origins": g_o, "directions": torch.from_numpy(t["g_d"]).float().to(DEV)})
    opt.step()
    assert torch.equal(opt.pose_adjustment.detach(), before) and opt.skipped_steps() == {"camera_opt": 1}
    assert float(opt.grad.abs().max()) == 0.0 and float(opt.exp_avg.abs().max()) == 0.0
    g_o[7, 1] = 0.0
    opt.backward(idx, {"origins": g_o, "directions": torch.from_numpy(t["g_d"]).float().to(DEV)})
    opt.step()
    assert not torch.equal(opt.pose_adjustment.detach(), before) and opt.skipped_steps() == {"camera_opt": 1}


# ---- the fused trainer ----
def _trainer(**over):
    from oracle import kplanes_oracle as KO
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    E = PR.STEP_E
    kw = dict(aabb_scale=E["aabb_scale"], spacetime_resolution=E["base_res"], multiscale_res=E["multiscale"], feature_dim=E["feat_dim"],
              proposal_resolutions=E["prop_res"], proposal_feature_dim=E["prop_feat"], sigma_net_hidden_dim=E["sigma_hidden"],
              rgb_net_hidden_dim=E["color_hidden"], mlp_operands="fp32", num_proposal_samples_per_ray=PR.STEP_S[0],
              num_nerf_samples_per_ray=PR.STEP_S[1], warm_up_end=2, deterministic=True)
    kw.update(over)
    tr = KPlanesTrainer(KPlanesTrainConfig(**kw), PR.STEP_R, DEV)
    tr.load_oracle_params(KO.make_kplanes_params(**E))
    return tr


def _step_cameras():
    from soccernerfs_amd.cameras import Cameras

    c = PR.step_cameras()
    H, W = PR.STEP_HW
    return Cameras(c["c2w"].to(DEV), c["fx"].to(DEV), c["fy"].to(DEV), c["cx"].to(DEV), c["cy"].to(DEV), W, H, times=c["times"].to(DEV))


def _run_steps(tr, opt, cams, n, on_step=None):
    from soccernerfs_amd import ops

    dv = lambda z: z.to(DEV).contiguous()
    for step in range(n):
        b = PR.step_draws(step)
        idx = dv(b["indices"])
        table = opt.adjusted_camera_to_worlds(cams) if opt is not None else cams.camera_to_worlds
        rays = ops.generate_rays(idx, cams.fx, cams.fy, cams.cx, cams.cy, table, cams.times)
        rgb = tr.train_step({"origins": rays["origins"], "directions": rays["directions"], "times": rays["times"]}, dv(b["target"]),
                            {"t_rand": dv(b["rng"]["t_rand"]), "u": [dv(u) for u in b["rng"]["u"]], "bg": dv(b["rng"]["bg"])})
        grad = None
        if opt is not None:
            grad = opt.backward(idx, tr.ray_grads).clone()
            opt.step()
        if on_step is not None:
            on_step(step, rgb, grad)


@pytest.fixture(scope="module")
def steps64():
    return PR.three_steps(torch.float64)


def test_three_joint_steps_match_the_detached_bin_reference(steps64, bounds):
    """ray_grads and grad_pose at step 1, pose_adjustment after steps 1 to 3 (every one of them updates the proposal networks: the interlevel
    loss reaches the poses through both proposal levels)."""
    cams = _step_cameras()
    opt = _optimizer(PR.STEP_M, PR.STEP_GROUPS)
    tr = _trainer(ray_gradients=True)
    fails = []

    def check(name, got, want, bound):
        dev = PR.rel_dev(got, want)
        print(f"three steps: {name} deviation {dev:.3e} (bound {bound:.3e})")
        if not dev <= bound:
            fails.append((name, dev, bound))

    def on_step(step, rgb, grad):
        ref, b = steps64[step], bounds["three_steps"][f"step{step + 1}"]
        if step == 0:
            check("ray_grads.origins", tr.ray_grads["origins"], ref["g_origins"], PR.FACTOR * b["dev32_g_origins"])
            check("ray_grads.directions", tr.ray_grads["directions"], ref["g_directions"], PR.FACTOR * b["dev32_g_directions"])
            check("grad_pose", grad, ref["grad_pose"], PR.FACTOR * b["dev32_grad_pose"])
        check(f"pose_adjustment after step {step + 1}", opt.pose_adjustment.detach(), ref["pose_adjustment"], PR.FACTOR * b["dev32_pose_adjustment"])

    _run_steps(tr, opt, cams, 3, on_step)
    tr.synchronize()
    assert not fails, fails


def test_switch_off_is_the_step_as_it_was_and_on_changes_no_output():
    """ray_gradients=False leaves no ray_grads and is bit-identical to a trainer built without naming the field; turning it on (fp32 operands,
    deterministic accumulation) adds launches but changes no bit of the step's outputs or parameters."""
    cams = _step_cameras()
    a, b, c = _trainer(), _trainer(ray_gradients=False), _trainer(ray_gradients=True)
    assert not hasattr(a, "ray_grads") and not hasattr(b, "ray_grads") and set(c.ray_grads) == {"origins", "directions"}
    outs = []
    for tr in (a, b, c):
        got = []
        _run_steps(tr, None, cams, 2, lambda step, rgb, grad: got.append(rgb.clone()))
        tr.synchronize()
        outs.append((got, tr.params.clone(), sum(tr.loss_dict().values()).clone()))
    for other in outs[1:]:
        for x, y in zip(outs[0][0], other[0]):
            assert torch.equal(x, y)
        assert torch.equal(outs[0][1], other[1]) and torch.equal(outs[0][2], other[2])
    assert float(c.ray_grads["origins"].abs().max()) > 0 and float(c.ray_grads["directions"].abs().max()) > 0


def test_deterministic_reruns_are_bit_identical_with_the_feature_on():
    cams = _step_cameras()
    res = []
    for _ in range(2):
        tr, opt = _trainer(ray_gradients=True), _optimizer(PR.STEP_M, PR.STEP_GROUPS)
        grads = []
        _run_steps(tr, opt, cams, 2, lambda step, rgb, grad: grads.append((tr.ray_grads["origins"].clone(), tr.ray_grads["directions"].clone(), grad)))
        tr.synchronize()
        res.append((grads, opt.pose_adjustment.detach().clone(), tr.params.clone()))
    for (o1, d1, g1), (o2, d2, g2) in zip(res[0][0], res[1][0]):
        assert torch.equal(o1, o2) and torch.equal(d1, d2) and torch.equal(g1, g2)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_default_execution_path_matches_its_unfused_flow_bit_for_bit():
    """The flow tools/train_psnr.py --optimize-cameras runs: bf16 operands, fused field forward, quotient scatter without the epilogue, and the
    fused proposal backward, whose gX output feeds the proposal levels' ray gradient.  Yardstick: the same operands through the UNFUSED
    proposal backward (snerf_mlp_bwd_ws writes the feature gradient), the kernel sequence whose fp32 form the three-step test checks against
    the oracle.  include/snerf.h promises gX bit-identical to that net backward, the forward and the field chain are the same launches in both,
    and snerf_kplanes_gather_bwd_coords has a fixed summation order: so the ray gradients must be the SAME BITS.  A wrong gX, or a wrong buffer
    handed to the coordinate kernel, cannot pass.  The cosine to the exact-fp32 path is printed (a figure: 16-bit operands move the PDF samples)."""
    cams = _step_cameras()
    fast = _trainer(ray_gradients=True, mlp_operands="bf16", deterministic=False)
    unfused = _trainer(ray_gradients=True, mlp_operands="bf16", deterministic=False, fused_proposal_backward=False)
    exact = _trainer(ray_gradients=True)
    assert fast.fused_field and fast.fused_proposal_backward and fast.quotient_scatter and not fast.quotient_epilogue
    assert unfused.fused_field and unfused.fused_proposal and not unfused.fused_proposal_backward
    for tr in (fast, unfused, exact):
        _run_steps(tr, None, cams, 1)
        tr.synchronize()
    for k in ("origins", "directions"):
        x, y = fast.ray_grads[k].double().reshape(-1), exact.ray_grads[k].double().reshape(-1)
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
        print(f"default path ray_grads[{k}]: cosine to the fp32 path {float(torch.dot(x, y) / (x.norm() * y.norm())):.6f}")
        assert torch.equal(fast.ray_grads[k], unfused.ray_grads[k]), k
    # the proposal levels' share is in there: without it (a step that does not update the proposal networks) the gradient is another one
    nerf_only = _trainer(ray_gradients=True, mlp_operands="bf16", deterministic=False)
    b = PR.step_draws(0)
    dv = lambda z: z.to(DEV).contiguous()
    from soccernerfs_amd import ops

    rays = ops.generate_rays(dv(b["indices"]), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, cams.times)
    rng = {"t_rand": dv(b["rng"]["t_rand"]), "u": [dv(u) for u in b["rng"]["u"]], "bg": dv(b["rng"]["bg"])}
    nerf_only.forward({"origins": rays["origins"], "directions": rays["directions"], "times": rays["times"]}, rng, 0.0, training=True)
    nerf_only.backward(dv(b["target"]), rng, proposal_grads=False)
    nerf_only.synchronize()
    assert not torch.equal(nerf_only.ray_grads["origins"], fast.ray_grads["origins"])


def test_unsupported_combinations_raise():
    with pytest.raises(NotImplementedError, match="disable_viewing_dependent=False"):
        _trainer(ray_gradients=True, disable_viewing_dependent=False)
    tr = _trainer(ray_gradients=True)
    cams = _step_cameras()
    from soccernerfs_amd import ops

    b = PR.step_draws(0)
    dv = lambda z: z.to(DEV).contiguous()
    rays = ops.generate_rays(dv(b["indices"]), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, cams.times)
    with pytest.raises(NotImplementedError, match="depth losses"):
        tr.train_step({"origins": rays["origins"], "directions": rays["directions"], "times": rays["times"]}, dv(b["target"]),
                      {"t_rand": dv(b["rng"]["t_rand"]), "u": [dv(u) for u in b["rng"]["u"]], "bg": dv(b["rng"]["bg"])},
                      depth=torch.ones(PR.STEP_R, device=DEV))


def test_renderer_takes_the_adjusted_cameras():
    """KPlanesRenderer.evaluate on CameraOptimizer.adjusted(cameras): zero adjustments render the table's own frames bit for bit, moved cameras
    render other frames."""
    from soccernerfs_amd.render import KPlanesRenderer

    tr, cams = _trainer(), _step_cameras()
    H, W = PR.STEP_HW
    imgs = torch.rand(PR.STEP_M, H, W, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    r = KPlanesRenderer(tr, rays_per_chunk=512)
    base = r.evaluate(cams, imgs, [0, 3])
    opt = _optimizer(PR.STEP_M, PR.STEP_GROUPS)
    assert r.evaluate(opt.adjusted(cams), imgs, [0, 3]) == base
    opt.pose_adjustment.data.copy_(PR.pose_adjustments(3, 3, True).to(DEV))
    moved = opt.adjusted(cams)
    assert type(moved) is type(cams) and moved.camera_to_worlds.data_ptr() != cams.camera_to_worlds.data_ptr()
    assert r.evaluate(moved, imgs, [0, 3])["psnr_per_image"] != base["psnr_per_image"]


def test_checkpoint_carries_the_pose_state(tmp_path):
    from soccernerfs_amd.camera_optimizers import PIPELINE_KEY

    cams = _step_cameras()
    tr, opt = _trainer(ray_gradients=True), _optimizer(PR.STEP_M, PR.STEP_GROUPS)
    _run_steps(tr, opt, cams, 2)
    on = tr.save_checkpoint(str(tmp_path / "on"), camera_optimizer=opt)
    off = tr.save_checkpoint(str(tmp_path / "off"))
    a, b = torch.load(on, weights_only=False), torch.load(off, weights_only=False)
    assert set(a["pipeline"]) - set(b["pipeline"]) == {PIPELINE_KEY} and set(a["optimizers"]) - set(b["optimizers"]) == {"camera_opt"}
    assert float(a["optimizers"]["camera_opt"]["state"][0]["step"]) == 2.0
    tr2, opt2 = _trainer(ray_gradients=True), _optimizer(PR.STEP_M, PR.STEP_GROUPS)
    tr2.load_checkpoint(str(tmp_path / "on"), camera_optimizer=opt2)
    assert torch.equal(opt2.pose_adjustment, opt.pose_adjustment) and torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    assert opt2.step_count == 2 and opt2.skipped_steps() == {"camera_opt": 0}
    tr2.load_checkpoint(str(tmp_path / "off"), camera_optimizer=opt2)  # written with the feature off: the poses start from zeros
    assert float(opt2.pose_adjustment.abs().max()) == 0.0

"""GPU: frames, camera paths and checkpoints from the fused NeRFPlayer-nerfacto trainer (soccernerfs_amd/render.py::NerfplayerRenderer,
NerfplayerTrainer.save_checkpoint / load_checkpoint, tools/render.py --method nerfplayer-nerfacto).

(a) a frame equals the eval path -- the same rays in R-sized slices through NerfplayerTrainer.forward(training=False), composited on black -- bit
    for bit, with the fused proposal density off and on, for fp32 and bf16 operands;
(b) the frame does not depend on the chunk size (rgb, accumulation and the per-ray clamped depth);
(c) a render between training steps leaves deterministic training bit-for-bit where it was;
(d) a render straight after train_step (asynchronous sweep + tiled pass pending) needs no host synchronise;
(e) checkpoints: parameters, moments, step and frame come back bit for bit; the file is the reference model's, and that model renders the frame;
(f) lens and fisheye cameras go through the matching ray entry and give Cameras.generate_rays' rays;
(g) render_camera_path, the tools/render.py command line, the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_TRAIN, N_IMG, W, H = 128, 5, 24, 20
PROP = {"hidden_dim": 16, "temporal_dim": 8, "log2_hashmap_size": 12, "num_levels": 5}
SMALL = dict(num_levels=4, log2_hashmap_size=12, temporal_dim=8, num_proposal_samples_per_ray=(32, 16), num_nerf_samples_per_ray=8,
             proposal_net_args_list=[{**PROP, "max_res": 64}, {**PROP, "max_res": 256}])


def _cfg(**kw):
    from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModelConfig

    return NerfplayerNerfactoModelConfig(**{**SMALL, **kw})


def _inputs(steps, seed=3):
    gen = torch.Generator().manual_seed(seed)
    g = lambda z: z.to(DEV).contiguous()
    out = []
    for _ in range(steps):
        R = R_TRAIN
        rays = {"origins": g((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.3),
                "directions": g(torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)), "times": g(torch.rand(R, 1, generator=gen))}
        cams = g(torch.randint(0, N_IMG, (R,), generator=gen))
        rng = {"t_rand": g(torch.rand(R, 1, generator=gen)), "u": [g(torch.rand(R, 1, generator=gen)), g(torch.rand(R, 1, generator=gen))],
               "bg": g(torch.rand(R, 3, generator=gen))}
        out.append((rays, cams, g(torch.rand(R, 3, generator=gen)), rng))
    return out


def _trainer(steps=3, inputs=None, seed=0, cfg=None, **kw):
    """A small trainer with O(1) tables (the 1e-4 init gives a featureless field), `steps` training steps taken."""
    from soccernerfs_amd.nerfplayer_trainer import NerfplayerTrainer

    tr = NerfplayerTrainer(cfg if cfg is not None else _cfg(), R_TRAIN, N_IMG, aabb_scale=1.0, device=DEV, seed=seed, warm_up_end=2, **kw)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 50)
        for name in ("field.table", "prop0.table", "prop1.table"):
            tr.views[name].copy_((torch.rand(tr.views[name].shape, generator=gen) * 2 - 1).to(DEV))
    for rays, cams, target, rng in (inputs if inputs is not None else _inputs(steps)):
        tr.train_step(rays, cams, target, rng)
    return tr


def _cameras(**kw):
    """Three cameras inside the box [-1,1]^3 looking at its centre, 24 x 20 pixels, at times 0, 0.37 and 1."""
    from soccernerfs_amd.cameras import Cameras

    c2w = []
    for p in ([0.7, 0.1, 0.2], [-0.3, 0.6, 0.4], [0.2, -0.5, 0.65]):
        p = torch.tensor(p)
        z = torch.nn.functional.normalize(p, dim=0)  # the camera looks along -z
        x = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]), z), dim=0)
        c2w.append(torch.stack([x, torch.linalg.cross(z, x), z, p], dim=1))
    return Cameras(torch.stack(c2w), 20.0, 21.0, W / 2, H / 2, W, H, times=torch.tensor([0.0, 0.37, 1.0]), **kw)


def _clamp_per_ray(depth, eb):
    return torch.clamp(depth, min=(eb[:, 0] + eb[:, 1]) / 2, max=(eb[:, -2] + eb[:, -1]) / 2)


def _eval_path_frame(tr, cams, k, anneal):
    """Today's route to a frame (tools/train_psnr_nerfplayer.py::eval_psnr): the meshgrid index table in R-sized slices through
    forward(training=False) -- the trainer's buffers take exactly R rays, so the ragged last slice is padded with its last pixel -- on black."""
    from soccernerfs_amd import ops

    c = cams.to(DEV)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
    rgb, acc, depth = torch.empty(H * W, 3, device=DEV), torch.empty(H * W, device=DEV), torch.empty(H * W, device=DEV)
    black = torch.zeros(tr.R, 3, device=DEV)
    for i in range(0, H * W, tr.R):
        sl = idx[i:i + tr.R]
        n = sl.shape[0]
        if n < tr.R:
            sl = torch.cat([sl, sl[-1:].expand(tr.R - n, 3)])
        rays = ops.generate_rays(sl.contiguous(), c.fx, c.fy, c.cx, c.cy, c.camera_to_worlds, c.times)
        rgb[i:i + n] = tr.forward(rays, None, {"bg": black}, anneal, training=False)[:n]
        acc[i:i + n] = tr.buf["acc"][:n]
        depth[i:i + n] = _clamp_per_ray(tr.buf["depth"], tr.buf["eb"][2])[:n]
    return rgb.view(H, W, 3), acc.view(H, W, 1), depth.view(H, W, 1)


# ---- (a) ----
@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_frame_equals_the_eval_path(operands):
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer(mlp_operands=operands)
    cams = _cameras()
    frames = {}
    for fused in (False, True):
        rn = NerfplayerRenderer(tr, rays_per_chunk=128, fused_density=fused)  # 480 pixels = 3 full chunks + a ragged one of 96
        assert rn.fused_density == [fused, fused]  # the small trainer's proposal levels have the preset's shape: L = 5, C = 2, net 10 -> 16 -> 1
        frames[fused] = rn.render_frame(cams, 1)
        assert {q: tuple(v.shape) for q, v in frames[fused].items()} == {"rgb": (H, W, 3), "accumulation": (H, W, 1), "depth": (H, W, 1)}
        anneal = rn.default_anneal()
    rgb, acc, depth = _eval_path_frame(tr, cams, 1, anneal)
    assert bool(torch.isfinite(rgb).all()) and float(rgb.std()) > 0 and 0.0 < float(acc.mean()) and float(acc.min()) < 0.999
    for fused in (False, True):
        assert torch.equal(frames[fused]["rgb"], rgb), (fused, float((frames[fused]["rgb"] - rgb).abs().max()))
        assert torch.equal(frames[fused]["accumulation"], acc), fused
        assert torch.equal(frames[fused]["depth"], depth), fused


# ---- (b) ----
@pytest.mark.parametrize("fused", [False, True], ids=["pair", "fused_density"])
def test_frame_does_not_depend_on_the_chunk_size(fused):
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer()
    cams = _cameras()
    a = NerfplayerRenderer(tr, rays_per_chunk=128, fused_density=fused).render_frame(cams, 2)
    b = NerfplayerRenderer(tr, rays_per_chunk=480, fused_density=fused).render_frame(cams, 2)
    for q in ("rgb", "accumulation", "depth"):
        assert torch.equal(a[q], b[q]), q
    # the clamp is a ray's own: no depth lies outside its ray's sample midpoints, and it is not the constant a shared clamp would give
    assert bool(torch.isfinite(a["depth"]).all()) and float(a["depth"].std()) > 0


# ---- (c) ----
def test_rendering_between_steps_leaves_training_undisturbed():
    from soccernerfs_amd.render import NerfplayerRenderer

    inputs = _inputs(4)
    cams = _cameras()
    a = _trainer(inputs=inputs[:2], deterministic=True)
    frame = NerfplayerRenderer(a, rays_per_chunk=128, fused_density=True).render_frame(cams, 0)
    assert bool(torch.isfinite(frame["rgb"]).all())
    for rays, cm, target, rng in inputs[2:]:
        a.train_step(rays, cm, target, rng)
    a.synchronize()
    b = _trainer(inputs=inputs, deterministic=True)
    b.synchronize()
    assert a.step == b.step == 4
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)


# ---- (d) ----
def test_no_host_synchronise_is_needed_after_train_step():
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer(async_field_sweep=True, tiled_field_backward=True)
    assert tr._sweeps_done is not None  # the field table's tile pass of the last step went to the side stream
    cams = _cameras()
    rn = NerfplayerRenderer(tr, rays_per_chunk=128)
    hot = {q: v.clone() for q, v in rn.render_frame(cams, 1).items()}
    tr.synchronize()
    cold = rn.render_frame(cams, 1)
    for q in hot:
        assert torch.equal(hot[q], cold[q]), q


# ---- (e) ----
def test_checkpoint_round_trip(tmp_path):
    from soccernerfs_amd import checkpoint as CK
    from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModel
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.render import NerfplayerRenderer
    from soccernerfs_amd.scene_colliders import SceneBox

    tr = _trainer(steps=3)
    cams = _cameras()
    rn = NerfplayerRenderer(tr, rays_per_chunk=480)
    want = rn.render_frame(cams, 1)
    path = tr.save_checkpoint(str(tmp_path))
    assert os.path.basename(path) == "step-000000002.ckpt"  # the last completed iteration
    fresh = _trainer(steps=0, seed=99)
    assert not torch.equal(fresh.params, tr.params)
    assert fresh.load_checkpoint(str(tmp_path)) == 3
    assert fresh.step == tr.step == 3
    assert torch.equal(fresh.params, tr.params) and torch.equal(fresh.exp_avg, tr.exp_avg) and torch.equal(fresh.exp_avg_sq, tr.exp_avg_sq)
    got = NerfplayerRenderer(fresh, rays_per_chunk=480).render_frame(cams, 1)
    for q in want:
        assert torch.equal(got[q], want[q]), q
    # params_only: the parameters, a fresh optimiser
    po = _trainer(steps=1, seed=7)
    assert po.load_checkpoint(str(tmp_path), params_only=True) == 0 and po.step == 0
    assert torch.equal(po.params, tr.params) and float(po.exp_avg.abs().max()) == 0.0 and float(po.exp_avg_sq.abs().max()) == 0.0
    # the file is NerfplayerNerfactoModel's: same keys, the strict loader accepts it, and the model renders the frame
    cfg = _cfg(background_color="black")
    model = NerfplayerNerfactoModel(cfg, SceneBox(aabb=torch.tensor(tr.aabb)), num_train_data=N_IMG)
    loaded = torch.load(path, map_location="cpu", weights_only=False)
    assert loaded["step"] == 2 and set(loaded["optimizers"]) == {"fields", "proposal_networks"}
    assert list(loaded["pipeline"]) == list(CK.reference_state_dict(model))
    CK.load_reference_state_dict(model, loaded["pipeline"], strict=True)
    model = model.to(DEV).eval()
    model.scene_box.aabb = model.scene_box.aabb.to(DEV)
    model.proposal_sampler.set_anneal(rn.default_anneal())
    rays = cams.to(DEV).generate_rays(1)
    flat = lambda t: t.reshape(H * W, -1)
    with torch.no_grad():
        out = model(RayBundle(origins=flat(rays.origins), directions=flat(rays.directions), pixel_area=flat(rays.pixel_area),
                              camera_indices=torch.zeros(H * W, 1, dtype=torch.long, device=DEV), times=flat(rays.times)))
    torch.testing.assert_close(out["rgb"].view(H, W, 3), want["rgb"], rtol=1e-5, atol=1e-6)  # DESIGN section 2's fp32 tolerance


# ---- (f) ----
@pytest.mark.parametrize("kind", ["lens", "fisheye"])
def test_lens_and_fisheye_cameras_take_the_matching_entry(kind):
    from soccernerfs_amd.cameras import CameraType
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer(steps=1)
    if kind == "lens":
        cams, entry = _cameras(distortion_params=torch.tensor([0.05, -0.02, 0.0, 0.0, 0.001, -0.002])), "raygen_frame_lens"
    else:
        cams, entry = _cameras(camera_type=CameraType.FISHEYE), "raygen_frame_cam"
    rn = NerfplayerRenderer(tr, rays_per_chunk=H * W)  # one chunk: the renderer's ray buffers hold the whole frame afterwards
    names, ck = [], rn._ck
    rn._ck = lambda rc, what="": (names.append(what), ck(rc, what))[1]
    frame = rn.render_frame(cams, 2)
    assert [n for n in names if n.startswith("raygen")] == [entry]
    assert bool(torch.isfinite(frame["rgb"]).all())
    want = cams.to(DEV).generate_rays(2)
    assert torch.equal(rn._rays["origins"], want.origins.reshape(-1, 3)) and torch.equal(rn._rays["directions"], want.directions.reshape(-1, 3))
    assert torch.equal(rn._rays["times"], want.times.reshape(-1))
    # and the frame is that of the same rays on the pair path in smaller chunks
    again = NerfplayerRenderer(tr, rays_per_chunk=100, fused_density=False).render_frame(cams, 2)
    assert torch.equal(again["rgb"], frame["rgb"])


# ---- (g) ----
def _path_json(cams, with_times=True):
    """A camera-path dict (the viewer's export) of the table's cameras."""
    entries = []
    for k in range(len(cams)):
        m = torch.eye(4)
        m[:3] = cams.camera_to_worlds[k]
        e = {"camera_to_world": m.reshape(-1).tolist(), "fov": 50.0, "aspect": W / H}
        if with_times:
            e["render_time"] = float(cams.times[k])
        entries.append(e)
    return {"render_height": H, "render_width": W, "camera_path": entries, "camera_type": "perspective", "seconds": 1.0}


def test_render_camera_path_writes_frames(tmp_path):
    from PIL import Image

    from soccernerfs_amd.camera_paths import get_path_from_json
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer(steps=2)
    path = _path_json(_cameras())
    cams = get_path_from_json(path)
    rn = NerfplayerRenderer(tr, rays_per_chunk=200)
    files = rn.render_camera_path(path, str(tmp_path / "png"), outputs=("rgb", "depth"))
    assert [os.path.basename(f) for f in files] == sorted(os.listdir(tmp_path / "png")) == [f"{k:05d}.png" for k in range(len(cams))]
    for k, f in enumerate(files):
        frame = rn.render_frame(cams, k)
        want = rn.to_uint8(torch.cat([frame["rgb"], frame["depth"].expand(-1, -1, 3)], dim=1)).cpu()
        assert torch.equal(torch.from_numpy(np.array(Image.open(f))), want)
    res = rn.evaluate(cams, torch.zeros(len(cams), H, W, 3, dtype=torch.uint8), [0, 2])
    assert len(res["psnr_per_image"]) == 2 and np.isfinite(res["psnr"])
    with pytest.raises(ValueError, match="default_time"):
        rn.render_camera_path(_path_json(_cameras(), with_times=False), str(tmp_path / "x"))


def test_tools_render_command_line(tmp_path):
    import importlib.util

    from PIL import Image

    from soccernerfs_amd.camera_paths import get_path_from_json
    from soccernerfs_amd.render import NerfplayerRenderer

    spec = importlib.util.spec_from_file_location("tools_render_cli_np", os.path.join(ROOT, "tools", "render.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    tr = _trainer(steps=2)
    tr.save_checkpoint(str(tmp_path / "ckpt"))
    path = _path_json(_cameras())
    (tmp_path / "path.json").write_text(json.dumps(path))
    argv = ["--method", "nerfplayer-nerfacto", "--load-dir", str(tmp_path / "ckpt"), "--camera-path-filename", str(tmp_path / "path.json"),
            "--output-path", str(tmp_path / "out"), "--eval-num-rays-per-chunk", "200", "--device", DEV]
    for k, v in SMALL.items():
        argv += ["--set", f"{k}={v!r}"]
    cli.main(argv)
    cams = get_path_from_json(path)
    rn = NerfplayerRenderer(tr, rays_per_chunk=200)
    assert sorted(os.listdir(tmp_path / "out")) == [f"{k:05d}.png" for k in range(len(cams))]
    for k in range(len(cams)):
        img = torch.from_numpy(np.array(Image.open(tmp_path / "out" / f"{k:05d}.png")))
        assert torch.equal(img, rn.to_uint8(rn.render_frame(cams, k)["rgb"]).cpu()), k
    with pytest.raises(SystemExit):
        cli.config_from_overrides(["no_such_field=1"], method="nerfplayer-nerfacto")


def test_refusals():
    from soccernerfs_amd.cameras import Cameras
    from soccernerfs_amd.nerfplayer import NerfplayerModelConfig
    from soccernerfs_amd.nerfplayer_full_trainer import NerfplayerFullTrainer
    from soccernerfs_amd.render import NerfplayerRenderer

    tr = _trainer(steps=0)
    with pytest.raises(ValueError, match="rays_per_chunk"):
        NerfplayerRenderer(tr, rays_per_chunk=0)
    with pytest.raises(ValueError, match="background_color"):
        NerfplayerRenderer(tr, background_color="green")
    with pytest.raises(ValueError, match="torch.Generator"):
        NerfplayerRenderer(tr, background_color="random")
    c = _cameras()
    no_times = Cameras(c.camera_to_worlds, c.fx, c.fy, c.cx, c.cy, W, H)
    rn = NerfplayerRenderer(tr, rays_per_chunk=128)
    before = rn.launches
    with pytest.raises(ValueError, match="default_time"):
        rn.render_frame(no_times, 0)
    assert rn.launches == before  # refused before any launch
    a, b = rn.render_frame(no_times, 1, default_time=0.37), rn.render_frame(c, 1)
    assert torch.equal(a["rgb"], b["rgb"])
    full = NerfplayerFullTrainer(NerfplayerModelConfig(**{**SMALL, "num_levels": 16}), 64, aabb_scale=1.0, device=DEV)
    with pytest.raises(TypeError, match="NerfplayerFullTrainer"):
        NerfplayerRenderer(full)
    # the other backgrounds: white adds 1 - accumulation, last_sample and random differ from black where the ray is not opaque
    white = NerfplayerRenderer(tr, rays_per_chunk=128, background_color="white").render_frame(c, 1)
    torch.testing.assert_close(white["rgb"], (b["rgb"] + (1.0 - b["accumulation"])).clamp(0, 1), rtol=0, atol=2e-6)
    gen = torch.Generator(device=DEV).manual_seed(5)
    rnd = NerfplayerRenderer(tr, rays_per_chunk=128, background_color="random", generator=gen).render_frame(c, 1)
    assert torch.equal(rnd["accumulation"], b["accumulation"]) and not torch.equal(rnd["rgb"], b["rgb"])
    last = NerfplayerRenderer(tr, rays_per_chunk=128, background_color="last_sample").render_frame(c, 1)
    assert torch.equal(last["depth"], b["depth"]) and bool(torch.isfinite(last["rgb"]).all())

#!/usr/bin/env python3
"""PSNR@N-iterations runs of the k-planes preset on the synthetic Broadcast-style scene (BASELINE.json metric, 2nd half).

Trains with the fused HIP trainer exactly as the reference schedules it (4096 rays/step, uniform pixels for the first
`iters_to_start_is` = 2000 steps, then 15 % IST importance rays; proposal-weight annealing; proposal updates every n steps;
Adam + cosine schedule), then renders held-out views (full images, eval-mode sampler, 'last_sample' background, clamp) and
reports PSNR = 10 log10(1/MSE) per image and averaged (NS/models/kplanes.py:291,472; NS/pipelines/base_pipeline.py:323-362).

Evaluation sets (all frames of every camera unless --eval-frames):
  * "camera_20": the 20th camera of the arc, the reference's "all" split eval camera (broadcaststyle_dataparser.py:166-190).  It sits at
    the END of the arc, i.e. it is an EXTRAPOLATED view;
  * "novel": three evaluation-only cameras half-way between training cameras (synthetic.make_novel_cameras): interpolated views;
  * "train": four training images (sanity: the fit itself).
Several seeds run in one process on the same dataset; the JSON holds every run and the mean / spread per set.

    python tools/train_psnr.py --steps 30000 --seeds 1,2,3 --out gpurun_out/psnr_r02_fp32.json
"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import ops, synthetic  # noqa: E402
from soccernerfs_amd.metrics import structural_similarity_index_measure as ssim_fn  # noqa: E402
from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler, compute_ist  # noqa: E402
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer, anneal_value  # noqa: E402


def collider_args(cfg) -> dict:
    """ops.generate_rays' collider for a trainer config: the box (default), or near / far constants for an unbounded scene."""
    return {} if getattr(cfg, "bounded", True) else {"collider": "near_far", "far_plane": cfg.far_plane}


@torch.no_grad()
def eval_set(trainer, data, image_ids, anneal, with_ssim=True):
    """PSNR (and SSIM) of full-image renders of data["images"][image_ids]."""
    imgs = data["images"]
    H, W = imgs.shape[1:3]
    R = getattr(trainer, "eval_chunk", trainer.R)
    ys, xs = torch.meshgrid(torch.arange(H, device=imgs.device), torch.arange(W, device=imgs.device), indexing="ij")
    psnrs, ssims = [], []
    for m in image_ids:
        idx = torch.stack([torch.full_like(ys, m), ys, xs], -1).reshape(-1, 3)
        out = torch.empty(H * W, 3, device=imgs.device)
        for i in range(0, H * W, R):
            rays = ops.generate_rays(idx[i:i + R].contiguous(), data["fx"], data["fy"], data["cx"], data["cy"], data["c2w"], data["times"],
                                     aabb=trainer.aabb, near_plane=trainer.cfg.near_plane, training=False, distortion_params=data.get("ray_distortion"),
                                     **collider_args(trainer.cfg))
            out[i:i + R] = trainer.forward(rays, None, anneal, training=False)
        gt = imgs[m].reshape(-1, 3).float() / 255.0
        mse = torch.mean((out - gt) ** 2)
        psnrs.append(float(10.0 * torch.log10(1.0 / mse)))
        if with_ssim:
            chw = lambda t: t.view(H, W, 3).permute(2, 0, 1)[None]
            ssims.append(float(ssim_fn(chw(gt), chw(out))))  # as get_image_metrics_and_images (kplanes.py:469-473)
    return psnrs, ssims


def perturb_poses(c2w, cam_id, pos_std, rot_std, seed):
    """A seeded SE(3) perturbation of a camera table on the host, ONE per physical camera (a static stadium camera is miscalibrated the same
    way in all of its frames): c2w' = [R exp(w) | t + dt] with w ~ N(0, rot_std^2) (radians, axis-angle) and dt ~ N(0, pos_std^2) per axis."""
    gen = torch.Generator().manual_seed(seed)
    ids = cam_id.cpu()
    uniq = torch.unique(ids)
    w = torch.randn(len(uniq), 3, generator=gen, dtype=torch.float64) * rot_std
    dt = torch.randn(len(uniq), 3, generator=gen, dtype=torch.float64) * pos_std
    row = torch.searchsorted(uniq, ids)
    th = w.norm(dim=1).clamp_min(1e-12)
    k = w / th[:, None]
    K = torch.zeros(len(uniq), 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    E = torch.eye(3, dtype=torch.float64)[None] + torch.sin(th)[:, None, None] * K + (1 - torch.cos(th))[:, None, None] * (K @ K)
    m = c2w.cpu().double()
    out = torch.cat([m[:, :, :3] @ E[row], m[:, :, 3:] + dt[row][:, :, None]], dim=-1)
    return out.float().to(c2w.device).contiguous()


def pose_error(c2w, c2w_true):
    """Error of a camera table against the true one: RMS of the camera-centre error and mean rotation angle (degrees), raw and after the rigid
    alignment (rotation + translation, Kabsch on the camera centres) that a joint optimisation is free to apply to the whole scene."""
    a, b = c2w.detach().cpu().double(), c2w_true.detach().cpu().double()

    def figures(m):
        d = m[:, :, 3] - b[:, :, 3]
        rel = m[:, :, :3].transpose(1, 2) @ b[:, :, :3]
        cos = ((rel[:, 0, 0] + rel[:, 1, 1] + rel[:, 2, 2]) - 1) / 2
        return {"centre_rms": float(d.pow(2).sum(1).mean().sqrt()), "rotation_mean_deg": float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))).mean())}

    ca, cb = a[:, :, 3].mean(0), b[:, :, 3].mean(0)
    H = (a[:, :, 3] - ca).t() @ (b[:, :, 3] - cb)
    U, _, Vt = torch.linalg.svd(H)
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.det(Vt.t() @ U.t())))], dtype=torch.float64))
    Rg = Vt.t() @ D @ U.t()
    aligned = torch.cat([Rg[None] @ a[:, :, :3], (Rg[None] @ (a[:, :, 3:] - ca[None, :, None])) + cb[None, :, None]], dim=-1)
    return {"raw": figures(a), "aligned": figures(aligned)}


def stats(xs):
    n = len(xs)
    mean = sum(xs) / n
    return {"mean": mean, "min": min(xs), "max": max(xs), "std": (sum((x - mean) ** 2 for x in xs) / max(n - 1, 1)) ** 0.5, "n": n}


def static_pretrain(args, cfg, trainer, train, R, dev):
    """Stage 1 of the reference's two-stage recipe (broadcaststyle_dataparser.py `static`): args.static_pretrain steps of a trainer with
    freeze_time_planes on the EMPTY scene seen by the training cameras (uniform pixels; one frame per camera, the scene does not move), then the
    hand-over: `trainer` starts its own schedule from the pre-trained planes (load_checkpoint(params_only=True))."""
    import dataclasses
    import tempfile

    empty = train["empty"]
    M, H, W = empty["images"].shape[:3]
    stage1 = KPlanesTrainer(dataclasses.replace(cfg, freeze_time_planes=True, ray_gradients=False), R, dev)
    t0 = time.time()
    for _ in range(args.static_pretrain):
        idx, target = ops.sample_pixels_uniform(torch.rand(R, 3, device=dev), M, H, W, images=empty["images"])
        rays = ops.generate_rays(idx, empty["fx"], empty["fy"], empty["cx"], empty["cy"], empty["c2w"], empty["times"], aabb=stage1.aabb,
                                 near_plane=cfg.near_plane, training=True, distortion_params=train.get("ray_distortion"), **collider_args(cfg))
        stage1.train_step(rays, target)
    with tempfile.TemporaryDirectory() as d:
        stage1.save_checkpoint(d)
        trainer.load_checkpoint(d, params_only=True)
    print(f"[seed {cfg.seed}] static pre-training: {args.static_pretrain} steps with frozen time planes on the empty scene in {time.time() - t0:.0f} s, "
          f"rgb_loss {float(stage1.loss_dict()['rgb_loss']):.5f}", flush=True)


def run_one(args, seed, train, sets, ist, dev, log_steps=True):
    torch.manual_seed(seed)
    random.seed(seed)
    cfg = KPlanesTrainConfig(max_steps=args.schedule_steps, mlp_operands=args.mlp_operands, seed=seed, deterministic=args.deterministic,
                             disable_viewing_dependent=not args.view_dependent,
                             nonfinite_policy=args.nonfinite_policy, fused_field=not args.no_fused_field, quotient_scatter=not args.no_quotient_scatter, gvec_dtype=args.gvec_dtype,
                             emulate_transports=args.emulate_transports, quotient_epilogue=not args.no_quotient_epilogue, fused_proposal=not args.no_fused_proposal,
                             sigma_operands=args.sigma_operands, color_operands=args.color_operands, proposal_operands=args.proposal_operands,
                             ray_gradients=args.optimize_cameras)
    if args.unbounded:  # contracted coordinates, near / far collider, piecewise spacing (KPlanesTrainConfig.bounded)
        cfg.bounded, cfg.near_plane, cfg.far_plane = False, args.near_plane, args.far_plane
    if args.static_scene:  # the original static K-Planes model: three planes per scale, no time axis (kplanes_field.py:59-61)
        cfg.spacetime_resolution = tuple(cfg.spacetime_resolution)[:3]
        cfg.proposal_resolutions = tuple(tuple(r)[:3] for r in cfg.proposal_resolutions)
    R = 4096
    if args.standin:
        # the reference's algorithm in stock PyTorch (oracle/torch_standin.py: checker / baseline code, imported ONLY for this mode) on the same
        # pixel draws (same sampler, same seed), the same rays and the same evaluation; F.grid_sample per plane as the reference calls it
        from oracle import kplanes_oracle as KO, torch_standin as TS
        KO.USE_GRID_SAMPLE = args.standin_layout != "hwc"
        trainer = TS.StandinTrainer(dev, R, seed=seed, max_steps=args.schedule_steps, plane_layout=args.standin_layout)
    else:
        trainer = KPlanesTrainer(cfg, R, dev)
        if args.oracle_init:  # the stand-in's initial parameters (same generator, same seed) instead of the trainer's own draw
            from oracle import kplanes_oracle as KO, torch_standin as TS
            trainer.load_oracle_params(KO.make_kplanes_params(seed=seed, **TS.PRESET))
        if args.no_overlap:
            trainer.overlap, trainer.async_field_adam = False, False
        if args.static_pretrain:
            static_pretrain(args, cfg, trainer, train, R, dev)
    M, H, W = train["images"].shape[:3]
    batch = {"image": train["images"], "image_idx": torch.arange(M, device=dev), "ist_weights": ist, "iter_steps": 0}
    # (an empty scene has no temporal differences to draw importance rays from: uniform pixels throughout)
    sampler = DynamicBasedPixelSampler(R, is_pixel_ratio=0.15, iters_to_start_ist=2000 if not args.static_scene else args.steps + 1, mask_ist_weights=args.mask_ist)
    mask = train.get("mask") if args.use_masks else None  # --use-masks: every uniform draw inside the mask (and with --mask-ist the IST draws too)
    if mask is not None:
        batch["mask"] = mask
        DynamicBasedPixelSampler.prepare_mask(batch)
    DynamicBasedPixelSampler.prepare(batch, args.mask_ist)
    time_key, n_time_keys = ops.image_time_keys(train["times"])
    run = {"seed": seed, "evals": []}
    cam_opt, cameras, c2w_given = None, None, train["c2w"]
    if "c2w_true" in train:
        run["pose_error_before"] = pose_error(c2w_given, train["c2w_true"])
    if args.optimize_cameras:
        # CameraOptimizer (SO3xR3): the training rays and the training-view evaluation go through the adjusted table; held-out cameras stay as given
        from soccernerfs_amd.camera_optimizers import CameraOptimizer, CameraOptimizerConfig
        from soccernerfs_amd.cameras import Cameras
        from soccernerfs_amd.dataparsers import camera_pose_groups

        cameras = Cameras(c2w_given, train["fx"], train["fy"], train["cx"], train["cy"], W, H, times=train["times"], ids=train["cam_id"],
                          distortion_params=train.get("ray_distortion"))
        cam_opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3", max_steps=args.schedule_steps), M, dev,
                                  groups=camera_pose_groups(cameras) if args.share_poses_per_camera else None)
        run["pose_rows"] = cam_opt.num_groups
    t_train, t_eval = 0.0, 0.0
    t_start, last_step = time.time(), args.steps - 1
    eval_at = {int(x) for x in args.eval_at.split(",") if x}

    def evaluate(step):
        nonlocal t_eval
        an = anneal_value(step, cfg.proposal_weights_anneal_max_num_iters, cfg.proposal_weights_anneal_slope)
        ev = {"step": step + 1}
        t2 = time.time()
        for name, (data, ids) in sets.items():
            if name == "train" and cam_opt is not None:  # training views are rendered from where the optimiser has moved their cameras
                data = dict(data, c2w=cam_opt.adjusted_camera_to_worlds(cameras))
            ps, ss = eval_set(trainer, data, ids, an, with_ssim=name != "train")
            ev[name] = {"psnr_mean": sum(ps) / len(ps), "psnr_min": min(ps), "images": len(ps), "psnr_per_image": [round(p, 3) for p in ps]}
            if ss:
                ev[name]["ssim_mean"] = sum(ss) / len(ss)
        run["evals"].append(ev)
        torch.cuda.synchronize()
        t_eval += time.time() - t2
        print(f"== [seed {seed}] step {step + 1}: " + "  ".join(f"{k} {v['psnr_mean']:.2f} dB" for k, v in ev.items() if k != "step") + f"  (eval {time.time() - t2:.0f} s)", flush=True)

    for step in range(args.steps):
        if args.train_budget_s and step % 100 == 0 and time.time() - t_start > args.train_budget_s:
            # out of wall-clock (a gpurun call is capped at one hour): stop here, evaluate, and SAY how far the run got
            last_step = step - 1
            run["stopped_early_at_step"] = step
            print(f"[seed {seed}] training budget of {args.train_budget_s} s spent at step {step}: evaluating there", flush=True)
            break
        if step % 1000 == 0:
            torch.cuda.synchronize()
            t1 = time.time()
        batch["iter_steps"] = step
        idx = sampler.sample_method(R, M, H, W, mask=batch.get("mask_index"), batch=batch, device=dev)
        if args.time_sorted_rays:  # the batch in order of frame time (ops.sort_rays_by_time: a batch is a set), as bench.py runs it
            idx = ops.sort_rays_by_time(idx, time_key, n_time_keys)
        target = train["images"][idx[:, 0], idx[:, 1], idx[:, 2]].float() / 255.0
        table = cam_opt.adjusted_camera_to_worlds(cameras) if cam_opt is not None else train["c2w"]
        rays = ops.generate_rays(idx, train["fx"], train["fy"], train["cx"], train["cy"], table, train["times"], aabb=trainer.aabb,
                                 near_plane=cfg.near_plane, training=True, distortion_params=train.get("ray_distortion"), **collider_args(cfg))
        trainer.train_step(rays, target)
        if cam_opt is not None:
            cam_opt.backward(idx, trainer.ray_grads)
            cam_opt.step()
        if args.standin and step % 100 == 99:
            print(f"[standin seed {seed}] step {step + 1} {time.time() - t1:.1f}s into this thousand", flush=True)
        if step % 1000 == 999:
            torch.cuda.synchronize()
            dt = time.time() - t1
            t_train += dt
            if log_steps:
                ld = {k: float(v) for k, v in trainer.loss_dict().items()}
                print(f"[seed {seed}] step {step + 1}: {R * 1000 / dt:,.0f} rays/s  rgb_loss {ld['rgb_loss']:.5f} "
                      f"(psnr~{-10 * torch.log10(torch.tensor(ld['rgb_loss'])).item():.2f}) interlevel {ld['interlevel_loss']:.2e} "
                      f"skipped steps {trainer.skipped_steps()}", flush=True)
        if ((step + 1) % args.eval_every == 0 or (step + 1) in eval_at) and step + 1 < args.steps:
            evaluate(step)
    evaluate(last_step)
    run["train_seconds"] = t_train
    run["train_rays_per_s_mean"] = R * ((last_step + 1) // 1000 * 1000) / max(t_train, 1e-9)
    run["skipped_steps"] = trainer.skipped_steps()
    if cam_opt is not None:
        run["skipped_steps"].update(cam_opt.skipped_steps())
        adj = cam_opt.pose_adjustment.detach()
        run["pose_adjustment_rms"] = {"translation": float(adj[:, :3].pow(2).mean().sqrt()), "rotation": float(adj[:, 3:].pow(2).mean().sqrt())}
        if "c2w_true" in train:
            run["pose_error_after"] = pose_error(cam_opt.adjusted_camera_to_worlds(cameras), train["c2w_true"])
    elif "c2w_true" in train:
        run["pose_error_after"] = run["pose_error_before"]
    trainer.synchronize()
    run["param_checksum"] = float(trainer.params.double().sum())
    run["eval_seconds"] = t_eval
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--schedule-steps", type=int, default=30000, help="max_steps of the cosine schedule")
    ap.add_argument("--seeds", default="20231029")
    ap.add_argument("--eval-frames", type=int, default=0, help="frames per held-out camera (0 = all)")
    ap.add_argument("--eval-every", type=int, default=10000)
    ap.add_argument("--out", default="gpurun_out/psnr.json")
    ap.add_argument("--mlp-operands", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--gvec-dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--sigma-operands", default=None)
    ap.add_argument("--color-operands", default=None)
    ap.add_argument("--proposal-operands", default=None)
    ap.add_argument("--deterministic", action="store_true", help="fixed-point gradient accumulation: bit-identical reruns")
    ap.add_argument("--view-dependent", action="store_true", help="colour net on [SH4 of the direction | geometry features] (KPlanesModelConfig's class default)")
    ap.add_argument("--nonfinite-policy", default="skip_step", choices=["skip_step", "drop_elements"])
    ap.add_argument("--no-fused-field", action="store_true", help="unfused forward kernels")
    ap.add_argument("--no-quotient-epilogue", action="store_true", help="round 3's flow: G = gfeat .* feat from the separate pass over fp32 features (A-B)")
    ap.add_argument("--no-fused-proposal", action="store_true", help="proposal levels as gather + net kernels (A-B; bit-identical densities)")
    ap.add_argument("--no-quotient-scatter", action="store_true", help="product form of the field's sorted scatter")
    ap.add_argument("--emulate-transports", default="", choices=["", "grad", "param", "both"],
                    help="single-GPU emulation of the bf16 gradient / parameter-update transports of the sharded multi-GPU step (KPlanesTrainConfig.emulate_transports)")
    ap.add_argument("--time-sorted-rays", action="store_true", help="every batch in order of frame time, as bench.py runs it")
    ap.add_argument("--standin", action="store_true",
                    help="train the REFERENCE'S ALGORITHM in stock PyTorch (oracle/torch_standin.StandinTrainer: F.grid_sample per plane, Linear stacks, autograd, "
                         "two torch.optim.Adam, fp32) instead of the HIP trainer -- same pixel draws, rays, schedule and evaluation; ~95 ms / step")
    ap.add_argument("--standin-layout", default="chw", choices=["chw", "hwc"], help="--standin: chw = planes [1,C,H,W] through F.grid_sample, the reference's own call; "
                    "hwc = the same algorithm on channel-last planes gathered as rows (oracle KO._bilinear_plane_rows, checked against F.grid_sample by "
                    "tests/test_standin_cpu.py): about twice the rate, so that 30 000 steps fit one GPU call")
    ap.add_argument("--eval-at", default="", help="extra evaluation steps, comma separated (e.g. the step a stand-in run got to)")
    ap.add_argument("--train-budget-s", type=float, default=0.0, help="stop training when this much wall-clock is spent (a gpurun call is capped at one hour), "
                    "evaluate there and record `stopped_early_at_step`")
    ap.add_argument("--oracle-init", action="store_true", help="HIP trainer from the stand-in's initial parameters of the same seed")
    ap.add_argument("--scene", default="default", choices=["default", "textured"], help="synthetic.shade variant (textured: grass grain, board, crowd, ten players)")
    ap.add_argument("--no-overlap", action="store_true", help="single-stream step (A/B against stream-ordering effects)")
    ap.add_argument("--static-pretrain", type=int, default=0, metavar="N", help="N steps with freeze_time_planes on the empty scene (no players, no ball) first, "
                    "then the usual run from those planes (KPlanesTrainer.load_checkpoint(params_only=True)); compare against --steps raised by N")
    ap.add_argument("--unbounded", action="store_true", help="KPlanesTrainConfig.bounded=False: L-inf scene contraction in the kernels, near / far collider, "
                    "piecewise spacing (DESIGN.md 4.15); compare with --backdrop, whose far content no scene box holds")
    ap.add_argument("--near-plane", type=float, default=0.05, help="with --unbounded: the collider's near plane in training (the reference model's default)")
    ap.add_argument("--far-plane", type=float, default=1000.0, help="with --unbounded: the collider's far plane")
    ap.add_argument("--backdrop", action="store_true", help="synthetic.shade(backdrop=True): a sky gradient, bare ground and a far stand at several scene "
                    "radii where a ray leaves the pitch scene")
    ap.add_argument("--static-scene", action="store_true", help="a 3-coordinate model (three planes per scale, no time axis) on the empty scene")
    # a value such as -0.25,0.08,... starts with '-' and is no plain number, so argparse would read it as an option: hand it over as --lens=VALUE
    argv = sys.argv[1:]
    for i in range(len(argv) - 1):
        if argv[i] == "--lens":
            argv[i:i + 2] = ["--lens=" + argv[i + 1]]
            break
    ap.add_argument("--lens", default="", help="k1,k2,k3,k4,p1,p2 (`--lens -0.25,0.08,-0.01,0,0.001,0.0005` or `--lens=...`): every training and held-out camera shoots the scene through this OpenCV lens, and "
                    "training and evaluation generate their rays through it (snerf_raygen_lens)")
    ap.add_argument("--ignore-lens", action="store_true", help="with --lens: the dataset is still shot through the lens, but training and evaluation use "
                    "pinhole rays -- what this package did before it generated rays through the distortion")
    ap.add_argument("--overlay", default="", help="Y0,Y1,X0,X1: every TRAINING image carries a broadcast banner in rows [Y0,Y1), columns [X0,X1) "
                    "(synthetic.add_broadcast_overlay: constant colour + a stripe that moves with the frame time); the held-out views stay clean")
    ap.add_argument("--use-masks", action="store_true", help="with --overlay: draw the training pixels inside the banner's mask (snerf_sample_pixels_masked)")
    ap.add_argument("--mask-ist", action="store_true", help="with --use-masks: DynamicBasedPixelSampler(mask_ist_weights=True), the IST maps are zeroed outside the mask")
    ap.add_argument("--pose-noise", default="", help="POS_STD,ROT_STD: the TRAINING camera table is perturbed on the host with a seeded SE(3) perturbation, one per "
                    "physical camera (scene units, radians); the dataset is shot with the exact cameras and the held-out cameras stay exact")
    ap.add_argument("--pose-noise-seed", type=int, default=7)
    ap.add_argument("--optimize-cameras", action="store_true", help="CameraOptimizer (SO3xR3, Adam lr 6e-4, eps 1e-15) on the training cameras: "
                    "KPlanesTrainConfig(ray_gradients=True), snerf_pose_apply / snerf_raygen_pose_bwd (DESIGN.md 4.13)")
    ap.add_argument("--share-poses-per-camera", action="store_true", help="with --optimize-cameras: one pose adjustment per physical camera "
                    "(dataparsers.camera_pose_groups) instead of the reference's one per image")
    args = ap.parse_args(argv)
    if args.share_poses_per_camera and not args.optimize_cameras:
        ap.error("--share-poses-per-camera needs --optimize-cameras")
    if args.optimize_cameras and (args.standin or args.view_dependent):
        ap.error("--optimize-cameras runs on the HIP trainer with disable_viewing_dependent=True")
    if args.unbounded and args.standin:
        ap.error("--unbounded runs on the HIP trainer (the stock-PyTorch stand-in is the bounded model)")
    if args.use_masks and not args.overlay:
        ap.error("--use-masks needs --overlay")
    if args.mask_ist and not args.use_masks:
        ap.error("--mask-ist needs --use-masks")
    if (args.static_pretrain or args.static_scene) and (args.standin or args.optimize_cameras):
        ap.error("--static-pretrain / --static-scene run on the HIP trainer without the camera optimiser")
    if args.static_pretrain and args.static_scene:
        ap.error("--static-pretrain prepares a dynamic model; a --static-scene model has no second stage")
    dev = torch.device("cuda:0")
    cams = synthetic.make_cameras(20, 960, 540)
    novel_cams = synthetic.make_novel_cameras(3, 960, 540)
    if args.lens:
        row = [float(v) for v in args.lens.split(",")]
        if len(row) != 6:
            ap.error("--lens takes six numbers: k1,k2,k3,k4,p1,p2")
        cams["distortion"], novel_cams["distortion"] = torch.tensor(row), torch.tensor(row)
    elif args.ignore_lens:
        ap.error("--ignore-lens needs --lens")
    times = synthetic.frame_times(100, 3)
    dyn = not args.static_scene
    train = synthetic.render_dataset(cams, times, list(range(19)), dev, chunk_rows=540, variant=args.scene, dynamic=dyn, backdrop=args.backdrop)
    held = synthetic.render_dataset(cams, times, [19], dev, chunk_rows=540, variant=args.scene, dynamic=dyn, backdrop=args.backdrop)
    novel = synthetic.render_dataset(novel_cams, times, [0, 1, 2], dev, chunk_rows=540, variant=args.scene, dynamic=dyn, backdrop=args.backdrop)
    if args.static_pretrain:  # the reference's "empty" directory: the training cameras' view of the scene without players and ball
        train["empty"] = synthetic.render_dataset(cams, times[:1], list(range(19)), dev, chunk_rows=540, variant=args.scene, dynamic=False, backdrop=args.backdrop)
    if args.overlay:
        box = [int(v) for v in args.overlay.split(",")]
        if len(box) != 4:
            ap.error("--overlay takes four numbers: Y0,Y1,X0,X1")
        train["mask"] = synthetic.add_broadcast_overlay(train, box)
    if args.pose_noise:
        std = [float(v) for v in args.pose_noise.split(",")]
        if len(std) != 2:
            ap.error("--pose-noise takes two numbers: POS_STD,ROT_STD")
        train["c2w_true"] = train["c2w"]
        train["c2w"] = perturb_poses(train["c2w"], train["cam_id"], std[0], std[1], args.pose_noise_seed)
    for data in (train, held, novel):  # the rows the rays of training and evaluation go through: the dataset's own, or none with --ignore-lens
        data["ray_distortion"] = None if args.ignore_lens else data.get("distortion")
    t0 = time.time()
    ist = compute_ist(train["images"], train["cam_id"], train["times"], ist_range=1.0)  # method_configs.py:503
    torch.cuda.synchronize()
    pick = lambda data: (list(range(data["images"].shape[0])) if not args.eval_frames else
                         [c * len(times) + int(f) for c in range(data["images"].shape[0] // len(times))
                          for f in torch.linspace(0, len(times) - 1, args.eval_frames).long().tolist()])
    sets = {"camera_20": (held, pick(held)), "novel": (novel, pick(novel)),
            "train": (train, torch.linspace(0, train["images"].shape[0] - 1, 4).long().tolist())}
    log = {"config": "k-planes preset, synthetic Broadcast-style (19 train cams x 33 frames 960x540)", "steps": args.steps, "scene": args.scene,
           "lens": args.lens or None, "ignore_lens": args.ignore_lens, "overlay": args.overlay or None, "use_masks": args.use_masks, "mask_ist": args.mask_ist, "eval_frames": args.eval_frames or "all",
           "trainer": ("oracle/torch_standin.StandinTrainer: the reference's algorithm in stock PyTorch-ROCm, fp32"
                       + (", planes stored channel-last and gathered as rows (index_select) instead of F.grid_sample" if args.standin_layout == "hwc" else ", F.grid_sample per plane"))
           if args.standin else "soccernerfs_amd KPlanesTrainer (HIP)",
           "oracle_init": bool(args.oracle_init or args.standin),
           "mlp_operands": args.mlp_operands, "gvec_dtype": args.gvec_dtype, "per_net_operands": [args.sigma_operands, args.color_operands, args.proposal_operands],
           "deterministic": args.deterministic, "view_dependent": args.view_dependent, "nonfinite_policy": args.nonfinite_policy,
           "emulate_transports": args.emulate_transports, "time_sorted_rays": args.time_sorted_rays, "fused_field": not args.no_fused_field, "quotient_scatter": not args.no_quotient_scatter,
           "quotient_epilogue": not args.no_quotient_epilogue, "fused_proposal": not args.no_fused_proposal,
           "pose_noise": args.pose_noise or None, "pose_noise_seed": args.pose_noise_seed if args.pose_noise else None,
           "optimize_cameras": args.optimize_cameras, "share_poses_per_camera": args.share_poses_per_camera,
           "static_pretrain_steps": args.static_pretrain, "static_scene": args.static_scene,
           "eval_sets": {"camera_20": "20th arc camera (reference 'all' split eval camera; extrapolated view), %d frames" % len(sets["camera_20"][1]),
                         "novel": "3 evaluation-only cameras between training cameras (interpolated views), %d images" % len(sets["novel"][1]),
                         "train": "4 training images"},
           "ist_precompute_s": time.time() - t0, "ist_nonzero_fraction": float((ist > 0).float().mean()), "runs": []}
    for seed in [int(s) for s in args.seeds.split(",")]:
        log["runs"].append(run_one(args, seed, train, sets, ist, dev))
        final = [r["evals"][-1] for r in log["runs"]]
        log["summary"] = {name: stats([f[name]["psnr_mean"] for f in final]) for name in sets}
        log["summary"]["novel_ssim"] = stats([f["novel"]["ssim_mean"] for f in final])
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(log, open(args.out, "w"), indent=1)
    print(json.dumps(log["summary"]))


if __name__ == "__main__":
    main()

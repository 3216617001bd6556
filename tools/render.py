#!/usr/bin/env python3
"""Render a camera path from a checkpoint: the `ns-render --traj filename --camera-path-filename ... --output-format images` counterpart
(scripts/render.py of the reference) on the fused K-Planes trainer or, with --method nerfplayer-nerfacto, on the fused NeRFPlayer-nerfacto trainer.

    python tools/render.py --load-dir outputs/ckpts --camera-path-filename camera_path.json --output-path renders/run1
    python tools/render.py --method nerfplayer-nerfacto --load-dir outputs/ckpts --camera-path-filename camera_path.json --output-path renders/run2

Builds a KPlanesTrainConfig (the k-planes preset unless overridden on the command line -- the checkpoint holds parameters, not the model
configuration, so the overrides must describe the model that was trained), loads the newest `step-*.ckpt` of --load-dir (or --load-step) with
KPlanesTrainer.load_checkpoint and writes one `%05d.png` (or `.npy`) per camera of the path into --output-path.  The path's "camera_type"
may be "perspective", "fisheye" or "equirectangular" (a 360-degree frame: fx = W / 2, fy = H, as the viewer exports it).  Video files are not
written: no encoder is assumed.

--method nerfplayer-nerfacto: --set names fields of NerfplayerNerfactoModelConfig (the nerfplayer-nerfacto preset unless overridden), the size of
the appearance table is read from the checkpoint's embedding, --aabb-scale gives the scene box, and the frames come from NerfplayerRenderer
(--background-color, --no-fused-density); the K-Planes-only switches are refused."""
import argparse
import ast
import dataclasses
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import checkpoint as CK  # noqa: E402
from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModelConfig  # noqa: E402
from soccernerfs_amd.nerfplayer_trainer import NerfplayerTrainer  # noqa: E402
from soccernerfs_amd.render import KPlanesRenderer, NerfplayerRenderer  # noqa: E402
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer  # noqa: E402

METHODS = {"k-planes": KPlanesTrainConfig, "nerfplayer-nerfacto": NerfplayerNerfactoModelConfig}


def config_from_overrides(pairs, method: str = "k-planes"):
    """`name=value` strings -> the method's configuration (KPlanesTrainConfig / NerfplayerNerfactoModelConfig); values are Python literals
    (`multiscale_res=(1,2,4)`), bare words stay strings."""
    cls = METHODS[method]
    fields = {f.name for f in dataclasses.fields(cls)}
    kw = {}
    for pair in pairs:
        name, sep, value = pair.partition("=")
        if not sep or name not in fields:
            raise SystemExit(f"--set {pair!r}: expected name=value with name a {cls.__name__} field")
        try:
            kw[name] = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            kw[name] = value
    return cls(**kw)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--method", default="k-planes", choices=sorted(METHODS), help="the model the checkpoint holds")
    ap.add_argument("--load-dir", required=True, help="directory holding step-*.ckpt (nerfstudio checkpoint format)")
    ap.add_argument("--load-step", type=int, default=None, help="checkpoint step (default: the newest)")
    ap.add_argument("--camera-path-filename", required=True, help="camera-path JSON as the viewer exports it")
    ap.add_argument("--output-path", default="renders/output", help="directory the frames are written to")
    ap.add_argument("--rendered-output-names", nargs="+", default=["rgb"], help="rgb, accumulation, depth; several are concatenated along the width")
    ap.add_argument("--output-format", default="png", choices=["png", "npy"])
    ap.add_argument("--eval-num-rays-per-chunk", type=int, default=None, help="default: 65536 (k-planes), 32768 (nerfplayer-nerfacto: the preset's)")
    ap.add_argument("--transmittance-cutoff", type=float, default=0.0, help="> 0: early ray termination (an approximation bounded by the cutoff)")
    ap.add_argument("--fused-tail", action="store_true", help="field forward + weights + compositing as ONE kernel (same bits; measured slower, DESIGN 4.9)")
    ap.add_argument("--default-time", type=float, default=None, help="time of every frame when the path carries no render_time")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="override of a field of the method's configuration, repeatable")
    ap.add_argument("--aabb-scale", type=float, default=1.0, help="nerfplayer-nerfacto: half the edge of the scene box the model was trained in")
    ap.add_argument("--mlp-operands", default="fp32", choices=["fp32", "bf16"], help="nerfplayer-nerfacto: NerfplayerTrainer(mlp_operands=...)")
    ap.add_argument("--background-color", default="black", choices=["black", "white", "last_sample"], help="nerfplayer-nerfacto: what shows behind the model")
    ap.add_argument("--no-fused-density", action="store_true", help="nerfplayer-nerfacto: the proposal density as snerf_tgrid_encode_fwd + snerf_mlp_fwd instead of "
                    "the one kernel snerf_tgrid_density_fwd (same bits; measured slower, DESIGN 4.16)")
    ap.add_argument("--freeze-time-planes", action="store_true", help="the checkpoint is a static pre-training stage (KPlanesTrainConfig.freeze_time_planes): "
                    "render from the space planes alone; the path needs no render_time and --default-time is ignored")
    ap.add_argument("--unbounded", action="store_true", help="the checkpoint is an unbounded scene (KPlanesTrainConfig.bounded=False): contracted "
                    "coordinates, near / far collider (near 0 at evaluation) and piecewise spacing; the checkpoint does not record this")
    ap.add_argument("--far-plane", type=float, default=None, help="with --unbounded: the far plane the model was trained with (default: the config's 1000)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.far_plane is not None and not args.unbounded:
        ap.error("--far-plane needs --unbounded")
    if args.method != "k-planes" and (args.transmittance_cutoff or args.fused_tail or args.freeze_time_planes or args.unbounded):
        ap.error("--transmittance-cutoff, --fused-tail, --freeze-time-planes and --unbounded belong to --method k-planes")
    if args.eval_num_rays_per_chunk is None:
        args.eval_num_rays_per_chunk = 65536 if args.method == "k-planes" else 32768
    return args


def config_from_args(args) -> KPlanesTrainConfig:
    """The trainer configuration a command line stands for: --set pairs, then the switches that name a config field of their own."""
    unbounded = (["bounded=False"] + ([f"far_plane={args.far_plane}"] if args.far_plane is not None else [])) if args.unbounded else []
    return config_from_overrides(args.set + (["freeze_time_planes=True"] if args.freeze_time_planes else []) + unbounded)


def nerfplayer_from_checkpoint(args):
    """-> (NerfplayerTrainer holding the checkpoint, the step it resumes at).  The appearance table's size is not part of the configuration: it is
    the number of training images, read from the checkpoint's `field.embedding_appearance.embedding.weight`."""
    step = args.load_step
    if step is None:
        steps = sorted(int(f[len("step-"):-len(".ckpt")]) for f in os.listdir(args.load_dir) if f.startswith("step-") and f.endswith(".ckpt"))
        if not steps:
            raise SystemExit(f"no step-*.ckpt in {args.load_dir}")
        step = steps[-1]
    pipeline = torch.load(CK.checkpoint_path(args.load_dir, step), map_location="cpu", weights_only=False)["pipeline"]
    num_images = pipeline["_model.field.embedding_appearance.embedding.weight"].shape[0]
    trainer = NerfplayerTrainer(config_from_overrides(args.set, args.method), 4096, num_images, aabb_scale=args.aabb_scale, device=args.device,
                                mlp_operands=args.mlp_operands)
    return trainer, trainer.load_checkpoint(args.load_dir, step)


def main(argv=None):
    args = parse_args(argv)
    if args.method == "nerfplayer-nerfacto":
        trainer, step = nerfplayer_from_checkpoint(args)
        renderer = NerfplayerRenderer(trainer, rays_per_chunk=args.eval_num_rays_per_chunk, background_color=args.background_color,
                                      fused_density=not args.no_fused_density)
        t0 = time.time()
        files = renderer.render_camera_path(args.camera_path_filename, args.output_path, outputs=tuple(args.rendered_output_names),
                                            format=args.output_format, default_time=args.default_time)
        torch.cuda.synchronize()
        dt = time.time() - t0
        print(f"checkpoint resumes at step {step}; {len(files)} frames -> {args.output_path} in {dt:.2f} s ({len(files) / max(dt, 1e-9):.2f} frames/s, "
              f"fused density {'on' if any(renderer.fused_density) else 'off'})")
        return
    cfg = config_from_args(args)
    trainer = KPlanesTrainer(cfg, 4096, args.device)
    step = trainer.load_checkpoint(args.load_dir, args.load_step)
    renderer = KPlanesRenderer(trainer, rays_per_chunk=args.eval_num_rays_per_chunk, transmittance_cutoff=args.transmittance_cutoff,
                               fused_tail=args.fused_tail)
    t0 = time.time()
    files = renderer.render_camera_path(args.camera_path_filename, args.output_path, outputs=tuple(args.rendered_output_names),
                                        format=args.output_format, default_time=args.default_time)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"checkpoint resumes at step {step}; {len(files)} frames -> {args.output_path} in {dt:.2f} s ({len(files) / max(dt, 1e-9):.2f} frames/s, "
          f"fused tail {'on' if renderer.fused_tail else 'off'})")


if __name__ == "__main__":
    main()

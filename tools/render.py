#!/usr/bin/env python3
"""Render a camera path from a checkpoint: the `ns-render --traj filename --camera-path-filename ... --output-format images` counterpart
(scripts/render.py of the reference) on the fused K-Planes trainer.

    python tools/render.py --load-dir outputs/ckpts --camera-path-filename camera_path.json --output-path renders/run1

Builds a KPlanesTrainConfig (the k-planes preset unless overridden on the command line -- the checkpoint holds parameters, not the model
configuration, so the overrides must describe the model that was trained), loads the newest `step-*.ckpt` of --load-dir (or --load-step) with
KPlanesTrainer.load_checkpoint and writes one `%05d.png` (or `.npy`) per camera of the path into --output-path.  The path's "camera_type"
may be "perspective", "fisheye" or "equirectangular" (a 360-degree frame: fx = W / 2, fy = H, as the viewer exports it).  Video files are not
written: no encoder is assumed."""
import argparse
import ast
import dataclasses
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd.render import KPlanesRenderer  # noqa: E402
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer  # noqa: E402


def config_from_overrides(pairs) -> KPlanesTrainConfig:
    """`name=value` strings -> KPlanesTrainConfig; values are Python literals (`multiscale_res=(1,2,4)`), bare words stay strings."""
    fields = {f.name for f in dataclasses.fields(KPlanesTrainConfig)}
    kw = {}
    for pair in pairs:
        name, sep, value = pair.partition("=")
        if not sep or name not in fields:
            raise SystemExit(f"--set {pair!r}: expected name=value with name a KPlanesTrainConfig field")
        try:
            kw[name] = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            kw[name] = value
    return KPlanesTrainConfig(**kw)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--load-dir", required=True, help="directory holding step-*.ckpt (nerfstudio checkpoint format)")
    ap.add_argument("--load-step", type=int, default=None, help="checkpoint step (default: the newest)")
    ap.add_argument("--camera-path-filename", required=True, help="camera-path JSON as the viewer exports it")
    ap.add_argument("--output-path", default="renders/output", help="directory the frames are written to")
    ap.add_argument("--rendered-output-names", nargs="+", default=["rgb"], help="rgb, accumulation, depth; several are concatenated along the width")
    ap.add_argument("--output-format", default="png", choices=["png", "npy"])
    ap.add_argument("--eval-num-rays-per-chunk", type=int, default=65536)
    ap.add_argument("--transmittance-cutoff", type=float, default=0.0, help="> 0: early ray termination (an approximation bounded by the cutoff)")
    ap.add_argument("--fused-tail", action="store_true", help="field forward + weights + compositing as ONE kernel (same bits; measured slower, DESIGN 4.9)")
    ap.add_argument("--default-time", type=float, default=None, help="time of every frame when the path carries no render_time")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="KPlanesTrainConfig override, repeatable")
    ap.add_argument("--freeze-time-planes", action="store_true", help="the checkpoint is a static pre-training stage (KPlanesTrainConfig.freeze_time_planes): "
                    "render from the space planes alone; the path needs no render_time and --default-time is ignored")
    ap.add_argument("--unbounded", action="store_true", help="the checkpoint is an unbounded scene (KPlanesTrainConfig.bounded=False): contracted "
                    "coordinates, near / far collider (near 0 at evaluation) and piecewise spacing; the checkpoint does not record this")
    ap.add_argument("--far-plane", type=float, default=None, help="with --unbounded: the far plane the model was trained with (default: the config's 1000)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.far_plane is not None and not args.unbounded:
        ap.error("--far-plane needs --unbounded")
    return args


def config_from_args(args) -> KPlanesTrainConfig:
    """The trainer configuration a command line stands for: --set pairs, then the switches that name a config field of their own."""
    unbounded = (["bounded=False"] + ([f"far_plane={args.far_plane}"] if args.far_plane is not None else [])) if args.unbounded else []
    return config_from_overrides(args.set + (["freeze_time_planes=True"] if args.freeze_time_planes else []) + unbounded)


def main(argv=None):
    args = parse_args(argv)
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

#!/usr/bin/env python3
"""Full-frame render throughput of the trained k-planes preset: the parent's eval loop against KPlanesRenderer.

One process, profiler off.  The preset model at full size (bf16 operands) is trained on the default synthetic scene for --train-steps steps
first (an untrained field is a fog: every ray walks all its samples), then 960 x 540 frames of the evaluation-only novel cameras are
rendered by five arms, alternating inside each of --rounds rounds:

  A  tools/train_psnr.py::eval_set: int64 index table, ops.generate_rays, KPlanesTrainer.forward(training=False) in 4096-ray slices
     (as eval_set does, it also forms each frame's MSE against the ground truth and reads it back: one host synchronise per frame)
  B  KPlanesRenderer, 65536-ray chunks, unfused tail (field_fwd + weights_fwd + render_fwd)
  C  KPlanesRenderer, fused tail (snerf_kplanes_field_render), cutoff 0
  D  fused tail, transmittance_cutoff 1e-3        E  fused tail, transmittance_cutoff 1e-2

Reported per arm: ms / frame and frames / s (median over the rounds, min and max as the spread), libsnerf launches per frame counted on the
host; the render-tail kernels alone by HIP events (the new kernel against field_fwd + weights + render); for D / E the share of 32-sample
tiles skipped (from samples_done), the PSNR of the frame against arm C's and the PSNR against ground truth beside arm C's.

    python tools/bench_render.py --out profiles/r09_render_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soccernerfs_amd import _lib, fused_step, ops, synthetic  # noqa: E402
from soccernerfs_amd.cameras import Cameras  # noqa: E402
from soccernerfs_amd.metrics import psnr  # noqa: E402
from soccernerfs_amd.render import KPlanesRenderer  # noqa: E402
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer  # noqa: E402
from tools.train_psnr import eval_set  # noqa: E402


class LaunchCounter:
    """Counts the libsnerf calls whose return code goes through _lib.check (every launch of the trainer and of ops does)."""

    def __enter__(self):
        self.n = 0
        self._check, self._ck = _lib.check, fused_step.FusedStep.__dict__["_ck"]

        def counting(rc, what=""):
            self.n += 1
            return self._check(rc, what)

        _lib.check = counting
        fused_step.FusedStep._ck = staticmethod(counting)
        return self

    def __exit__(self, *exc):
        _lib.check = self._check
        fused_step.FusedStep._ck = self._ck


def main_nerfplayer(args):
    """--method nerfplayer-nerfacto: 960 x 540 frames of the config-4 shape (the nerfplayer-nerfacto preset, R = 4096, stadium-scene cameras) through
      i    tools/train_psnr_nerfplayer.py::eval_psnr: index table, ops.generate_rays, NerfplayerTrainer.forward(training=False) in 4096-ray slices
           (whole slices only; one host read-back per frame for its PSNR)
      ii   NerfplayerRenderer, 32768-ray chunks, proposal density = snerf_tgrid_encode_fwd + snerf_mlp_fwd
      iii  NerfplayerRenderer, proposal density = snerf_tgrid_density_fwd
    alternating inside each round, and snerf_tgrid_density_fwd alone against the pair at N = 32768 x 256 and 32768 x 96 by HIP events."""
    import ctypes as C

    from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModelConfig
    from soccernerfs_amd.nerfplayer_trainer import NerfplayerTrainer
    from soccernerfs_amd.render import NerfplayerRenderer
    from tools.train_psnr_nerfplayer import eval_psnr

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    R, Wd, Hd = 4096, 960, 540
    cams = synthetic.make_stadium_cameras(30, 6, Wd, Hd)
    frame_ids = torch.linspace(0, 99, 8).long()
    data = synthetic.render_dataset(cams, frame_ids.float() / 99, list(range(30)), dev, chunk_rows=Hd, variant="stadium")
    held = synthetic.render_dataset(cams, frame_ids.float()[:1] / 99 + 0.37, list(range(30, 36)), dev, chunk_rows=Hd, variant="stadium")
    M, H, W = data["images"].shape[:3]
    tr = NerfplayerTrainer(NerfplayerNerfactoModelConfig(), R, M, aabb_scale=1.0, device=dev, mlp_operands=args.mlp_operands, async_field_sweep=True,
                           tiled_field_backward=True)
    state = "initialised (NerfplayerTrainer's own initialisation, no training)"
    if args.load_dir:
        tr.load_checkpoint(args.load_dir)
        state = f"loaded from a checkpoint, resumes at step {tr.step}"
    elif args.train_steps:
        for _ in range(args.train_steps):
            idx, target = ops.sample_pixels_uniform(torch.rand(R, 3, device=dev), M, H, W, data["images"])
            rays = ops.generate_rays(idx, data["fx"], data["fy"], data["cx"], data["cy"], data["c2w"], data["times"])
            tr.train_step(rays, idx[:, 0].contiguous(), target)
        state = f"trained {args.train_steps} steps here on the synthetic stadium scene (no checkpoint at hand)"
    tr.synchronize()
    n_frames = min(args.frames, held["images"].shape[0])
    frames = list(range(n_frames))
    hcams = Cameras(held["c2w"], held["fx"], held["fy"], held["cx"], held["cy"], W, H, held["times"])
    rn = {"ii": NerfplayerRenderer(tr, 32768, fused_density=False), "iii": NerfplayerRenderer(tr, 32768, fused_density=True)}
    assert rn["iii"].fused_density == [True, True] and rn["ii"].fused_density == [False, False]
    anneal = rn["ii"].default_anneal()
    few = {k: v[:n_frames] if isinstance(v, torch.Tensor) and v.shape[0] == held["images"].shape[0] else v for k, v in held.items()}
    arms = {"i": lambda: eval_psnr(tr, few, n_frames, anneal), "ii": lambda: [rn["ii"].render_frame(hcams, m, anneal=anneal)["rgb"] for m in frames],
            "iii": lambda: [rn["iii"].render_frame(hcams, m, anneal=anneal)["rgb"] for m in frames]}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t1) * 1e3 / n_frames)
    launches = {}
    with LaunchCounter() as lc:
        eval_psnr(tr, {k: v[:1] if isinstance(v, torch.Tensor) and v.shape[0] == held["images"].shape[0] else v for k, v in held.items()}, 1, anneal)
        launches["i"] = lc.n
    for k, r in rn.items():
        n0 = r.launches
        r.render_frame(hcams, 0, anneal=anneal)
        launches[k] = r.launches - n0
    same_bits = all(torch.equal(a, b) for a, b in zip(arms["ii"](), arms["iii"]()))
    groups = {}
    for k, r in rn.items():
        r.enable_kernel_timing()
        for m in frames:
            r.render_frame(hcams, m, anneal=anneal)
        kt = r.kernel_times_ms()
        r.disable_kernel_timing()
        groups[k] = {name: round(v[0] * v[1] / n_frames, 3) for name, v in sorted(kt.items())}

    # the kernel alone against the pair: a full 32768-ray chunk of the last frame's rays and bins, level by level
    r3, kernel = rn["iii"], {}
    o, d, t = (r3._rays[q] for q in ("origins", "directions", "times"))
    for lvl, S in enumerate(tr.S[:2]):
        enc, net, N = tr.prop_enc[lvl], tr.prop_mlp[lvl], 32768 * tr.S[lvl]
        co = ops.coords_from_rays(o, d, t, r3.buf["eb"][lvl], tr.aabb, False)
        dens_f, dens_p = torch.empty(N, device=dev), torch.empty(N, device=dev)
        feat, raw = torch.empty(N, enc.output_dim, device=dev), torch.empty(N, 1, device=dev)
        st, p = ops._stream(), ops._ptr

        def fused():
            _lib.call("tgrid_density_fwd", C.byref(enc.desc), p(enc.embeddings), C.byref(co), p(t), S, N, C.byref(net.desc), p(net.params), p(dens_f), st)

        def pair():
            _lib.call("tgrid_encode_fwd", C.byref(enc.desc), p(enc.embeddings), C.byref(co), None, p(t), S, N, p(feat), st)
            _lib.call("mlp_fwd", C.byref(net.desc), p(net.params), p(feat), enc.output_dim, N, p(raw), 1, 0, p(dens_p), st)

        times = {"fused": [], "pair": []}
        for rep in range(2 + 3 * args.rounds):
            for name, fn in (("fused", fused), ("pair", pair)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append(a.elapsed_time(b))
        kernel[f"N=32768x{S}"] = {"fused_ms": {"median": statistics.median(times["fused"]), "min": min(times["fused"]), "max": max(times["fused"])},
                                  "pair_ms": {"median": statistics.median(times["pair"]), "min": min(times["pair"]), "max": max(times["pair"])},
                                  "bit_identical": bool(torch.equal(dens_f, dens_p))}

    stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": [round(x, 3) for x in xs]}
    names = {"i": "eval_psnr: index table + trainer.forward(training=False) in 4096-ray slices (126 whole slices of the 126.6)",
             "ii": "renderer, 32768-ray chunks, tgrid_encode_fwd + mlp_fwd per proposal level", "iii": "renderer, 32768-ray chunks, tgrid_density_fwd"}
    res = {"what": f"960x540 frames of the stadium scene's evaluation cameras, nerfplayer-nerfacto preset ({args.mlp_operands} operands), R = 4096", "state": state,
           "device": torch.cuda.get_device_name(0), "frames_per_arm_and_round": n_frames, "rounds": args.rounds, "anneal": anneal, "arms": {},
           "arm_ii_and_iii_frames_bit_identical": same_bits, "kernel_groups_ms_per_frame_hip_events": groups, "density_kernel_alone": kernel,
           "launch_count_note": "libsnerf launches per frame; arm i also issues ATen kernels per slice (the appearance mean, the random background, copies)"}
    for k in arms:
        s = stat(ms[k])
        res["arms"][k] = {"arm": names[k], "ms_per_frame": s, "spread_ms": s["max"] - s["min"], "launches_per_frame": launches[k]}
    ii, iii = res["arms"]["ii"]["ms_per_frame"], res["arms"]["iii"]["ms_per_frame"]
    spread = max(ii["max"] - ii["min"], iii["max"] - iii["min"])
    res["fused_density_default"] = {"iii_beats_ii_by_more_than_the_spread": bool(ii["median"] - iii["median"] > spread), "gain_ms": ii["median"] - iii["median"],
                                    "spread_ms": spread}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {"ms_per_frame": round(v["ms_per_frame"]["median"], 2), "spread_ms": round(v["spread_ms"], 2), "launches": v["launches_per_frame"]}
                      for k, v in res["arms"].items()}))
    print(json.dumps({"kernel": kernel, "fused_density_default": res["fused_density_default"], "bit_identical_ii_iii": same_bits, "state": state}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="k-planes", choices=["k-planes", "nerfplayer-nerfacto"])
    ap.add_argument("--train-steps", type=int, default=None, help="default: 5000 (k-planes), 0 (nerfplayer-nerfacto)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6, help="frames per arm and round (novel cameras x times)")
    ap.add_argument("--out", default=None, help="default: profiles/r09_render_bench.json (k-planes), profiles/r29_nerfplayer_render_bench.json")
    ap.add_argument("--load-dir", default=None, help="nerfplayer-nerfacto: a checkpoint directory of the preset trained on the stadium scene (30 x 8 images)")
    ap.add_argument("--mlp-operands", default="bf16", choices=["fp32", "bf16"], help="nerfplayer-nerfacto: NerfplayerTrainer(mlp_operands=...)")
    args = ap.parse_args()
    if args.method == "nerfplayer-nerfacto":
        args.train_steps = 0 if args.train_steps is None else args.train_steps
        args.out = args.out or "profiles/r29_nerfplayer_render_bench.json"
        return main_nerfplayer(args)
    args.train_steps = 5000 if args.train_steps is None else args.train_steps
    args.out = args.out or "profiles/r09_render_bench.json"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = KPlanesTrainConfig(seed=0)
    R = 4096
    trainer = KPlanesTrainer(cfg, R, dev)
    cams = synthetic.make_cameras(20, 960, 540)
    times = synthetic.frame_times(100, 3)
    data = synthetic.render_dataset(cams, times, list(range(19)), dev, chunk_rows=540)
    images = data["images"]
    M, H, W = images.shape[:3]
    n_times = max(1, (args.frames + 2) // 3)
    novel = synthetic.render_dataset(synthetic.make_novel_cameras(3, 960, 540), times[torch.linspace(0, len(times) - 1, n_times).long()], [0, 1, 2], dev,
                                     chunk_rows=540)
    frame_ids = list(range(novel["images"].shape[0]))[:args.frames]
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.train_steps):
        idx, target = ops.sample_pixels_uniform(torch.rand(R, 3, device=dev), M, H, W, images)
        rays = ops.generate_rays(idx, data["fx"], data["fy"], data["cx"], data["cy"], data["c2w"], data["times"], aabb=trainer.aabb,
                                 near_plane=cfg.near_plane, training=True)
        trainer.train_step(rays, target)
    trainer.synchronize()
    train_s = time.time() - t0
    ld = {k: float(v) for k, v in trainer.loss_dict().items()}
    print(f"trained {args.train_steps} steps in {train_s:.1f} s, rgb_loss {ld['rgb_loss']:.5f}", flush=True)

    ncams = Cameras(novel["c2w"], novel["fx"], novel["fy"], novel["cx"], novel["cy"], W, H, novel["times"])
    gt = lambda m: novel["images"][m].float() / 255.0
    renderers = {"B": KPlanesRenderer(trainer, 65536, fused_tail=False), "C": KPlanesRenderer(trainer, 65536, fused_tail=True),
                 "D": KPlanesRenderer(trainer, 65536, transmittance_cutoff=1e-3), "E": KPlanesRenderer(trainer, 65536, transmittance_cutoff=1e-2)}
    assert not renderers["B"].fused_tail and all(renderers[k].fused_tail for k in "CDE")
    anneal = renderers["C"].default_anneal()

    def arm_a():
        return eval_set(trainer, novel, frame_ids, anneal, with_ssim=False)[0]

    def arm_r(name):
        return [renderers[name].render_frame(ncams, m, anneal=anneal)["rgb"] for m in frame_ids]

    arms = {"A": arm_a, **{k: (lambda k=k: arm_r(k)) for k in "BCDE"}}
    for fn in arms.values():  # warm-up: allocator, code objects, the renderers' host camera table
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t1) * 1e3 / len(frame_ids))

    # launches per frame, counted on the host (outside the timed rounds)
    launches = {}
    with LaunchCounter() as lc:
        eval_set(trainer, novel, frame_ids[:1], anneal, with_ssim=False)
        launches["A"] = lc.n
    for k, rn in renderers.items():
        n0 = rn.launches
        rn.render_frame(ncams, frame_ids[0], anneal=anneal)
        launches[k] = rn.launches - n0

    # the render tail alone (HIP events around the launches, summed over a frame's chunks)
    tail = {}
    for k in ("B", "C", "D", "E"):
        rn = renderers[k]
        rn.enable_kernel_timing()
        for m in frame_ids:
            rn.render_frame(ncams, m, anneal=anneal)
        kt = rn.kernel_times_ms()
        rn.disable_kernel_timing()
        per_frame = lambda name: kt[name][0] * kt[name][1] / len(frame_ids) if name in kt else 0.0
        tail[k] = ({"field_fwd_ms": per_frame("kplanes_field_fwd"), "weights_render_ms": per_frame("weights_render_fwd"),
                    "tail_ms": per_frame("kplanes_field_fwd") + per_frame("weights_render_fwd")} if k == "B" else {"tail_ms": per_frame("kplanes_field_render")})
        tail[k]["proposal_levels_ms"] = per_frame("kplanes_density_fwd") + per_frame("pdf_resample")

    # quality and the share of tiles skipped
    S2 = trainer.S[2]
    quality = {}
    exact = {m: renderers["C"].render_frame(ncams, m, anneal=anneal)["rgb"].clone() for m in frame_ids}
    same_bits = all(torch.equal(renderers["B"].render_frame(ncams, m, anneal=anneal)["rgb"], exact[m]) for m in frame_ids)
    psnr_gt_a = arm_a()
    for k in ("C", "D", "E"):
        rn = renderers[k]
        rn.record_samples_done = True
        p_c, p_gt, skipped = [], [], []
        for m in frame_ids:
            rgb = rn.render_frame(ncams, m, anneal=anneal)["rgb"]
            mse = float(torch.mean((rgb - exact[m]) ** 2))
            p_c.append(float("inf") if mse == 0.0 else float(psnr(rgb, exact[m])))
            p_gt.append(float(psnr(rgb, gt(m))))
            skipped.append(1.0 - float(rn.samples_done.float().mean()) / S2)
        rn.record_samples_done = False
        quality[k] = {"psnr_vs_arm_C_db_min": None if min(p_c) == float("inf") else min(p_c),  # None: the frames are the same bits
                      "psnr_vs_ground_truth_db_mean": sum(p_gt) / len(p_gt), "tiles_skipped_share_mean": sum(skipped) / len(skipped),
                      "tiles_skipped_share_per_frame": [round(s, 4) for s in skipped]}

    stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": [round(x, 3) for x in xs]}
    res = {"what": "960x540 frames of the novel cameras, k-planes preset (bf16 operands), trained %d steps on the default synthetic scene" % args.train_steps,
           "device": torch.cuda.get_device_name(0), "frames_per_arm_and_round": len(frame_ids), "rounds": args.rounds, "train_seconds": train_s,
           "train_rgb_loss": ld["rgb_loss"], "anneal": anneal, "arms": {}, "arm_B_and_C_frames_bit_identical": same_bits,
           "psnr_vs_ground_truth_db_mean_arm_A": sum(psnr_gt_a) / len(psnr_gt_a),
           "launch_count_note": "libsnerf launches per frame; arm A also issues ATen kernels for the index table (4 per frame), one copy per slice and the "
                                "per-frame MSE, which are not in its count"}
    names = {"A": "eval_set: index table + trainer.forward in 4096-ray slices", "B": "renderer, 65536-ray chunks, unfused tail",
             "C": "renderer, fused tail, cutoff 0", "D": "renderer, fused tail, cutoff 1e-3", "E": "renderer, fused tail, cutoff 1e-2"}
    for k in arms:
        s = stat(ms[k])
        res["arms"][k] = {"arm": names[k], "ms_per_frame": s, "frames_per_s_median": 1e3 / s["median"], "spread_ms": s["max"] - s["min"],
                          "launches_per_frame": launches[k], **({"render_tail_hip_events": tail[k]} if k in tail else {}),
                          **({"quality": quality[k]} if k in quality else {})}
    a, b, c = (res["arms"][k]["ms_per_frame"] for k in "ABC")
    res["acceptance"] = {"B_faster_than_A_by_more_than_spread_of_A": bool(a["median"] - b["median"] > a["max"] - a["min"]),
                         "C_not_slower_than_B_beyond_spread": bool(c["median"] - b["median"] <= max(b["max"] - b["min"], c["max"] - c["min"]))}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {"ms_per_frame": round(v["ms_per_frame"]["median"], 2), "spread_ms": round(v["spread_ms"], 2), "launches": v["launches_per_frame"]}
                      for k, v in res["arms"].items()}))
    print(json.dumps({"tail": tail, "quality": quality, "acceptance": res["acceptance"], "bit_identical_B_C": same_bits}))


if __name__ == "__main__":
    main()

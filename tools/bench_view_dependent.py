"""View-dependent colour net (KPlanesTrainConfig.disable_viewing_dependent = False) against the `k-planes` preset's view-independent one, in ONE
process: (1) the colour-net backward alone at N = 4096 x 64 (HIP events, 30 launches): the view-dependent wave-owns-rows kernel that forms
[SH | h] on chip, the 15-input kernel of the preset, and the workgroup-tile kernel on a materialised [N, 32] input; (2) whole training steps
at the preset (4096 rays, default switches), view-independent and view-dependent trainers alternating, median of 3 legs; (3) the colour
kernels' mean times inside the step (enable_kernel_timing); (4) for context, the autograd KPlanesModel(disable_viewing_dependent=False) step
(forward, loss, backward, torch.optim.Adam) on the same batch.  Dev tool.

    python tools/bench_view_dependent.py [--steps 40] [--warmup 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def colour_backward_alone(R=4096, S=64):
    L = _lib.lib()
    N = R * S
    out = {}
    for name, d_in in (("vd_rows_31", 31), ("vi_rows_15", 15), ("vd_tile_31", 31)):
        d = _lib.MlpDesc()
        d.d_in, d.d_out, d.hidden, d.n_hidden, d.hidden_act, d.out_act, d.operands = d_in, 3, 64, 2, 1, 1, 1
        W = (torch.rand(L.snerf_mlp_param_count(C.byref(d)), device=DEV) - 0.5) * 0.4
        dirs = torch.nn.functional.normalize(torch.rand(R, 3, device=DEV) * 2 - 1, dim=-1)
        h = torch.rand(N, 16, device=DEV) - 0.3
        gY = torch.rand(N, 3, device=DEV) - 0.5
        gh = torch.zeros(N, 16, device=DEV)
        ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(d))), device=DEV)
        gW = torch.zeros_like(W)
        if name == "vd_rows_31":
            call = lambda: _lib.check(L.snerf_kplanes_color_bwd_vd_ws(C.byref(d), ops._ptr(W), ops._ptr(dirs), S, ops._ptr(h), C.c_int64(N), ops._ptr(gY), 3,
                                                                      ops._ptr(gh), ops._ptr(ws), ops._stream()), name)
        elif name == "vi_rows_15":
            call = lambda: _lib.check(L.snerf_mlp_bwd_ws(C.byref(d), ops._ptr(W), ops._ptr(h), 16, C.c_int64(N), ops._ptr(gY), 3, -1, None, ops._ptr(gh), 16,
                                                         ops._ptr(ws), ops._stream()), name)
        else:
            cx = torch.empty(N, 32, device=DEV)
            gcx = torch.empty(N, 32, device=DEV)
            _lib.check(L.snerf_kplanes_color_input_fwd(ops._ptr(dirs), S, ops._ptr(h), C.c_int64(N), ops._ptr(cx), ops._stream()), "cx")
            call = lambda: _lib.check(L.snerf_mlp_bwd_tile(C.byref(d), ops._ptr(W), ops._ptr(cx), 32, C.c_int64(N), ops._ptr(gY), 3, -1, None, ops._ptr(gcx), 32,
                                                           ops._ptr(gW), ops._stream()), name)
        out[name + "_ms"] = round(timed(call), 4)
    return out


def batch(tr, gen):
    R = tr.R
    o = (torch.rand(R, 3, device=DEV, generator=gen) * 2 - 1) * 0.9
    d = torch.nn.functional.normalize(torch.rand(R, 3, device=DEV, generator=gen) * 2 - 1, dim=-1)
    return {"origins": o, "directions": d, "times": torch.rand(R, 1, device=DEV, generator=gen)}, torch.rand(R, 3, device=DEV, generator=gen)


def leg(tr, steps, warmup, gen):
    rays, target = batch(tr, gen)
    for _ in range(warmup):
        tr.train_step(rays, target)
    tr.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step(rays, target)
    tr.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    res = {"colour_backward_alone": colour_backward_alone()}
    print(json.dumps(res["colour_backward_alone"]), flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    trs = {"view_independent": KPlanesTrainer(KPlanesTrainConfig(seed=1), 4096, DEV),
           "view_dependent": KPlanesTrainer(KPlanesTrainConfig(seed=1, disable_viewing_dependent=False), 4096, DEV)}
    assert trs["view_dependent"].color_bwd_vd and trs["view_dependent"].fused_field
    ms = {k: [] for k in trs}
    for _ in range(args.legs):  # alternating legs, both from where the previous leg left them
        for k, tr in trs.items():
            ms[k].append(leg(tr, args.steps, args.warmup, gen))
    res["ms_per_step"] = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    res["ms_per_step_legs"] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
    res["ratio_vd_over_vi"] = round(res["ms_per_step"]["view_dependent"] / res["ms_per_step"]["view_independent"], 4)
    print(json.dumps({k: res[k] for k in ("ms_per_step", "ratio_vd_over_vi")}), flush=True)
    kt = {}
    for k, tr in trs.items():
        tr.enable_kernel_timing(["kplanes_field_fwd", "color_bwd_vd", "mlp_bwd.15x64x2"])
        rays, target = batch(tr, gen)
        for _ in range(10):
            tr.train_step(rays, target)
        kt[k] = {n: round(v[0], 4) for n, v in tr.kernel_times_ms().items()}
        tr.disable_kernel_timing()
    res["kernel_ms_in_step"] = kt
    print(json.dumps(kt), flush=True)
    # context: the autograd model (nerfstudio-shaped face of the same kernels) on the same batch
    del trs
    torch.cuda.empty_cache()
    from soccernerfs_amd.kplanes import KPlanesModel, KPlanesModelConfig
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.scene_colliders import SceneBox

    mcfg = KPlanesModelConfig.k_planes_preset()
    mcfg.disable_viewing_dependent = False
    model = KPlanesModel(mcfg, SceneBox(aabb=torch.tensor([[-1.5] * 3, [1.5] * 3]))).to(DEV).train()
    model.scene_box.aabb = model.scene_box.aabb.to(DEV)
    opts = [torch.optim.Adam([p for p in v if p.requires_grad], lr=1e-2, eps=1e-12) for v in model.get_param_groups().values()]
    g2 = torch.Generator(device=DEV).manual_seed(0)
    o = (torch.rand(4096, 3, device=DEV, generator=g2) * 2 - 1) * 0.9
    d = torch.nn.functional.normalize(torch.rand(4096, 3, device=DEV, generator=g2) * 2 - 1, dim=-1)
    rb = RayBundle(origins=o, directions=d, pixel_area=torch.ones(4096, 1, device=DEV), times=torch.rand(4096, 1, device=DEV, generator=g2))
    target = torch.rand(4096, 3, device=DEV, generator=g2)

    def model_step():
        out = model(rb)
        loss = sum(model.get_loss_dict(out, {"image": target}).values())
        for op in opts:
            op.zero_grad(set_to_none=True)
        loss.backward()
        for op in opts:
            op.step()

    for _ in range(3):
        model_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        model_step()
    torch.cuda.synchronize()
    res["autograd_model_vd_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / 5, 2)
    print(json.dumps({"autograd_model_vd_ms_per_step": res["autograd_model_vd_ms_per_step"]}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()

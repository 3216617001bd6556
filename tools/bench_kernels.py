"""Micro-benchmarks of individual libsnerf kernels at BASELINE config-2 sizes (GPU only; dev tool)."""
import sys
import os
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soccernerfs_amd import ops  # noqa: E402
from soccernerfs_amd.plane_set import PlaneSet  # noqa: E402


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ray_like_points(R, S, dev, lo=-1.0, hi=1.0):
    """Samples along R random rays through the box (spatially coherent like the real workload)."""
    o = torch.rand(R, 1, 3, device=dev) * 2 - 1
    d = torch.nn.functional.normalize(torch.rand(R, 1, 3, device=dev) * 2 - 1, dim=-1)
    t = torch.sort(torch.rand(R, S, 1, device=dev) * 0.5, dim=1).values
    p = (o * 0.3 + d * t).clamp(-1, 1)
    p = (p + 1) / 2 * (hi - lo) + lo
    tm = (torch.rand(R, 1, 1, device=dev) * 2 - 1).expand(R, S, 1)
    return torch.cat([p, tm], -1).reshape(-1, 4).contiguous()


def bench_sort(dev, R=4096, S=64, n_times=34):
    """The sample sort alone (snerf_kplanes_sort_samples) at the k-planes preset's shape -- 262 144 ray-like points whose rays share ~34 distinct
    times, as a batch drawn from a few dozen frames does -- for the preset's five scales (finest 1024^2) and config 3's six (finest 2048^2)."""
    pts = ray_like_points(R, S, dev).view(R, S, 4).clone()
    tv = torch.rand(n_times, device=dev) * 2 - 1
    pts[:, :, 3] = tv[torch.randint(0, n_times, (R,), device=dev)][:, None]
    pts = pts.view(-1, 4).contiguous()
    co = ops.coords_from_points(pts)
    for name, ms in (("preset, scales 1-16", (1, 2, 4, 8, 16)), ("config 3, scales 1-32", (1, 2, 4, 8, 16, 32))):
        # C = 8, the smallest the scatter takes: the sort reads the resolutions only, and a 32-channel config-3 plane set would be 2 GB for nothing
        ps = PlaneSet(8, [[64 * m] * 3 + [100] for m in ms], concat=True, device=dev)
        ss = ops.SortedScatter(ps, pts.shape[0], dev)
        ms_sort = timeit(lambda: ss.sort(co), iters=50, warm=5)
        print(f"sample sort alone, {name}: N = {pts.shape[0]}, {ms_sort * 1e3:.1f} us ({ss.hist.numel() * 4 / 1e6:.1f} MB workspace)")


def bench_field_fwd(dev, R=4096, repeats=5, iters=50):
    """field_fwd_kernel alone on a batch of the benchmark's own data (bench.py's cameras and frame times, the preset's trainer after a few steps), as
    a training step launches it (16-bit feature tile and sigma_net outputs kept): in the drawn order and, where the library has it, with its tiles
    walked in order of frame time (snerf_kplanes_field_fwd_ordered).  `repeats` alternating rounds of `iters` launches each; every round is printed,
    so the spread of repeated alone runs stands beside the difference.  --iters / --repeats: a short run for a counter pass."""
    import ctypes as C
    from soccernerfs_amd import _lib, synthetic
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    torch.manual_seed(20231029)
    L = _lib.lib()
    tr = KPlanesTrainer(KPlanesTrainConfig(), R, dev)
    cams = synthetic.make_cameras(20, 960, 540)
    data = synthetic.render_dataset(cams, synthetic.frame_times(100, 3), list(range(19)), dev, chunk_rows=540)
    M, H, W = data["images"].shape[:3]
    for _ in range(3):
        idx, target = ops.sample_pixels_uniform(torch.rand(R, 3, device=dev), M, H, W, data["images"])
        rays = ops.generate_rays(idx, data["fx"], data["fy"], data["cx"], data["cy"], data["c2w"], data["times"], aabb=tr.aabb, near_plane=tr.cfg.near_plane,
                                 training=True)
        tr.train_step(rays, target)
    tr.synchronize()
    b, co, N = tr.buf, tr._coords[2], R * tr.S[2]
    P = lambda t: C.c_void_p(t.data_ptr())
    head = (C.byref(tr._desc_field), P(tr.field_planes.planes), C.byref(co), C.c_int64(N), C.byref(tr.sigma_net.desc), P(tr.sigma_net.params),
            C.byref(tr.color_net.desc), P(tr.color_net.params), P(b["dens"][2]), P(b["rgb"]), P(b["feat16"]), P(b["h"]), None)
    variants = {"drawn order": lambda: _lib.check(L.snerf_kplanes_field_fwd(*head, ops._stream()), "field_fwd")}
    if hasattr(L, "snerf_kplanes_field_fwd_ordered"):
        order = ops.ray_time_order(tr.rays["times"])
        variants["time order"] = lambda: _lib.check(L.snerf_kplanes_field_fwd_ordered(*head, P(order), ops._stream()), "field_fwd_ordered")
    n_times = int(torch.unique(tr.rays["times"]).numel())
    print(f"field forward alone: R = {R}, N = {N}, {n_times} distinct frame times in the batch, {iters} launches per figure")
    res = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            res[k].append(timeit(fn, iters=iters, warm=3) * 1e3)
    for k, v in res.items():
        s = sorted(v)
        print(f"  {k:12s} us: " + " ".join(f"{x:7.1f}" for x in v) + f"   median {s[len(s) // 2]:.1f}  min {s[0]:.1f}  max {s[-1]:.1f}")


def bench_prop_bwd_budget(dev, wg_per_cu, R=4096, repeats=5, iters=20, lag_us=100.0):
    """The fused proposal backward (snerf_kplanes_density_bwd_budget) at a residency budget of `wg_per_cu` workgroups per CU (0 = uncapped), on the
    state a training step of the preset leaves behind (bench.py's data): alone, and with pass B of the field scatter on a second stream, enqueued
    `lag_us` behind it -- the situation of a step that updates the proposal networks.  Both streams are held back by a spin kernel while the host
    enqueues, so the lag is the device's, not the host's.  Spans are between HIP events around each kernel (an event's time is the dispatch)."""
    import ctypes as C
    from soccernerfs_amd import synthetic
    from soccernerfs_amd.fused_step import _On
    from soccernerfs_amd.streams import side_stream
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    torch.manual_seed(20231029)
    tr = KPlanesTrainer(KPlanesTrainConfig(proposal_backward_workgroups_per_cu=wg_per_cu), R, dev)
    tr.step = 20
    cams = synthetic.make_cameras(20, 960, 540)
    data = synthetic.render_dataset(cams, synthetic.frame_times(100, 3), list(range(19)), dev, chunk_rows=540)
    M, H, W = data["images"].shape[:3]
    for _ in range(4):  # the early schedule updates the proposal networks every second step: gdens, the sorted records and G are a step's own
        idx, target = ops.sample_pixels_uniform(torch.rand(R, 3, device=dev), M, H, W, data["images"])
        rays = ops.generate_rays(idx, data["fx"], data["fy"], data["cx"], data["cy"], data["c2w"], data["times"], aabb=tr.aabb, near_plane=tr.cfg.near_plane,
                                 training=True)
        tr.train_step(rays, target)
    tr.synchronize()
    assert tr.fused_proposal_backward and tr.quotient_scatter
    main, side = torch.cuda.current_stream(), side_stream(dev, "bench_pass_b")
    n_scales = tr._desc_field.n_scales
    pass_b = lambda: tr._ss.quotient_pass_b_scales(tr.field_planes.planes, tr.gviews["field.planes"], 0, n_scales, C.c_void_p(side.cuda_stream))
    t0 = time.perf_counter()
    torch.cuda._sleep(10_000_000)
    torch.cuda.synchronize()
    cyc_per_us = 10_000_000 / ((time.perf_counter() - t0) * 1e6)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def once(with_fused, with_b):
        a0, a1, b0, b1, go = ev(), ev(), ev(), ev(), ev()
        torch.cuda._sleep(int(400 * cyc_per_us))  # the host enqueues everything below while this spins
        go.record(main)
        side.wait_event(go)
        a0.record(main)
        if with_fused:
            with _On(tr, main):
                tr._fused_proposal_backward()
        a1.record(main)
        with torch.cuda.stream(side):
            if with_fused:
                torch.cuda._sleep(int(lag_us * cyc_per_us))
            b0.record(side)
            if with_b:
                pass_b()
            b1.record(side)
        torch.cuda.synchronize()
        return a0.elapsed_time(a1) * 1e3, b0.elapsed_time(b1) * 1e3, max(a0.elapsed_time(a1), a0.elapsed_time(b1)) * 1e3, a0.elapsed_time(b0) * 1e3

    med = lambda v: sorted(v)[len(v) // 2]
    print(f"proposal backward at {wg_per_cu:g} workgroups per CU ({tr._prop_bwd_workgroups or 'resident'} workgroups), R = {R}; medians of {iters} launches, {repeats} rounds")
    for _ in range(repeats):
        for _ in range(3):
            once(True, True)
        alone = med([once(True, False)[0] for _ in range(iters)])
        b_alone = med([once(False, True)[1] for _ in range(iters)])
        both = [once(True, True) for _ in range(iters)]
        print(f"  fused backward alone {alone:7.1f} us | pass B alone {b_alone:7.1f} us | together: fused {med([x[0] for x in both]):7.1f} us, pass B {med([x[1] for x in both]):7.1f} us "
              f"(enqueued {med([x[3] for x in both]):6.1f} us behind), first start to last end {med([x[2] for x in both]):7.1f} us")
    tr.grads.zero_()


def _int_flag(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    dev = torch.device("cuda:0")
    if "--sort" in sys.argv[1:]:  # the sort alone, nothing else
        return bench_sort(dev)
    if "--field-fwd" in sys.argv[1:]:  # the fused field forward alone, nothing else
        return bench_field_fwd(dev, repeats=_int_flag("--repeats", 5), iters=_int_flag("--iters", 50))
    if "--prop-bwd-wg-per-cu" in sys.argv[1:]:  # the fused proposal backward at a residency budget, alone and with pass B beside it
        return bench_prop_bwd_budget(dev, float(sys.argv[sys.argv.index("--prop-bwd-wg-per-cu") + 1]), repeats=_int_flag("--repeats", 5), iters=_int_flag("--iters", 20))
    R = 4096
    res = {}
    # main field: 5 scales, C=32
    ps = PlaneSet(32, [[64 * m] * 3 + [100] for m in (1, 2, 4, 8, 16)], concat=True, device=dev)
    for name, pts in (("random", torch.rand(R * 64, 4, device=dev) * 2 - 1), ("raylike", ray_like_points(R, 64, dev))):
        N = pts.shape[0]
        out = ops.interpolate_kplanes(pts, ps)
        gout = torch.rand_like(out)
        ms_f = timeit(lambda: ops.interpolate_kplanes(pts, ps.requires_grad_(False)))
        ps.requires_grad_(True)
        import ctypes as C
        from soccernerfs_amd import _lib
        desc, co = ps.desc(), ops.coords_from_points(pts)
        gpl = torch.zeros_like(ps.planes)
        def bwd():
            _lib.check(_lib.lib().snerf_kplanes_gather_bwd(C.byref(desc), C.c_void_p(ps.planes.data_ptr()), C.byref(co), C.c_int64(N),
                                                           C.c_void_p(gout.data_ptr()), C.c_void_p(gpl.data_ptr()), ops._stream()))
        ms_b = timeit(bwd)
        bytes_f = N * 5 * 6 * 4 * 32 * 4
        print(f"field gather {name}: fwd {ms_f:.3f} ms ({bytes_f / ms_f / 1e9:.2f} TB/s alg), bwd {ms_b:.3f} ms ({2 * bytes_f / ms_b / 1e9:.2f} TB/s alg rmw)")
    for lvl, (S, r) in enumerate(((256, 128), (128, 256))):
        pp = PlaneSet(8, [[r, r, r, 100]], concat=False, a=0.1, b=0.15, device=dev)
        pts = ray_like_points(R, S, dev, 0.0, 1.0)
        N = pts.shape[0]
        pp.requires_grad_(False)
        ms_f = timeit(lambda: ops.interpolate_kplanes(pts, pp))
        bytes_f = N * 6 * 4 * 8 * 4
        print(f"prop{lvl} gather: fwd {ms_f:.3f} ms ({bytes_f / ms_f / 1e9:.2f} TB/s alg)")
    # proposal backward on an updated step, both levels: unfused (per level: snerf_mlp_bwd_ws + snerf_kplanes_gather_bwd from the [N,8] features)
    # against the fused snerf_kplanes_density_bwd (both levels in one launch, features re-gathered on chip)
    import ctypes as C
    from soccernerfs_amd import _lib
    from soccernerfs_amd.tcnn_compat import Network
    L = _lib.lib()
    lv = []
    for lvl, (S, r) in enumerate(((256, 128), (128, 256))):
        pp = PlaneSet(8, [[r, r, r, 100]], concat=False, a=0.1, b=0.9, device=dev).requires_grad_(False)
        net = Network(8, 1, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1},
                      seed=lvl, operands="bf16").to(dev)
        pts = ray_like_points(R, S, dev, 0.0, 1.0)
        N = pts.shape[0]
        d, co = pp.desc(), ops.coords_from_points(pts)
        feat = ops.interpolate_kplanes(pts, pp).contiguous()
        gd = torch.randn(N, device=dev) * 1e-3
        ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), device=dev)
        gX, gpl = torch.empty(N, 8, device=dev), torch.zeros_like(pp.planes)
        lv.append(dict(pp=pp, net=net, pts=pts, N=N, d=d, co=co, feat=feat, gd=gd, ws=ws, gX=gX, gpl=gpl))
    P = lambda t: C.c_void_p(t.data_ptr())

    def unfused_net(v):
        _lib.check(L.snerf_mlp_bwd_ws(C.byref(v["net"].desc), P(v["net"].params), P(v["feat"]), 8, C.c_int64(v["N"]), None, 1, 0, P(v["gd"]), P(v["gX"]), 8,
                                      P(v["ws"]), ops._stream()))

    def unfused_scatter(v):
        _lib.check(L.snerf_kplanes_gather_bwd(C.byref(v["d"]), P(v["pp"].planes), C.byref(v["co"]), C.c_int64(v["N"]), P(v["gX"]), P(v["gpl"]), ops._stream()))

    arr = (_lib.DensityBwdLevel * 2)()
    for a, v in zip(arr, lv):
        a.desc, a.planes, a.coords, a.N = C.addressof(v["d"]), v["pp"].planes.data_ptr(), C.addressof(v["co"]), v["N"]
        a.net, a.W, a.gdens = C.addressof(v["net"].desc), v["net"].params.data_ptr(), v["gd"].data_ptr()
        a.grad_planes, a.workspace, a.gX = v["gpl"].data_ptr(), v["ws"].data_ptr(), None
    t_net = [timeit(lambda v=v: unfused_net(v)) for v in lv]
    t_sc = [timeit(lambda v=v: unfused_scatter(v)) for v in lv]
    t_fused = timeit(lambda: _lib.check(L.snerf_kplanes_density_bwd(arr, 2, ops._stream()), "kplanes_density_bwd"))
    print(f"proposal backward, both levels: unfused {sum(t_net) + sum(t_sc):.3f} ms (net backward {t_net[0]:.3f} + {t_net[1]:.3f}, "
          f"plane scatter {t_sc[0]:.3f} + {t_sc[1]:.3f}; the forward's [N,8] feature write not counted), fused {t_fused:.3f} ms (one launch)")
    z = torch.zeros(156_000_000, device=dev)
    ms = timeit(lambda: z.zero_())
    print(f"memset 624MB: {ms:.3f} ms ({z.numel() * 4 / ms / 1e9:.2f} TB/s)")
    y = torch.empty_like(z)
    ms = timeit(lambda: y.copy_(z))
    print(f"copy 624MB: {ms:.3f} ms ({2 * z.numel() * 4 / ms / 1e9:.2f} TB/s)")


if __name__ == "__main__":
    main()

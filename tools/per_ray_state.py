"""Same results before and after a change to the per-ray kernels (csrc/ray_ops.hip, csrc/render_loss.hip, csrc/render_eval.hip and
csrc/per_ray_common.hpp).  None of them uses atomics, so every output is determined bit for bit.  On host-generated inputs (the seeded
generators of tests/per_ray_reference.py) it calls every entry point directly and saves every output, one state_*.pt per case:

  snerf_weights_fwd; snerf_weights_bwd (accumulate 0 and 1, the non-finite flag); snerf_pdf_resample from densities (explicit u, eval u,
  annealed); snerf_render_fwd (training and eval, bg_mode 0 / 1 / 2, every optional output); snerf_render_bwd (with and without g_acc,
  accumulate 0 and 1); snerf_render_mse_bwd; snerf_distortion (accumulate 0 and 1); snerf_ray_train_fwd_bwd (bg_mode 0 and 2)
      at (S, R) = (1, 5) (63, 1) (64, 2) (65, 3) (129, 4) (319, 3) (320, 133) (48, 133), on three input families: finite, one with an
      overflowed density (inf on a zero-width bin, inf on a wide one, 3e38 over a third of a ray), one with NaN / inf colours in eval mode;
  snerf_kplanes_field_render at S = 32 and 64 with cutoff 0 and 1e-2 on a small plane set, plain and view-dependent.

The inputs are saved beside the outputs, so cmp also shows that both trees were fed the same bits.  Dev tool.

    python tools/per_ray_state.py run TREE OUTDIR   # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/per_ray_state.py cmp A B           # every tensor of every file equal in dtype, shape and BITS (NaN payloads included); exit 1 otherwise.
                                                    # One line per file, input family and entry point; a tensor that differs is named
"""
import ctypes as C
import os
import sys

import torch


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.int8}[t.element_size()])


def compare(a, b):
    bad = n = 0
    fa, fb = (sorted(f for f in os.listdir(d) if f.startswith("state_")) for d in (a, b))
    if fa != fb:
        print("file lists differ:", sorted(set(fa) ^ set(fb)))
        bad += 1
    for f in sorted(set(fa) & set(fb)):
        x, y = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
        if sorted(x) != sorted(y):
            print(f"{f}: tensor names differ")
            bad += 1
        groups = {}  # (input family, entry point) -> [tensors, elements, non-zero, non-finite, different]
        for k in sorted(set(x) & set(y)):
            ok = x[k].shape == y[k].shape and x[k].dtype == y[k].dtype and bool(torch.equal(bits(x[k]), bits(y[k])))
            g = groups.setdefault(".".join(k.split(".")[:2]), [0, 0, 0, 0, 0])
            g[0] += 1
            g[1] += x[k].numel()
            g[2] += int((x[k] != 0).sum())
            g[3] += int((~torch.isfinite(x[k])).sum()) if x[k].dtype.is_floating_point else 0
            g[4] += not ok
            if not ok:
                print(f"{f:24s} {k}: DIFFERENT")
            bad += not ok
            n += 1
        for name, g in groups.items():
            print(f"{f:24s} {name:28s} tensors = {g[0]:3d} n = {g[1]:8d} non-zero = {g[2]:8d} non-finite = {g[3]:5d}  {'equal' if g[4] == 0 else f'{g[4]} DIFFERENT'}")
    print("VERDICT", f"{n} of {n} tensors equal" if bad == 0 else f"{bad} differ")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
from soccernerfs_amd import _lib, ops
from soccernerfs_amd.plane_set import PlaneSet
from soccernerfs_amd.tcnn_compat import Network
from tests import per_ray_reference as PR

os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
ST = ops._stream
CASES = ((1, 5), (63, 1), (64, 2), (65, 3), (129, 4), (319, 3), (320, 133), (48, 133))  # (S, R)
SENTINEL = -7.0
new = lambda *sh, dtype=torch.float32: torch.full(sh, SENTINEL, dtype=dtype, device=DEV)


def overflowed(case):
    """densities that overflowed in the field's exp: inf on a zero-width bin (0 * inf), inf on a wide bin, 3e38 over a third of a ray"""
    c = dict(case)
    R, S = case["R"], case["S"]
    dens, eb = case["density"].clone(), case["ebins"].clone()
    dens[0, S // 2] = float("inf")
    if S > 1:
        eb[0, S // 2 + 1] = eb[0, S // 2]
    if R > 1:
        dens[1, S // 3] = float("inf")
    if R > 2:
        dens[2, : max(1, S // 3)] = 3e38
    c["density"], c["ebins"] = dens.contiguous(), eb.contiguous()
    return c


def per_ray(res, tag, case, eval_only=False):
    R, S = case["R"], case["S"]
    gen = PR._gen("per_ray_state", tag, R, S)
    rnd = lambda *sh: torch.rand(*sh, generator=gen)
    dv = lambda t: t.to(DEV).contiguous()
    dens, eb, sb, rgb, bg, target = (dv(case[k]) for k in ("density", "ebins", "c_bins", "rgb", "bg", "target"))
    w_in = dv(case["weights"])
    bg1 = bg[0].contiguous()
    for k in ("density", "ebins", "c_bins", "rgb", "bg", "target", "weights"):
        res[f"{tag}.input.{k}"] = case[k].clone()
    put = lambda name, t: res.__setitem__(f"{tag}.{name}", t.detach().cpu().clone())

    def render(mode, training):
        o = {"rgb": new(R, 3), "acc": new(R), "depth_median": new(R), "depth_expected": new(R), "median_rgb": new(R, 3),
             "median_index": new(R, dtype=torch.int64)}
        a = _lib.RenderArgs()
        a.weights, a.rgb, a.ebins, a.R, a.S, a.bg_mode, a.training = w_in.data_ptr(), rgb.data_ptr(), eb.data_ptr(), R, S, mode, training
        a.bg = None if mode == 1 else (bg if mode == 0 else bg1).data_ptr()
        a.rgb_out, a.acc_out, a.depth_median, a.depth_expected = (o[k].data_ptr() for k in ("rgb", "acc", "depth_median", "depth_expected"))
        a.median_rgb, a.median_index = o["median_rgb"].data_ptr(), o["median_index"].data_ptr()
        _lib.check(L.snerf_render_fwd(C.byref(a), ST()), "render_fwd")
        for k, t in o.items():
            put(f"render_fwd.bg{mode}.{'train' if training else 'eval'}.{k}", t)

    for mode in (0, 1, 2):
        render(mode, 0)
        if not eval_only:
            render(mode, 1)
    if eval_only:
        return
    # ---- weights forward / backward ----
    w = new(R, S)
    _lib.check(L.snerf_weights_fwd(P(dens), P(eb), R, S, P(w), ST()), "weights_fwd")
    put("weights_fwd", w)
    g_up = dv(rnd(R, S) - 0.5)
    prefill = dv(rnd(R, S) - 0.5)
    for accumulate in (0, 1):
        g, flag = prefill.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(L.snerf_weights_bwd(P(dens), P(eb), P(g_up), R, S, P(g), accumulate, P(flag), ST()), "weights_bwd")
        put(f"weights_bwd.acc{accumulate}.g_density", g)
        put(f"weights_bwd.acc{accumulate}.flag", flag)
    # ---- resampling from densities ----
    nears, fars = dv(rnd(R) * 0.5 + 0.05), dv(rnd(R) * 4.0 + 2.6)
    for So in sorted({S, max(1, S // 2)}):
        u = dv(torch.sort(rnd(R, So + 1), -1).values)
        for name, kw in (("u", dict(u=u)), ("eval", dict()), ("anneal", dict(u=u, anneal=0.5, kind="piecewise"))):
            sbo, ebo, inds, wo = ops.pdf_resample(sb, nears, fars, So, density=dens, ebins_prev=eb, return_inds=True, return_weights=True, **kw)
            for k, t in (("sbins", sbo), ("ebins", ebo), ("inds", inds), ("weights", wo)):
                put(f"pdf_resample.S{So}.{name}.{k}", t)
    # ---- render backward, MSE backward ----
    go, ga, out = (dv(t) for t in PR.upstream(case, "state"))
    for mode, b in ((0, bg), (2, bg1)):
        for use_acc in (0, 1):
            for accumulate in (0, 1):
                gw, grgb = prefill.clone(), new(R, S, 3)
                _lib.check(L.snerf_render_bwd(P(w_in), P(rgb), P(b), mode, P(go), P(ga) if use_acc else None, R, S, P(gw), P(grgb), accumulate, ST()),
                           "render_bwd")
                put(f"render_bwd.bg{mode}.gacc{use_acc}.acc{accumulate}.g_weights", gw)
                put(f"render_bwd.bg{mode}.gacc{use_acc}.acc{accumulate}.g_rgb", grgb)
        gw, grgb, sq = new(R, S), new(R, S, 3), new(R)
        _lib.check(L.snerf_render_mse_bwd(P(w_in), P(rgb), P(b), mode, P(out), P(target), 2 * 0.7 / (3 * R), R, S, P(gw), P(grgb), P(sq), ST()),
                   "render_mse_bwd")
        for k, t in (("g_weights", gw), ("g_rgb", grgb), ("sqerr", sq)):
            put(f"render_mse_bwd.bg{mode}.{k}", t)
    # ---- distortion ----
    for accumulate in (0, 1):
        val, g = new(R), prefill.clone()
        _lib.check(L.snerf_distortion(P(w_in), P(sb), R, S, 1e-3 / R, P(val), P(g), accumulate, ST()), "distortion")
        put(f"distortion.acc{accumulate}.loss_rays", val)
        put(f"distortion.acc{accumulate}.g_weights", g)
    # ---- the one-launch training kernel ----
    for mode, b in ((0, bg), (2, bg1)):
        o = {"weights": new(R, S), "rgb_out": new(R, 3), "acc": new(R), "depth_median": new(R), "sqerr": new(R), "dist_rays": new(R), "g_rgb": new(R, S, 3),
             "g_density": new(R, S), "g_weights": new(R, S), "flag": torch.zeros(1, dtype=torch.int32, device=DEV)}
        ra = _lib.RayTrainArgs()
        ra.density, ra.ebins, ra.sbins, ra.rgb, ra.bg, ra.target = dens.data_ptr(), eb.data_ptr(), sb.data_ptr(), rgb.data_ptr(), b.data_ptr(), target.data_ptr()
        ra.R, ra.S, ra.bg_mode, ra.go_scale, ra.dist_scale = R, S, mode, 2.0 / (3 * R), 1e-3 / R
        ra.weights, ra.rgb_out, ra.acc_out, ra.depth_median = (o[k].data_ptr() for k in ("weights", "rgb_out", "acc", "depth_median"))
        ra.sqerr_rays, ra.dist_rays, ra.g_rgb, ra.g_density = (o[k].data_ptr() for k in ("sqerr", "dist_rays", "g_rgb", "g_density"))
        ra.g_weights, ra.nonfinite_flag = o["g_weights"].data_ptr(), o["flag"].data_ptr()
        _lib.check(L.snerf_ray_train_fwd_bwd(C.byref(ra), ST()), "ray_train_fwd_bwd")
        for k, t in o.items():
            put(f"ray_train.bg{mode}.{k}", t)


def field_render(res, S, vd, R=301):
    gen = torch.Generator().manual_seed(100 + S + int(vd))
    base = (12, 10, 9, 6)
    ps = PlaneSet(32, [[r * m for r in base[:3]] + [base[3]] for m in (1, 2)], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.9 + 0.3)
    mk = lambda i, o, h, nh, act: Network(i, o, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h,
                                                   "n_hidden_layers": nh}, seed=7 * i, operands="bf16")
    ps, sigma, color = ps.to(DEV), mk(64, 16, 128, 1, "None").to(DEV), mk(31 if vd else 15, 3, 64, 2, "Sigmoid").to(DEV)
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    t = torch.rand(R, generator=gen)
    steps = torch.cumsum(torch.rand(R, S + 1, generator=gen) * 0.8 + 0.6, dim=1)
    steps = (steps - steps[:, :1]) / (steps[:, -1:] - steps[:, :1])
    eb = torch.rand(R, 1, generator=gen) * 0.2 + (torch.rand(R, generator=gen) * 2.5 + 0.5)[:, None] * steps
    o, d, t, eb = (x.to(DEV).contiguous() for x in (o, d, t, eb))
    co = ops.coords_from_rays(o, d, t, eb, [[-1.5] * 3, [1.5] * 3], True)
    desc = ps.desc()
    assert L.snerf_kplanes_field_render_supported(C.byref(desc), C.byref(sigma.desc), C.byref(color.desc), S) == 1
    for cutoff in (0.0, 1e-2):
        out = {"rgb": new(R, 3), "acc": new(R), "depth_median": new(R), "depth_expected": new(R), "median_index": new(R, dtype=torch.int64),
               "samples_done": new(R, dtype=torch.int32)}
        _lib.check(L.snerf_kplanes_field_render(C.byref(desc), P(ps.planes), C.byref(co), R, C.byref(sigma.desc), P(sigma.params), C.byref(color.desc),
                                                P(color.params), cutoff, P(out["rgb"]), P(out["acc"]), P(out["depth_median"]), P(out["depth_expected"]),
                                                P(out["median_index"]), P(out["samples_done"]), ST()), "field_render")
        for k, x in out.items():
            res[f"S{S}.{'vd' if vd else 'plain'}.cutoff{cutoff:g}.{k}"] = x.cpu().clone()
    res[f"S{S}.{'vd' if vd else 'plain'}.input.ebins"] = eb.cpu()


for S, R in CASES:
    res = {}
    case = PR.pipeline_case(R, S, S, "a")
    per_ray(res, "finite", case)
    per_ray(res, "overflow", overflowed(case))
    per_ray(res, "nan_rgb", PR.with_nonfinite_rgb(case), eval_only=True)
    torch.cuda.synchronize()
    torch.save(res, os.path.join(out, f"state_S{S:03d}_R{R:03d}.pt"))
    print(f"S {S} R {R}: {len(res)} tensors", flush=True)
res = {}
for S in (32, 64):
    for vd in (False, True):
        field_render(res, S, vd)
torch.cuda.synchronize()
torch.save(res, os.path.join(out, "state_field_render.pt"))
print(f"field_render: {len(res)} tensors", flush=True)

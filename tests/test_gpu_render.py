"""GPU: rendering whole frames (csrc/render_eval.hip, soccernerfs_amd/render.py).

1. snerf_raygen_frame against snerf_raygen on the meshgrid index table (bit for bit) and against the reference's own rays for the G16 camera;
2. snerf_kplanes_field_render with cutoff 0 against snerf_kplanes_field_fwd -> snerf_weights_fwd -> snerf_render_fwd (bit for bit);
3. early ray termination: which rays stop where, and the error bounds that follow from the cutoff;
4. KPlanesRenderer.render_frame against the existing eval path (4096-ray slices through KPlanesTrainer.forward(training=False));
5. rendering between training steps leaves training undisturbed and sees the finished step's parameters;
6. render_camera_path writes the frames; 7. a checkpoint round trip renders the same bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _measure

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]


def _g16():
    from soccernerfs_amd.camera_paths import get_path_from_json

    with open(os.path.join(GOLD, "g16_camera_path.json")) as f:
        path = json.load(f)
    return path, get_path_from_json(path), np.load(os.path.join(GOLD, "g16_camera_path.npz"))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. ray generation for a frame
# ---------------------------------------------------------------------------------------------------------------------------
def _raygen_frame(cams, k, p0, p1, with_times=True):
    from soccernerfs_amd import _lib, ops

    n = p1 - p0
    f = lambda *s: torch.full(s, -7.0, device=DEV)
    out = {"origins": f(n, 3), "directions": f(n, 3), "pixel_area": f(n), "directions_norm": f(n), "times": f(n), "nears": f(n), "fars": f(n)}
    a = _lib.RaygenFrameArgs()
    a.fx, a.fy, a.cx, a.cy = float(cams.fx[k]), float(cams.fy[k]), float(cams.cx[k]), float(cams.cy[k])
    for i, v in enumerate(cams.camera_to_worlds[k].reshape(-1).tolist()):
        a.c2w[i] = v
    a.time, a.W, a.H, a.p0, a.p1, a.near_plane = float(cams.times[k]), cams.width, cams.height, p0, p1, 0.05
    for i in range(3):
        a.aabb_min[i], a.aabb_max[i] = AABB[0][i], AABB[1][i]
    a.origins, a.dirs, a.pixel_area, a.dir_norm = (out[q].data_ptr() for q in ("origins", "directions", "pixel_area", "directions_norm"))
    a.times = out["times"].data_ptr() if with_times else None
    a.nears, a.fars = out["nears"].data_ptr(), out["fars"].data_ptr()
    _lib.check(_lib.lib().snerf_raygen_frame(C.byref(a), ops._stream()), "raygen_frame")
    return out


def _raygen_table(cams, k, p0, p1):
    from soccernerfs_amd import ops

    H, W = cams.height, cams.width
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)[p0:p1].contiguous().to(DEV)
    c = cams.to(DEV)
    return ops.generate_rays(idx, c.fx, c.fy, c.cx, c.cy, c.camera_to_worlds, c.times, aabb=AABB, near_plane=0.05, training=False)


@pytest.mark.parametrize("span", ["frame", "mid_row"])
def test_raygen_frame_equals_raygen_on_the_meshgrid_table(span):
    _, cams, _ = _g16()
    H, W = cams.height, cams.width
    assert (H, W) == (54, 96)
    p0, p1 = (0, H * W) if span == "frame" else (5 * W + 37, 31 * W + 11)  # starts and ends in the middle of a row
    for k in range(len(cams)):
        got, want = _raygen_frame(cams, k, p0, p1), _raygen_table(cams, k, p0, p1)
        for key in ("origins", "directions", "pixel_area", "directions_norm", "times", "nears", "fars"):
            assert torch.equal(got[key].reshape(-1), want[key].reshape(-1)), (k, key)
    # times is optional
    got = _raygen_frame(cams, 0, p0, p1, with_times=False)
    assert float(got["times"].min()) == -7.0 and float(got["times"].max()) == -7.0


def test_raygen_frame_rejects_ranges_outside_the_frame():
    _, cams, _ = _g16()
    with pytest.raises(RuntimeError, match="pixel range"):
        _raygen_frame(cams, 0, 10, cams.height * cams.width + 1)


def test_raygen_frame_against_reference_rays():
    """Origins and times exact, directions at the tolerance the G1 check of tests/test_gpu_render_loss.py uses for snerf_raygen (rtol 1e-6,
    atol 2e-7).  The reference's path cameras carry float64 focal lengths; its rays come out float32 and are compared as float32."""
    _, cams, g = _g16()
    k = int(g["ray_camera"])
    got = _raygen_frame(cams, k, 0, cams.height * cams.width)
    want_o, want_d = (torch.from_numpy(g[q]).float().reshape(-1, 3) for q in ("ray_origins", "ray_directions"))
    print("g16 raygen_frame deviation:", _measure.record("g16.raygen_frame.directions", got["directions"], want_d))
    assert torch.equal(got["origins"].cpu(), want_o)
    assert torch.equal(got["times"].cpu(), torch.from_numpy(g["ray_times"]).float().reshape(-1))
    torch.testing.assert_close(got["directions"].cpu(), want_d, rtol=1e-6, atol=2e-7)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the fused render tail
# ---------------------------------------------------------------------------------------------------------------------------
def _field(ms, operands, vd, seed=0):
    from soccernerfs_amd.plane_set import PlaneSet
    from soccernerfs_amd.tcnn_compat import Network

    gen = torch.Generator().manual_seed(seed)
    base = (12, 10, 9, 6)
    ps = PlaneSet(32, [[r * m for r in base[:3]] + [base[3]] for m in ms], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.9 + 0.3)
    mk = lambda i, o, h, nh, act: Network(i, o, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h,
                                                   "n_hidden_layers": nh}, seed=seed + 7 * i, operands=operands)
    sigma, color = mk(32 * len(ms), 16, 128, 1, "None"), mk(31 if vd else 15, 3, 64, 2, "Sigmoid")
    return ps.to(DEV), sigma.to(DEV), color.to(DEV)


def _rays(R, S, gen, span=None):
    """Rays from inside the box; S + 1 increasing bin edges per ray (uneven widths).  span [R]: the rays' far - near."""
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    t = torch.rand(R, generator=gen)
    near = torch.rand(R, 1, generator=gen) * 0.2
    if span is None:
        span = torch.rand(R, generator=gen) * 2.5 + 0.5
    steps = torch.cumsum(torch.rand(R, S + 1, generator=gen) * 0.8 + 0.6, dim=1)
    steps = (steps - steps[:, :1]) / (steps[:, -1:] - steps[:, :1])
    eb = near + span[:, None] * steps
    return tuple(x.to(DEV).contiguous() for x in (o, d, t, eb))


def _chain(ps, sigma, color, rays, S):
    """The unfused tail: snerf_kplanes_field_fwd -> snerf_weights_fwd -> snerf_render_fwd(training = 0, bg_mode = 1)."""
    from soccernerfs_amd import _lib, ops

    o, d, t, eb = rays
    R = o.shape[0]
    L, p = _lib.lib(), ops._ptr
    co = ops.coords_from_rays(o, d, t, eb, AABB, True)
    desc = ps.desc()
    dens, rgb, w = torch.empty(R, S, device=DEV), torch.empty(R * S, 3, device=DEV), torch.empty(R, S, device=DEV)
    _lib.check(L.snerf_kplanes_field_fwd(C.byref(desc), p(ps.planes), C.byref(co), C.c_int64(R * S), C.byref(sigma.desc), p(sigma.params),
                                         C.byref(color.desc), p(color.params), p(dens), p(rgb), None, None, None, ops._stream()))
    _lib.check(L.snerf_weights_fwd(p(dens), p(eb), R, S, p(w), ops._stream()))
    out = {"rgb": torch.empty(R, 3, device=DEV), "acc": torch.empty(R, device=DEV), "depth_median": torch.empty(R, device=DEV),
           "depth_expected": torch.empty(R, device=DEV), "median_index": torch.empty(R, dtype=torch.int64, device=DEV)}
    a = _lib.RenderArgs()
    a.weights, a.rgb, a.ebins, a.R, a.S, a.bg_mode, a.training = w.data_ptr(), rgb.data_ptr(), eb.data_ptr(), R, S, 1, 0
    a.rgb_out, a.acc_out, a.depth_median, a.depth_expected, a.median_index = (out[k].data_ptr() for k in ("rgb", "acc", "depth_median", "depth_expected",
                                                                                                          "median_index"))
    _lib.check(L.snerf_render_fwd(C.byref(a), ops._stream()))
    out["density"] = dens
    return out


def _fused(ps, sigma, color, rays, S, cutoff=0.0):
    from soccernerfs_amd import _lib, ops

    o, d, t, eb = rays
    R = o.shape[0]
    L, p = _lib.lib(), ops._ptr
    co = ops.coords_from_rays(o, d, t, eb, AABB, True)
    desc = ps.desc()
    assert L.snerf_kplanes_field_render_supported(C.byref(desc), C.byref(sigma.desc), C.byref(color.desc), S) == 1
    out = {"rgb": torch.full((R, 3), -1.0, device=DEV), "acc": torch.full((R,), -1.0, device=DEV), "depth_median": torch.full((R,), -1.0, device=DEV),
           "depth_expected": torch.full((R,), -1.0, device=DEV), "median_index": torch.full((R,), -1, dtype=torch.int64, device=DEV),
           "samples_done": torch.full((R,), -1, dtype=torch.int32, device=DEV)}
    _lib.check(L.snerf_kplanes_field_render(C.byref(desc), p(ps.planes), C.byref(co), R, C.byref(sigma.desc), p(sigma.params), C.byref(color.desc),
                                            p(color.params), cutoff, p(out["rgb"]), p(out["acc"]), p(out["depth_median"]), p(out["depth_expected"]),
                                            p(out["median_index"]), p(out["samples_done"]), ops._stream()), "field_render")
    return out


EXACT = ("rgb", "acc", "depth_median", "depth_expected", "median_index")


@pytest.mark.parametrize("S", [32, 64, 96])
@pytest.mark.parametrize("vd", [False, True], ids=["plain", "view_dependent"])
@pytest.mark.parametrize("ms", [(1, 2, 4, 8, 16), (1, 2, 3, 4, 6, 8)], ids=["5scales", "6scales"])
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_field_render_equals_the_unfused_chain(operands, ms, vd, S):
    ps, sigma, color = _field(ms, operands, vd)
    R = 777 if S == 64 else 301  # 301 < the persistent grid of 512 workgroups; 777: some workgroups walk two rays, some one
    rays = _rays(R, S, torch.Generator().manual_seed(S))
    want, got = _chain(ps, sigma, color, rays, S), _fused(ps, sigma, color, rays, S)
    for k in EXACT:
        assert torch.equal(got[k], want[k]), (k, float((got[k].double() - want[k].double()).abs().max()))
    assert bool((got["samples_done"] == S).all())
    assert float(want["acc"].min()) > 0.0 and float(want["acc"].max()) <= 1.0 + 1e-6  # a live input: not all-transparent, not all-zero


def test_field_render_optional_outputs_and_unsupported_shapes():
    from soccernerfs_amd import _lib, ops

    ps, sigma, color = _field((1, 2), "bf16", False)
    S, R = 64, 70
    rays = _rays(R, S, torch.Generator().manual_seed(1))
    want = _chain(ps, sigma, color, rays, S)
    o, d, t, eb = rays
    L, p = _lib.lib(), ops._ptr
    co = ops.coords_from_rays(o, d, t, eb, AABB, True)
    desc = ps.desc()
    rgb, acc = torch.empty(R, 3, device=DEV), torch.empty(R, device=DEV)
    _lib.check(L.snerf_kplanes_field_render(C.byref(desc), p(ps.planes), C.byref(co), R, C.byref(sigma.desc), p(sigma.params), C.byref(color.desc),
                                            p(color.params), 0.0, p(rgb), p(acc), None, None, None, None, ops._stream()))
    assert torch.equal(rgb, want["rgb"]) and torch.equal(acc, want["acc"])
    for bad_S in (16, 48, 352):
        assert L.snerf_kplanes_field_render_supported(C.byref(desc), C.byref(sigma.desc), C.byref(color.desc), bad_S) == 0
    ps32, s32, c32 = _field((1, 2), "fp32", False)
    assert L.snerf_kplanes_field_render_supported(C.byref(ps32.desc()), C.byref(s32.desc), C.byref(c32.desc), 64) == 0
    eb48 = eb[:, :49].contiguous()
    co48 = ops.coords_from_rays(o, d, t, eb48, AABB, True)
    assert L.snerf_kplanes_field_render(C.byref(desc), p(ps.planes), C.byref(co48), R, C.byref(sigma.desc), p(sigma.params), C.byref(color.desc),
                                        p(color.params), 0.0, p(rgb), p(acc), None, None, None, None, ops._stream()) != 0


@pytest.mark.parametrize("vd", [False, True], ids=["plain", "view_dependent"])
def test_field_render_nan_texel_and_overflowing_density(vd):
    """Non-finite values take the same way through both paths.  (a) A NaN in one plane texel: every sample whose footprint holds it gets NaN
    features; fmaxf(NaN, 0) = 0 in sigma_net's ReLU then gives those samples the density and colour of an all-zero hidden layer -- finite, and
    different from the clean field's.  (b) sigma_net's output layer scaled up so that exp(.) overflows to inf for some samples, with one
    zero-width bin per ray: delta * sigma = 0 * inf = NaN there, which get_weights' nan_to_num turns into weight 0."""
    ps, sigma, color = _field((1, 2, 4, 8, 16), "bf16", vd)
    S, R = 64, 301
    rays = _rays(R, S, torch.Generator().manual_seed(5))
    clean = _chain(ps, sigma, color, rays, S)
    with torch.no_grad():
        ps.planes[2115] = float("nan")  # one channel of one texel in the middle of the coarsest XY plane (12 x 10 texels x 32 channels = 3840 floats)
    want, got = _chain(ps, sigma, color, rays, S), _fused(ps, sigma, color, rays, S)
    touched = (want["density"] != clean["density"]).any(1)
    assert 0 < int(touched.sum()) < R, "mis-built: the NaN texel must be inside some rays' footprints and outside others'"
    for k in EXACT:
        assert bool(torch.isfinite(got[k].double()).all()), k
        assert torch.equal(got[k], want[k]), k
    assert bool((got["samples_done"] == S).all())
    with torch.no_grad():
        k0 = 32 * 5 * 128
        sigma.params[k0:k0 + 128 * 16] *= 3e3
    o, d, t, eb = rays
    eb = eb.clone()
    eb[:, 10] = eb[:, 9]  # a zero-width bin
    rays = (o, d, t, eb)
    want, got = _chain(ps, sigma, color, rays, S), _fused(ps, sigma, color, rays, S)
    assert bool(torch.isinf(want["density"][:, 9]).any()), "mis-built: no density overflowed on the zero-width bin"
    for k in EXACT:
        assert bool(torch.isfinite(got[k].double()).all()), k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("cutoff", [1e-3, 1e-2])
@pytest.mark.parametrize("S", [64, 96])
def test_field_render_early_termination(S, cutoff):
    """Densities of order one (sigma_net's output layer scaled down, so exp(.) ~ 1) and ray spans far - near drawn log-uniformly over 4.5 decades
    (0.01 .. 316): short rays stay transparent, long ones saturate inside their first tiles.  The reference for where a ray must stop is the
    UNFUSED chain's densities: T_k = exp(-sum_{i < k} sigma_i delta_i) at the tile boundaries k = 32, 64, ...

      * rays with T_k < cutoff / 2 at some boundary must report samples_done = the first such boundary (or an earlier boundary at which T
        was already inside the undecided band);
      * rays with T_k > 2 cutoff at every boundary in front of the last tile must report samples_done = S (behind the last tile nothing is
        left to skip, so that boundary decides nothing);
      * the band between may go either way.

    At least a quarter of the rays must be in the first set WITH a boundary in front of the last tile (a real skip) and at least a tenth in
    the second, or the test fails as mis-built.  Shares the unfused chain gave (must stop early / must not stop), 2000 rays:
    S = 64: 0.274 / 0.704 at cutoff 1e-3, 0.313 / 0.660 at 1e-2; S = 96: 0.305 / 0.674 and 0.341 / 0.628 (a density of exactly 1 and even bins
    would give 0.29 / 0.69 at S = 64, cutoff 1e-3: span > 15.2 resp. span < 12.4).

    Against the cutoff-0 outputs: |d rgb| <= cutoff + 1e-6 and |d acc| <= cutoff + 1e-6 (colours in [0,1], the dropped weights and the
    background share sum to T < cutoff), the median index is equal (acc > 1 - cutoff >= 0.5 is reached inside the evaluated samples),
    |d depth_expected| <= cutoff far / (acc + 1e-10) + 1e-5 far.  The additive terms are fp32 rounding slack."""
    ps, sigma, color = _field((1, 2, 4, 8, 16), "bf16", False, seed=3)
    with torch.no_grad():
        k0 = 32 * 5 * 128
        sigma.params[k0:k0 + 128 * 16] *= 0.05  # the output layer [128 x 16]: y ~ 0, density = exp(y) of order one
    R = 2000
    gen = torch.Generator().manual_seed(11)
    span = 10.0 ** (torch.rand(R, generator=gen) * 4.5 - 2.0)
    rays = _rays(R, S, gen, span=span)
    eb = rays[3]
    ref = _chain(ps, sigma, color, rays, S)
    dens = ref["density"].double()
    assert bool(torch.isfinite(dens).all()) and 0.2 < float(dens.median()) < 5.0, "mis-built: densities are not of order one"
    tau = torch.cumsum(dens * (eb[:, 1:] - eb[:, :-1]).double(), dim=1)
    bounds = list(range(32, S + 1, 32))
    T = torch.exp(-tau[:, [b - 1 for b in bounds]])  # [R, boundaries]
    below = T < cutoff / 2
    first = torch.where(below.any(1), torch.tensor(bounds, device=DEV)[below.float().argmax(1)], torch.full((R,), -1, device=DEV))
    must_stop = first > 0
    must_stop_early = must_stop & (first < S)
    must_not = (T[:, :-1] > 2 * cutoff).all(1)
    share_stop, share_not = float(must_stop_early.float().mean()), float(must_not.float().mean())
    print(f"early termination S={S} cutoff={cutoff}: must stop early {share_stop:.3f}, must not stop {share_not:.3f}")
    assert share_stop >= 0.25 and share_not >= 0.10, f"mis-built input: shares {share_stop:.3f} / {share_not:.3f}"

    exact = _fused(ps, sigma, color, rays, S, 0.0)
    got = _fused(ps, sigma, color, rays, S, cutoff)
    done = got["samples_done"].long()
    # a ray whose T sits in the undecided band at an EARLIER boundary may stop there already: it must have stopped by `first`, and no ray stops
    # at a boundary where it is surely above the cutoff.  Where no earlier boundary is in the band the two sides meet: samples_done == first
    maybe = T <= 2 * cutoff
    bt = torch.tensor(bounds, device=DEV)
    earliest = torch.where(maybe[:, :-1].any(1), bt[:-1][maybe[:, :-1].float().argmax(1)], torch.full((R,), S, device=DEV))
    assert bool((done[must_stop] <= first[must_stop]).all())
    assert bool((done >= earliest).all())
    clean = must_stop & (earliest == first)
    assert float(clean.float().mean()) >= 0.2 and bool((done[clean] == first[clean]).all())
    assert bool((done[must_not] == S).all())
    assert bool(((done % 32 == 0) & (done >= 32) & (done <= S)).all())
    assert bool((exact["samples_done"] == S).all())
    d_rgb = (got["rgb"] - exact["rgb"]).abs().max(dim=1).values
    d_acc = (got["acc"] - exact["acc"]).abs()
    print(f"  max |d rgb| {float(d_rgb.max()):.3e}  max |d acc| {float(d_acc.max()):.3e}  tiles skipped {1 - float(done.float().mean()) / S:.3f}")
    assert bool((d_rgb <= cutoff + 1e-6).all()), float(d_rgb.max())
    assert bool((d_acc <= cutoff + 1e-6).all()), float(d_acc.max())
    assert torch.equal(got["median_index"], exact["median_index"])
    far = eb[:, -1]
    bound = cutoff * far / (got["acc"] + 1e-10) + 1e-5 * far
    d_depth = (got["depth_expected"] - exact["depth_expected"]).abs()
    assert bool((d_depth <= bound).all()), float((d_depth - bound).max())
    # rays that did not stop are the exact path
    full = done == S
    for k in EXACT:
        assert torch.equal(got[k][full], exact[k][full]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 4. - 7. the renderer
# ---------------------------------------------------------------------------------------------------------------------------
SMALL = dict(aabb_scale=1.5, spacetime_resolution=(16, 16, 16, 4), multiscale_res=(1, 2), feature_dim=32,
             proposal_resolutions=((24, 24, 24, 4), (32, 32, 32, 4)), proposal_feature_dim=8, num_proposal_samples_per_ray=(64, 32),
             num_nerf_samples_per_ray=32, warm_up_end=2)
R_TRAIN = 512


def _inputs(R, steps, seed=3):
    gen = torch.Generator().manual_seed(seed)
    out = []
    g = lambda z: z.to(DEV).contiguous()
    for _ in range(steps):
        o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
        d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
        rays = {"origins": g(o), "directions": g(d), "times": g(torch.rand(R, 1, generator=gen))}
        rng = {"t_rand": g(torch.rand(R, 65, generator=gen)), "u": [g(torch.rand(R, 33, generator=gen)), g(torch.rand(R, 33, generator=gen))],
               "bg": g(torch.rand(R, 3, generator=gen))}
        out.append((rays, g(torch.rand(R, 3, generator=gen)), rng))
    return out


def _trainer(steps=0, inputs=None, **kw):
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    tr = KPlanesTrainer(KPlanesTrainConfig(**{**SMALL, **kw}), R_TRAIN, DEV)
    for rays, target, rng in (inputs if inputs is not None else _inputs(R_TRAIN, steps)):
        tr.train_step(rays, target, rng)
    return tr


def _eval_path_frame(tr, cams, k, anneal):
    """The parent's way to a full frame (tools/train_psnr.py::eval_set): the meshgrid index table, 4096-ray slices through forward(training=False)."""
    from soccernerfs_amd import ops

    H, W = cams.height, cams.width
    c = cams.to(DEV)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
    rgb, acc, depth = torch.empty(H * W, 3, device=DEV), torch.empty(H * W, device=DEV), torch.empty(H * W, device=DEV)
    Rs = tr.R
    for i in range(0, H * W, Rs):
        rays = ops.generate_rays(idx[i:i + Rs].contiguous(), c.fx, c.fy, c.cx, c.cy, c.camera_to_worlds, c.times, aabb=tr.aabb,
                                 near_plane=tr.cfg.near_plane, training=False)
        n = rays["origins"].shape[0]
        rgb[i:i + n] = tr.forward(rays, None, anneal, training=False)
        acc[i:i + n], depth[i:i + n] = tr.buf["acc"][:n], tr.buf["depth"][:n]
    return rgb.view(H, W, 3), acc.view(H, W, 1), depth.view(H, W, 1)


@pytest.mark.parametrize("cfg_kw", [dict(), dict(disable_viewing_dependent=False), dict(num_nerf_samples_per_ray=16), dict(mlp_operands="fp32")],
                         ids=["preset_nets", "view_dependent", "S16_unfused_tail", "fp32_operands"])
def test_render_frame_equals_the_eval_path(cfg_kw):
    from soccernerfs_amd.render import KPlanesRenderer
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    cfg = {**SMALL, **cfg_kw}
    S2 = cfg["num_nerf_samples_per_ray"]
    tr = KPlanesTrainer(KPlanesTrainConfig(**cfg), 4096, DEV)  # 4096-ray eval slices, as tools/train_psnr.py
    gen = torch.Generator().manual_seed(3)
    g = lambda z: z.to(DEV).contiguous()
    for _ in range(4):
        R = 4096
        rays = {"origins": g((torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2),
                "directions": g(torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)), "times": g(torch.rand(R, 1, generator=gen))}
        tr.train_step(rays, g(torch.rand(R, 3, generator=gen)))
    _, cams, _ = _g16()
    k = 2
    frames = {}
    for fused in (True, False):
        rn = KPlanesRenderer(tr, rays_per_chunk=4000, fused_tail=fused)  # 96 x 54 = 5184 = 4000 + 1184: the chunk does not divide the frame
        assert rn.fused_tail == (fused and S2 % 32 == 0 and cfg.get("mlp_operands", "bf16") != "fp32")
        frames[fused] = rn.render_frame(cams, k)
        assert {q: tuple(v.shape) for q, v in frames[fused].items()} == {"rgb": (54, 96, 3), "accumulation": (54, 96, 1), "depth": (54, 96, 1)}
        anneal = rn.default_anneal()
    rgb, acc, depth = _eval_path_frame(tr, cams, k, anneal)
    assert float(rgb.std()) > 0 and bool(torch.isfinite(rgb).all())
    for fused in (True, False):
        assert torch.equal(frames[fused]["rgb"], rgb), fused
        assert torch.equal(frames[fused]["accumulation"], acc), fused
        assert torch.equal(frames[fused]["depth"], depth), fused


def test_renderer_needs_a_time_and_checks_the_cutoff():
    from soccernerfs_amd.camera_paths import get_path_from_json
    from soccernerfs_amd.render import KPlanesRenderer

    tr = _trainer(steps=1)
    path, cams, _ = _g16()
    p = json.loads(json.dumps(path))
    del p["camera_path"][0]["render_time"]
    rn = KPlanesRenderer(tr, rays_per_chunk=4000)
    with pytest.raises(ValueError, match="default_time"):
        rn.render_frame(get_path_from_json(p), 1)
    a = rn.render_frame(get_path_from_json(p), 1, default_time=float(cams.times[1]))
    b = rn.render_frame(cams, 1)
    assert torch.equal(a["rgb"], b["rgb"])
    with pytest.raises(ValueError, match="cutoff"):
        KPlanesRenderer(tr, transmittance_cutoff=1.5)
    # the fused tail is off by default (measured slower); a cutoff turns it on, and raises where the kernel is not built for the shape
    assert not KPlanesRenderer(tr).fused_tail and KPlanesRenderer(tr, fused_tail=True).fused_tail
    assert KPlanesRenderer(tr, transmittance_cutoff=1e-3).fused_tail
    with pytest.raises(ValueError, match="fused render tail"):
        KPlanesRenderer(_trainer(steps=0, num_nerf_samples_per_ray=16), transmittance_cutoff=1e-3)
    # an opted-in cutoff stays inside its bound on a real frame
    c = KPlanesRenderer(tr, rays_per_chunk=4000, transmittance_cutoff=1e-2).render_frame(cams, 1)
    assert float((c["rgb"] - b["rgb"]).abs().max()) <= 1e-2 + 1e-6


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default_async_sweep"])
def test_rendering_between_steps_leaves_training_undisturbed(deterministic):
    """Train k steps, render, train k more.  deterministic=True: the parameters equal 2k uninterrupted steps bit for bit.  Both modes: the frame,
    rendered straight after train_step returned (no synchronise: the field planes' sweep may still be running on its side stream, the live
    parameter buffer has just been swapped), equals the frame of a trainer that ran the same k steps and was synchronised and idle."""
    from soccernerfs_amd.render import KPlanesRenderer

    k = 3
    inputs = _inputs(R_TRAIN, 2 * k)
    _, cams, _ = _g16()
    kw = dict(deterministic=deterministic)
    a = _trainer(inputs=inputs[:k], **kw)
    if not deterministic:
        assert a.async_field_adam and a._field_adam_done is not None  # the sweep of step k is pending when the frame is asked for
    frame_mid = KPlanesRenderer(a, rays_per_chunk=4000, fused_tail=True).render_frame(cams, 0)
    frame_mid = {q: v.clone() for q, v in frame_mid.items()}
    for rays, target, rng in inputs[k:]:
        a.train_step(rays, target, rng)
    a.synchronize()
    idle = _trainer(inputs=inputs[:k], **kw)
    idle.synchronize()
    frame_idle = KPlanesRenderer(idle, rays_per_chunk=4000).render_frame(cams, 0)
    if deterministic:
        for q in frame_idle:
            assert torch.equal(frame_mid[q], frame_idle[q]), q
        for rays, target, rng in inputs[k:]:
            idle.train_step(rays, target, rng)
        idle.synchronize()
        b = _trainer(inputs=inputs, **kw)
        b.synchronize()
        assert a.step == b.step == 2 * k
        for x, y in ((a, b), (idle, b)):
            assert torch.equal(x.params, y.params) and torch.equal(x.exp_avg, y.exp_avg) and torch.equal(x.exp_avg_sq, y.exp_avg_sq)
    else:
        # float atomics: two runs of the same k steps differ by the order of the gradient sums, so "the same frame" is checked on ONE trainer:
        # render without a synchronise, then synchronise and render again -- the parameters have not changed in between
        a2 = _trainer(inputs=inputs[:k], **kw)
        rn = KPlanesRenderer(a2, rays_per_chunk=4000, fused_tail=True)
        hot = {q: v.clone() for q, v in rn.render_frame(cams, 0).items()}
        a2.synchronize()
        cold = rn.render_frame(cams, 0)
        for q in hot:
            assert torch.equal(hot[q], cold[q]), q


def test_render_camera_path_writes_frames(tmp_path):
    from PIL import Image

    from soccernerfs_amd.render import KPlanesRenderer

    tr = _trainer(steps=3)
    path, cams, _ = _g16()
    rn = KPlanesRenderer(tr, rays_per_chunk=4000)
    fn = tmp_path / "path.json"
    fn.write_text(json.dumps(path))
    files = rn.render_camera_path(str(fn), str(tmp_path / "png"), outputs=("rgb", "accumulation"))
    assert [os.path.basename(f) for f in files] == [f"{k:05d}.png" for k in range(len(cams))]
    assert sorted(os.listdir(tmp_path / "png")) == [f"{k:05d}.png" for k in range(len(cams))]
    for k, f in enumerate(files):
        img = torch.from_numpy(np.array(Image.open(f)))
        frame = rn.render_frame(cams, k)
        assert tuple(img.shape) == (54, 2 * 96, 3) and img.dtype == torch.uint8
        want = torch.cat([frame["rgb"], frame["accumulation"].expand(-1, -1, 3)], dim=1)
        want = torch.floor(255.0 * want.clamp(0, 1) + 0.5).to(torch.uint8).cpu()
        assert torch.equal(img, want)
    files = rn.render_camera_path(path, str(tmp_path / "npy"), format="npy")
    assert [os.path.basename(f) for f in files] == [f"{k:05d}.npy" for k in range(len(cams))]
    for k, f in enumerate(files):
        arr = np.load(f)
        assert arr.dtype == np.float32 and arr.shape == (54, 96, 3)
        assert torch.equal(torch.from_numpy(arr), rn.render_frame(cams, k)["rgb"].cpu())
    with pytest.raises(ValueError, match="format"):
        rn.render_camera_path(path, str(tmp_path / "x"), format="mp4")
    with pytest.raises(KeyError):
        rn.render_camera_path(path, str(tmp_path / "x"), outputs=("normals",))
    p = json.loads(json.dumps(path))
    del p["camera_path"][2]["render_time"]
    with pytest.raises(ValueError, match="default_time"):
        rn.render_camera_path(p, str(tmp_path / "x"))


def test_evaluate_reports_psnr_and_ssim():
    from soccernerfs_amd import metrics
    from soccernerfs_amd.render import KPlanesRenderer

    tr = _trainer(steps=2)
    _, cams, _ = _g16()
    rn = KPlanesRenderer(tr, rays_per_chunk=4000)
    images = torch.randint(0, 256, (len(cams), 54, 96, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
    res = rn.evaluate(cams, images, [1, 3])
    assert len(res["psnr_per_image"]) == len(res["ssim_per_image"]) == 2
    rgb = rn.render_frame(cams, 3)["rgb"]
    assert res["psnr_per_image"][1] == pytest.approx(float(metrics.psnr(rgb, images[3].float() / 255.0)), rel=1e-6)
    assert res["psnr"] == pytest.approx(sum(res["psnr_per_image"]) / 2) and res["ssim"] == pytest.approx(sum(res["ssim_per_image"]) / 2)


def test_checkpoint_round_trip_renders_the_same_bits(tmp_path):
    from soccernerfs_amd.render import KPlanesRenderer

    tr = _trainer(steps=4)
    _, cams, _ = _g16()
    want = KPlanesRenderer(tr, rays_per_chunk=4000).render_frame(cams, 1)
    tr.save_checkpoint(str(tmp_path))
    fresh = _trainer(steps=0, seed=99)
    assert not torch.equal(fresh.params, tr.params)
    fresh.load_checkpoint(str(tmp_path))
    anneal = KPlanesRenderer(tr).default_anneal()
    got = KPlanesRenderer(fresh, rays_per_chunk=4000).render_frame(cams, 1, anneal=anneal)
    for q in want:
        assert torch.equal(got[q], want[q]), q


def test_tools_render_command_line(tmp_path):
    """tools/render.py: configuration overrides -> load_checkpoint -> render_camera_path writes the frames the renderer gives on the trainer
    that saved the checkpoint."""
    import importlib.util

    from PIL import Image

    from soccernerfs_amd.render import KPlanesRenderer

    spec = importlib.util.spec_from_file_location("tools_render_cli", os.path.join(os.path.dirname(GOLD), os.pardir, "tools", "render.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    tr = _trainer(steps=3)
    tr.save_checkpoint(str(tmp_path / "ckpt"))
    argv = ["--load-dir", str(tmp_path / "ckpt"), "--camera-path-filename", os.path.join(GOLD, "g16_camera_path.json"), "--output-path", str(tmp_path / "out"),
            "--eval-num-rays-per-chunk", "4000", "--device", DEV]
    for k, v in SMALL.items():
        argv += ["--set", f"{k}={v!r}"]
    cli.main(argv)
    _, cams, _ = _g16()
    rn = KPlanesRenderer(tr, rays_per_chunk=4000)
    assert sorted(os.listdir(tmp_path / "out")) == [f"{k:05d}.png" for k in range(len(cams))]
    for k in range(len(cams)):
        img = torch.from_numpy(np.array(Image.open(tmp_path / "out" / f"{k:05d}.png")))
        assert torch.equal(img, KPlanesRenderer.to_uint8(rn.render_frame(cams, k)["rgb"]).cpu()), k
    with pytest.raises(SystemExit):
        cli.config_from_overrides(["no_such_field=1"])
    assert cli.config_from_overrides(["mlp_operands=fp16", "multiscale_res=(1,2)"]).multiscale_res == (1, 2)

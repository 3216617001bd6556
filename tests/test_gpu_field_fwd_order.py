"""GPU: the fused field forward's tiles walked in order of frame time (csrc/raygen.hip: snerf_ray_time_order; csrc/field_fused.hip:
snerf_kplanes_field_fwd_ordered; KPlanesTrainConfig.field_fwd_time_order).

* the order kernel against a stable host sort of the same floats, exactly;
* the ordered forward against snerf_kplanes_field_fwd on the raw bits of every output it writes, over a lattice of shapes and three orders;
* the trainer with the switch on and off: the walk is the only thing that changes, so everything is bit-identical."""
import ctypes as C

import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------- the order kernel
def _times(kind, R, gen):
    if kind == "equal":
        return torch.full((R,), 0.375)
    if kind == "three":
        return torch.tensor([0.5, 0.0, 1.0])[torch.randint(0, 3, (R,), generator=gen)]
    if kind == "ascending":
        return torch.arange(R, dtype=torch.float32) / max(R, 1)
    if kind == "descending":
        return 1.0 - torch.arange(R, dtype=torch.float32) / max(R, 1)
    assert kind == "frames34"
    return (torch.arange(34, dtype=torch.float32) / 33.0)[torch.randint(0, 34, (R,), generator=gen)]


@pytest.mark.parametrize("kind", ["equal", "three", "ascending", "descending", "frames34"])
@pytest.mark.parametrize("R", [1, 2, 255, 256, 257, 4096, 16384])
def test_ray_time_order_is_the_stable_host_sort(R, kind):
    from soccernerfs_amd import ops

    times = _times(kind, R, torch.Generator().manual_seed(R))
    want = torch.sort(times, stable=True).indices.to(torch.int32)
    t_dev = times.to(DEV)
    got = ops.ray_time_order(t_dev).cpu()
    again = ops.ray_time_order(t_dev.view(R, 1)).cpu()
    assert got.dtype == torch.int32 and torch.equal(torch.sort(got.long()).values, torch.arange(R))  # a permutation
    ordered = times[got.long()]
    assert bool((ordered[1:] >= ordered[:-1]).all())
    ties = ordered[1:] == ordered[:-1]
    assert bool((got[1:][ties] > got[:-1][ties]).all())  # ties in ray order
    assert torch.equal(got, want)
    assert torch.equal(again, got)  # two launches, the same bits


def test_ray_time_order_refuses_more_than_16384_rays():
    from soccernerfs_amd import _lib, ops

    R = 16385
    times = torch.rand(R, device=DEV)
    out = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    rc = _lib.lib().snerf_ray_time_order(ops._ptr(times), R, ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc < 0 and b"16384" in _lib.lib().snerf_last_error()
    assert bool((out == -7).all())  # nothing was launched
    with pytest.raises(RuntimeError, match="ray_time_order"):
        ops.ray_time_order(times)


# ---------------------------------------------------------------- the ordered forward
def _field(ms, R, S, vd, seed):
    """A plane set, both nets (bf16 operands) and R rays x S samples in per-ray coordinates (coords.mode = 1): times from seven frames, so that
    rays tie, and bin edges that run past the box on some rays (border clamp)."""
    from soccernerfs_amd import ops
    from soccernerfs_amd.plane_set import PlaneSet
    from soccernerfs_amd.tcnn_compat import Network

    gen = torch.Generator().manual_seed(seed)
    base = (12, 10, 9, 6)
    ps = PlaneSet(32, [[r * m for r in base[:3]] + [base[3]] for m in ms], concat=True, generator=gen)
    with torch.no_grad():
        ps.planes.copy_(torch.rand(ps.numel, generator=gen) * 0.9 + 0.3)
    mk = lambda i, o, h, nh, act: Network(i, o, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h,
                                                   "n_hidden_layers": nh}, seed=seed + 7 * i, operands="bf16")
    sigma, color = mk(32 * len(ms), 16, 128, 1, "None"), mk(31 if vd else 15, 3, 64, 2, "Sigmoid")
    o = torch.rand(R, 3, generator=gen) * 2 - 1
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    t = (torch.arange(7, dtype=torch.float32) / 6.0)[torch.randint(0, 7, (R,), generator=gen)]
    eb = torch.sort(torch.rand(R, S + 1, generator=gen) * 1.5, dim=-1).values
    g = lambda z: z.to(DEV).contiguous()
    rays = {"o": g(o), "d": g(d), "t": g(t), "eb": g(eb)}
    aabb = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]
    co = ops.coords_from_rays(rays["o"], rays["d"], rays["t"], rays["eb"], aabb, True)
    return ps.to(DEV), sigma.to(DEV), color.to(DEV), rays, co


def _run(ps, sigma, color, co, N, keep, order):
    """-> the outputs the KEEP variant writes, prefilled with NaN.  order None: snerf_kplanes_field_fwd."""
    from soccernerfs_amd import _lib, ops

    L, nan = _lib.lib(), float("nan")
    K0 = ps.out_dim
    out = {"dens": torch.full((N,), nan, device=DEV), "rgb": torch.full((N, 3), nan, device=DEV)}
    if keep >= 1:
        out["feat16"] = torch.full((N, K0), nan, dtype=torch.bfloat16, device=DEV)
        out["h"] = torch.full((N, 16), nan, device=DEV)
    if keep == 2:
        out["feat32"] = torch.full((N, K0), nan, device=DEV)
    p = lambda k: ops._ptr(out[k]) if k in out else None
    desc = ps.desc()
    head = (C.byref(desc), ops._ptr(ps.planes), C.byref(co), C.c_int64(N), C.byref(sigma.desc), ops._ptr(sigma.params), C.byref(color.desc),
            ops._ptr(color.params), p("dens"), p("rgb"), p("feat16"), p("h"), p("feat32"))
    if order is None:
        _lib.check(L.snerf_kplanes_field_fwd(*head, ops._stream()), "field_fwd")
    else:
        _lib.check(L.snerf_kplanes_field_fwd_ordered(*head, ops._ptr(order), ops._stream()), "field_fwd_ordered")
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


# every value of R (1; 5: fewer tiles than workgroups and than 8; 300: 300-900 tiles on at most 512 workgroups), S (tiles per ray 1, 2, 3), n_scales
# (4, 6), KEEP (0, 1, 2) and colour net (plain, view-dependent) at least once
LATTICE = [
    (1, 32, 4, 0, False),
    (5, 64, 6, 1, True),
    (300, 96, 4, 2, False),
    (300, 64, 6, 2, True),
    (5, 96, 4, 0, True),
    (300, 32, 6, 1, False),
]


@pytest.mark.parametrize("R,S,n_scales,keep,vd", LATTICE)
def test_ordered_forward_equals_the_unordered_one_bit_for_bit(R, S, n_scales, keep, vd):
    from soccernerfs_amd import ops

    ms = (1, 2, 3, 4) if n_scales == 4 else (1, 2, 3, 4, 6, 8)
    ps, sigma, color, rays, co = _field(ms, R, S, vd, seed=R + S + n_scales)
    N = R * S
    want = _run(ps, sigma, color, co, N, keep, None)
    assert not any(bool(torch.isnan(v.float()).any()) for v in want.values())
    ident = torch.arange(R, dtype=torch.int32, device=DEV)
    orders = {"time": ops.ray_time_order(rays["t"]), "identity": ident, "reversed": ident.flip(0).contiguous()}
    assert torch.equal(orders["time"].cpu(), torch.sort(rays["t"].cpu(), stable=True).indices.to(torch.int32))
    for name, order in orders.items():
        got = _run(ps, sigma, color, co, N, keep, order)
        assert set(got) == set(want)
        for k, v in got.items():
            assert not bool(torch.isnan(v.float()).any()), (name, k)  # every sample written
            assert torch.equal(_bits(v), _bits(want[k])), (name, k)


def test_null_order_is_the_unordered_kernel():
    """ray_order == NULL: accepted for every shape the unordered entry point takes (here S = 48, not a multiple of the tile), and the same bits."""
    from soccernerfs_amd import _lib, ops

    R, S = 37, 48
    ps, sigma, color, rays, co = _field((1, 2), R, S, False, seed=3)
    want = _run(ps, sigma, color, co, R * S, 1, None)
    dens, rgb = torch.empty(R * S, device=DEV), torch.empty(R * S, 3, device=DEV)
    f16, h = torch.empty(R * S, ps.out_dim, dtype=torch.bfloat16, device=DEV), torch.empty(R * S, 16, device=DEV)
    desc = ps.desc()
    _lib.check(_lib.lib().snerf_kplanes_field_fwd_ordered(
        C.byref(desc), ops._ptr(ps.planes), C.byref(co), C.c_int64(R * S), C.byref(sigma.desc), ops._ptr(sigma.params), C.byref(color.desc),
        ops._ptr(color.params), ops._ptr(dens), ops._ptr(rgb), ops._ptr(f16), ops._ptr(h), None, None, ops._stream()), "field_fwd_ordered")
    torch.cuda.synchronize()
    for k, v in (("dens", dens), ("rgb", rgb), ("feat16", f16), ("h", h)):
        assert torch.equal(_bits(v), _bits(want[k])), k


@pytest.mark.parametrize("case", ["S48", "mode0"])
def test_ordered_forward_rejects_what_has_no_whole_ray_tiles(case):
    from soccernerfs_amd import _lib, ops

    R, S = 8, 48 if case == "S48" else 32
    ps, sigma, color, rays, co = _field((1, 2), R, S, False, seed=4)
    N = R * S
    if case == "mode0":
        pts = (torch.rand(N, 4, device=DEV) * 2 - 1).contiguous()
        co = ops.coords_from_points(pts)
    dens, rgb = torch.full((N,), -1.0, device=DEV), torch.full((N, 3), -1.0, device=DEV)
    order = torch.arange(R, dtype=torch.int32, device=DEV)
    desc = ps.desc()
    L = _lib.lib()
    rc = L.snerf_kplanes_field_fwd_ordered(C.byref(desc), ops._ptr(ps.planes), C.byref(co), C.c_int64(N), C.byref(sigma.desc), ops._ptr(sigma.params),
                                           C.byref(color.desc), ops._ptr(color.params), ops._ptr(dens), ops._ptr(rgb), None, None, None,
                                           ops._ptr(order), ops._stream())
    torch.cuda.synchronize()
    assert rc < 0 and b"kplanes_field_fwd_ordered" in L.snerf_last_error()
    assert bool((dens == -1.0).all()) and bool((rgb == -1.0).all())  # an error, not a fallback to the unordered kernel


# ---------------------------------------------------------------- the trainer
def _g11_trainers(**kw):
    from oracle import kplanes_oracle as KO
    from oracle.gen_golden import E2E_CFG
    from soccernerfs_amd.trainer import KPlanesTrainer
    from tests.test_gpu_default_path import _default_cfg

    g = load_golden("g11_model")
    R = g["origins"].shape[0]
    trs = [KPlanesTrainer(_default_cfg(E2E_CFG, field_fwd_time_order=on, **kw), R, DEV) for on in (True, False)]
    for tr in trs:
        tr.load_oracle_params(KO.make_kplanes_params(**E2E_CFG))
    assert trs[0].field_fwd_time_order and not trs[1].field_fwd_time_order and all(tr.fused_field for tr in trs)
    t = lambda k: g[k].to(DEV).contiguous()
    rays = {"origins": t("origins"), "directions": t("directions"), "times": t("times")}
    rng = {"t_rand": t("t_rand"), "u": [t("u0"), t("u1")], "bg": t("bg")}
    return trs, rays, t("target"), rng


def test_trainer_first_step_is_bit_identical_with_the_switch_on_and_off():
    """The G11 batch through the default path, switch on and off, same seed: after step 1 rgb and every loss term are bit-identical (the forward's
    outputs are, and the parameters both steps start from).  Later steps of this mode differ by float-atomic order only, as two runs of either
    setting do; the deterministic test below carries the comparison over three steps."""
    trs, rays, target, rng = _g11_trainers()
    outs = [tr.train_step(rays, target, rng).clone() for tr in trs]
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    lds = [tr.loss_dict() for tr in trs]
    assert set(lds[0]) == set(lds[1]) and len(lds[0]) > 0
    for k in lds[0]:
        assert torch.equal(_bits(lds[0][k].reshape(-1)), _bits(lds[1][k].reshape(-1))), k
    # the order the forward walked is the stable sort of the batch's times
    want = torch.sort(rays["times"].reshape(-1).cpu(), stable=True).indices.to(torch.int32)
    for tr in trs:
        tr.synchronize()
    assert torch.equal(trs[0]._ray_order.cpu(), want)


def test_deterministic_trainer_is_bit_identical_over_three_steps():
    """Deterministic mode (fixed-point gradient accumulation) runs the fused forward too: with the ordered walk the parameters after three steps are
    the same bits."""
    trs, rays, target, rng = _g11_trainers(deterministic=True)
    for _ in range(3):
        outs = [tr.train_step(rays, target, rng).clone() for tr in trs]
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    for tr in trs:
        tr.synchronize()
    assert trs[0].step == 3 and torch.equal(_bits(trs[0].params), _bits(trs[1].params))

"""CPU: the unbounded-scene restatement (tests/unbounded_reference.py) tied to the oracle, to values recorded from the reference and to float64
autograd; the generators' planted categories and margins; the host refusals of snerf_coords.contract, which run before any launch; defaults
that must not move; the config a render command line rebuilds."""
import ctypes as C
import dataclasses
import importlib.util
import os

import pytest
import torch

from oracle import kplanes_oracle as KO
from tests import pose_reference as PR
from tests import unbounded_reference as U
from tests.conftest import ROOT, load_golden


def test_restatement_equals_oracle_and_reference_recording_in_float32():
    g = load_golden("g6c_contraction")
    pos = torch.as_tensor(g["positions"])
    want = torch.as_tensor(g["contracted"])
    assert pos.dtype == torch.float32
    assert torch.equal(U.contract_half(pos) * 2, want)  # the halving is exact: y / 2 * 2 == y
    assert torch.equal(U.contract_half(pos), KO.scene_contraction_inf(pos) / 2)
    from soccernerfs_amd.spatial_distortions import SceneContraction

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4096, 3, generator=gen) * torch.tensor([0.5, 2.0, 30.0])[torch.randint(0, 3, (4096, 1), generator=gen)]
    x[:64] = torch.tensor([U.planted_points()[i % len(U.planted_points())][1] for i in range(64)])
    assert torch.equal(U.contract_half(x), KO.scene_contraction_inf(x) / 2)
    assert torch.equal(U.contract_half(x), SceneContraction(order=float("inf"))(x) / 2.0)
    assert torch.equal(U.contract_half(x.double()), KO.scene_contraction_inf(x.double()) / 2)
    one = torch.tensor([[1.0, 0.5, -0.25], [-0.5, -1.0, 0.75]])
    assert torch.equal(U.contract_half(one), one / 2)  # m == 1: the second branch, which returns pos there too


def test_points_are_the_field_route():
    """points() equals what KPlanesField computes on the torch route: _pts_from_positions(get_positions, times, distortion)."""
    from soccernerfs_amd.kplanes_field import _pts_from_positions
    from soccernerfs_amd.spatial_distortions import SceneContraction

    rs = U.coordinate_rounds(5, 7)[0]
    pos = U.positions(rs["origins"], rs["dirs"], rs["ebins"])
    got = _pts_from_positions(pos, rs["times"][:, None], None, True, SceneContraction(order=float("inf")))
    assert torch.equal(got, U.points(rs["origins"], rs["dirs"], rs["ebins"], rs["times"]))
    assert torch.equal(got, U.expected_points(rs))
    assert torch.equal(got[:, :3].contiguous(), U.expected_points(rs, 3))


def test_jacobian_against_float64_autograd():
    gen = torch.Generator().manual_seed(11)
    pos = torch.randn(20000, 3, generator=gen, dtype=torch.float64) * torch.tensor([0.6, 3.0, 200.0], dtype=torch.float64)[torch.randint(0, 3, (20000, 1), generator=gen)]
    ab = pos.abs().sort(dim=-1, descending=True).values
    keep = ((ab[:, 0] - ab[:, 1]) > 1e-6 * ab[:, 0]) & ((ab[:, 0] - 1).abs() > 1e-6)  # away from ties and from m = 1
    pos = pos[keep]
    m = pos.abs().max(-1).values
    assert int((m < 1).sum()) > 1000 and all(int(((pos.abs().argmax(-1) == k) & (m > 1) & ((pos[:, k] > 0) == s)).sum()) > 300 for k in range(3) for s in (True, False))
    g = torch.randn(pos.shape[0], 3, generator=gen, dtype=torch.float64)
    x = pos.clone().requires_grad_(True)
    (KO.scene_contraction_inf(x) / 2 * g).sum().backward()
    got = U.contract_half_vjp(pos, g)
    assert PR.rel_dev(got, x.grad) < 1e-14, PR.rel_dev(got, x.grad)
    # the tie rule: the first maximal axis takes the whole of the max's gradient (autograd splits it evenly: a measure-zero difference)
    tie = torch.tensor([[2.0, 2.0, 0.5], [0.5, -1.5, -1.5]], dtype=torch.float64)
    gt = torch.ones(2, 3, dtype=torch.float64)
    out = U.contract_half_vjp(tie, gt)
    a = 2 / tie.abs().max(-1).values - 1 / tie.abs().max(-1).values ** 2
    assert torch.allclose(out[0, 1], a[0] / 2) and out[0, 0] != out[0, 1]      # axis 1 of the first row got no share of b
    assert torch.allclose(out[1, 2], a[1] / 2) and out[1, 1] != out[1, 2]


def test_near_far_collider_restatement():
    from soccernerfs_amd.rays import RayBundle
    from soccernerfs_amd.scene_colliders import NearFarCollider

    col = NearFarCollider(near_plane=0.05, far_plane=37.5)
    for training in (True, False):
        col.train(training)
        rb = col(RayBundle(origins=torch.zeros(6, 3), directions=torch.ones(6, 3), pixel_area=torch.ones(6, 1)))
        n, f = U.near_far(6, 0.05, 37.5, training)
        assert torch.equal(rb.nears, n) and torch.equal(rb.fars, f)
    assert float(U.near_far(2, 0.05, 9.0, False)[0].max()) == 0.0


@pytest.mark.parametrize("shape", U.RAY_SHAPES, ids=lambda s: f"R{s[0]}-S{s[1]}")
def test_equality_cases_hold_every_category(shape):
    rounds = U.coordinate_rounds(*shape)  # asserts the categories itself, on the float32 positions
    seen = {cat for rs in rounds for _, _, cat in rs["planted"]}
    assert seen == set(U.CATEGORIES) and len(U.CATEGORIES) == 1 + 1 + 6 + 1 + 10
    for rs in rounds:
        p = U.expected_points(rs)
        assert bool(torch.isfinite(p).all()) and float(p[:, :3].abs().max()) <= 1.0
        assert torch.equal(p, U.points(rs["origins"], rs["dirs"], rs["ebins"], rs["times"]))
    far = torch.cat([U.expected_points(rs)[:, :3].abs().amax(-1) for rs in rounds])
    assert float(far.max()) > 0.999  # m = 1024: p = 1 - 2^-11, crowded against the face


def test_gradient_cases_keep_their_samples_and_hold_the_categories():
    axes = set()
    inside = outside = 0
    for c in U.GRAD_CASES:
        d = U.make_gradient_case(c)
        ok = U.grad_comparable(c, d)
        assert float(ok.double().mean()) >= U.KEEP_SHARE, (U.grad_case_id(c), float(ok.double().mean()))
        assert bool(U.grad_rays_comparable(c, d).all()), U.grad_case_id(c)
        pos = U.positions(d["origins"].double(), d["dirs"].double(), d["ebins"].double()).reshape(-1, 3)
        m = pos.abs().max(-1).values
        inside += int((m < 1).sum())
        outside += int((m >= 1).sum())
        if c["S"] >= 64 and c["R"] == 5:
            assert int((m < 1).sum()) > 0 and all(int(((pos.abs().argmax(-1) == k) & (m > 1)).sum()) > 0 for k in range(3)), U.grad_case_id(c)
        axes |= {int(k) for k in pos.abs().argmax(-1)[m > 1]}
    assert inside > 0 and outside > 0 and axes == {0, 1, 2}
    assert {c["R"] for c in U.GRAD_CASES} == {1, 5} and {c["S"] for c in U.GRAD_CASES} == {1, 7, 64, 65}
    assert {c["C"] for c in U.GRAD_CASES} == {8, 32} and {len(c["mult"]) for c in U.GRAD_CASES} == {1, 2} and {len(c["base"]) for c in U.GRAD_CASES} == {3, 4}


def test_recorded_deviations_cover_the_cases():
    rec = U.load_bounds()
    assert rec["factor"] == PR.FACTOR == 5.0
    for c in U.GRAD_CASES:
        r = rec["coords_gradient"][U.grad_case_id(c)]
        assert r["seed"] == c["seed"] and r["kept_share"] >= U.KEEP_SHARE
        assert all(0 < r[k] < 1e-5 for k in ("dev32_grad_pts", "dev32_grad_origins", "dev32_grad_dirs"))


def test_three_step_restatement_is_recorded():
    rec = U.load_bounds()["three_steps"]
    dev = U.three_steps_deviation()
    for k in ("rgb", "loss", "param"):
        assert rec["floor"][k] == U.STEP_TOLERANCES[k] and rec["dev32"][k] == pytest.approx(dev[k], rel=0.5), (k, rec["dev32"][k], dev[k])
    rays, _, _ = U.step_rays(256, 20)
    o, d = rays["origins"][128:], rays["directions"][128:]
    t = torch.linspace(0, 30, 200)
    assert float((o[:, None, :] + d[:, None, :] * t[None, :, None]).abs().amax(-1).min()) > 1.0  # those rays never meet the unit cube


def test_backdrop_is_opt_in_and_only_changes_rays_that_leave_the_scene():
    from soccernerfs_amd import synthetic as S

    gen = torch.Generator().manual_seed(0)
    o = torch.rand(4000, 3, generator=gen) * 2 - 1
    o[:, 2] = o[:, 2].abs() * 0.5 + 0.1
    d = torch.nn.functional.normalize(torch.randn(4000, 3, generator=gen), dim=-1)
    t = torch.rand(4000, generator=gen)
    for variant in ("default", "textured"):
        plain, back = S.shade(o, d, t, variant), S.shade(o, d, t, variant, True, True)
        assert torch.equal(plain, S.shade(o, d, t, variant, True, False))
        changed = (plain != back).any(-1)
        assert 0.2 < float(changed.float().mean()) < 0.95 and bool(torch.isfinite(back).all()) and 0 <= float(back.min()) and float(back.max()) <= 1
        sky = torch.stack([0.55 + 0.2 * d[:, 2], 0.7 + 0.15 * d[:, 2], 0.95 * torch.ones_like(d[:, 2])], -1).clamp(0, 1)
        assert bool((plain[changed] == sky[changed]).all())  # only what showed the plain sky changed
    with pytest.raises(ValueError):
        S.shade(o, d, t, "stadium", True, True)


# ---- host refusals: before any launch, so no GPU is needed ----
def _desc(C_=8, n_coords=4):
    from soccernerfs_amd.plane_set import PlaneSet

    return PlaneSet(C_, [[4, 4, 4, 2][:n_coords]], concat=False).desc()


def _coords(mode, contract):
    from soccernerfs_amd import _lib

    c = _lib.Coords()
    c.mode, c.S, c.contract = mode, 1, contract
    return c


def _refused(rc, *words):
    from soccernerfs_amd import _lib

    assert rc != 0
    msg = _lib.lib().snerf_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_contract_field_is_the_old_padding_slot():
    from soccernerfs_amd import _lib

    assert _lib.Coords.contract.offset == 12 and _lib.Coords.contract.size == 4 and _lib.Coords.pts.offset == 16
    assert _lib.Coords().contract == 0
    hdr = open(os.path.join(ROOT, "include", "snerf.h")).read()
    assert "int32_t contract;" in hdr and "snerf_coords.contract" in hdr


@pytest.mark.parametrize("mode,contract,word", [(0, 1, "mode 0"), (1, 2, "must be 0"), (0, 2, "must be 0"), (1, -1, "must be 0")])
def test_kplanes_entries_refuse_bad_contract(mode, contract, word):
    from soccernerfs_amd import _lib

    L, d, co = _lib.lib(), _desc(), _coords(mode, contract)
    null = None
    _refused(L.snerf_kplanes_gather_fwd(C.byref(d), null, C.byref(co), C.c_int64(4), null, null), "kplanes", "contract", word)
    _refused(L.snerf_kplanes_gather_bwd(C.byref(d), null, C.byref(co), C.c_int64(4), null, null, null), "contract", word)
    _refused(L.snerf_kplanes_gather_bwd_fx(C.byref(d), null, C.byref(co), C.c_int64(4), null, null, null), "contract", word)
    _refused(L.snerf_kplanes_gather_bwd_coords(C.byref(d), null, C.byref(co), C.c_int64(4), null, null, null, null, null), "kplanes_gather_bwd_coords", "contract", word)
    _refused(L.snerf_kplanes_sort_samples(C.byref(d), C.byref(co), C.c_int64(4), null, null, null, null), "kplanes_sorted", "contract", word)
    net = _lib.MlpDesc()
    net.d_in, net.hidden, net.n_hidden, net.d_out, net.hidden_act, net.out_act, net.operands = 8, 64, 1, 1, 1, 0, 1
    _refused(L.snerf_kplanes_density_fwd(C.byref(d), null, C.byref(co), C.c_int64(4), C.byref(net), null, null, null, null), "kplanes_density_fwd", "contract", word)
    lv = (_lib.DensityBwdLevel * 2)()
    lv[0].desc, lv[0].coords, lv[0].net, lv[0].N = C.addressof(d), C.addressof(co), C.addressof(net), 4
    _refused(L.snerf_kplanes_density_bwd(lv, 1, null), "kplanes_density_bwd", "contract", word)
    d32 = _desc(32)
    d32.concat = 1
    sig, col = _lib.MlpDesc(), _lib.MlpDesc()
    sig.d_in, sig.hidden, sig.n_hidden, sig.d_out, sig.hidden_act, sig.out_act, sig.operands = 32, 128, 1, 16, 1, 0, 1
    col.d_in, col.hidden, col.n_hidden, col.d_out, col.hidden_act, col.out_act, col.operands = 15, 64, 2, 3, 1, 1, 1
    _refused(L.snerf_kplanes_field_fwd(C.byref(d32), null, C.byref(co), C.c_int64(4), C.byref(sig), null, C.byref(col), null, null, null, null, null, null, null),
             "kplanes_field", "contract", word)


def test_table_encoder_entries_refuse_contract_by_name():
    from soccernerfs_amd import _lib

    L = _lib.lib()
    td = _lib.TgridDesc()
    td.D, td.C, td.L, td.grid_C, td.gridtype = 3, 2, 4, 6, 0
    co = _coords(1, 1)
    times = (C.c_float * 1)(0.5)
    rc = L.snerf_tgrid_encode_fwd(C.byref(td), None, C.byref(co), None, times, 1, C.c_int64(1), None, None)
    _refused(rc, "tgrid", "coords.contract=1", "no scene contraction")


def test_library_that_ignores_contract_is_refused_at_load(tmp_path):
    """snerf_coords.contract added no symbol and no revision: the binding asks the library once whether it refuses contract = 2.  A stub with
    every entry returning 0 (what a library from before the field does for that call) must fail at load with the rebuild message."""
    import subprocess

    from soccernerfs_amd import _lib
    from tests.test_binding_cpu import _cc

    body = [f"int snerf_abi_version(void) {{ return {_lib.ABI_VERSION}; }}", f"int snerf_abi_revision(void) {{ return {_lib.ABI_REVISION}; }}"]
    body += [f"long {name}() {{ return 0; }}" for name in _lib.SIGNATURES if name not in ("snerf_abi_version", "snerf_abi_revision")]
    src, so = tmp_path / "stub.c", tmp_path / "libstub.so"
    src.write_text("\n".join(body) + "\n")
    subprocess.run([_cc(), "-shared", "-fPIC", "-w", "-o", str(so), str(src)], check=True)
    with pytest.raises(RuntimeError, match="predates snerf_coords.contract.*rebuild the library"):
        _lib.bind(str(so))
    assert _lib.lib() is _lib.lib()


def test_unbounded_config_checks_its_planes():
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    for near, far in ((-0.1, 10.0), (2.0, 1.0), (0.5, 0.5)):
        with pytest.raises(ValueError, match="far_plane > near_plane >= 0"):
            KPlanesTrainer(KPlanesTrainConfig(bounded=False, near_plane=near, far_plane=far), 8, "cpu")


def test_defaults_are_unchanged():
    import inspect

    from soccernerfs_amd import ops
    from soccernerfs_amd.trainer import KPlanesTrainConfig

    cfg = KPlanesTrainConfig()
    assert cfg.bounded is True and cfg.far_plane == 1000.0 and cfg.near_plane == 0.0 and cfg.aabb_scale == 1.5
    sig = inspect.signature(ops.generate_rays)
    assert sig.parameters["collider"].default == "aabb" and sig.parameters["far_plane"].default is None
    assert sig.parameters["near_plane"].default == 0.0 and sig.parameters["aabb"].default is None and sig.parameters["training"].default is True
    assert inspect.signature(ops.coords_from_rays).parameters["contract"].default is False
    assert inspect.signature(ops.interpolate_kplanes_rays).parameters["contract"].default is False
    o = torch.zeros(1, 3)
    c = ops.coords_from_rays(o, o, None, torch.zeros(1, 2), [[-1.5] * 3, [1.5] * 3], True)
    assert c.contract == 0 and c.rescale == 1 and c.aabb_max[0] == 1.5
    c = ops.coords_from_rays(o, o, None, torch.zeros(1, 2), None, True, contract=True)
    assert c.contract == 1 and c.mode == 1
    with pytest.raises(ValueError):
        ops.coords_from_rays(o, o, None, torch.zeros(1, 2), None, True)
    idx = torch.zeros(1, 3, dtype=torch.int64)
    for kw in ({"collider": "box"}, {"collider": "near_far"}):  # refused before the device check
        with pytest.raises(ValueError):
            ops.generate_rays(idx, o, o, o, o, o, **kw)


def test_render_command_line_rebuilds_the_unbounded_config():
    spec = importlib.util.spec_from_file_location("snerf_tools_render", os.path.join(ROOT, "tools", "render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--load-dir", "x", "--camera-path-filename", "y"]
    cfg = mod.config_from_args(mod.parse_args(base))
    assert cfg.bounded is True and cfg.far_plane == 1000.0
    cfg = mod.config_from_args(mod.parse_args(base + ["--unbounded", "--far-plane", "64", "--set", "near_plane=0.05"]))
    assert cfg.bounded is False and cfg.far_plane == 64.0 and cfg.near_plane == 0.05
    again = mod.config_from_overrides([f"{k}={v!r}" for k, v in dataclasses.asdict(cfg).items() if k in ("bounded", "far_plane", "near_plane")])
    assert (again.bounded, again.far_plane, again.near_plane) == (False, 64.0, 0.05)
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--far-plane", "64"])

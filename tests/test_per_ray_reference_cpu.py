"""CPU: the float64 references of tests/per_ray_reference.py are made trustworthy before a GPU is involved.

  * each reference reproduces the golden fixtures G7, G8 and G8b at the tolerances tests/test_oracle_golden.py uses for the oracle;
  * the input families have the properties they are built for (tied edges, wide envelopes, depth midpoints off the window edges, exact hits
    in family (d));
  * E32 -- the deviation of the float32 oracle (the KO.* functions on float32 CPU tensors) from the reference, max |got - want| over the
    largest |want| of a case, maximised over the lattice -- is measured for every quantity and written to
    profiles/r10_per_ray_reference_e32.json.  The GPU bounds of tests/test_gpu_per_ray_lattice.py are 5 x these figures: a property of the
    reference program's own arithmetic, measured without the code under test.
"""
import json
import os

import torch

from oracle import kplanes_oracle as KO
from tests import per_ray_reference as PR
from tests.conftest import load_golden

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E32_JSON = os.path.join(_ROOT, "profiles", "r10_per_ray_reference_e32.json")


def close(a, b, rtol=1e-5, atol=1e-6):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    torch.testing.assert_close(a.float(), b.float(), rtol=rtol, atol=atol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the references against the golden fixtures
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_render_reference_reproduces_g7():
    g = load_golden("g7_render")
    w, rgb, eb = g["weights"], g["rgb"], g["ebins"]
    o = PR.render_ref(w, rgb, eb, g["bg"], 0, True)
    close(o["rgb"], g["rgb_random_train"])
    close(PR.render_ref(w, rgb, eb, torch.zeros(3), 2, True)["rgb"], g["rgb_black_train"])
    close(PR.render_ref(w, rgb, eb, torch.ones(3), 2, False)["rgb"], g["rgb_white_eval"])
    close(PR.render_ref(w, rgb, eb, None, 1, True)["rgb"], g["rgb_last_sample_train"])
    close(PR.render_ref(w, rgb, eb, None, 1, False)["rgb"], g["rgb_last_sample_eval"])
    close(o["accumulation"], g["accumulation"][:, 0])
    assert torch.equal(o["median_index"], g["median_index"][:, 0])
    close(o["depth_median"], g["depth_median"][:, 0], atol=1e-7)
    steps = (eb[:, :-1] + eb[:, 1:]) / 2
    close(torch.clip(o["depth_expected"].float(), steps.min(), steps.max()), g["depth_expected"][:, 0])
    close(o["median_rgb"], g["median_rgb"][:, 0], rtol=0, atol=0)


def test_loss_references_reproduce_g8():
    g = load_golden("g8_losses")
    ws = [g[f"w_{i}"] for i in range(3)]
    sb = [g[f"sbins_{i}"] for i in range(3)]
    R, S = ws[2].shape
    total, grads = 0.0, []
    for lvl in range(2):
        v, gp = PR.interlevel_ref(sb[2], ws[2], sb[lvl], ws[lvl], grad_scale=1.0 / (R * S))
        total = total + v.sum() / (R * S)
        grads.append(gp)
    close(total, torch.as_tensor(g["interlevel"]), rtol=1e-5, atol=1e-8)
    close(grads[0], g["grad_w0"], rtol=1e-4, atol=1e-8)
    close(grads[1], g["grad_w1"], rtol=1e-4, atol=1e-8)
    v, gw = PR.distortion_ref(ws[2], sb[2], grad_scale=1.0 / R)
    close(v.mean(), torch.as_tensor(g["distortion"]), rtol=1e-5, atol=1e-8)
    close(gw, g["grad_w2_distortion"], rtol=1e-4, atol=1e-8)


def test_depth_references_reproduce_g8b():
    g = load_golden("g8b_depth")
    R = g["weights"].shape[0]
    case = {"weights": g["weights"], "ebins": g["bins"], "termination_depth": g["termination_depth"], "directions_norm": g["directions_norm"],
            "predicted_depth": g["predicted_depth"]}
    for tag, eucl in (("eucl_s001", True), ("eucl_s02", True), ("z_s02", False)):
        case["sigma"] = float(g["sigma_" + tag])
        v, gw = PR.ds_nerf_depth_ref(case, not eucl, grad_scale=1.0 / R)
        close(v.mean(), torch.as_tensor(g["loss_" + tag]), rtol=1e-6, atol=1e-8)
        close(gw, g["grad_" + tag], rtol=1e-5, atol=1e-9)
    for tag, eucl in (("urf_eucl_s02", True), ("urf_z_s05", False), ("urf_eucl_s001", True)):
        case["sigma"] = float(g["sigma_" + tag])
        v, gw, gp = PR.urf_depth_ref(case, not eucl, grad_scale=1.0 / R)
        close(v.mean(), torch.as_tensor(g["loss_" + tag]), rtol=1e-5, atol=1e-8)
        close(gw, g["grad_" + tag], rtol=1e-5, atol=1e-8)
        close(gp, g["gpred_" + tag], rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the lattice and the input families
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_covers_what_it_promises():
    assert {s for s, _ in PR.LATTICE} == set(PR.SAMPLE_COUNTS) and {r for _, r in PR.LATTICE} == set(PR.RAY_COUNTS)
    for S in PR.SAMPLE_COUNTS:
        assert any(r % 4 for s, r in PR.LATTICE if s == S), S
    for R in PR.RAY_COUNTS:
        assert len({s for s, r in PR.LATTICE if r == R}) >= 3, R
    cases = PR.interlevel_cases()
    assert {(s, sp) for s, sp, *_ in cases} == set(PR.INTERLEVEL_PAIRS)
    assert any(r % 4 for *_, r, _f, _m in cases) and {f for *_, f, _m in cases} == {"a", "b", "c"}
    assert (7, 256) in {(s, sp) for s, sp, _r, f, _m in cases if f == "c"} and (7, 1) in {(s, sp) for s, sp, _r, f, _m in cases if f == "c"}


def test_family_conditions():
    for S, Sp, R, fam, _mode in PR.interlevel_cases():
        case = PR.pipeline_case(R, S, Sp, fam)
        for key, n in (("c_bins", S + 1), ("p_bins", Sp + 1)):
            assert case[key].shape == (R, n) and bool((case[key][:, 1:] >= case[key][:, :-1]).all()), (S, Sp, fam, key)
        if fam == "b":
            assert PR.tied_share(case) >= 0.25, (S, Sp, PR.tied_share(case))
            if S >= 48:
                assert bool((case["c_bins"][:, 1:] == case["c_bins"][:, :-1]).any()), "family (b) is meant to hold zero-width nerf bins"
        if fam == "c" and Sp >= 32 * S:
            assert PR.envelope_width(case) >= 16, (S, Sp, PR.envelope_width(case))
        if S == 1:
            assert bool((case["density"] != 0).all()) and bool((case["weights"] != 0).any())  # the only sample is never zeroed
        elif R * S >= 64:
            assert bool((case["weights"] == 0).any())
    assert PR.envelope_width(PR.pipeline_case(2, 7, 256, "c")) >= 16
    for k in range(len(PR.LATTICE)):
        case = PR.lattice_depth_case(k)
        assert PR.depth_margin(case) > PR.MARGIN
        if case["S"] == 1:
            assert bool((case["density"] != 0).all()) and bool((case["weights"] != 0).any())
    gated = torch.cat([PR.lattice_depth_case(k)["termination_depth"] for k in range(len(PR.LATTICE))])
    assert bool((gated == 0).any()) and bool((gated < 0).any()) and bool((gated > 0).any())


def test_exact_value_families():
    for S in PR.SAMPLE_COUNTS:
        case = PR.exact_render_case(S)
        w = case["weights"]
        cw = torch.cumsum(w.double(), -1)  # dyadic: exact in any order
        idx = PR.median_index_ref(w)
        assert bool((cw[torch.arange(9), idx] == 0.5)[[0, 6]].all()) and int(idx[0]) == 0 and int(idx[6]) == S - 1
        if S >= 4:
            assert [int(idx[r]) for r in (1, 5)] == [1, 3] and float(cw[5, 3]) == 0.5 and float(cw[5, 2]) < 0.5
        assert int(idx[2]) == S - 1 and float(cw[2, -1]) == 0.0 and int(idx[3]) == S - 1 and float(cw[3, -1]) < 0.5
        assert float(cw[4, -1]) > 1.0 or S == 1
        if S > 64:
            assert int(idx[7]) == 64 and float(cw[7, 64]) == 0.5
        if S > 2:
            assert int(idx[8]) == S - 1 and float(cw[8, -1]) == 0.5 and float(cw[8, -2]) < 0.5
        assert torch.equal(KO.median_index(w)[:, 0], idx)  # the oracle agrees on every tie
        d = PR.exact_depth_case(S)
        up, down = PR.edge_hits(d)
        assert up >= 1 and down >= 1, (S, up, down)
        t64 = (d["ebins"][:, :-1].double() + d["ebins"][:, 1:].double()) / 2
        t32 = (d["ebins"][:, :-1] + d["ebins"][:, 1:]) / 2
        assert torch.equal(t64, t32.double())  # the dyadic grid is exact in both precisions
        assert bool((d["termination_depth"] == 0).any()) and bool((d["termination_depth"] < 0).any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# E32: the float32 oracle against the references, over the whole lattice
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bg_for(case, mode):
    return {0: case["bg"], 1: None, 2: case["bg"][0].contiguous()}[mode]


def _oracle_bg(case, mode):
    return "last_sample" if mode == 1 else _bg_for(case, mode)


def _render_e32(E, case):
    w, rgb, eb = case["weights"], case["rgb"], case["ebins"]
    for mode in (0, 1, 2):
        for training in (True, False):
            ref = PR.render_ref(w, rgb, eb, _bg_for(case, mode), mode, training)
            E("render.rgb", KO.render_rgb(rgb, w, _oracle_bg(case, mode), training), ref["rgb"])
    E("render.accumulation", KO.render_accumulation(w)[:, 0], ref["accumulation"])
    steps = (eb[:, :-1] + eb[:, 1:]) / 2
    E("render.depth_expected", torch.sum(w * steps, -1) / (torch.sum(w, -1) + 1e-10), ref["depth_expected"])
    assert torch.equal(KO.median_index(w)[:, 0], ref["median_index"])
    assert torch.equal(KO.render_depth_median(w, eb[:, :-1], eb[:, 1:])[:, 0], ref["depth_median"])
    assert torch.equal(KO.render_median_rgb(rgb, w, False)[:, 0], ref["median_rgb"])


def _render_bwd_e32(E, case, k):
    go, ga, out = PR.upstream(case, k)
    for mode in (0, 2):
        bg = _bg_for(case, mode)
        for use_acc in (False, True):
            w, rgb = case["weights"].clone().requires_grad_(True), case["rgb"].clone().requires_grad_(True)
            tot = (KO.render_rgb(rgb, w, bg, True) * go).sum()
            if use_acc:
                tot = tot + (KO.render_accumulation(w)[:, 0] * ga).sum()
            tot.backward()
            gw, grgb = PR.render_bwd_ref(case["weights"], case["rgb"], bg, mode, go, ga if use_acc else None)
            E("render_bwd.g_weights", w.grad, gw)
            E("render_bwd.g_rgb", rgb.grad, grgb)
            pre = PR.prefill_like(gw, "render_bwd", k, mode, use_acc)
            E("render_bwd.g_weights", pre + w.grad, PR.render_bwd_ref(case["weights"], case["rgb"], bg, mode, go, ga if use_acc else None, pre)[0])
        scale = 2 * 0.7 / (3 * case["R"])
        w, rgb = case["weights"].clone().requires_grad_(True), case["rgb"].clone().requires_grad_(True)
        d32 = out - case["target"]
        (KO.render_rgb(rgb, w, bg, True) * (d32 * scale)).sum().backward()
        gw, grgb, sq = PR.render_mse_bwd_ref(case["weights"], case["rgb"], bg, mode, out, case["target"], scale)
        E("render_mse_bwd.g_weights", w.grad, gw)
        E("render_mse_bwd.g_rgb", rgb.grad, grgb)
        E("render_mse_bwd.sqerr", (d32 * d32).sum(-1), sq)


def _distortion_e32(E, case, k):
    scale = 1e-3 / case["R"]
    w = case["weights"].clone().requires_grad_(True)
    v32 = KO.lossfun_distortion(case["c_bins"], w)
    v32.sum().backward()
    v, g = PR.distortion_ref(case["weights"], case["c_bins"], scale)
    E("distortion.value", v32, v)
    E("distortion.g_weights", w.grad * scale, g)
    pre = PR.prefill_like(g, "distortion", k)
    E("distortion.g_weights", pre + w.grad * scale, PR.distortion_ref(case["weights"], case["c_bins"], scale, pre)[1])


def _interlevel_e32(E, case, w_nerf, tag=""):
    scale = 1.0 / (case["R"] * case["S"])
    wp = case["w_prop"].clone().requires_grad_(True)
    v32 = KO.lossfun_outer(case["c_bins"], w_nerf, case["p_bins"], wp).sum(-1)
    v32.sum().backward()
    v, g = PR.interlevel_ref(case["c_bins"], w_nerf, case["p_bins"], case["w_prop"], scale)
    E("interlevel.value", v32, v)
    E("interlevel.g_wprop", wp.grad * scale, g)
    v64, g64 = PR.interlevel_ref(case["c_bins"], w_nerf, case["p_bins"], case["w_prop"], scale, plain_float64=True)
    E("interlevel.value.vs_plain_float64", v32, v64)
    E("interlevel.g_wprop.vs_plain_float64", wp.grad * scale, g64)


def _depth_e32(E, case, k):
    R = case["R"]
    scale = 0.5 / R
    for use_norm in (False, True):
        w = case["weights"].clone().requires_grad_(True)
        args = (case["ebins"], case["termination_depth"], case["sigma"], case["directions_norm"], not use_norm)
        (KO.depth_loss(w, *args) * R).backward()
        v32 = torch.stack([KO.depth_loss(case["weights"][r:r + 1], case["ebins"][r:r + 1], case["termination_depth"][r:r + 1], case["sigma"],
                                         case["directions_norm"][r:r + 1], not use_norm) for r in range(R)])
        v, g = PR.ds_nerf_depth_ref(case, use_norm, scale)
        E("ds_nerf.value", v32, v)
        E("ds_nerf.g_weights", w.grad * scale, g)
        pre = PR.prefill_like(g, "ds_nerf", k, use_norm)
        E("ds_nerf.g_weights", pre + w.grad * scale, PR.ds_nerf_depth_ref(case, use_norm, scale, pre)[1])
        w = case["weights"].clone().requires_grad_(True)
        pd = case["predicted_depth"].clone().requires_grad_(True)
        (KO.urf_depth_loss(w, case["ebins"], case["termination_depth"], pd, case["sigma"], case["directions_norm"], not use_norm) * R).backward()
        v32 = torch.stack([KO.urf_depth_loss(case["weights"][r:r + 1], case["ebins"][r:r + 1], case["termination_depth"][r:r + 1],
                                             case["predicted_depth"][r:r + 1], case["sigma"], case["directions_norm"][r:r + 1], not use_norm)
                           for r in range(R)])
        v, g, gp = PR.urf_depth_ref(case, use_norm, scale)
        E("urf.value", v32, v)
        E("urf.g_weights", w.grad * scale, g)
        E("urf.g_pred", pd.grad * scale, gp)
        pre = PR.prefill_like(g, "urf", k, use_norm)
        E("urf.g_weights", pre + w.grad * scale, PR.urf_depth_ref(case, use_norm, scale, pre)[1])


def _ray_train_e32(E, case):
    R = case["R"]
    go_scale, dist_scale = 2.0 / (3 * R), 1e-3 / R
    dens = case["density"].clone().requires_grad_(True)
    eb = case["ebins"]
    w = KO.get_weights(eb[:, 1:] - eb[:, :-1], dens)
    w.retain_grad()
    rgb = case["rgb"].clone().requires_grad_(True)
    out = KO.render_rgb(rgb, w, case["bg"], True)
    dist = KO.lossfun_distortion(case["c_bins"], w)
    d = out - case["target"]
    (go_scale / 2 * (d * d).sum() + dist_scale * dist.sum()).backward()
    ref = PR.ray_train_ref(case, go_scale, dist_scale)
    E("ray_train.weights", w, ref["weights"])
    E("ray_train.rgb_out", out, ref["rgb_out"])
    E("ray_train.acc", KO.render_accumulation(w)[:, 0], ref["acc"])
    E("ray_train.dist_rays", dist, ref["dist_rays"])
    E("ray_train.g_density", dens.grad, ref["g_density"])
    E("ray_train.g_weights", w.grad, ref["g_weights"])
    E("ray_train.g_rgb", rgb.grad, ref["g_rgb"])
    E("ray_train.sqerr", (d * d).sum(-1), ref["sqerr"])


def measure_e32():
    worst, where = {}, {}

    def run(label):
        def E(name, got, want):
            d = PR.deviation(got, want)
            if d >= worst.get(name, -1.0):
                worst[name], where[name] = d, label
        return E

    for k, (S, R) in enumerate(PR.LATTICE):
        case = PR.pipeline_case(R, S, S, "a")
        E = run(f"S={S} R={R} (a)")
        _render_e32(E, case)
        _render_bwd_e32(E, case, k)
        _distortion_e32(E, case, k)
        _depth_e32(E, PR.lattice_depth_case(k), k)
        if S in (48, 64, 320):
            _ray_train_e32(E, case)
    for S, R, Sp, fam in PR.RENDER_FAMILY_CASES:
        _render_e32(run(f"S={S} R={R} ({fam})"), PR.pipeline_case(R, S, Sp, fam))
    for S in PR.SAMPLE_COUNTS:
        _render_e32(run(f"S={S} (d)"), PR.exact_render_case(S))
        _depth_e32(run(f"S={S} (d)"), PR.exact_depth_case(S), 1000 + S)
    for S, Sp, R, fam, mode in PR.interlevel_cases():
        case = PR.pipeline_case(R, S, Sp, fam)
        _interlevel_e32(run(f"S={S} Sp={Sp} R={R} ({fam}, {mode})"), case, case["weights"] if mode == "natural" else PR.scaled_nerf_weights(case))
    return worst, where


def _two_digits(v):
    return float(f"{v:.1e}")


def test_e32_of_the_float32_oracle_over_the_lattice():
    """Measures E32 for every quantity and writes profiles/r10_per_ray_reference_e32.json (two digits: the last ones move with the host's
    SIMD summation order and libm).  The table the GPU bounds are computed from (tests/test_gpu_per_ray_lattice.py: E32) is that measurement
    rounded up; here it is held to it loosely, as a sanity limit on both sides: the measurement may not exceed the table by more than a
    quarter (the table would understate the oracle's error) nor fall below a third of it (the table would be inflated)."""
    from tests.test_gpu_per_ray_lattice import E32

    worst, where = measure_e32()
    try:
        os.makedirs(os.path.dirname(E32_JSON), exist_ok=True)
        json.dump({"metric": "max |float32 oracle - reference| / max |reference| per case, maximised over the lattice",
                   "e32": {k: _two_digits(worst[k]) for k in sorted(worst)}, "worst_case": {k: where[k] for k in sorted(where)}},
                  open(E32_JSON, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    for name, v in sorted(worst.items()):
        print(f"E32 {name:40s} {v:.3e}   at {where[name]}")
    measured = {k for k in worst if not k.endswith("vs_plain_float64")}
    assert measured == set(E32), measured ^ set(E32)
    for name in sorted(measured):
        assert E32[name] / 3 <= worst[name] <= 1.25 * E32[name], (name, worst[name], E32[name])
    # the interlevel gradient: plain float64 is the wrong yardstick, the float32-rounded w_outer the right one
    assert worst["interlevel.g_wprop.vs_plain_float64"] > 1e-2 > 1e-5 > worst["interlevel.g_wprop"]
    assert worst["interlevel.value.vs_plain_float64"] < 1e-5

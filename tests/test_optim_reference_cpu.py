"""CPU: the reference side of the optimiser-sweep tests (tests/optim_reference.py) is itself pinned -- against oracle/kplanes_oracle.py's plane
losses under autograd, against torch.optim.Adam in float64, and against the committed yardsticks (profiles/r16_optim_deviations.json)."""
import numpy as np
import pytest
import torch

from oracle import kplanes_oracle as KO
from tests import optim_reference as OR

SIX_PLANE = [c for c in OR.PLANE_CASES if len(c["base"]) == 4]
SMALL = [c for c in OR.PLANE_CASES if OR.plane_layout(c["C"], OR.resolutions(c["base"], c["mult"]))[1] <= 16000]


def test_deviation_file_holds_every_case():
    b = OR.load_bounds()
    assert b["factor"] == OR.FACTOR == 5.0
    assert set(b["planes"]) == {c["case_id"] for c in OR.PLANE_CASES} and len(OR.PLANE_CASES) == 40
    assert set(b["flat"]) == {c["case_id"] for c in OR.FLAT_CASES} and len(b["flat"]) == len(OR.FLAT_CASES)
    assert set(b["tv"]) == {c["case_id"] for c in OR.TV_CASES} and len(b["tv"]) == len(OR.TV_CASES)
    for c in OR.PLANE_CASES:
        r = b["planes"][c["case_id"]]
        assert r["seed"] == c["seed"] and all(np.isfinite(r[k]) for k in ("dev32_p_out", "dev32_m", "dev32_v", "dev32_reg_grad")) and len(r["dev32_values"]) == 3
    assert all(i in b["planes"] for i in OR.RANGE_CASE_IDS)


def test_lattice_covers_every_axis_value():
    cs = OR.PLANE_CASES
    assert {c["C"] for c in cs} == {8, 16, 32} and {len(c["mult"]) for c in cs} == {1, 2, 3} and {len(c["base"]) for c in cs} == {3, 4}
    assert {c["params"] for c in cs} == {"random", "time_one", "quarter_one", "constant"} and {c["grad"] for c in cs} == {"dense", "half_zero", "zero", "wide"}
    assert {c["coefs"] for c in cs} == set(OR.COEFS) and {c["state"] for c in cs} == set(OR.STATES)
    assert {c["grad_scale"] for c in cs} == {1.0, 0.5} and {c["zero_grad"] for c in cs} == {0, 1}
    for c in cs:  # the reference divides by zero below these
        assert min(c["base"][:3]) >= 2 and (len(c["base"]) == 3 or c["base"][3] >= 3)
    assert {c["n"] for c in OR.FLAT_CASES} == set(OR.FLAT_NS) and {c["eps"] for c in OR.FLAT_CASES} == set(OR.FLAT_EPS)
    assert {c["in_place"] for c in OR.FLAT_CASES if c["n"] == 3} == {0, 1}
    assert {(c["rows"], c["grid_C"]) for c in OR.TV_CASES} == {(r, g) for r in (8, 24) for g in (4, 6, 34, 66)}
    assert any(c["cols"] == (0, c["grid_C"] - 1) for c in OR.TV_CASES) and any(c["cols"][0] // 4 == c["cols"][1] // 4 for c in OR.TV_CASES)


def test_layout_equals_the_plane_set():
    from soccernerfs_amd.plane_set import PlaneSet

    for c in (OR.PLANE_CASES[7], OR.PLANE_CASES[33]):
        d = OR.make_case(c)
        ps = PlaneSet(c["C"], d["res"], concat=True)
        assert ps.numel == d["n"] and [o for s in ps.offsets for o in s] == [e[2] for e in d["layout"]]
        with torch.no_grad():
            ps.planes.copy_(d["p"])
        for a, b in zip(ps.to_reference(), OR.to_grids(d["p"], c["C"], d["res"])):
            assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("c", SIX_PLANE[:20], ids=lambda c: c["case_id"])
def test_float64_restatement_equals_the_oracle_losses(c):
    d = OR.make_case(c)
    coefs = OR.COEFS["big"]  # every term, whatever the case's own coefficients
    vals, grad = OR.reg_values_and_grad(d["p"].double(), c["C"], d["res"], coefs)
    x = d["p"].double().requires_grad_(True)
    grids = OR.to_grids(x, c["C"], d["res"])
    want = [KO.space_tv_loss(grids), KO.time_smoothness_loss(grids), KO.sparse_transients_loss(grids)]
    (g,) = torch.autograd.grad(sum(OR.f32(k) * w for k, w in zip(coefs, want)), x)
    torch.testing.assert_close(vals, torch.stack([w.detach() for w in want]), rtol=1e-13, atol=0)
    torch.testing.assert_close(grad, g, rtol=1e-12, atol=1e-18)


def test_three_plane_sets_have_no_time_terms():
    c = OR.PLANE_CASES[33]
    d = OR.make_case(c)
    vals, grad = OR.reg_values_and_grad(d["p"].double(), c["C"], d["res"], (0.0, 0.7, 1.1))
    assert float(vals[0]) > 0 and float(vals[1]) == 0.0 and float(vals[2]) == 0.0 and float(grad.abs().max()) == 0.0
    # every one of the three planes takes the 2-D total variation: sums and divisors by hand
    by_hand = 0.0
    for planes in OR.to_grids(d["p"].double(), c["C"], d["res"]):
        assert len(planes) == 3
        for t in planes:
            H, W = t.shape[2], t.shape[3]
            by_hand += float(((t[..., 1:, :] - t[..., :-1, :]) ** 2).sum()) / (c["C"] * (H - 1) * W)
            by_hand += float(((t[..., :, 1:] - t[..., :, :-1]) ** 2).sum()) / (c["C"] * H * (W - 1))
    assert float(vals[0]) == pytest.approx(by_hand, rel=1e-12)


@pytest.mark.parametrize("state", ["zero1", "rand3", "rand30000"])
def test_float64_adam_equals_torch_adam_over_three_steps(state):
    gen = torch.Generator().manual_seed(7)
    n = 513
    kind, step0 = OR.STATES[state]
    p = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1)
    m, v = (x.double() for x in OR.random_state(n, gen, kind))
    for eps in OR.FLAT_EPS:
        q = torch.nn.Parameter(p.clone())
        opt = torch.optim.Adam([q], lr=OR.f32(OR.LR), betas=(OR.BETA1, OR.BETA2), eps=OR.f32(eps))
        opt.state[q] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        pr, mr, vr = p.clone(), m.clone(), v.clone()
        for k in range(3):
            g = OR.signed_magnitudes(n, gen, ("dense", "half_zero", "wide")[k]).double()
            q.grad = g.clone()
            opt.step()
            pr, mr, vr, dropped = OR.adam(pr, g, mr, vr, step0 + k, eps=eps)
            assert dropped == 0
        # adam() rounds lr / bc1 and 1 / sqrt(bc2) to float as the kernels' host side does: 6e-8 each on every step's update, not on p
        # torch forms m by lerp and v by addcmul: double roundings apart, absolute where m's two terms cancel
        torch.testing.assert_close(mr, opt.state[q]["exp_avg"], rtol=1e-13, atol=1e-16 * float(mr.abs().max()))
        torch.testing.assert_close(vr, opt.state[q]["exp_avg_sq"], rtol=1e-13, atol=0)
        assert OR.rel_dev(pr - p, q.detach() - p) < 3 * 2.0 ** -23  # three steps' updates may cancel in an element: relative to the largest


def test_adam_drops_and_counts_non_finite_elements():
    g = torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), 0.5], dtype=torch.float64)
    p, m, v = torch.ones(5, dtype=torch.float64), torch.full((5,), 0.1, dtype=torch.float64), torch.full((5,), 0.01, dtype=torch.float64)
    po, mo, vo, dropped = OR.adam(p, g, m, v, 3)
    assert dropped == 3 and bool(torch.isfinite(po).all())
    assert torch.equal(mo[1:4], OR.BETA1 * m[1:4]) and torch.equal(vo[1:4], OR.BETA2 * v[1:4])


def test_abi_beta_deviation_is_pinned():
    """The kernels receive float betas and form 1.f - b2 = 0.0009999871 where torch.optim.Adam given the decimal 0.999 forms 0.001 in double: 1.29e-5
    (relative) on v and up to half of that on the update.  A property of the float ABI, recorded and pinned, not an error of the kernels."""
    rec = OR.load_bounds()["abi_beta"]
    one_minus = float(np.float32(1.0) - np.float32(0.999))
    assert one_minus == 1.0 - OR.BETA2 == rec["one_minus_beta2_float_abi"]  # 1.f - b2 is exact in float
    assert abs(one_minus - 0.0009999871) < 1e-10
    assert abs(rec["rel_difference_one_minus_beta2"] - 1.29e-5) < 1e-7
    worst_v, worst_u = 0.0, 0.0
    for c in SMALL:
        d = OR.make_case(c)
        a, b = OR.planes_step(d, torch.float64, b1=0.9, b2=0.999), OR.planes_step(d, torch.float64)
        p = d["p"].double()
        worst_v, worst_u = max(worst_v, OR.rel_dev(a["v"], b["v"])), max(worst_u, OR.rel_dev(a["p_out"] - p, b["p_out"] - p))
    print(f"abi beta: v {worst_v:.3e} (recorded {rec['max_rel_change_v']:.3e}), update {worst_u:.3e} (recorded {rec['max_rel_change_update']:.3e})")
    assert 0 < worst_v <= 2 * rec["max_rel_change_v"] and 0 < worst_u <= 2 * rec["max_rel_change_update"]
    assert rec["max_rel_change_v"] < 2e-5  # and the record itself is the 1.29e-5 of 1 - beta2, not something larger


def test_yardsticks_reproduce_on_small_cases():
    """tools/measure_optim_deviations.py regenerates the committed figures (same seeds, same torch CPU arithmetic up to its vector width)."""
    b = OR.load_bounds()["planes"]
    for c in SMALL[:8]:
        d = OR.make_case(c)
        r64, r32 = OR.planes_step(d, torch.float64), OR.planes_step(d, torch.float32)
        for k in ("p_out", "m", "v", "reg_grad"):
            now, rec = OR.rel_dev(r32[k], r64[k]), b[c["case_id"]][f"dev32_{k}"]
            assert (now == 0.0) == (rec == 0.0) and now <= 2 * rec and rec <= 2 * now, (c["case_id"], k, now, rec)


def test_value_summation_bound_counts_the_tree():
    assert OR.value_summation_bound(1, 1024) == pytest.approx(13 * OR.U32, rel=1e-5)
    assert OR.value_summation_bound(2049, 1024) == pytest.approx(15 * OR.U32, rel=1e-5)


@pytest.mark.parametrize("c", OR.tile_cases(), ids=lambda c: c["case_id"])
def test_tile_cases_are_well_conditioned_in_float32_alone(c):
    """The tile passes' cases (tests/test_gpu_tile_adam_oracle.py), judged with the float32 ORACLE alone: it touches exactly the entries the float64
    oracle touches, and in the zero-state step the share of touched entries whose gradient lies below GRAD_RESOLVED x its own largest absolute error
    (where the sign Adam's first step follows is not determined in float32) stays under the cap.  The committed yardsticks are reproduced."""
    rec = OR.load_bounds()["tiles"][c["case_id"]]
    d = OR.make_tile_case(c)
    assert bool(OR.well_placed(d["x"], OR._level_scales(c)).all()) and float(d["v"].min()) >= 1e-8 and float(d["gout"].abs().min()) >= 0.5e-3 * (1 - 1e-6)
    assert set(rec) - {"seed", "B", "table_shape"} == {OR.tile_key(tv, st) for tv, st in OR.tile_variants(c)}
    for tv, st in OR.tile_variants(c):
        now, was = OR.tile_deviations(d, tv, st), rec[OR.tile_key(tv, st)]
        assert now["same_touched_set_in_float32"] and was["same_touched_set_in_float32"] and now["touched"] == was["touched"] > 0
        if st == "zero":
            print(f"{c['case_id']} {OR.tile_key(tv, st)} unresolved share {now['unresolved_share']:.4f} (cap {OR.UNRESOLVED_CAP})")
            assert now["unresolved_share"] < OR.UNRESOLVED_CAP and was["unresolved_share"] < OR.UNRESOLVED_CAP
        for k in ("dev32_m", "dev32_v", "dev32_p_out", "grad_abs_err32"):
            assert 0 < now[k] <= 2 * was[k] and was[k] <= 2 * now[k], (k, now[k], was[k])


def test_tile_gradient_has_the_tv_term_of_the_old_table():
    c = OR.tile_cases()[1]
    d = OR.make_tile_case(c)
    a, b = d["tv_cols"]
    diff = OR.tile_gradient(d, torch.float64, True) - OR.tile_gradient(d, torch.float64, False)
    s = OR.f32(OR.TV_WEIGHT) * torch.sign(d["table"][:, a].double() - d["table"][:, b].double()) / d["shape"][0]
    want = torch.zeros(d["shape"], dtype=torch.float64)
    want[:, a], want[:, b] = s, -s
    torch.testing.assert_close(diff, want, rtol=1e-9, atol=1e-18)

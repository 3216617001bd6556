"""CPU: pins tests/sampler_reference.py, the yardstick of tests/test_gpu_sampler_lattice.py.

  * the float32 restatement equals oracle.kplanes_oracle bit for bit -- pdf_sample (cdf, indices, bins) and spacing_to_euclidean directly,
    spaced_bins and pdf_u given ATen's per-element linspace formula (the one a GPU evaluates and csrc/ray_ops.hip restates): torch.linspace on
    the CPU is vectorised (base + step * lane) and differs from that formula in the last ulp, which is measured and asserted here;
  * it reproduces the indices of the committed fixtures G4 a-d and G4e;
  * every generator precondition holds (family X exact in float32 and float64, with its shares of u on knots and of zero-width bins; P and Z
    independent of the order of summation; A well conditioned);
  * E32 -- the float32 restatement's deviation from the float64 reference per bounded quantity -- is measured over the lattice, and the table
    sampler_reference.E32 (the GPU bounds are 5 x it) is held to the measurement and to profiles/r30_sampler_reference_e32.json.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import kplanes_oracle as KO
from tests import sampler_reference as SR
from tests.conftest import load_golden

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E32_JSON = os.path.join(_ROOT, "profiles", "r30_sampler_reference_e32.json")
PAIRS = SR.resample_pairs()
T = torch.from_numpy
ULP1 = 2.0 ** -24  # one ulp of a float32 in [0.5, 1): the largest spacing of a bin edge or of u below 1


def _formula_linspace(start, end, steps, **kw):
    """torch.linspace as ATen defines it per element (what a GPU evaluates)."""
    return T(SR.linspace(np.float32(start), np.float32(end), steps))


def test_lattice_covers_what_it_promises():
    assert 150 <= len(PAIRS) <= 400
    for c in SR.COUNTS:
        as_sp = {s for sp, s, _ in PAIRS if sp == c}
        as_s = {sp for sp, s, _ in PAIRS if s == c}
        for partners in (as_sp, as_s):
            assert partners & set(SR.SMALL) and partners & set(SR.LARGE), (c, sorted(partners))
    have = {(sp, s) for sp, s, _ in PAIRS}
    assert set(SR.PRODUCTION_PAIRS + SR.FIXTURE_PAIRS) <= have
    assert {r for *_, r in PAIRS} == set(SR.RAY_COUNTS)
    for r in SR.RAY_COUNTS:  # every R with small and large sizes
        sizes = {sp for sp, _, rr in PAIRS if rr == r} | {s for _, s, rr in PAIRS if rr == r}
        assert sizes & set(SR.SMALL) and sizes & set(SR.LARGE), r
    sc = SR.spaced_cases()
    assert {s for s, _ in sc} >= set(SR.COUNTS)
    assert any(r * (s + 1) % 256 == 0 for s, r in sc) and any(r * (s + 1) % 256 != 0 and r * (s + 1) > 256 for s, r in sc)
    assert {s for s, _ in SR.WEIGHT_CASES} >= set(SR.COUNTS) and {r for _, r in SR.WEIGHT_CASES} == set(SR.RAY_COUNTS)
    assert all((s + 1) & s == 0 for s in SR.POW2_S)


def test_cpu_linspace_is_within_an_ulp_of_the_per_element_formula():
    """How far torch.linspace on the CPU is from the symmetric-halves formula, for every edge count 2 ... 321: never more than one ulp, on
    linspace(0, 1, n) and on u's linspace(0, 1 - 1 / n, n); and for which n the kernel's float32 end 1 - 1 / n differs from the reference
    program's, which rounds the double 1.0 - 1.0 / n once (one ulp, four values of n)."""
    worst01 = worst_u = 0.0
    n01 = nu = 0
    ends = []
    for n in range(2, 322):
        a, b = SR.linspace(0, 1, n), torch.linspace(0, 1, n).numpy()
        worst01, n01 = max(worst01, float(np.abs(a.astype(np.float64) - b).max())), n01 + int((a != b).sum())
        end_ref = np.float32(1.0 - 1.0 / n)
        a, b = SR.linspace(0, end_ref, n), torch.linspace(0.0, 1.0 - 1.0 / n, n).numpy()
        worst_u, nu = max(worst_u, float(np.abs(a.astype(np.float64) - b).max())), nu + int((a != b).sum())
        end_kernel = np.float32(1) - np.float32(1) / np.float32(n)
        if end_kernel != end_ref:
            assert abs(float(end_kernel) - float(end_ref)) <= ULP1
            ends.append(n)
    print(f"torch.linspace (CPU) against the formula: {n01} elements of linspace(0, 1, n) differ (max {worst01:.3e}), {nu} of u's (max {worst_u:.3e}); "
          f"the float32 end differs from the rounded double end at n = {ends}")
    assert worst01 <= ULP1 and worst_u <= ULP1
    assert ends == [3, 11, 31, 251]
    for n in range(2, 9):  # short ranges take ATen's scalar path: equal
        assert np.array_equal(SR.linspace(0, 1, n), torch.linspace(0, 1, n).numpy())


@pytest.mark.parametrize("kind", ["uniform", "piecewise"])
def test_spaced_restatement_equals_the_oracle(kind, monkeypatch):
    """Restatement (a) against KO.spaced_bins and KO.spacing_to_euclidean on every spaced_bins case, t_rand None, [R, 1] and [R, S + 1]: bit
    for bit given the per-element linspace; within one ulp of an edge with the CPU's own."""
    for S, R in SR.spaced_cases():
        rng = SR._rng("spaced_cpu", S, R)
        near = (rng.random(R) * 0.5 + 0.05).astype(np.float32)
        far = (near + 2.0 + rng.random(R) * 4.0).astype(np.float32)
        full = rng.random((R, S + 1)).astype(np.float32)
        for t_rand in (None, full[:, :1].copy(), full):
            mine = SR.spaced_bins(R, S, t_rand)
            plain = KO.spaced_bins(R, S, None if t_rand is None else T(t_rand)).numpy()
            # (jittered: lower and upper each move by an ulp at most, the edge between them by that and one more rounding)
            assert float(np.abs(mine.astype(np.float64) - plain).max()) <= (ULP1 if t_rand is None else 2 * ULP1), (S, R)
            with monkeypatch.context() as m:
                m.setattr(torch, "linspace", _formula_linspace)
                patched = KO.spaced_bins(R, S, None if t_rand is None else T(t_rand)).numpy()
            assert np.array_equal(mine, patched), (S, R, None if t_rand is None else t_rand.shape)
            want = KO.spacing_to_euclidean(T(mine), T(near)[:, None], T(far)[:, None], kind).numpy()
            assert np.array_equal(SR.to_euclidean(mine, near, far, kind), want), (S, R, kind)
    # both branches of the piecewise spacing and of its inverse were taken
    assert near.min() < 1 < far.max()


def test_pdf_u_restatement_equals_the_oracle(monkeypatch):
    """u per :316-327: bit for bit given the per-element linspace, except at the four edge counts whose float32 end differs (one ulp there)."""
    for S in sorted(set(SR.COUNTS) | set(SR.POW2_S) | {2, 10, 30, 250, 7, 48}):
        R = 3
        rand = SR._rng("u", S).random((R, S + 1)).astype(np.float32)
        for r in (None, rand[:, :1].copy(), rand):
            mine = SR.pdf_u(R, S, r)
            with monkeypatch.context() as m:
                m.setattr(torch, "linspace", _formula_linspace)
                want = KO.pdf_u(R, S, None if r is None else T(r)).numpy()
            if S + 1 in (3, 11, 31, 251):
                assert float(np.abs(mine.astype(np.float64) - want).max()) <= ULP1, S
            else:
                assert np.array_equal(mine, want), S
            assert float(np.abs(mine.astype(np.float64) - KO.pdf_u(R, S, None if r is None else T(r)).numpy()).max()) <= 2 * ULP1, S


def _equals_oracle(case, label):
    u = SR.case_u(case)
    for kind in ("uniform", "piecewise"):
        mine = SR.reference(case, kind)
        w = SR.case_weights(case)
        bins, inds, cdf = KO.pdf_sample(T(w), T(case["sbins_prev"]), T(u), case["histogram_padding"], case["eps"])
        assert np.array_equal(mine["cdf"], cdf.numpy()), label
        assert np.array_equal(mine["inds"], inds.numpy()), label
        assert np.array_equal(mine["sbins"], bins.numpy()), label
        eb = KO.spacing_to_euclidean(bins, T(case["nears"])[:, None], T(case["fars"])[:, None], kind).numpy()
        assert np.array_equal(mine["ebins"], eb), label
        assert np.array_equal(mine["inds"], np.stack([np.searchsorted(c, x, side="right") for c, x in zip(mine["cdf"], u)])), label


def test_pdf_restatement_equals_the_oracle_bit_for_bit():
    """Restatement (b) against KO.pdf_sample on the whole lattice: families P (all u modes), X (both paddings), Z; cdf, indices, bins, and the
    indices against numpy's searchsorted(side="right") as well."""
    n = 0
    for k, (Sp, S, R) in enumerate(PAIRS):
        mode, cols = ((0, None), (1, 1), (1, S + 1), (2, None))[k % 4]
        case = SR.pipeline_case(R, Sp, S, mode, cols)
        assert SR.prefix_sums_off_midpoints(case)
        _equals_oracle(case, ("P", Sp, S, R))
        _equals_oracle(SR.exact_case(R, Sp, S, (0, 1, 2, 4)[k % 4], 0), ("X", Sp, S, R))
        n += 2
    for which in SR.DEGENERATE:
        for Sp, S, R in ((1, 1, 1), (3, 2, 5), (64, 65, 4), (320, 320, 133), (257, 1, 2)):
            case = SR.degenerate_case(which, R, Sp, S)
            assert SR.prefix_sums_off_midpoints(case)
            _equals_oracle(case, ("Z", which, Sp, S, R))
            n += 1
    assert n > 300


@pytest.mark.parametrize("name,tags", [("g4_pdf", "abcd"), ("g4e_pdf_preset", "ab")])
def test_pdf_restatement_reproduces_the_fixtures(name, tags):
    """G4 a-d and G4e (the reference program's own PDFSampler): every index equal, the bins within the 5e-6 that its torch.sum association
    order, amplified by the inverse cdf, moves them (tests/test_gpu_ray_ops.py)."""
    g = load_golden(name)
    for tag in tags:
        w, prev, rand = g[f"{tag}_weights"], g[f"{tag}_prev_sbins"], g[f"{tag}_rand"]
        R, S = w.shape[0], rand.shape[1] - 1
        u = KO.pdf_u(R, S, rand).numpy()
        mine = SR.pdf_sample(w.numpy(), prev.numpy(), u)
        assert np.array_equal(mine["inds"], g[f"{tag}_inds"].long().numpy()), (name, tag)
        assert float(np.abs(mine["sbins"] - g[f"{tag}_new_sbins"].numpy()).max()) <= 5e-6
        # u as the restatement forms it differs from the oracle's only in the last ulp
        assert float(np.abs(SR.pdf_u(R, S, rand.numpy()).astype(np.float64) - u).max()) <= 2 * ULP1


def test_exact_family_preconditions():
    """Family X: assert_exact on every case the GPU file runs; per case with at least 16 new edges and 8 bins the shares of u on a knot and (with
    histogram_padding 0) of zero-width pdf bins are at least 10 %, and so are the shares over the whole family."""
    knots, zeros = [], []
    for k, (Sp, S, R) in enumerate(PAIRS):
        for p in (0, (1, 2, 4)[k % 3]):
            case = SR.exact_case(R, Sp, S, p, 0)
            on_knot, zero_width = SR.assert_exact(case)
            u = case["u"]
            if S + 1 >= 6:
                for r in range(R):  # per ray: 0, 1, a value above the last cdf entry, a knot, a midpoint
                    assert {0.0, 1.0, 1.25} <= set(u[r].tolist()), (Sp, S, R, r)
            knots.append(on_knot)
            if S + 1 >= 16:
                assert on_knot >= 0.10, (Sp, S, R, p, on_knot)
            if p == 0:
                zeros.append(zero_width)
                if Sp >= 8:
                    assert zero_width >= 0.10, (Sp, S, R, zero_width)
                    dup = (np.diff(case["sbins_prev"], axis=-1) == 0).mean()
            else:
                assert zero_width == 0.0
    assert np.mean(knots) >= 0.10 and np.mean(zeros) >= 0.10
    print(f"family X: u on a knot {np.mean(knots):.3f}, zero-width pdf bins (padding 0) {np.mean(zeros):.3f}, repeated edges in the last case {dup:.3f}")
    hit = 0
    for S in SR.POW2_S:
        for mode, cols in ((1, 1), (1, S + 1), (2, None)):
            for Sp in (1, 3, 64, 65, 257, 320):
                on_knot, _ = SR.assert_exact(SR.exact_case(5, Sp, S, 0, mode, cols))
                hit += on_knot > 0
    assert hit >= 30  # u formed in the kernel lands on knots as well (rand = 0 on the strata edges)


def test_order_independence_guard_bites():
    """sums_order_independent accepts rows whose subset sums are exact and rejects a row with an inexact prefix sum on a rounding midpoint."""
    ok = np.array([[0.25, 0.5, 2.0 ** -24, 1.0]], dtype=np.float32)  # 0.75 + 2^-24 is a float32 midpoint, and exact in float64
    assert SR.sums_order_independent(ok).all()
    big = np.float32(2.0 ** 60)
    bad = np.array([[big, np.float32(2.0 ** 36), 1.0]], dtype=np.float32)  # 2^60 + 2^36 is a midpoint of float32; + 1 is not exact in float64
    assert not SR.sums_order_independent(bad).all()
    assert SR.sums_order_independent(np.array([[big, np.float32(2.0 ** 37), 1.0]], dtype=np.float32)).all()


def test_inexact_family_is_well_conditioned():
    for case in SR.inexact_cases():
        Sp = case["Sp"]
        assert np.all(np.diff(case["u"], axis=-1) >= 0)
        assert np.all(np.diff(case["sbins_prev"], axis=-1) >= 0.25 / Sp)
        dens = case["density"] if case.get("density") is not None else None
        assert dens is None or dens.min() >= 0.5


def test_float64_weights_and_gradient_equal_autograd():
    for S, R in SR.WEIGHT_CASES:
        c = SR.weights_case(R, S)
        d = T(c["density"]).double().requires_grad_(True)
        e = T(c["ebins"]).double()
        dd = (e[:, 1:] - e[:, :-1]) * d
        w = (1 - torch.exp(-dd)) * torch.exp(-(torch.cumsum(dd, -1) - dd))
        w.backward(T(c["grad_weights"]).double())
        np.testing.assert_allclose(SR.get_weights(c["density"], c["ebins"], SR.f64), w.detach().numpy(), rtol=1e-12, atol=1e-300)
        g = SR.get_weights_grad(c["density"], c["ebins"], c["grad_weights"], SR.f64)
        np.testing.assert_allclose(g, d.grad.numpy(), rtol=0, atol=1e-13 * float(np.abs(g).max()))
        if S > 1:  # the float32 restatement against the float32 oracle: each lies within E32 of float64 (their exp differ in the last ulp)
            w32 = KO.get_weights(T(c["ebins"][:, 1:] - c["ebins"][:, :-1]), T(c["density"])).numpy()
            assert SR.deviation(SR.get_weights(c["density"], c["ebins"]), w32) <= 2 * SR.E32["weights_fwd.weights"], (S, R)


def test_criteria_accept_the_restatement_and_reject_a_shifted_index():
    """The family A criteria on the float32 restatement itself (it must pass them with room: the kernel gets tau = 5 x E32), and on indices
    shifted by one, which must fail."""
    for case in SR.inexact_cases():
        r32, r64 = SR.reference(case, "uniform", SR.f32), SR.reference(case, "uniform", SR.f64)
        u = SR.case_u(case, SR.f64)
        assert SR.index_within(r32["inds"], r64["cdf"], u, SR.TAU).all()
        assert SR.bins_inside(r32["inds"], r32["sbins"], case["sbins_prev"]).all()
        assert np.all(np.diff(r32["sbins"], axis=-1) >= 0)
        assert float(np.abs(SR.u_back(r32["sbins"], case["sbins_prev"], r64["cdf"]) - u).max()) <= SR.TAU / 2
        assert SR.index_within(r64["inds"], r64["cdf"], u, 0.0).all()
        if case["Sp"] >= 64:
            assert not SR.index_within(r32["inds"] + 1, r64["cdf"], u, SR.TAU).all()
            assert not SR.index_within(r32["inds"] - 1, r64["cdf"], u, SR.TAU).all()


def test_e32_of_the_float32_restatement_over_the_lattice():
    """Measures E32 per bounded quantity (two digits: the last ones move with the host's libm) and holds the table the GPU bounds are computed
    from, and the committed record, to the measurement."""
    worst = SR.measure_e32()
    for name, (v, where) in sorted(worst.items()):
        print(f"E32 {name:28s} {v:.3e}   at {where}")
    assert set(worst) == set(SR.E32), set(worst) ^ set(SR.E32)
    rec = json.load(open(E32_JSON))
    assert set(rec["E32"]) == set(SR.E32) and rec["margin"] == SR.MARGIN and rec["tau"] == SR.TAU
    for name, (v, _) in worst.items():
        assert SR.E32[name] / 3 <= v <= 1.25 * SR.E32[name], (name, v, SR.E32[name])
        assert SR.E32[name] / 3 <= rec["E32"][name] <= 1.0001 * SR.E32[name], (name, rec["E32"][name])

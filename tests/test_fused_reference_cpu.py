"""CPU: tests/fused_reference.py is tied down before the GPU tests trust it.

(i)   its features equal oracle.kplanes_oracle (interpolate_kplanes / bilinear_plane) in float64, on the lattice and on random points;
(ii)  its plane, weight and input gradients equal torch autograd in float64 through that oracle and a plain torch MLP (roundings off);
(iii) for every case the float32 run of the restatement has the bits of the float64 run on everything the GPU tests compare by equality;
(iv)  every lattice case passes the generator's assertions, one eighth of the rows are planted, the coverage the pruning rule claims holds;
(v)   mode-1 coordinates equal sample_positions + normalize_positions in float64."""
import json
import os

import pytest
import torch

from oracle import kplanes_oracle as KO
from tests import fused_reference as F
from tests import mlp_reference as R
from tests.conftest import ROOT

F64 = torch.float64
CASES = F.all_cases()
IDS = [F.case_id(c) for c in CASES]


def _oracle_features(ps, planes, p, view):
    grids = ps.to_reference(planes)
    if view == "4":
        return KO.interpolate_kplanes(p, grids, ps.concat)
    outs = []
    for sc in grids:
        prod = 1.0
        for q, comb in F.plane_list(ps, view):
            prod = prod * KO.bilinear_plane(sc[q], p[:, list(comb)])
        outs.append(prod)
    return torch.cat(outs, dim=-1) if ps.concat else sum(outs)


def _representatives():
    """One case per (kernel, view, kind, mode): the autograd comparison is slow on the largest shapes and says the same on each."""
    seen, out = set(), []
    for c in CASES:
        k = (c.kernel, c.view, c.kind, c.mode)
        N = c.N if c.mode == 0 else c.R * c.S
        if k not in seen and 8 <= N <= 2000:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_case_meets_the_exactness_conditions_and_plants_an_eighth(c):
    m = F.make(c)  # raises where a condition fails
    assert int(m["planted"].sum()) * 8 >= m["N"]
    if c.kernel != "gather":
        R.check_trace(m["trace"], F.case_id(c))
        assert any(r[0] == "acc" for r in m["trace"]) and any(r[0] == "round" for r in m["trace"])
    if c.view == "frozen":
        assert bool(torch.isnan(m["planes"]).any()) and not bool(torch.isnan(m["feat"]).any())


def test_the_lattice_covers_what_its_pruning_rule_claims():
    assert len(set(IDS)) == len(IDS)
    for kernel, cases in (("gather", F.gather_cases()), ("dfwd", F.density_fwd_cases()), ("dbwd", F.density_bwd_cases()), ("field", F.field_cases())):
        assert {c.N for c in cases if c.mode == 0} >= set(F.POINT_N), kernel
        assert {(c.R, c.S, c.rescale) for c in cases if c.mode == 1} >= {(r, s, rs) for r, s in F.RAY_SHAPES for rs in (0, 1)}, kernel
        assert any(c.same for c in cases), kernel
        views = ("4",) if kernel == "dbwd" else F.VIEWS
        assert {(c.view, c.kind) for c in cases} == {(v, k) for v in views for k in ("values", "weights")}, kernel
        assert {(c.kind, c.A) for c in cases} == {(k, A) for k in ("values", "weights") for A in (1, 2)}, kernel
        if kernel != "gather":
            assert {(c.view, c.operands) for c in cases} == {(v, o) for v in views for o in (1, 2)}, kernel
    assert {(c.C, c.concat, c.view) for c in F.gather_cases()} == {(C, cc, v) for C, cc in ((8, 0), (32, 1)) for v in F.VIEWS}
    assert {c.relu for c in F.density_bwd_cases()} == {0, 1} and {c.relu for c in F.density_fwd_cases()} == {0, 1}
    bw = F.density_bwd_cases()
    assert {c.nogx for c in bw} == {0, 1} and {c.ws0 for c in bw} == {0.0, 0.25} and {c.gp0 for c in bw} == {0.0, 0.5} and {c.ms for c in bw} == {(1,), (2,)}
    fc = F.field_cases()
    assert {len(c.ms) for c in fc} == {1, 2, 3, 5, 6} and {c.keep for c in fc} == {0, 1, 2}
    assert {c.keep for c in fc if c.order} == {0, 1, 2} and all(c.view == "4" and c.S % 32 == 0 for c in fc if c.order)
    for a, b in F.density_bwd_pairs():
        assert a.operands == b.operands and a.ms != b.ms and a.mode != b.mode
    assert {(a.mode, b.mode) for a, b in F.density_bwd_pairs()} == {(0, 1), (1, 0)}
    # clamped samples (outside the box) and samples exactly on the last texel are met by every kernel, on points and on ray samples
    for cases in (F.gather_cases(), F.density_fwd_cases(), F.density_bwd_cases(), F.field_cases()):
        for mode in (0, 1):
            ps_ = [F.make(c)["p"] for c in cases if c.mode == mode]
            assert sum(bool((p.abs() > 1).any()) for p in ps_) >= 3 and sum(bool((p == 1).any()) for p in ps_) >= 3
    # exactly-zero plane values reach the backward (the leave-one-out products)
    assert sum(bool((F.make(c)["feat"] == 0).any()) for c in bw if c.kind == "values") >= 5
    # the special plane of the "weights" cases is a space plane in some cases and a time plane in others
    kinds = set()
    for c in CASES:
        if c.kind == "weights" and c.view == "4":
            ps = F.make(c)["ps"]
            kinds.add(3 in ps.combs[F._special(c, ps)[1]])
    assert kinds == {True, False}
    # at least one kind has two non-zero weights per hidden unit
    m = F.make(next(c for c in F.density_bwd_cases() if c.kind == "weights"))
    assert bool(((m["Ws"][0] != 0).sum(0) == 2).all())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_features_equal_the_oracle_on_the_lattice(c):
    m = F.make(c)
    planes = torch.nan_to_num(m["planes"], nan=3.0)  # the oracle has no frozen view of a buffer: whatever the time planes hold is not read
    want = _oracle_features(m["ps"], planes, m["p"], c.view)
    assert torch.equal(m["feat"], want)


@pytest.mark.parametrize("view", F.VIEWS)
@pytest.mark.parametrize("C,concat", [(8, 0), (32, 1)])
def test_features_equal_the_oracle_on_random_points(view, C, concat):
    c = F._case("gather", "values", view, 0, N=700, ms=(1, 2, 3), C=C, concat=concat)
    ps = F._plane_set(c)
    gen = torch.Generator().manual_seed(5)
    planes = torch.rand(ps.numel, generator=gen, dtype=F64) + 0.25
    n = 3 if view != "4" else 4
    p = torch.rand(700, n, generator=gen, dtype=F64) * 2.6 - 1.3  # some outside the box: the border clamp
    p[::9] = 1.0
    got = F.gather(ps, planes, p, view)[0]
    torch.testing.assert_close(got, _oracle_features(ps, planes, p, view), rtol=1e-13, atol=0)


@pytest.mark.parametrize("c", [c for c in CASES if c.mode == 1], ids=[i for c, i in zip(CASES, IDS) if c.mode == 1])
def test_ray_sample_coordinates_equal_the_oracle(c):
    co = F.make(c)["co"]
    aabb = torch.tensor(co["aabb"], dtype=F64)
    pos = KO.sample_positions(co["o"], co["d"], co["eb"][:, :-1], co["eb"][:, 1:])
    q = KO.normalize_positions(pos, aabb)
    want = (q * 2 - 1 if c.rescale else q).reshape(-1, 3)
    got = F.coordinates(co, F.make(c)["n_coords"])
    assert torch.equal(got[:, :3], want)
    if got.shape[1] == 4:
        assert torch.equal(got[:, 3], (co["t"] * 2 - 1).repeat_interleave(c.S))


def _autograd(ps, planes, p, view, Ws_list, heads):
    """Features through the oracle with planes that ask for a gradient; heads(feat) -> scalar loss.  -> (plane grads flat, feat.grad, weight grads)."""
    grids = [[t.clone().requires_grad_(True) for t in sc] for sc in ps.to_reference(planes)]
    outs = []
    for sc in grids:
        prod = 1.0
        for q, comb in F.plane_list(ps, view):
            prod = prod * KO.bilinear_plane(sc[q], p[:, list(comb)])
        outs.append(prod)
    feat = torch.cat(outs, dim=-1) if ps.concat else sum(outs)
    feat.retain_grad()
    Ws = [w.clone().requires_grad_(True) for w in Ws_list]
    heads(feat, Ws).backward()
    flat = torch.zeros(ps.numel, dtype=F64)
    for s, sc in enumerate(grids):
        for q, _ in F.plane_list(ps, view):
            flat_view = ps.plane_view(s, q, flat)
            flat_view.copy_(sc[q].grad[0].permute(1, 2, 0))
    return flat, feat.grad, torch.cat([w.grad.reshape(-1) for w in Ws]) if Ws else None


@pytest.mark.parametrize("c", [c for c in _representatives() if c.kernel in ("dfwd", "dbwd")], ids=F.case_id)
def test_proposal_gradients_equal_autograd(c):
    m = F.make(c)
    planes = torch.nan_to_num(m["planes"], nan=1.0)
    gd = m["gdens"].double()

    def heads(feat, Ws):
        hid = feat @ Ws[0]
        z = (torch.relu(hid) if c.relu else hid) @ Ws[1]
        return (KO.trunc_exp(z[:, 0]) * gd).sum()

    gp, gX, gW = _autograd(m["ps"], planes, m["p"], c.view, m["Ws"], heads)
    ref = F.proposal(m["feat"], m["Ws"], c.relu, 0, m["gdens"])  # operands = 0: the roundings switched off
    mine = F.plane_grads(m["ps"], planes, m["p"], c.view, ref["gX"])
    scale = lambda t: 1e-13 * max(float(t.abs().max()), 1e-30)
    assert float(gp.abs().max()) > 0 or m["N"] < 8
    torch.testing.assert_close(ref["gX"], gX, rtol=0, atol=scale(gX))
    torch.testing.assert_close(ref["gW"], gW, rtol=0, atol=scale(gW))
    torch.testing.assert_close(mine, gp, rtol=0, atol=scale(gp))
    # and the exact answer of the case differs from the unrounded one only by the head's product snapping to its dyadic target
    torch.testing.assert_close(m["ref"]["gX"], gX, rtol=0, atol=1e-5 * max(float(gX.abs().max()), 1e-30))


@pytest.mark.parametrize("c", [c for c in _representatives() if c.kernel == "gather"], ids=F.case_id)
def test_plane_gradients_with_exact_zero_values_equal_autograd(c):
    """An arbitrary dyadic feature gradient through the gather alone: the leave-one-out products against autograd's product rule."""
    m = F.make(c)
    planes = torch.nan_to_num(m["planes"], nan=1.0)
    gen = torch.Generator().manual_seed(3)
    g = torch.randint(-8, 9, tuple(m["feat"].shape), generator=gen).to(F64)
    gp, _, _ = _autograd(m["ps"], planes, m["p"], c.view, [], lambda feat, Ws: (feat * g).sum())
    assert torch.equal(F.plane_grads(m["ps"], planes, m["p"], c.view, g), gp)


@pytest.mark.parametrize("c", [c for c in _representatives() if c.kernel == "field"], ids=F.case_id)
def test_field_forward_equals_the_plain_torch_field(c):
    m = F.make(c)
    ref = F.field(m["feat"], m["Wsig"], m["Wcol"], 0)
    h = KO.mlp(m["feat"], [w.t() for w in m["Wsig"]])
    rgb = KO.mlp(h[:, :15], [w.t() for w in m["Wcol"]], out_act="Sigmoid")
    assert torch.equal(ref["h"], h) and torch.equal(m["ref"]["h"], h)  # the roundings are identities on these inputs
    torch.testing.assert_close(ref["density"], torch.exp(h[:, 15]), rtol=1e-14, atol=0)
    torch.testing.assert_close(ref["rgb"], rgb, rtol=1e-14, atol=0)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_float32_run_has_the_bits_of_the_float64_run(c):
    m = F.make(c)
    f32 = torch.float32
    p32 = F.coordinates({k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in m["co"].items()}, m["n_coords"], f32)
    assert torch.equal(p32.double(), m["p"])
    planes32 = m["planes"].float()
    feat32 = F.gather(m["ps"], planes32, p32, c.view)[0]
    assert feat32.dtype == f32 and torch.equal(feat32.double(), m["feat"])
    pl = m["planted"]
    if c.kernel in ("dfwd", "dbwd"):
        r = F.proposal(feat32, m["Ws"], c.relu, c.operands, m["gdens"], dtype=f32)
        assert r["gX"].dtype == f32
        for k in ("z", "g_out", "gX", "gW"):
            assert torch.equal(r[k].double(), m["ref"][k]), k
        assert torch.equal(F.plane_grads(m["ps"], planes32, p32, c.view, r["gX"]).double().nan_to_num(), m["gp"].nan_to_num())
        assert bool((r["aux"][pl] == 1.0).all())
    elif c.kernel == "field":
        r = F.field(feat32, m["Wsig"], m["Wcol"], c.operands, dtype=f32)
        assert torch.equal(r["h"].double(), m["ref"]["h"])
        assert bool((r["density"][pl] == 1.0).all()) and bool((r["rgb"][pl] == 0.5).all())
        assert bool((m["ref"]["density"][pl] == 1.0).all()) and bool((m["ref"]["rgb"][pl] == 0.5).all())


def test_the_committed_yardsticks_are_those_of_the_lattice():
    with open(os.path.join(ROOT, "profiles", "r25_fused_deviations.json")) as f:
        rec = json.load(f)["cases"]
    want = {F.case_id(F.content_key(c)) for c in CASES if F.needs_bound(c)}
    assert set(rec) == want
    # exp and the Sigmoid of an exact float32 argument: between half an ulp and four ulps of float32, and what this machine's float32 gives within a
    # factor of two (a vectorised exp may differ in the last bit from one instruction set to the next; the GPU bound is 5 x the record)
    for v in rec.values():
        assert all(2.0 ** -25 <= d <= 2.0 ** -22 for d in v.values()), v
    for c in [c for c in CASES if F.needs_bound(c)][::9]:
        now = F.deviations(c)
        for k, d in rec[F.case_id(F.content_key(c))].items():
            assert 0.5 * d <= now[k] <= 2.0 * d, (F.case_id(c), k, d, now[k])

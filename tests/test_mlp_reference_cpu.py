"""CPU: the exact-case lattice of the MLP kernel family (tests/mlp_reference.py) is what it claims to be -- every case satisfies the preconditions of
the exactness argument, the restatement is the oracle's MLP under autograd, a float32 evaluation in another order gives the float64 bits, the head
construction rounds to the dyadic targets, the yardstick file is complete, and every shape the library accepts has a case."""
import ctypes as C
import json
import os

import torch

from tests import mlp_reference as R
from tests.conftest import ROOT

BACKWARD, FORWARD, DENSE, CROSS = R.mlp_backward_cases(), R.mlp_forward_cases(), R.dense_cases(), R.cross_kernel_cases()


def _sample(cases, n):
    return cases[::max(1, len(cases) // n)]


def test_every_lattice_case_satisfies_the_preconditions():
    """make_mlp / make_dense raise where a rounded tensor is not a fixed point of its rounding, an accumulation could be inexact in some order, a head's
    rounded tile is not the dyadic target or a planted value is missing.  The case ids are unique and the lattice is a few hundred cases."""
    ids = [R.case_id(c) for c in BACKWARD + FORWARD + DENSE + CROSS]
    assert len(set(ids)) == len(ids)
    assert 300 <= len(ids) <= 600, len(ids)
    for c in BACKWARD + FORWARD + CROSS:
        R.make_mlp(c)
    for c in DENSE:
        R.make_dense(c)


def test_the_lattice_holds_every_axis_value():
    ops = {0, 1, 2}
    assert {c.N for c in BACKWARD} >= set(R.ROWS) and {c.N for c in FORWARD} >= set(R.ROWS) and {c.N for c in DENSE} >= set(R.ROWS)
    for op in ops:
        assert {c.N for c in BACKWARD if c.operands == op} >= set(R.ROWS), op
        assert {c.d_out for c in BACKWARD if c.operands == op} == set(R.D_OUTS), op
    calls = {c.call for c in BACKWARD}
    assert calls == {"bwd", "bwd_tile", "bwd_ws", "bwd_fx", "bwd_x16", "quot", "quot_ws"}
    for call in ("bwd_x16", "quot", "quot_ws"):
        assert {c.rows for c in BACKWARD if c.call == call} == {"", "0"}, call
    assert {c.null for c in BACKWARD} == {"", "gX", "gW"} and {c.gw0 for c in BACKWARD} == {0.0, 0.25}
    assert {(c.hidden_act, c.out_act) for c in BACKWARD} == {(0, 0), (1, 0), (0, 1), (1, 1)} and {c.aux for c in BACKWARD} == {0, 1, 2}
    assert {c.aux for c in FORWARD} == {0, 1} and {c.out_act for c in FORWARD} == {0, 1}
    assert any(c.ldx % 4 and c.hidden == 64 and c.operands and c.call == "bwd" for c in BACKWARD)  # an ldx that is no multiple of 4
    assert any(c.call.startswith("quot") and c.ldx == c.d_in + 8 for c in BACKWARD)                # the trainer's x16 layout
    for letter in "zaco":
        assert any(letter in c.plant for c in BACKWARD), letter
    assert any(c.pattern == "addr" for c in BACKWARD) and any(c.pattern == "addr" for c in FORWARD)
    # the exact-fp32 kernels' heads: exact on rows with raw head outputs 0 ('o'), bounded elsewhere, the trunc_exp clamp's planted rows included
    fp32 = [c for c in BACKWARD if c.operands == 0]
    assert {(c.out_act, c.aux) for c in fp32 if "o" in c.plant} == {(1, 0), (0, 1), (0, 2)}
    assert {(c.out_act, c.aux) for c in fp32 if R.is_bounded_backward(c)} == {(1, 0), (0, 1), (0, 2)}
    assert {c.aux for c in fp32 if R.is_bounded_backward(c) and "a" in c.plant} == {1, 2}
    assert any(c.plant == "o" and c.out_act == 1 for c in CROSS) and any(c.plant == "o" and c.aux for c in CROSS)
    assert any(c.operands == 0 and c.n_hidden == 2 and c.N == R.TWO_TILES["fp32"] for c in FORWARD)
    assert {(c.K, c.M) for c in DENSE if c.operands == 0} == set(R.DENSE_FP32) and {(c.K, c.M) for c in DENSE if c.operands == 1} == set(R.DENSE_LP)
    assert {c.act for c in DENSE} == {0, 1, 2} and {c.call for c in DENSE} == {"fwd", "bwd", "bwd_fx", "bwd_nogx", "bwd_nogw"}
    for name, n in R.TWO_TILES.items():
        assert any(c.N == n for c in BACKWARD + FORWARD + DENSE), name
    big = [c for c in BACKWARD + FORWARD + DENSE if c.N > 1000]
    assert len(big) <= 24 and all(c.N in R.TWO_TILES.values() for c in big)  # the only large N, one case per kernel


def test_planted_rows_are_there():
    for c in BACKWARD:
        m = R.make_mlp(c)
        ref = m["ref"]
        if "z" in c.plant:
            n = c.N // 2
            assert not bool(m["X"][n].any()) and all(not bool(a[n].any()) for a in ref["acts"]) and bool(m["target"][n].any())
        if "a" in c.plant:
            assert {-16.0, -15.0, 15.0, 16.0} <= set(ref["z"][:, m["aux_col"]].tolist())
        if "c" in c.plant and c.operands == 2:
            assert float(ref["g_out"].abs().max()) == 7.99609375  # 65504 / 8192: the clamp acted, and the clamped value is representable
    # ... and on a HIDDEN layer's gradient: before cvtg's clamp it exceeds 65504 / 8192 in the two-hidden-layer 'c' cases
    hidden = [R.make_mlp(c)["ref"]["g_hidden_pre_max"] for c in BACKWARD if "c" in c.plant and c.operands == 2 and c.n_hidden == 2]
    assert len(hidden) >= 2 and all(h > R.FP16_MAX / R.GS for h in hidden), hidden
    # zero pre-activations with a live upstream gradient occur without planting, too: where `> 0` against `>= 0` decides
    m = R.make_mlp(next(c for c in BACKWARD if c.d_in == 15 and c.n_hidden == 2 and c.N == 1000))
    pre_zero = (m["ref"]["acts"][0] @ m["Ws"][0]) == 0
    assert 0.02 < float(pre_zero.double().mean()) < 0.5


def test_restatement_is_the_oracle_mlp_under_autograd():
    """operands = 0, float64: Y, aux, gX and gW equal oracle.kplanes_oracle.mlp (+ trunc_exp) differentiated by autograd, exactly."""
    from oracle import kplanes_oracle as KO

    n = 0
    for c in _sample([c for c in BACKWARD if c.out_act == 0], 24):
        m = R.make_mlp(c)
        ref = R.restate(m["X"], m["Ws"], c.hidden_act, 0, 0, m["gY"], m["aux_col"], m["gaux"])
        x = m["X"].clone().requires_grad_(True)
        ws = [w.t().clone().requires_grad_(True) for w in m["Ws"]]  # the oracle's layers are [out, in]
        y = KO.mlp(x, ws, out_act="None", hidden_act="ReLU" if c.hidden_act else "None")
        loss = 0.0
        if m["gY"] is not None:
            loss = loss + (y * m["gY"].double()).sum()
        if m["gaux"] is not None:
            aux = KO.trunc_exp(y[:, m["aux_col"]])
            assert torch.equal(aux.detach(), ref["aux"])
            loss = loss + (aux * m["gaux"].double()).sum()
        loss.backward()
        assert torch.equal(y.detach(), ref["Y"]) and torch.equal(x.grad, ref["gX"]), R.case_id(c)
        assert torch.equal(torch.cat([w.grad.t().reshape(-1) for w in ws]), ref["gW"]), R.case_id(c)
        n += 1
    assert n >= 20


def test_float32_in_another_order_gives_the_float64_bits():
    """Samples shuffled, the contraction indices (inputs and hidden units) flipped, everything in float32: the bits of the float64 restatement."""
    gen = torch.Generator().manual_seed(5)
    for c in _sample([c for c in BACKWARD if c.N <= 1000 and not R.is_bounded_backward(c)], 30):
        m = R.make_mlp(c)
        ref = m["ref"]
        perm = torch.randperm(c.N, generator=gen)
        Ws = [w.flip(0) if l == 0 else w for l, w in enumerate(m["Ws"])]
        Ws = [w.flip(1) if l < c.n_hidden else w for l, w in enumerate(Ws)]
        Ws = [w.flip(0) if l > 0 else w for l, w in enumerate(Ws)]
        r = R.restate(m["X"].flip(1)[perm], Ws, c.hidden_act, c.out_act, c.operands, None if m["gY"] is None else m["gY"][perm], m["aux_col"],
                      None if m["gaux"] is None else m["gaux"][perm], dtype=torch.float32)
        inv = torch.argsort(perm)
        assert torch.equal(r["gX"].flip(1)[inv].double(), ref["gX"]), R.case_id(c)
        assert torch.equal(r["z"][inv].double(), ref["z"]), R.case_id(c)
        off, back = 0, []
        for l, w in enumerate(m["Ws"]):
            g = r["gW"][off:off + w.numel()].reshape(w.shape)
            off += w.numel()
            g = g.flip(0)
            back.append((g.flip(1) if l < c.n_hidden else g).reshape(-1))
        assert torch.equal(torch.cat(back).double(), ref["gW"]), R.case_id(c)
    for c in _sample([c for c in DENSE if c.call != "fwd" and c.N <= 1000], 12):
        m = R.make_dense(c)
        perm = torch.randperm(c.N, generator=gen)
        r = R.restate_dense(m["X"].flip(1)[perm], m["W"].flip(0), c.act, c.operands, m["Y"][perm], m["gY"][perm], dtype=torch.float32)
        assert torch.equal(r["gX"].flip(1)[torch.argsort(perm)].double(), m["ref"]["gX"]), R.case_id(c)
        assert torch.equal(r["gW"].reshape(c.K, c.M).flip(0).reshape(-1).double(), m["ref"]["gW"]), R.case_id(c)


def test_head_construction_rounds_to_the_dyadic_targets():
    """The float32 product gY * act' (+ gaux * exp(clamp(z))) formed with torch's own float32 sigmoid and exp, rounded to bf16 and to fp16 after
    the 8192 scale, is the dyadic target everywhere: the margin stated in tests/mlp_reference.py holds for an independent float32 activation."""
    n = 0
    for c in BACKWARD:
        if not (c.out_act == 1 or c.aux):
            continue
        m = R.make_mlp(c)
        z = m["ref"]["z"].float()
        g = torch.zeros_like(z)
        if m["gY"] is not None:
            s = torch.sigmoid(z)
            g = m["gY"] * s * (1.0 - s) if c.out_act == 1 else m["gY"].clone()
        if m["gaux"] is not None:
            g[:, m["aux_col"]] += m["gaux"] * torch.exp(z[:, m["aux_col"]].clamp(-15.0, 15.0))
        assert g.dtype == torch.float32
        t = m["target"]
        assert torch.equal(g.to(torch.bfloat16).double(), t), R.case_id(c)
        assert torch.equal((g * R.GS).clamp(-R.FP16_MAX, R.FP16_MAX).to(torch.float16).double() / R.GS, t), R.case_id(c)
        # the margin itself: the product lies within 2^-12 / 16 relative of the target, the nearest midpoint 2^-12 (fp16) away; |z| <= 4 on Sigmoid columns
        nz = t != 0
        assert not bool(nz.any()) or float(((g.double() - t).abs()[nz] / t.abs()[nz]).max()) < 2.0 ** -12 / 16
        assert c.out_act == 0 or float(z.abs().max()) <= 4.0
        n += 1
    assert n >= 60


def test_yardstick_file_holds_every_case_that_needs_it():
    with open(os.path.join(ROOT, "profiles", "r17_mlp_deviations.json")) as f:
        rec = json.load(f)
    need = {R.case_id(c): c for c in FORWARD + DENSE + BACKWARD if R.needs_bound(c)}
    assert set(rec["cases"]) == set(need) and rec["factor"] == 5
    for cid, c in need.items():
        want = set()
        if R.is_bounded_backward(c):
            want = {"gX", "gW"}
        elif isinstance(c, R.DenseCase) or c.out_act == 1:
            want.add("Y")
        if isinstance(c, R.MlpCase) and c.aux and not R.is_bounded_backward(c):
            want.add("aux")
        assert set(rec["cases"][cid]) == want, cid
        # a yardstick is a float32 figure: between a tenth of an ulp and a few ulps
        # (a bounded backward's figure is taken against the output's largest element and, under a Sigmoid, carries the cancellation of 1 - s:
        # up to e^4 ulps of s at |z| = 4, tests/mlp_reference.py 4. -- hence the wider range on both sides)
        lo, hi = (2.0 ** -28, 2.0 ** -19) if R.is_bounded_backward(c) else (2.0 ** -27, 2.0 ** -21)
        assert all(lo < v < hi for v in rec["cases"][cid].values()), (cid, rec["cases"][cid])
    for cid in list(need)[::9]:  # and the file is what the tool writes today
        assert rec["cases"][cid] == R.case_deviations(need[cid]), cid


def test_every_supported_shape_has_a_lattice_case():
    """For every (d_in, hidden, n_hidden, operands) that snerf_mlp_supported accepts the lattice holds a case of the same padding class (16 for the
    exact-fp32 kernels, 32 for the 16-bit ones), forward and backward: a shape added to the tables without a case here fails this test."""
    from soccernerfs_amd import _lib, build

    build.build(verbose=False)
    L = _lib.lib()
    have_b = {R.padding_class(c.d_in, c.hidden, c.n_hidden, c.operands) for c in BACKWARD}
    have_f = {R.padding_class(c.d_in, c.hidden, c.n_hidden, c.operands) for c in FORWARD}
    n = 0
    for op in (0, 1, 2):
        for hidden in (16, 64, 128):
            for nh in (1, 2):
                for d_in in range(1, 193):
                    d = _lib.MlpDesc()
                    d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d_in, hidden, nh, 3, 1, 0, op
                    if L.snerf_mlp_supported(C.byref(d)):
                        cls = R.padding_class(d_in, hidden, nh, op)
                        assert cls in have_b and cls in have_f, f"no lattice case for d_in={d_in} hidden={hidden} n_hidden={nh} operands={op}"
                        n += 1
    assert n > 800
    # the other direction: every case of the lattice is a shape the library accepts (the cross-kernel nets with fp32 operands as well)
    for c in BACKWARD + FORWARD + CROSS:
        for op in ({c.operands, 0} if c.call == "cross" else {c.operands}):
            d = _lib.MlpDesc()
            d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = c.d_in, c.hidden, c.n_hidden, c.d_out, c.hidden_act, c.out_act, op
            assert L.snerf_mlp_supported(C.byref(d)), R.case_id(c)
    for c in DENSE:
        assert c.operands == 0 or L.snerf_dense_lp_supported(c.K, c.M, c.operands), R.case_id(c)
    # and the tables this file restates are the library's: every listed shape is accepted, at its padded width
    for shapes, op in ((R.FP32_SHAPES, 0), (R.LP_SHAPES, 1), (R.LP_SHAPES, 2)):
        for d0p, hidden, nh in shapes:
            d = _lib.MlpDesc()
            d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d0p, hidden, nh, 3, 1, 0, op
            assert L.snerf_mlp_supported(C.byref(d)), (d0p, hidden, nh, op)

"""GPU: the dense optimiser sweeps (csrc/optim.hip) against float64 references over a lattice of cases (tests/optim_reference.py).

Every call goes through the C ABI.  A bound is FACTOR (5) x the float32 restatement's deviation from the float64 one on the same inputs
(profiles/r16_optim_deviations.json, measured on the CPU by tools/measure_optim_deviations.py); where that deviation is 0 the kernel must be
exact.  Deviations are max |got - want| / max |want| over an output.  Every buffer a kernel may write has 64 guard floats behind it, prefilled
with a sentinel, and p_out is prefilled with the sentinel too.

The three loss VALUES are summed in a tree torch does not share, so their bound is 5 x the recorded deviation PLUS the float32 bound of that
tree, derived from the kernel's own chain lengths (plane_reg_kernel, plane_reg_grad): a term d^2 / n enters a float4's sum of squares (3 adds),
a lane adds at most a second such term (w and h direction: 1 add), wave_sum is a 6-level butterfly (6 adds), a workgroup adds its four
wavefronts in sequence (3 adds), and workgroup `blk` adds atomically into slot blk % n_slots (ceil(n_blocks / n_slots) - 1 adds behind the
first; 0 here: every set of the lattice has fewer workgroups than the 1024 slots).  The slots are summed in float64 by the test.  Every term
is >= 0, so with L = 13 roundings on any term's way |error| <= L u / (1 - L u) x value, u = 2^-24: 7.7e-7.

Each test prints `case output deviation / bound` lines before it asserts; profiles/r16_optim_INDEX.md keeps them per case family."""
import ctypes as C
import functools

import pytest
import torch

from tests import optim_reference as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -71234.5  # no input, output or intermediate of any case comes near it
BOUNDS = OR.load_bounds()
BY_ID = {c["case_id"]: c for c in OR.PLANE_CASES}


# ------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats on the GPU with GUARD sentinel floats behind them; `t` is the view a kernel is given."""

    def __init__(self, n, src=None, fill=SENT):
        self.buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[:n]
        if src is not None:
            self.t.copy_(src)
        elif fill != SENT:
            self.t.fill_(fill)

    def intact(self) -> bool:
        return bool((self.buf[self.t.numel():] == SENT).all())


def _report(cid, name, dev, dev32):
    bound = OR.FACTOR * dev32
    print(f"{cid} {name} {dev:.3e} / {bound:.3e}")
    return dev <= bound


def _check_outputs(cid, got, ref, rec, names=("p_out", "m", "v"), sl=slice(None)):
    """got[k][sl] against ref[k][sl], relative to the whole reference output's largest magnitude, as the yardstick was measured."""
    bad = []
    for k in names:
        want = ref[k]
        err = float((got[k].double().cpu()[sl] - want[sl]).abs().max()) if want[sl].numel() else 0.0
        scale = float(want.abs().max())
        dev = 0.0 if err == 0.0 else (float("inf") if scale == 0.0 else err / scale)
        if not _report(cid, k, dev, rec[f"dev32_{k}"]):
            bad.append((k, dev, OR.FACTOR * rec[f"dev32_{k}"]))
    return bad


@functools.lru_cache(maxsize=None)
def _case_data(cid):
    d = OR.make_case(BY_ID[cid])
    return d, OR.planes_step(d, torch.float64)


def _plane_set(d):
    from soccernerfs_amd.plane_set import PlaneSet

    return PlaneSet(d["case"]["C"], d["res"], concat=True)  # on the host: only its descriptor is used


def _run_planes(d, coefs, g=None, dyn=None, shard_range=None, zero_grad=None):
    """One snerf_adam_planes_step(_range) on guarded copies of the case's buffers."""
    from soccernerfs_amd import ops

    c, n = d["case"], d["n"]
    B = {"p_in": Guarded(n, d["p"]), "p_out": Guarded(n), "g": Guarded(n, d["g"] if g is None else g), "m": Guarded(n, d["m"]), "v": Guarded(n, d["v"]),
         "losses": Guarded(ops.REG_SLOTS * 16, fill=0.0)}
    zg = c["zero_grad"] if zero_grad is None else zero_grad
    ops.adam_planes_step(_plane_set(d), B["p_in"].t, B["p_out"].t, B["g"].t, B["m"].t, B["v"].t, coefs, B["losses"].t.view(ops.REG_SLOTS, 16), d["step"], OR.LR,
                         eps=1e-12, grad_scale=c["grad_scale"], zero_grad=bool(zg), shard_range=shard_range, dyn=dyn)
    torch.cuda.synchronize()
    out = {k: B[k].t for k in ("p_out", "m", "v", "g")}
    out["losses"] = B["losses"].t.view(ops.REG_SLOTS, 16)
    out["bufs"] = B
    return out


def _assert_guards(B, d):
    assert all(b.intact() for b in B.values()), [k for k, b in B.items() if not b.intact()]
    assert torch.equal(B["p_in"].t.cpu(), d["p"])  # the old parameters are read only


def _values(losses):
    return losses.double()[:, :3].sum(0).cpu()


def _check_values(cid, got, want, rec, d):
    from soccernerfs_amd import ops

    tree = OR.value_summation_bound(OR.n_workgroups(d["case"]["C"], d["layout"]), ops.REG_SLOTS)
    ok = True
    for i, name in enumerate(("space_tv", "time_smooth", "sparse_transients")):
        w = float(want[i])
        bound = (OR.FACTOR * rec["dev32_values"][i] + tree) * abs(w)
        err = abs(float(got[i]) - w)
        print(f"{cid} value_{name} {err / abs(w) if w else err:.3e} / {bound / abs(w) if w else 0.0:.3e}")
        ok = ok and err <= bound
    return ok


def _dyn_at(step, policy="skip_step", force=False):
    from soccernerfs_amd import ops

    dyn = ops.new_adam_dyn(DEV)
    dyn[1] = step - 1
    ops.adam_prepare(dyn, OR.LR, policy=policy, force_nonfinite=force)
    return dyn


def _plane_reg(d, coefs, grad, losses, overwrite):
    from soccernerfs_amd import _lib, ops

    desc = _plane_set(d).desc()
    _lib.check(_lib.lib().snerf_plane_reg(C.byref(desc), ops._ptr(d["p_dev"]), ops._ptr(grad) if grad is not None else None, coefs[0], coefs[1], coefs[2],
                                          ops._ptr(losses) if losses is not None else None, ops.REG_SLOTS if losses is not None else 0, overwrite, ops._stream()),
               "plane_reg")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------------
# the plane sweeps over the lattice
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["case_id"] for c in OR.PLANE_CASES])
def test_adam_planes_step_against_float64(cid):
    """snerf_adam_planes_step: p_out, m, v within the bounds (m and v carry the sharp check: m_out - b1 m_in is the total gradient times 1 - b1,
    so a wrong regulariser weight cannot hide behind Adam's normalisation), guards intact, no sentinel left in p_out, the gradient buffer cleared
    (zero_grad = 1) or bit-unchanged (zero_grad = 0), loss slots equal to the float64 values with columns 3-15 untouched; the same step with the
    device-side state (dyn, adam_prepare) within the same bounds."""
    d, ref = _case_data(cid)
    c, rec = d["case"], BOUNDS["planes"][cid]
    coefs = OR.COEFS[c["coefs"]]
    got = _run_planes(d, coefs)
    bad = _check_outputs(cid, got, ref, rec)
    values_ok = _check_values(cid, _values(got["losses"]), ref["values"], rec, d)
    _assert_guards(got["bufs"], d)
    assert not bool((got["p_out"] == SENT).any())
    if c["zero_grad"]:
        assert float(got["g"].abs().max()) == 0.0
    else:
        assert torch.equal(got["g"].cpu(), d["g"])
    assert float(got["losses"][:, 3:].abs().max()) == 0.0
    assert not bad, bad
    assert values_ok
    # ---- device-side state: the same step through dyn (pow in the device's library: bits may differ, the bounds may not) ----
    dyn = _dyn_at(d["step"])
    got_d = _run_planes(d, coefs, dyn=dyn)
    bad = _check_outputs(cid + " dyn", got_d, ref, rec)
    same = all(torch.equal(got_d[k], got[k]) for k in ("p_out", "m", "v"))
    print(f"{cid} dyn bits_equal_host_step {int(same)}")
    _assert_guards(got_d["bufs"], d)
    assert dyn.cpu().tolist()[:4] == [0, d["step"], 0, 0]
    assert not bad, bad


@pytest.mark.parametrize("cid", [c["case_id"] for c in OR.PLANE_CASES])
def test_zero_coefficients_equal_flat_adam_bit_for_bit(cid):
    """With coefficients (0, 0, 0) the fused sweep is snerf_adam_step on the same flat buffers: same bits in p_out, m, v and the gradient buffer."""
    from soccernerfs_amd import ops

    d, _ = _case_data(cid)
    c, n = d["case"], d["n"]
    got = _run_planes(d, (0.0, 0.0, 0.0))
    p, po, g, m, v = Guarded(n, d["p"]), Guarded(n), Guarded(n, d["g"]), Guarded(n, d["m"]), Guarded(n, d["v"])
    ops.adam_step(p.t, g.t, m.t, v.t, d["step"], OR.LR, eps=1e-12, grad_scale=c["grad_scale"], zero_grad=bool(c["zero_grad"]), p_out=po.t)
    torch.cuda.synchronize()
    for k, x in (("p_out", po), ("m", m), ("v", v), ("g", g)):
        assert torch.equal(got[k], x.t), k
        assert x.intact()
    assert torch.equal(p.t.cpu(), d["p"])
    _assert_guards(got["bufs"], d)


@pytest.mark.parametrize("cid", [c["case_id"] for c in OR.PLANE_CASES])
def test_plane_reg_against_float64(cid):
    """snerf_plane_reg: values and gradient within the bounds in both modes (overwrite = 1 into a zeroed buffer, overwrite = 0 accumulating onto a
    random buffer); grad = NULL leaves values only."""
    from soccernerfs_amd import ops

    d, ref = _case_data(cid)
    c, rec, n = d["case"], BOUNDS["planes"][cid], d["n"]
    coefs = OR.COEFS[c["coefs"]]
    d = dict(d, p_dev=d["p"].to(DEV))
    bad, values_ok = [], True
    for overwrite, key in ((1, "reg_grad"), (0, "reg_grad_accumulated")):
        grad = Guarded(n, None if overwrite else d["acc"], fill=0.0)
        losses = Guarded(ops.REG_SLOTS * 16, fill=0.0)
        _plane_reg(d, coefs, grad.t, losses.t, overwrite)
        want = ref["reg_grad"] if overwrite else d["acc"].double() + ref["reg_grad"]
        bad += _check_outputs(cid, {key: grad.t}, {key: want}, rec, names=(key,))
        lv = losses.t.view(ops.REG_SLOTS, 16)
        values_ok = _check_values(f"{cid} overwrite={overwrite}", _values(lv), ref["values"], rec, d) and values_ok
        assert grad.intact() and losses.intact() and float(lv[:, 3:].abs().max()) == 0.0
    losses = Guarded(ops.REG_SLOTS * 16, fill=0.0)
    _plane_reg(d, coefs, None, losses.t, 0)
    values_ok = _check_values(f"{cid} grad=NULL", _values(losses.t.view(ops.REG_SLOTS, 16)), ref["values"], rec, d) and values_ok
    assert losses.intact() and torch.equal(d["p_dev"].cpu(), d["p"])
    assert not bad, bad
    assert values_ok


def _range_cuts(d):
    """Cuts (float offsets, multiples of 4) that tile the segment: inside a plane row, exactly on a plane boundary, at a multiple of 1024 floats
    inside a plane (where a plane is that large), and the segment's ends."""
    C_, n, layout = d["case"]["C"], d["n"], d["layout"]
    cuts = {0, n}
    _, _, off, H, W, _ = layout[1]
    cuts.add(off + ((H // 2) * W * C_ + C_ // 2) // 4 * 4 + 4)      # inside a row of the second plane, inside a texel's channels
    cuts.add(layout[len(layout) // 2][2])                            # a plane boundary
    cuts.add(layout[-1][2] + 4)                                      # one float4 into the last plane
    big = [e for e in layout if e[3] * e[4] * C_ > 2048]
    if big:
        cuts.add(big[-1][2] + 1024 * ((big[-1][3] * big[-1][4] * C_) // 2048))  # a workgroup boundary inside a plane
    return sorted(cuts), bool(big)


@pytest.mark.parametrize("cid", OR.RANGE_CASE_IDS)
def test_adam_planes_step_ranges_against_float64(cid):
    """snerf_adam_planes_step_range against the REFERENCE (tests/test_gpu_sharded.py compares ranges with the whole sweep): inside a range the result
    is within the bounds; outside it p_out keeps its sentinel and m, v, g keep their bits; the ranges' value partial sums add up to the whole; an
    empty range and a range entirely past the segment touch nothing."""
    d, ref = _case_data(cid)
    c, rec, n = d["case"], BOUNDS["planes"][cid], d["n"]
    coefs = OR.COEFS[c["coefs"]]
    cuts, _ = _range_cuts(d)
    total = torch.zeros(3, dtype=torch.float64)
    bad = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = _run_planes(d, coefs, shard_range=(lo, hi), zero_grad=1)
        bad += _check_outputs(f"{cid} range[{lo},{hi})", got, ref, rec, sl=slice(lo, hi))
        out = torch.ones(n, dtype=torch.bool)
        out[lo:hi] = False
        assert bool((got["p_out"].cpu()[out] == SENT).all()) and not bool((got["p_out"][lo:hi] == SENT).any())
        for k in ("m", "v", "g"):
            assert torch.equal(got[k].cpu()[out], d[k][out]), k
        assert float(got["g"][lo:hi].abs().max()) == 0.0
        _assert_guards(got["bufs"], d)
        total += _values(got["losses"])
    assert _check_values(f"{cid} ranges_sum", total, ref["values"], rec, d)
    for lo, hi in ((cuts[1], cuts[1]), (n + 1024, n + 4096)):
        got = _run_planes(d, coefs, shard_range=(lo, hi), zero_grad=1)
        assert bool((got["p_out"] == SENT).all()) and float(got["losses"].abs().max()) == 0.0
        for k in ("m", "v", "g"):
            assert torch.equal(got[k].cpu(), d[k]), k
        _assert_guards(got["bufs"], d)
    assert not bad, bad


def _planted(d, ref):
    """Positions of planted NaN / +Inf / -Inf: the first texel of the first plane (a border texel), the last element of the segment, the middle, and
    the position of the largest regulariser gradient (non-zero: checked)."""
    n = d["n"]
    hot = int(ref["reg_grad"].abs().argmax())
    assert float(ref["reg_grad"][hot]) != 0.0
    pos = sorted({0, 1, n - 1, n // 2, hot, hot ^ 1})
    vals = [float("nan"), float("inf"), -float("inf")]
    g = d["g"].clone()
    for i, q in enumerate(pos):
        g[q] = vals[i % 3]
    return pos, g


@pytest.mark.parametrize("cid", OR.RANGE_CASE_IDS)
def test_adam_planes_step_non_finite_elements(cid):
    """NaN, +Inf, -Inf VALUES in the gradient through the documented paths.  drop_elements: each such element takes total gradient 0 (its regulariser
    share included), m and v decay, dyn.dropped counts them.  skip_step with force_nonfinite: p_out = p_in bit for bit, m and v untouched, the
    gradient cleared, dyn.skipped = 1 and dyn.t does not advance."""
    d, ref0 = _case_data(cid)
    c, rec, n = d["case"], BOUNDS["planes"][cid], d["n"]
    coefs = OR.COEFS[c["coefs"]]
    pos, g = _planted(d, ref0)
    ref = OR.planes_step(dict(d, g=g), torch.float64)
    assert ref["dropped"] == len(pos)
    dyn = _dyn_at(d["step"], policy="drop_elements")
    got = _run_planes(d, coefs, g=g, dyn=dyn, zero_grad=1)
    bad = _check_outputs(f"{cid} drop", got, ref, rec)
    b1, b2 = torch.tensor(OR.BETA1, dtype=torch.float32), torch.tensor(OR.BETA2, dtype=torch.float32)
    assert torch.equal(got["m"].cpu()[pos], b1 * d["m"][pos]) and torch.equal(got["v"].cpu()[pos], b2 * d["v"][pos])
    assert bool(torch.isfinite(got["p_out"]).all()) and float(got["g"].abs().max()) == 0.0
    assert dyn.cpu().tolist()[:4] == [0, d["step"], 0, len(pos)]
    _assert_guards(got["bufs"], d)
    assert not bad, bad
    # ---- the skipped step ----
    dyn = _dyn_at(d["step"], policy="skip_step", force=True)
    got = _run_planes(d, coefs, g=g, dyn=dyn, zero_grad=1)
    assert torch.equal(got["p_out"].cpu(), d["p"]) and torch.equal(got["m"].cpu(), d["m"]) and torch.equal(got["v"].cpu(), d["v"])
    assert float(got["g"].abs().max()) == 0.0
    assert dyn.cpu().tolist()[:4] == [0, d["step"] - 1, 1, 0]
    assert _check_values(f"{cid} skipped", _values(got["losses"]), ref0["values"], rec, d)  # the values are still reported
    _assert_guards(got["bufs"], d)


# ------------------------------------------------------------------------------------------------------------------------------------
# snerf_adam_step alone
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_flat(d, g=None, dyn=None, zero_grad=True):
    from soccernerfs_amd import ops

    c, n = d["case"], d["case"]["n"]
    B = {"p": Guarded(n, d["p"]), "g": Guarded(n, d["g"] if g is None else g), "m": Guarded(n, d["m"]), "v": Guarded(n, d["v"])}
    if not c["in_place"]:
        B["p_out"] = Guarded(n)
    ops.adam_step(B["p"].t, B["g"].t, B["m"].t, B["v"].t, d["step"], OR.LR, eps=c["eps"], grad_scale=c["grad_scale"], zero_grad=zero_grad,
                  p_out=None if c["in_place"] else B["p_out"].t, dyn=dyn)
    torch.cuda.synchronize()
    assert all(b.intact() for b in B.values()), [k for k, b in B.items() if not b.intact()]
    if not c["in_place"]:
        assert torch.equal(B["p"].t.cpu(), d["p"])
    return {"p_out": B["p" if c["in_place"] else "p_out"].t, "m": B["m"].t, "v": B["v"].t, "g": B["g"].t}


@pytest.mark.parametrize("cid", [c["case_id"] for c in OR.FLAT_CASES])
def test_adam_step_against_float64(cid):
    """snerf_adam_step over n in {1..5, 255, 1023, 1024, 1025, 4099} (the n % 4 tail in every phase; n < 4: only the tail runs), in place and with
    p_out != p, three eps: within the bounds, guards intact, the gradient cleared or bit-unchanged; drop and skip semantics as the plane sweep's."""
    c = next(x for x in OR.FLAT_CASES if x["case_id"] == cid)
    d, rec, n = OR.make_flat_case(c), BOUNDS["flat"][cid], c["n"]
    ref = OR.flat_step(d, torch.float64)
    zg = c["seed"] % 2 == 0
    got = _run_flat(d, zero_grad=zg)
    bad = _check_outputs(cid, got, ref, rec)
    assert not bool((got["p_out"] == SENT).any())
    assert float(got["g"].abs().max()) == 0.0 if zg else torch.equal(got["g"].cpu(), d["g"])
    assert not bad, bad
    got_d = _run_flat(d, dyn=_dyn_at(d["step"]), zero_grad=zg)
    bad = _check_outputs(cid + " dyn", got_d, ref, rec)
    print(f"{cid} dyn bits_equal_host_step {int(all(torch.equal(got_d[k], got[k]) for k in ('p_out', 'm', 'v')))}")
    assert not bad, bad
    # ---- non-finite values: the first element, the last (in the scalar tail when n % 4 != 0), the middle ----
    pos = sorted({0, n - 1, n // 2})
    g = d["g"].clone()
    for i, q in enumerate(pos):
        g[q] = [float("nan"), float("inf"), -float("inf")][i % 3]
    ref_n = OR.flat_step(dict(d, g=g), torch.float64)
    dyn = _dyn_at(d["step"], policy="drop_elements")
    got = _run_flat(d, g=g, dyn=dyn)
    bad = _check_outputs(cid + " drop", got, ref_n, rec)
    b1, b2 = torch.tensor(OR.BETA1, dtype=torch.float32), torch.tensor(OR.BETA2, dtype=torch.float32)
    assert torch.equal(got["m"].cpu()[pos], b1 * d["m"][pos]) and torch.equal(got["v"].cpu()[pos], b2 * d["v"][pos])
    assert bool(torch.isfinite(got["p_out"]).all()) and float(got["g"].abs().max()) == 0.0
    assert dyn.cpu().tolist()[:4] == [0, d["step"], 0, len(pos)]
    assert not bad, bad
    dyn = _dyn_at(d["step"], policy="skip_step", force=True)
    got = _run_flat(d, g=g, dyn=dyn)
    assert torch.equal(got["p_out"].cpu(), d["p"]) and torch.equal(got["m"].cpu(), d["m"]) and torch.equal(got["v"].cpu(), d["v"])
    assert float(got["g"].abs().max()) == 0.0 and dyn.cpu().tolist()[:4] == [0, d["step"] - 1, 1, 0]


# ------------------------------------------------------------------------------------------------------------------------------------
# snerf_adam_step_tv
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["case_id"] for c in OR.TV_CASES])
def test_adam_step_tv_against_float64(cid):
    """snerf_adam_step_tv on [rows, grid_C] tables, grid_C in {4, 6, 34, 66} (a float4 straddles a row end whenever grid_C % 4 != 0), against
    float64 Adam on g * grad_scale plus srow[r] on column a and -srow[r] on column b."""
    from soccernerfs_amd import _lib, ops

    c = next(x for x in OR.TV_CASES if x["case_id"] == cid)
    d, rec = OR.make_tv_case(c), BOUNDS["tv"][cid]
    ref = OR.tv_step(d, torch.float64)
    n = c["rows"] * c["grid_C"]
    B = {"p": Guarded(n, d["p"]), "g": Guarded(n, d["g"]), "m": Guarded(n, d["m"]), "v": Guarded(n, d["v"]), "srow": Guarded(c["rows"], d["srow"])}
    _lib.check(_lib.lib().snerf_adam_step_tv(ops._ptr(B["p"].t), ops._ptr(B["g"].t), ops._ptr(B["m"].t), ops._ptr(B["v"].t), c["rows"], c["grid_C"], c["cols"][0],
                                             c["cols"][1], ops._ptr(B["srow"].t), OR.LR, 0.9, 0.999, 1e-12, d["step"], c["grad_scale"], 1, None, ops._stream()),
               "adam_step_tv")
    torch.cuda.synchronize()
    bad = _check_outputs(cid, {"p_out": B["p"].t, "m": B["m"].t, "v": B["v"].t}, ref, rec)
    assert all(b.intact() for b in B.values()) and torch.equal(B["srow"].t.cpu(), d["srow"])
    assert float(B["g"].t.abs().max()) == 0.0
    assert not bad, bad

"""GPU: the residency budget of the fused proposal density backward (snerf_kplanes_density_bwd_budget, csrc/proposal_bwd.hip).

The budget changes only how many workgroups the persistent grid has, so how long a range of 32-sample pairs each wave owns: grid =
min(needed, resident, max(budget, live levels)).  Against budget 0 (the entry snerf_kplanes_density_bwd forwards to), through the raw entry:

* gX on the raw bits, for every budget of {1, 2, 3, 7, resident, 0, above resident};
* plane and weight gradients within max(1e-6, 4 x the spread of two budget-0 runs) relative L2 -- the bound of tests/test_gpu_proposal_bwd_fused.py:
  the same terms, run-length combined along longer ranges and added by float atomics in another order;
* cells behind every buffer keep a sentinel and the padding between the workspace replicas stays zero.  (These comparisons accumulate from ZERO:
  on top of 0.5 every atomic add rounds at 2^-25, a thousand times the gradients' own rounding, and the arrival order of the atomics alone then
  moves a tiny plane's gradient by 6e-5 relative L2 between two launches of the same grid);
* on the exact lattice of tests/fused_reference.py every output is the float64 answer in bits for every budget (regrouping exact sums changes
  nothing), with EVERY level's workspace replicas started from 0.25 and gradient planes from 0.5: a workgroup or wave without pairs, or one that
  took a pair twice, would show in the sum on top of the sentinel;
* shapes: two tiny levels with fewer pairs than workgroups and a ragged last pair, two levels large enough that the budgets give different grids, one
  level of N = 31, two levels one of which is empty (its buffers stay untouched), budget 1 on two levels (clamped to one workgroup per level); both
  operand types;
* the trainer at R = 64: the gradients of an updating step with the default budget, with 1.0 workgroup per CU and with 0 agree under the same bound."""
import ctypes as C

import pytest
import torch

from tests import fused_reference as F
from tests import test_gpu_fused_lattice as LT
from tests import test_gpu_proposal_bwd_fused as PB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPS, SENT, TAIL = PB.REPS, 7.0, 64


def _budgets():
    resident = 2 * torch.cuda.get_device_properties(0).multi_processor_count  # two 4-wave workgroups of 242 registers per CU
    return [1, 2, 3, 7, resident, 0, resident + 37]


def _make_level(res, operands, N_or_rays, seed):
    """(ps, net, co, N, gdens, keep): one level on ray samples (R, S) or on N explicit points."""
    from soccernerfs_amd import ops

    ps, net, gen = PB._level(res, operands, seed=seed)
    if isinstance(N_or_rays, tuple):
        R, S = N_or_rays
        rays = PB._rays(gen, R, S)
        return ps, net, ops.coords_from_rays(*rays, [[-1.5] * 3, [1.5] * 3], False), R * S, PB._gdens(gen, max(R * S, 1)), rays
    N = N_or_rays
    pts = (torch.rand(max(N, 1), 4, generator=gen) * 2.4 - 1.2).to(DEV)
    return ps, net, ops.coords_from_points(pts), N, PB._gdens(gen, max(N, 1)), pts


def _run(levels, budget, entry="budget"):
    """One launch of all `levels`; per level (gX, gp, ws, P) with gp and ws started from zero and 64 guard cells behind each."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    arr = (_lib.DensityBwdLevel * 2)()
    keep, outs = [], []
    for i, (ps, net, co, N, gdens, _) in enumerate(levels):
        desc = ps.desc()
        n_ws, P = int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), int(net.params.numel())
        ws = torch.full((n_ws + TAIL,), SENT, device=DEV)
        ws[:n_ws] = 0.0
        gp = torch.full((ps.planes.numel() + TAIL,), SENT, device=DEV)
        gp[:ps.planes.numel()] = 0.0
        gX = torch.full((N + 3, 8), SENT, device=DEV)
        a = arr[i]
        a.desc, a.planes, a.coords, a.N = C.addressof(desc), ps.planes.data_ptr(), C.addressof(co), N
        a.net, a.W, a.gdens = C.addressof(net.desc), net.params.data_ptr(), gdens.data_ptr()
        a.grad_planes, a.workspace, a.gX = gp.data_ptr(), ws.data_ptr(), gX.data_ptr()
        keep.append(desc)
        outs.append((gX, gp, ws, n_ws, P, ps.planes.numel(), N))
    if entry == "budget":
        _lib.check(L.snerf_kplanes_density_bwd_budget(arr, len(levels), budget, ops._stream()), "kplanes_density_bwd_budget")
    else:
        _lib.check(L.snerf_kplanes_density_bwd(arr, len(levels), ops._stream()), "kplanes_density_bwd")
    torch.cuda.synchronize()
    res = []
    for gX, gp, ws, n_ws, P, n_gp, N in outs:
        assert bool((gX[N:] == SENT).all()) and bool((gp[n_gp:] == SENT).all()) and bool((ws[n_ws:] == SENT).all()), "cells behind a buffer were written"
        reps = ws[:n_ws].view(REPS, -1)
        assert not bool(reps[:, P:].any()), "the padding between the workspace replicas was written"
        res.append((gX[:N], gp[:n_gp], reps[:, :P].sum(0)))
    return res


def _compare(levels, budgets):
    """Every budget against budget 0, with the spread of two budget-0 runs (one of them through the entry without a budget) as the yardstick."""
    ref, ref2 = _run(levels, 0), _run(levels, 0, entry="plain")
    for budget in budgets:
        got = _run(levels, budget)
        for lvl, ((gX, gp, gw), (gX0, gp0, gw0), (gX1, gp1, gw1)) in enumerate(zip(got, ref, ref2)):
            assert torch.equal(gX1.view(torch.int32), gX0.view(torch.int32))
            assert torch.equal(gX.view(torch.int32), gX0.view(torch.int32)), f"budget {budget} level {lvl}: gX differs in bits"
            if gX0.numel() == 0:  # an empty level: nothing is added to its buffers
                assert not bool(gp.any()) and not bool(gw.any()), f"budget {budget}: the empty level {lvl} was written"
                continue
            assert float(gp0.abs().sum()) > 0 and float(gw0.abs().sum()) > 0
            for what, x, x0, x1 in (("planes", gp, gp0, gp1), ("weights", gw, gw0, gw1)):
                err, spread = PB._rel_l2(x, x0), PB._rel_l2(x1, x0)
                print(f"budget {budget} level {lvl} {what}: rel L2 {err:.3e}, two budget-0 runs {spread:.3e}")
                assert err <= max(1e-6, 4.0 * spread), (budget, lvl, what, err, spread)


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_two_tiny_levels_fewer_pairs_than_workgroups(operands):
    """5 rays x 48 and 5 x 24 samples: 8 and 4 pairs, the last of each ragged; every budget ends at one workgroup per level (budget 1 is clamped to
    the two levels, the larger ones to the two workgroups the twelve pairs need)."""
    levels = [_make_level((16, 16, 16, 8), operands, (5, 48), 0), _make_level((32, 32, 32, 8), operands, (5, 24), 1)]
    _compare(levels, _budgets())


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_two_levels_whose_grid_follows_the_budget(operands):
    """64 rays x 50 and 1031 points: 100 + 33 pairs need 17 workgroups, so budgets 1 (clamped to 2), 2, 3 and 7 give four different grids and the
    resident ones the uncapped grid; neither N is a multiple of 32."""
    levels = [_make_level((16, 16, 16, 8), operands, (64, 50), 2), _make_level((32, 32, 32, 8), operands, 1031, 3)]
    _compare(levels, _budgets())


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_one_level_of_31_samples(operands):
    """One ragged pair: three of the workgroup's four waves have no pair."""
    _compare([_make_level((16, 16, 16, 8), operands, 31, 4)], _budgets())


@pytest.mark.parametrize("empty", [0, 1])
def test_two_levels_one_of_them_empty(empty):
    """The empty level is not launched: the grid is split as for one level, whatever the budget."""
    levels = [_make_level((16, 16, 16, 8), "bf16", 0 if empty == 0 else 777, 5), _make_level((32, 32, 32, 8), "bf16", 0 if empty == 1 else 777, 6)]
    _compare(levels, _budgets())


def test_budget_one_on_two_levels_is_clamped_to_the_levels():
    """Budget 1 cannot be met by two levels: one workgroup each, and both levels' gradients are whole (a level left without workgroups would stay at
    zero)."""
    levels = [_make_level((16, 16, 16, 8), "bf16", (37, 50), 7), _make_level((32, 32, 32, 8), "bf16", (37, 20), 8)]
    _compare(levels, [1])


def test_bad_arguments_are_refused_as_without_a_budget():
    from soccernerfs_amd import _lib

    L = _lib.lib()
    assert L.snerf_kplanes_density_bwd_budget(None, 1, 3, None) != 0 and b"kplanes_density_bwd" in L.snerf_last_error()


# ------------------------------------------------------------------------------------------------ the exact lattice
LATTICE = [0, 2, 4, 6]  # F.density_bwd_pairs(): (1000 points, 37 x 50 ray samples) and (12 x 5 ray samples, 129 points), bf16 and fp16 operands


@pytest.mark.parametrize("k", LATTICE)
def test_lattice_every_budget_gives_the_float64_answer_in_bits(k):
    """Products and sums are exact in fp32 here, so the grouping cannot show: gX, the weight gradients (replicas summed, on top of 0.25) and
    the plane gradients (on top of 0.5) equal the float64 answer for every budget, and so each other."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    pair = [c._replace(ws0=0.25, gp0=0.5) for c in F.density_bwd_pairs()[k]]
    inputs = [LT._Inputs(c) for c in pair]
    first = None
    for budget in _budgets():
        levels = [(inp, LT._level_buffers(inp, L)) for inp in inputs]
        arr = (_lib.DensityBwdLevel * 2)()
        for i, (inp, b) in enumerate(levels):
            LT._fill_level(arr[i], inp, b)
        _lib.check(L.snerf_kplanes_density_bwd_budget(arr, 2, budget, ops._stream()), "kplanes_density_bwd_budget")
        torch.cuda.synchronize()
        for i, (inp, b) in enumerate(levels):
            LT._check_level(inp, b, f"pair {k} budget {budget} level {i} {F.case_id(inp.c)}", "fused", L, reduce=False)
        # the workspace itself is not compared: which of its 16 replicas a workgroup adds to follows its index, so only their sum is an output
        bits = [t.view(torch.int32).clone() for _, b in levels for t in (b["gX"], b["gp"]) if t is not None]
        bits += [b["ws"][:b["n_ws"]].view(REPS, -1).double().sum(0) for _, b in levels]
        if first is None:
            first = bits
        assert all(torch.equal(x, y) for x, y in zip(bits, first)), f"pair {k}: budget {budget} differs in bits from budget {_budgets()[0]}"


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_gradients_with_and_without_the_budget():
    """One forward + backward that updates the proposal networks at R = 64: every gradient segment with the default budget, with one workgroup
    per CU and with four workgroups in all within the bound of two uncapped runs."""
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    R = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grads = []
    for budget in (None, 1.0, 4.0 / cus, 0.0, 0.0):  # 4 / cus: four workgroups, fewer than the 28 this batch would take
        kw = {} if budget is None else {"proposal_backward_workgroups_per_cu": budget}
        tr = KPlanesTrainer(KPlanesTrainConfig(**kw, **PB.SMALL), R, DEV)
        assert tr.fused_proposal_backward
        assert tr._prop_bwd_workgroups == int(round(tr.cfg.proposal_backward_workgroups_per_cu * cus))
        rays, target, rng = PB._batch(torch.Generator(device=DEV).manual_seed(5), R)
        tr.forward(rays, rng, 1.0, training=True)
        tr.backward(target, rng, proposal_grads=True)
        tr.synchronize()
        grads.append({k: v.clone() for k, v in tr.gviews.items()})
    g_def, g_one, g_four, g_0, g_0b = grads
    assert set(g_0) >= {"prop0.planes", "prop1.planes", "prop0.mlp", "prop1.mlp"}
    for k in g_0:
        assert float(g_0[k].abs().sum()) > 0, k
        spread = PB._rel_l2(g_0b[k], g_0[k])
        for name, g in (("default", g_def), ("1.0 per CU", g_one), ("4 workgroups", g_four)):
            err = PB._rel_l2(g[k], g_0[k])
            print(f"{k} {name}: rel L2 {err:.3e}, two uncapped runs {spread:.3e}")
            assert err <= max(1e-6, 4.0 * spread), (k, name, err, spread)

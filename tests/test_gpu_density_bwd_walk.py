"""GPU: the block walk of the fused proposal density backward (csrc/proposal_bwd.hip: density_bwd_kernel's run-length combined scatter).

The kernel walks a 32-sample pair in blocks of eight: it reads a block's taps and gradient factors from LDS before the first use, forms the 3 x 8
keys and values of the lane's streams lane-parallel, and then runs the run logic over registers in sample order; a short last pair's remainder
goes one sample at a time.  A run continues across blocks, pairs and the wave's whole range; a flush is one atomic under the lane's predicate,
addressed by a 32-bit byte offset from the level's gradient view (or by the 64-bit form where that view reaches 2^31 bytes).

Planted cases (the lattice of tests/fused_reference.py with THIS file's coordinates; every sum is exact, so the comparison is equality with the
float64 answer, for every budget of {0, 1, 2, 3} workgroups -- a wave's range is then one pair, several pairs or none):

* N in {1, 7, 8, 9, 31, 32, 33, 40, 69}: one lane, a short block, one block, a block and a remainder, a full pair, a pair and a remainder of
  less and of more than a block;
* every sample in ONE cell of every plane (one run across blocks, pairs and the wave's range); another cell on EVERY sample (every link
  flushes); another cell exactly at samples 8k, and at 32k (runs end on block and on pair boundaries); samples on and beyond the last texel and
  before the first (i1 == i0: the clamped corner's sums are zero and are not sent);
* coords.mode 0 (points) and 1 (ray samples: direction 0 puts a ray in one cell, so runs end every S samples, S = 5, 8, 32);
* one level, and two levels of different resolutions in one launch, in both orders (a stream's plane width and base are its own level's);
* bf16 and fp16 operands, with and without the hidden ReLU.

Against the unfused kernels (snerf_mlp_bwd_ws + snerf_kplanes_gather_bwd), with the bound of tests/test_gpu_proposal_bwd_fused.py (gX in bits;
plane and weight gradients within max(1e-6, 4 x the spread of two unfused runs) relative L2):

* contracted ray coordinates (coords.contract = 1) at the same N, both operand types, every budget;
* a level whose descriptor puts its last plane 2^31 bytes into the buffer: the 64-bit flush, beside a level on the 32-bit one in the same call."""
import ctypes as C

import pytest
import torch

from tests import fused_reference as F
from tests import mlp_reference as R
from tests import test_gpu_fused_lattice as LT
from tests import test_gpu_proposal_bwd_fused as PB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
BUDGETS = (0, 1, 2, 3)
NS = (1, 7, 8, 9, 31, 32, 33, 40, 64 + 5)
PATTERNS = ("one_cell", "every_sample", "every_8", "every_32", "border")
# two cells that differ on every axis at both resolutions ([5,5,5,3] and [9,9,9,3]): x in {0, 1/8} and x in {-1/2, -3/8}; time likewise
CELL = (0.0, -0.5)
BORDER = (1.0, 1.25, -1.25, -1.0)


def _cells(pattern, n):
    """Which of the two cells sample n lies in."""
    return {"one_cell": 0 * n, "every_sample": n % 2, "every_8": (n // 8) % 2, "every_32": (n // 32) % 2}[pattern]


def _points(pattern, N, gen):
    n = torch.arange(N)
    if pattern == "border":
        vals = torch.tensor(BORDER, dtype=F64)
        return torch.stack([vals[(n + k) % 4] for k in range(4)], dim=1).contiguous()
    base = torch.tensor(CELL, dtype=F64)[_cells(pattern, n)]
    return (base[:, None] + 0.125 * torch.randint(0, 2, (N, 4), generator=gen).to(F64)).contiguous()  # another place in the cell per sample


def _rays(Rn, S, moving, gen):
    """Rays alternating between the two cells; direction 0 (every sample of a ray in its cell) or steps of 1/8 per unit of e[s] + e[s+1]."""
    base = torch.tensor(CELL, dtype=F64)[torch.arange(Rn) % 2]
    o = (base[:, None] + 0.125 * torch.randint(0, 2, (Rn, 3), generator=gen).to(F64)).contiguous()
    d = 0.25 * torch.randint(-1, 2, (Rn, 3), generator=gen).to(F64) if moving else torch.zeros(Rn, 3, dtype=F64)
    eb = torch.cumsum((torch.rand(Rn, S + 1, generator=gen) < 0.5).to(F64), dim=1)
    t = (base + 0.125 * torch.randint(0, 2, (Rn,), generator=gen).to(F64) + 1) / 2
    return {"mode": 1, "o": o, "d": d, "eb": eb, "t": t, "rescale": 1, "aabb": [[-1.0] * 3, [1.0] * 3]}


def _plant(c, co):
    """F._make's proposal-backward case on THIS file's coordinates: the case's planes and nets, the float64 answer, and its conditions of
    exactness asserted (the nets' roundings and sums, the dyadic target, float32 answers, every texel's sum within 2^24 units)."""
    cid = F.case_id(c)
    gen = torch.Generator().manual_seed(F._seed(c))
    ps = F._plane_set(c)
    planes = F._planes(c, ps, gen)
    p = F.coordinates(co, 4)
    N = p.shape[0]
    feat, _ = F.gather(ps, planes, p, "4")
    Ws = F._proposal_net(c, feat, gen)
    T = torch.tensor(R.TARGETS, dtype=F64)[torch.randint(0, 3, (N,), generator=gen)]
    z = F.proposal(feat, Ws, c.relu, c.operands)["z"][:, 0]
    gdens = (T / torch.exp(z.clamp(-15.0, 15.0))).float()
    trace = []
    ref = F.proposal(feat, Ws, c.relu, c.operands, gdens, trace=trace)
    R.check_trace(trace, cid)
    assert torch.equal(ref["g_out"][:, 0], T), f"{cid}: the rounded gradient tile is not the dyadic target"
    gp = F.plane_grads(ps, planes, p, "4", ref["gX"])
    ab, u = F.plane_grads(ps, planes, p, "4", ref["gX"], absolute=True)
    assert float(ab.max()) / u < 2.0 ** 24, f"{cid}: a texel's gradient sums {float(ab.max()) / u:.3g} units"
    for name, t in (("gX", ref["gX"]), ("gW", ref["gW"]), ("plane gradient", gp)):
        assert torch.equal(t.float().double(), t), f"{cid}: {name} is not a float32 value"
    return {"ps": ps, "planes": planes, "co": co, "N": N, "n_coords": 4, "p": p, "feat": feat, "Ws": Ws, "W": torch.cat([w.reshape(-1) for w in Ws]),
            "gdens": gdens, "T": T, "ref": ref, "gp": gp}


class _Planted(LT._Inputs):
    """The device side of a planted case (LT._Inputs on a case made here, not by F.make)."""

    def __init__(self, c, m):
        from soccernerfs_amd import ops

        self.c, self.m = c, m
        self.N, self.ps = m["N"], m["ps"]
        self.planes = m["planes"].float().to(DEV)
        self.desc = self.ps.desc()
        co = m["co"]
        g = lambda t: t.float().to(DEV).contiguous()
        if co["mode"] == 0:
            self.keep = [g(torch.cat([co["pts"], torch.full((LT.GR, 4), float("nan"), dtype=F64)]))]  # guard rows: nothing reads past N
            self.co = ops.coords_from_points(self.keep[0])
        else:
            self.o, self.d, self.eb, self.t = g(co["o"]), g(co["d"]), g(co["eb"]), g(co["t"])
            self.co = ops.coords_from_rays(self.o, self.d, self.t, self.eb, co["aabb"], True)


def _case(k, m, **shape):
    """The k-th planted case: resolution multiplier m, operands and ReLU rotating with k; `special` = k walks the plane that holds the integers."""
    return F._case("dbwd", "weights", "4", k, ms=(m,), operands=k % 2 + 1, relu=int(k % 3 != 2), **shape)


def _planted_points(k, pattern, N, m):
    c = _case(k, m, N=N)
    return _Planted(c, _plant(c, {"mode": 0, "pts": _points(pattern, N, torch.Generator().manual_seed(100 + k))}))


def _planted_rays(k, Rn, S, moving, m):
    c = _case(k, m, R_=Rn, S=S)
    return _Planted(c, _plant(c, _rays(Rn, S, moving, torch.Generator().manual_seed(200 + k))))


def _launch(levels, budget, L):
    from soccernerfs_amd import _lib, ops

    arr = (_lib.DensityBwdLevel * 2)()
    for i, (inp, b) in enumerate(levels):
        LT._fill_level(arr[i], inp, b)
    _lib.check(L.snerf_kplanes_density_bwd_budget(arr, len(levels), budget, ops._stream()), "kplanes_density_bwd_budget")
    torch.cuda.synchronize()


def _exact(inputs, what):
    """Every budget gives the float64 answer in bits: gX, the weight gradients (replicas summed) and the plane gradients of every level."""
    from soccernerfs_amd import _lib

    L = _lib.lib()
    for budget in BUDGETS:
        levels = [(inp, LT._level_buffers(inp, L)) for inp in inputs]
        _launch(levels, budget, L)
        for i, (inp, b) in enumerate(levels):
            LT._check_level(inp, b, f"{what} budget {budget} level {i} {F.case_id(inp.c)}", "fused", L, reduce=False)


ONE_LEVEL = [(pattern, N) for pattern in PATTERNS for N in NS]


@pytest.mark.parametrize("pattern,N", ONE_LEVEL, ids=[f"{p}-N{n}" for p, n in ONE_LEVEL])
def test_planted_points_one_level(pattern, N):
    k = ONE_LEVEL.index((pattern, N))
    inp = _planted_points(k, pattern, N, (1, 2)[(k // 2) % 2])
    _exact([inp], pattern)
    if N == NS[-1]:  # the unfused pair gives the same answer: the planted case is one both sides meet
        from soccernerfs_amd import _lib

        L = _lib.lib()
        LT._check_level(inp, LT._unfused(inp, LT._level_buffers(inp, L), L), f"{pattern} {F.case_id(inp.c)}", "unfused", L, reduce=False)


RAYS = [(4, 8, 0), (3, 32, 0), (7, 5, 0), (8, 5, 1), (2, 33, 1), (1, 1, 0)]


@pytest.mark.parametrize("Rn,S,moving", RAYS, ids=[f"R{r}xS{s}-{'moving' if mv else 'still'}" for r, s, mv in RAYS])
def test_planted_ray_samples_one_level(Rn, S, moving):
    k = RAYS.index((Rn, S, moving))
    _exact([_planted_rays(k, Rn, S, moving, (1, 2)[k % 2])], "rays")


# two levels of different resolutions in one launch, in both orders; operands alike, as the ABI asks (k and k + 2 have the same parity)
TWO_LEVELS = [("one_cell", 40, "every_sample", 69), ("every_8", 69, "border", 33), ("every_32", 69, "one_cell", 7), ("every_sample", 9, "every_8", 31)]


@pytest.mark.parametrize("pa,Na,pb,Nb", TWO_LEVELS, ids=[f"{a}-N{na}+{b}-N{nb}" for a, na, b, nb in TWO_LEVELS])
def test_planted_two_levels_in_one_launch(pa, Na, pb, Nb):
    k = TWO_LEVELS.index((pa, Na, pb, Nb))
    a, b = _planted_points(k, pa, Na, 1), _planted_points(k + 2, pb, Nb, 2)
    assert a.c.operands == b.c.operands and a.ps.resolutions != b.ps.resolutions
    _exact([a, b], "two levels")
    _exact([b, a], "two levels, swapped")


def test_planted_points_beside_ray_samples():
    """coords.mode 0 and 1 in one launch, the ray level's runs ending every 5 samples."""
    a, b = _planted_points(1, "every_8", 69, 2), _planted_rays(3, 7, 5, 0, 1)
    assert a.c.operands == b.c.operands
    _exact([a, b], "points + rays")
    _exact([b, a], "rays + points")


# ------------------------------------------------------------------------------------------------ against the unfused kernels
def _fused(levels, budget):
    """PB._fused through the entry with a budget.  levels: (ps, net, co, N, gdens, desc or None)."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    arr = (_lib.DensityBwdLevel * len(levels))()
    keep, outs = [], []
    for i, (ps, net, co, N, gdens, desc) in enumerate(levels):
        desc = ps.desc() if desc is None else desc
        ws = torch.zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(net.desc))), device=DEV)
        gX = torch.full((N, 8), -7.0, device=DEV)
        gp = torch.zeros_like(ps.planes)
        a = arr[i]
        a.desc, a.planes, a.coords, a.N = C.addressof(desc), ps.planes.data_ptr(), C.addressof(co), N
        a.net, a.W, a.gdens = C.addressof(net.desc), net.params.data_ptr(), gdens.data_ptr()
        a.grad_planes, a.workspace, a.gX = gp.data_ptr(), ws.data_ptr(), gX.data_ptr()
        keep.append(desc)
        outs.append((gX, gp, ws))
    _lib.check(L.snerf_kplanes_density_bwd_budget(arr, len(levels), budget, ops._stream()), "kplanes_density_bwd_budget")
    torch.cuda.synchronize()
    return [(gX, gp, ws.view(PB.REPS, -1).sum(0)) for gX, gp, ws in outs]


def _bounded(fused, unfused, unfused2, what):
    """PB._check's rule against unfused results computed once."""
    (gX_f, gp_f, gw_f), (gX_u, gp_u, gw_u), (_, gp_u2, gw_u2) = fused, unfused, unfused2
    assert torch.equal(gX_f, gX_u), f"{what}: gX differs in bits"
    assert float(gp_u.abs().sum()) > 0 and float(gw_u.abs().sum()) > 0
    for name, f, u, u2 in (("planes", gp_f, gp_u, gp_u2), ("weights", gw_f, gw_u, gw_u2)):
        err, spread = PB._rel_l2(f, u), PB._rel_l2(u2, u)
        print(f"{what} {name}: rel L2 {err:.3e}, two unfused runs {spread:.3e}")
        assert err <= max(1e-6, 4.0 * spread), (what, name, err, spread)


CONTRACTED = [(1, 1), (1, 7), (1, 8), (3, 3), (1, 31), (4, 8), (3, 11), (5, 8), (3, 23)]  # R x S = 1, 7, 8, 9, 31, 32, 33, 40, 69


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_contracted_ray_samples_against_the_unfused_kernels(operands):
    """coords.contract = 1 (the kernel's other instantiation), far samples crowded against the planes' border."""
    from soccernerfs_amd import ops

    ps, net, gen = PB._level((24, 20, 18, 5), operands, seed=11)
    for Rn, S in CONTRACTED:
        o, d, t, eb = PB._rays(gen, Rn, S)
        co = ops.coords_from_rays(o, d, t, eb * 4.0, None, True, contract=True)
        N = Rn * S
        gd = PB._gdens(gen, N) if N > 8 else (torch.randn(N, generator=gen) * 1e-3).to(DEV)  # N = 1, 7, 8: no sample without gradient
        u, u2 = PB._unfused(ps, net, co, N, gd), PB._unfused(ps, net, co, N, gd)
        for budget in BUDGETS:
            _bounded(_fused([(ps, net, co, N, gd, None)], budget)[0], u, u2, f"contracted {operands} R{Rn}xS{S} budget {budget}")


def test_a_view_that_reaches_2_to_the_31_bytes_takes_the_64_bit_flush():
    """A descriptor whose last plane starts 2^29 floats into the buffer (nothing in between is read or written): its level cannot be addressed
    by 32-bit byte offsets, so the call takes the kernel's 64-bit form -- for the ordinary level beside it as well."""
    from soccernerfs_amd import ops

    ps, net, gen = PB._level((16, 12, 9, 4), "bf16", seed=21)
    ps2, net2, _ = PB._level((9, 7, 5, 3), "bf16", seed=22)
    n5 = ps.shapes[0][5][0] * ps.shapes[0][5][1] * 8
    far = 1 << 29
    big = torch.empty(far + n5, device=DEV)
    big[:ps.numel] = ps.planes.detach()
    big[far:] = ps.planes.detach()[ps.offsets[0][5]:ps.offsets[0][5] + n5]
    desc = ps.desc()
    desc.off[0][5] = far

    class _Far:  # what _fused and PB._unfused read of a plane set
        planes = big

        @staticmethod
        def desc():
            return desc

    N = 1031
    pts = (torch.rand(N, 4, generator=gen) * 3.0 - 1.5).to(DEV)
    co = ops.coords_from_points(pts)
    gd = PB._gdens(gen, N)
    fused = _fused([(_Far, net, co, N, gd, desc), (ps2, net2, co, N, gd, None)], 0)
    near_u, near_u2 = PB._unfused(ps, net, co, N, gd), PB._unfused(ps, net, co, N, gd)

    def fold(gp):  # the far level's gradient in the near layout
        assert not bool(gp[ps.offsets[0][5]:far].any()), "cells between the planes were written"
        return torch.cat([gp[:ps.offsets[0][5]], gp[far:]])

    _bounded((fused[0][0], fold(fused[0][1]), fused[0][2]), near_u, near_u2, "far plane")
    _bounded(fused[1], PB._unfused(ps2, net2, co, N, gd), PB._unfused(ps2, net2, co, N, gd), "the level beside it")

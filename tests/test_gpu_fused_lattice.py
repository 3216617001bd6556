"""The fused gather-to-MLP kernels and the plane gather against exact float64 answers (tests/fused_reference.py), through the C ABI.

Every case is built so that coordinates, tap weights, plane values, features, operand roundings, both nets, the product rule and the scatter are
exact at once (the generator asserts it in float64), so every comparison is an EQUALITY with the float64 answer rounded to fp32: features, feat16,
feat32, h, gX, the weight gradients (the 16 workspace replicas summed, or folded by snerf_mlp_gw_reduce) and the plane gradients.  Density and rgb
are exact (1.0 and 0.5) on the planted rows, at least one eighth of every case, and bounded on the others by 5 x the float32 restatement's
deviation (profiles/r25_fused_deviations.json; a case missing from it fails).

  A  snerf_kplanes_gather_fwd: points and ray samples, C = 8 summed and C = 32 concatenated, every view.
  B  snerf_kplanes_density_fwd: features, densities; the same densities with the feature output NULL.
  C  snerf_kplanes_density_bwd: each level alone (the absent second level's buffers untouched), both levels in one launch and swapped; gX asked
     for and NULL, workspace from 0 and 0.25, plane gradients from 0 and 0.5; the unfused pair snerf_mlp_bwd_ws + snerf_kplanes_gather_bwd against
     the same answer, so that a disagreement names its side.
  D  snerf_kplanes_field_fwd, its three-plane instantiation and _ordered (an order from snerf_ray_time_order on times with ties): feat32,
     feat16, h exact; ordered equals unordered in bits.
Views: four coordinates, three coordinates, and the frozen-time view (PlaneSet.space_desc) of a four-coordinate buffer whose time planes hold NaN.
Every output is prefilled with a sentinel and carries guard rows after N (cells after the end, for flat buffers) that must keep it."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import fused_reference as F
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, GR, TAIL, REPS = 7.0, F.GUARD_ROWS, 64, 16
_X16 = {1: torch.bfloat16, 2: torch.float16}

with open(os.path.join(ROOT, "profiles", "r25_fused_deviations.json")) as _f:
    _REC = json.load(_f)
BOUNDS, FACTOR = _REC["cases"], _REC["factor"]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _out(N, w=None, dtype=torch.float32):
    return torch.full((N + GR,) if w is None else (N + GR, w), SENT, device=DEV, dtype=dtype)


def _flat(n, start):
    b = torch.full((n + TAIL,), SENT, device=DEV)
    b[:n] = start
    return b


def _same(got, want, cid, what):
    """Equality of a device result with the float64 answer (itself a float32 value); prints the count of differing cells and the largest difference."""
    w32 = want.float()
    assert torch.equal(w32.double().nan_to_num(), want.double().nan_to_num()), f"{cid}: the answer's {what} is not a float32 value"
    g = got.detach().cpu().double().nan_to_num(nan=-123.0)
    w = w32.double().nan_to_num(nan=-123.0)
    diff = g != w
    print(f"{cid} {what}: {int(diff.sum())} of {g.numel()} cells differ, max |diff| {float((g - w).abs().max()) if g.numel() else 0.0:.3g}")
    if bool(diff.any()):
        i = tuple(diff.nonzero()[0].tolist())
        raise AssertionError(f"{cid}: {what} differs in {int(diff.sum())} of {g.numel()} cells; first at {list(i)}: kernel {float(g[i])!r}, answer {float(w[i])!r}")


def _guards(buf, N, cid, what):
    assert bool((buf[N:].float() == SENT).all()), f"{cid}: {what}: cells behind element {N} were written"


def _heads(got, want64, planted, exact, cid, what):
    """Planted rows: exactly `exact`.  The others: elementwise within FACTOR x the case's float32 yardstick of the float64 answer."""
    key = F.case_id(F.content_key(_CASE[cid.split(" ")[0]]))
    assert key in BOUNDS and what in BOUNDS[key], f"{cid}: no yardstick for {what} in profiles/r25_fused_deviations.json"
    g = got.detach().cpu().double()
    assert bool((want64[planted] == exact).all())
    bad = int((g[planted] != exact).sum())
    rest = ~planted
    rel = float(((g[rest] - want64[rest]).abs() / want64[rest].abs()).max()) if bool(rest.any()) else 0.0
    bound = FACTOR * BOUNDS[key][what]
    print(f"{cid} {what}: {bad} of {int(planted.sum())} planted rows differ from {exact}; other rows deviate {rel:.3e} / bound {bound:.3e}")
    assert bad == 0, f"{cid}: {what} is not exactly {exact} on {bad} planted rows"
    assert rel <= bound, f"{cid}: {what} deviates {rel:.3e} from float64, bound {bound:.3e}"


_CASE = {}


def _ids(cases):
    out = []
    for c in cases:
        _CASE[F.case_id(c)] = c
        out.append(F.case_id(c))
    return out


class _Inputs:
    """The device side of a case: the plane buffer, the descriptor of its view and the coordinates (buffers kept alive here)."""

    def __init__(self, c):
        from soccernerfs_amd import ops

        self.c, self.m = c, F.make(c)
        m = self.m
        self.N, self.ps = m["N"], m["ps"]
        self.planes = m["planes"].float().to(DEV)
        self.desc = self.ps.space_desc() if c.view == "frozen" else self.ps.desc()
        co = m["co"]
        if co["mode"] == 0:
            pts = torch.cat([co["pts"].float(), torch.full((GR, m["n_coords"]), float("nan"))])  # guard rows: nothing reads past N
            self.keep = [pts.to(DEV).contiguous()]
            self.co = ops.coords_from_points(self.keep[0])
        else:
            g = lambda t: t.float().to(DEV).contiguous()
            self.o, self.d, self.eb = g(co["o"]), g(co["d"]), g(co["eb"])
            self.t = g(co["t"]) if co["t"] is not None else None
            self.co = ops.coords_from_rays(self.o, self.d, self.t, self.eb, co["aabb"], bool(co["rescale"]))

    def net(self, d_in, hidden, n_hidden, d_out, hidden_act, out_act):
        from soccernerfs_amd import _lib

        d = _lib.MlpDesc()
        d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d_in, hidden, n_hidden, d_out, hidden_act, out_act, self.c.operands
        return d


def _gather(inp):
    from soccernerfs_amd import _lib, ops

    out = _out(inp.N, inp.ps.out_dim)
    _lib.check(_lib.lib().snerf_kplanes_gather_fwd(C.byref(inp.desc), _p(inp.planes), C.byref(inp.co), C.c_int64(inp.N), _p(out), ops._stream()), "gather_fwd")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ A
GATHER = F.gather_cases()


@pytest.mark.parametrize("cid", _ids(GATHER))
def test_gather_forward_is_exact(cid):
    c = _CASE[cid]
    assert F.SUPPORT[("gather", c.view)] == 1
    inp = _Inputs(c)
    out = _gather(inp)
    _same(out[:inp.N], inp.m["feat"], cid, "features")
    _guards(out, inp.N, cid, "features")


# ------------------------------------------------------------------------------------------------ B
DFWD = F.density_fwd_cases()


@pytest.mark.parametrize("cid", _ids(DFWD))
def test_density_forward(cid):
    from soccernerfs_amd import _lib, ops

    c = _CASE[cid]
    inp = _Inputs(c)
    m, N, L = inp.m, inp.N, _lib.lib()
    net = inp.net(8, 64, 1, 1, c.relu, 0)
    assert L.snerf_kplanes_density_fwd_supported(C.byref(inp.desc), C.byref(net)) == F.SUPPORT[("dfwd", c.view)] == 1
    W = m["W"].float().to(DEV)
    dens, feat, dens2 = _out(N), _out(N, 8), _out(N)
    head = (C.byref(inp.desc), _p(inp.planes), C.byref(inp.co), C.c_int64(N), C.byref(net), _p(W))
    _lib.check(L.snerf_kplanes_density_fwd(*head, _p(dens), _p(feat), ops._stream()), "density_fwd")
    _lib.check(L.snerf_kplanes_density_fwd(*head, _p(dens2), None, ops._stream()), "density_fwd")
    torch.cuda.synchronize()
    _same(feat[:N], m["feat"], cid, "features")
    _heads(dens[:N], m["ref"]["aux"], m["planted"], 1.0, cid, "density")
    assert torch.equal(dens2.view(torch.int32), dens.view(torch.int32)), f"{cid}: the densities change when the feature output is NULL"
    _guards(feat, N, cid, "features")
    _guards(dens, N, cid, "density")


# ------------------------------------------------------------------------------------------------ C
def _level_buffers(inp, L):
    from soccernerfs_amd import _lib

    c, N = inp.c, inp.N
    b = {"net": inp.net(8, 64, 1, 1, c.relu, 0), "W": inp.m["W"].float().to(DEV)}
    b["P"] = inp.m["W"].numel()
    n = int(L.snerf_mlp_gw_workspace_floats(C.byref(b["net"])))
    assert n % REPS == 0 and n // REPS >= b["P"]
    b["ws"] = _flat(n, 0.0)
    if c.ws0:
        b["ws"][:n].view(REPS, -1)[:, :b["P"]] = c.ws0  # an earlier launch's share: the kernel ACCUMULATES into the replicas
    b["n_ws"] = n
    b["gX"] = None if c.nogx else _out(N, 8)
    b["gp"] = _flat(inp.ps.numel, c.gp0)
    b["gdens"] = torch.cat([inp.m["gdens"], torch.full((GR,), float("nan"))]).to(DEV)
    return b


def _fill_level(a, inp, b):
    a.desc, a.planes, a.coords, a.N = C.addressof(inp.desc), inp.planes.data_ptr(), C.addressof(inp.co), inp.N
    a.net, a.W, a.gdens = C.addressof(b["net"]), b["W"].data_ptr(), b["gdens"].data_ptr()
    a.grad_planes, a.workspace, a.gX = b["gp"].data_ptr(), b["ws"].data_ptr(), b["gX"].data_ptr() if b["gX"] is not None else None


def _check_level(inp, b, cid, side, L, reduce):
    from soccernerfs_amd import _lib, ops

    c, m, N, P = inp.c, inp.m, inp.N, b["P"]
    if b["gX"] is not None:
        _same(b["gX"][:N], m["ref"]["gX"], cid, f"{side} gX")
        _guards(b["gX"], N, cid, f"{side} gX")
    reps = b["ws"][:b["n_ws"]].view(REPS, -1).cpu().double()
    assert not bool(reps[:, P:].any()), f"{cid}: {side}: the padding between the workspace replicas was written"
    _same(reps[:, :P].sum(0), m["ref"]["gW"] + REPS * c.ws0, cid, f"{side} weight gradients (16 replicas summed)")
    _guards(b["ws"], b["n_ws"], cid, f"{side} workspace")
    if reduce:
        gW = _flat(P, 0.25)
        _lib.check(L.snerf_mlp_gw_reduce(C.byref(b["net"]), _p(b["ws"]), _p(gW), ops._stream()), "gw_reduce")
        torch.cuda.synchronize()
        _same(gW[:P], m["ref"]["gW"] + REPS * c.ws0 + 0.25, cid, f"{side} weight gradients (snerf_mlp_gw_reduce)")
        _guards(gW, P, cid, f"{side} gW")
    _same(b["gp"][:inp.ps.numel], m["gp"] + c.gp0, cid, f"{side} plane gradients")
    _guards(b["gp"], inp.ps.numel, cid, f"{side} plane gradients")


def _unfused(inp, b, L):
    """snerf_kplanes_gather_fwd + snerf_mlp_bwd_ws + snerf_kplanes_gather_bwd on the same inputs, into buffers that start as the fused ones did."""
    from soccernerfs_amd import _lib, ops

    u = _level_buffers(inp, L)
    if u["gX"] is None:
        u["gX"] = _out(inp.N, 8)
    feat = _gather(inp)
    st = ops._stream()
    _lib.check(L.snerf_mlp_bwd_ws(C.byref(u["net"]), _p(u["W"]), _p(feat), 8, C.c_int64(inp.N), None, 1, 0, _p(u["gdens"]), _p(u["gX"]), 8, _p(u["ws"]), st), "mlp_bwd_ws")
    _lib.check(L.snerf_kplanes_gather_bwd(C.byref(inp.desc), _p(inp.planes), C.byref(inp.co), C.c_int64(inp.N), _p(u["gX"]), _p(u["gp"]), st), "gather_bwd")
    torch.cuda.synchronize()
    return u


def _launch(levels, n_levels, L):
    from soccernerfs_amd import _lib, ops

    arr = (_lib.DensityBwdLevel * 2)()
    for i, (inp, b) in enumerate(levels):
        _fill_level(arr[i], inp, b)
    _lib.check(L.snerf_kplanes_density_bwd(arr, n_levels, ops._stream()), "kplanes_density_bwd")
    torch.cuda.synchronize()


DBWD = F.density_bwd_cases()


@pytest.mark.parametrize("cid", _ids(DBWD))
def test_density_backward_one_level(cid):
    from soccernerfs_amd import _lib

    c, L = _CASE[cid], _lib.lib()
    inp = _Inputs(c)
    b = _level_buffers(inp, L)
    assert L.snerf_kplanes_density_bwd_supported(C.byref(inp.desc), C.byref(b["net"])) == F.SUPPORT[("dbwd", c.view)] == 1
    # the absent second level: a valid entry behind n_levels = 1 whose buffers must stay as they are
    other = _Inputs(F.density_bwd_pairs()[0][1 if c.operands == 1 else 0]._replace(operands=c.operands))
    ob = _level_buffers(other, L)
    before = {k: ob[k].clone() for k in ("ws", "gp")}
    _launch([(inp, b), (other, ob)], 1, L)
    _check_level(inp, b, cid, "fused", L, reduce=c.special % 2 == 0)
    assert torch.equal(ob["ws"], before["ws"]) and torch.equal(ob["gp"], before["gp"]), f"{cid}: the absent second level's buffers were written"
    if ob["gX"] is not None:
        assert bool((ob["gX"] == SENT).all()), f"{cid}: the absent second level's gX was written"
    u = _unfused(inp, b, L)
    _check_level(inp, u, cid, "unfused", L, reduce=False)


PAIRS = F.density_bwd_pairs()


@pytest.mark.parametrize("k", range(len(PAIRS)), ids=[f"{i}-" + "+".join(_ids(pr)) for i, pr in enumerate(PAIRS)])
def test_density_backward_two_levels_in_one_launch(k):
    from soccernerfs_amd import _lib

    L = _lib.lib()
    levels = []
    for c in PAIRS[k]:
        inp = _Inputs(c)
        levels.append((inp, _level_buffers(inp, L)))
    _launch(levels, 2, L)
    for i, (inp, b) in enumerate(levels):
        _check_level(inp, b, f"pair {k} level {i} {F.case_id(inp.c)}", "fused", L, reduce=(k + i) % 2 == 0)


# ------------------------------------------------------------------------------------------------ D
FIELD = F.field_cases()


def _field_run(inp, sig, col, Wsig, Wcol, keep, order, L):
    from soccernerfs_amd import _lib, ops

    N, K0 = inp.N, inp.ps.out_dim
    out = {"density": _out(N), "rgb": _out(N, 3)}
    if keep >= 1:
        out["feat16"], out["h"] = _out(N, K0, _X16[inp.c.operands]), _out(N, 16)
    if keep == 2:
        out["feat32"] = _out(N, K0)
    head = (C.byref(inp.desc), _p(inp.planes), C.byref(inp.co), C.c_int64(N), C.byref(sig), _p(Wsig), C.byref(col), _p(Wcol), _p(out["density"]), _p(out["rgb"]),
            _p(out.get("feat16")), _p(out.get("h")), _p(out.get("feat32")))
    if order is None:
        rc = L.snerf_kplanes_field_fwd(*head, ops._stream())
    else:
        rc = L.snerf_kplanes_field_fwd_ordered(*head, _p(order), ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _field_nets(inp):
    sig, col = inp.net(inp.ps.out_dim, 128, 1, 16, 1, 0), inp.net(15, 64, 2, 3, 1, 1)
    return sig, col, inp.m["Wsig_flat"].float().to(DEV), inp.m["Wcol_flat"].float().to(DEV)


def _check_field(inp, out, cid):
    m, N = inp.m, inp.N
    ref = m["ref"]
    if "feat32" in out:
        _same(out["feat32"][:N], m["feat"], cid, "feat32")
    if "feat16" in out:
        _same(out["feat16"][:N].float(), m["feat"], cid, "feat16")
        _same(out["h"][:N], ref["h"], cid, "h")
    _heads(out["density"][:N], ref["density"], m["planted"], 1.0, cid, "density")
    pl3 = m["planted"][:, None].expand(N, 3)
    _heads(out["rgb"][:N], ref["rgb"], pl3, 0.5, cid, "rgb")
    for k, v in out.items():
        _guards(v, N, cid, k)


@pytest.mark.parametrize("cid", _ids(FIELD))
def test_field_forward(cid):
    from soccernerfs_amd import _lib, ops

    c, L = _CASE[cid], _lib.lib()
    inp = _Inputs(c)
    sig, col, Wsig, Wcol = _field_nets(inp)
    assert L.snerf_kplanes_field_fwd_supported(C.byref(inp.desc), C.byref(sig), C.byref(col)) == F.SUPPORT[("field", c.view)] == 1
    rc, out = _field_run(inp, sig, col, Wsig, Wcol, c.keep, None, L)
    _lib.check(rc, "field_fwd")
    _check_field(inp, out, cid)
    if c.keep:  # the optional outputs do not change the others
        rc, bare = _field_run(inp, sig, col, Wsig, Wcol, 0, None, L)
        _lib.check(rc, "field_fwd")
        assert torch.equal(bare["density"].view(torch.int32), out["density"].view(torch.int32)) and torch.equal(bare["rgb"].view(torch.int32), out["rgb"].view(torch.int32))
    if c.order:
        assert F.SUPPORT[("field_ordered", c.view)] == 1
        times = inp.m["co"]["t"]
        assert times.unique().numel() < times.numel()  # ties
        order = ops.ray_time_order(inp.t)
        assert torch.equal(order.cpu(), torch.sort(inp.t.cpu(), stable=True).indices.to(torch.int32))
        rc, got = _field_run(inp, sig, col, Wsig, Wcol, c.keep, order, L)
        _lib.check(rc, "field_fwd_ordered")
        _check_field(inp, got, cid + " ordered")
        assert set(got) == set(out)
        for k, v in got.items():
            a, b = (v.view(torch.int16), out[k].view(torch.int16)) if v.element_size() == 2 else (v.view(torch.int32), out[k].view(torch.int32))
            assert torch.equal(a, b), f"{cid}: {k} of the ordered walk differs from the unordered one"


# ------------------------------------------------------------------------------------------------ what is refused
@pytest.mark.parametrize("view", ["3", "frozen"])
def test_density_backward_refuses_three_coordinates(view):
    """(kernel, view) pairs the `_supported` entry point refuses at HEAD: asserted, and the call is an error that writes nothing."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    c = next(c for c in DFWD if c.view == view and c.mode == 0 and c.N >= 31)._replace(kernel="dbwd")
    inp = _Inputs(c)
    b = _level_buffers(inp, L)
    assert L.snerf_kplanes_density_bwd_supported(C.byref(inp.desc), C.byref(b["net"])) == F.SUPPORT[("dbwd", view)] == 0
    before = {k: b[k].clone() for k in ("ws", "gp", "gX")}
    arr = (_lib.DensityBwdLevel * 2)()
    _fill_level(arr[0], inp, b)
    rc = L.snerf_kplanes_density_bwd(arr, 1, ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"kplanes_density_bwd" in L.snerf_last_error()
    for k, v in before.items():
        assert torch.equal(b[k], v), k


@pytest.mark.parametrize("view", ["3", "frozen"])
def test_ordered_field_forward_refuses_three_coordinates(view):
    from soccernerfs_amd import _lib

    L = _lib.lib()
    c = F._case("field", "values", view, 40, R_=3, S=32, rescale=1, ms=(1, 2), C=32, concat=1, operands=1, keep=1)
    inp = _Inputs(c)
    sig, col, Wsig, Wcol = _field_nets(inp)
    assert L.snerf_kplanes_field_fwd_supported(C.byref(inp.desc), C.byref(sig), C.byref(col)) == 1  # the unordered forward takes the view
    order = torch.arange(3, dtype=torch.int32, device=DEV)
    rc, out = _field_run(inp, sig, col, Wsig, Wcol, 1, order, L)
    assert F.SUPPORT[("field_ordered", view)] == 0 and rc != 0 and b"kplanes_field_fwd_ordered" in L.snerf_last_error()
    for k, v in out.items():
        assert bool((v.float() == SENT).all()), k

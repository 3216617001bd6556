"""GPU: both table encoders -- the temporal hash grid (csrc/tgrid.hip, csrc/tgrid_tiles.hip) and the static hash grid (csrc/hashgrid.hip,
csrc/hashgrid_tiles.hip) -- and every route to their gradients against the float64 restatement in tests/table_reference.py.

Part A, exact lattices.  Integer scales, dyadic coordinates, times, table values and integer upstream gradients make every product and every
partial sum a float32 in any order (tests/test_table_reference_cpu.py asserts that condition per case), so atomics, run-length combining,
tiling and fixed point cannot change a bit: every route must equal the reference rounded to float32 under torch.equal.  The cases hold what
random points never hit: coordinates exactly 0 and 1, (1, 1, 1) at t == 1, every time knot (the w_a == 1 single-column branch), out-of-range
samples, align_corners, a tiled grid type, negative coordinates that wrap through the static grid's uint32 cast on dense and hashed levels.
Outputs are prefilled with a sentinel, every buffer has guard words behind it, and buffers a route accumulates into are checked from zero and
from START.

Part B, cell boundaries at non-dyadic scales.  For every level and axis the points x = fl32(k / scale), fl32((k - 0.5) / scale) and their
float32 neighbours, with random values, against bounds k u A (u = 2^-24, A = the reference's sum of |terms| of that element):
  temporal grid   value 16 (K_TG_OUT), dy_dx 15 (K_TG_DYDX), coordinate gradient 16 + L C, table entry 8 + n (K_TG_TERM + n - 1 adds among its n
                  terms + 1 add into the buffer);
  static grid     value 13 (K_HT_OUT), coordinate gradient 11 + log2 F + L, table entry 6 + n (K_HT_TERM);
  fixed point     one more rounding (the conversion back) and n 2^-51.
The counts are taken from the kernel text and itemised next to the constants in tests/table_reference.py; no bound was measured against a
kernel and none is a fallback to a recorded deviation.  A route that lands in the neighbouring cell at one of the boundary points is off by
O(scale x value difference) in dy_dx or the coordinate gradient -- the CPU test shows the jump across such a boundary to be > 10^3 bounds --
and reads other table rows.  Elements whose A is 0 (entries no sample touches, out-of-range samples) must be exactly 0.  Nothing is excluded:
the reference takes the cell from the kernel's documented float32 pos.

Each test prints `case route: n differing / max |diff|` (part A) or `case route: max err / bound` (part B) before it asserts;
profiles/r22_table_lattice_INDEX.md keeps the lines of one run."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import table_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -71234.5  # no input, output or intermediate of any case comes near it
TG_TILINGS = {"a": (4, 0), "b": (6, 1)}   # (tile_rows_log2, first_tiled_level): 16-row tiles cut every dense level; b leaves level 0 to the atomic kernel
HT_TILINGS = {"a": (3, 0), "b": (5, 1)}


# ------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n elements on the GPU with GUARD sentinel elements behind them; `t` is the view a kernel is given."""

    def __init__(self, n, fill=SENT, dtype=torch.float32):
        self.sent = SENT if dtype == torch.float32 else -71234
        self.buf = torch.full((n + GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[:n]
        if fill != SENT:
            self.t.fill_(fill)

    def intact(self) -> bool:
        return bool((self.buf[self.t.numel():] == self.sent).all())


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


class Routes:
    """Collects name -> (kind, result on the host as float64 numpy, start value) and the guarded buffers of one case."""

    def __init__(self):
        self.got, self.guards = {}, []

    def buf(self, n, fill=SENT, dtype=torch.float32):
        g = Guarded(n, fill, dtype)
        self.guards.append(g)
        return g.t

    def add(self, name, kind, tensor, start=0.0):
        torch.cuda.synchronize()
        self.got[name] = (kind, tensor.detach().double().cpu().numpy().reshape(-1), start)

    def guard_tile_base(self, tb):
        n = tb.plan.n_tiles + 1
        g = Guarded(n, dtype=torch.int32)
        self.guards.append(g)
        tb.tile_base = g.t

    def assert_guards(self):
        torch.cuda.synchronize()
        assert all(g.intact() for g in self.guards)


def _fx_result(R, fx, n, start):
    """fixed-point cells -> float32 through snerf_fx_to_float: written over a sentinel-filled buffer, or accumulated onto `start`"""
    from soccernerfs_amd import ops

    out = R.buf(n, fill=start if start else SENT)
    ops.fx_to_float(fx, out, accumulate=bool(start))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# temporal grid: every route
# ------------------------------------------------------------------------------------------------------------------------------------
def _tgrid_routes(d, monkeypatch, starts):
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.temporal_grid import TemporalGridEncoder, TiledTableBackward

    lib = _lib.lib()
    geo = d["geo"]
    B, D, Cn, L, spr = d["B"], geo["D"], geo["C"], geo["L"], d["spr"]
    enc = TemporalGridEncoder(**d["case"]["kw"])
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(d["emb"]))
    enc = enc.to(DEV)
    emb, desc = enc.embeddings.detach(), enc.desc
    n_emb = emb.numel()
    pts, times, trow, gout = _dev(d["x"]), _dev(d["times"]), _dev(d["trow"]), _dev(d["gout"])
    co_pts = ops.coords_from_points(pts)
    rays = d["case"].get("mode") == "rays"
    if rays:
        ray_bufs = (_dev(d["origins"]), _dev(d["dirs"]), _dev(d["ebins"]))
        co_rays = ops.coords_from_rays(ray_bufs[0], ray_bufs[1], times, ray_bufs[2], d["aabb"], False)
    monkeypatch.delenv("SNERF_TGRID_LEVELS", raising=False)
    R = Routes()
    st = ops._stream

    def runs(on):
        monkeypatch.setenv("SNERF_TGRID_RUNS", "1" if on else "0")

    # the input forms: name -> (run-length kernels?, coords, explicit rows, times, samples per row)
    forms = {"per_sample_times": (False, co_pts, None, times, spr), "per_sample_rows": (False, co_pts, trow, None, 1)}
    if D == 3:
        forms["runs_points"] = (True, co_pts, None, times, spr)
    if rays:
        forms["per_sample_rays"] = (False, co_rays, None, times, spr)
        forms["runs_rays"] = (True, co_rays, None, times, spr)

    def P(t):
        return ops._ptr(t) if t is not None else None

    # ---- forward ----
    for name, (on, co, tr, tm, sp) in forms.items():
        runs(on)
        out = R.buf(B * L * Cn)
        _lib.check(lib.snerf_tgrid_encode_fwd(C.byref(desc), P(emb), C.byref(co), P(tr), P(tm), sp, C.c_int64(B), P(out), st()), "tgrid_encode_fwd")
        R.add("fwd/" + name, "out", out)
    runs(True)  # the dy_dx form has no run-length kernel: the switch must not matter
    out, dydx, gx = R.buf(B * L * Cn), R.buf(B * L * D * Cn), R.buf(B * D)
    _lib.check(lib.snerf_tgrid_encode_fwd_dydx(C.byref(desc), P(emb), C.byref(co_pts), None, P(times), spr, C.c_int64(B), P(out), P(dydx), st()), "tgrid_encode_fwd_dydx")
    R.add("fwd_dydx/out", "out", out)
    R.add("fwd_dydx/dy_dx", "dy_dx", dydx)
    _lib.check(lib.snerf_tgrid_input_bwd(P(gout), P(dydx), C.c_int64(B), D, Cn, L, P(gx), st()), "tgrid_input_bwd")
    R.add("input_bwd", "gx", gx)

    # ---- table gradient ----
    for start in starts:
        tag = f"@{start:g}"
        for name, (on, co, tr, tm, sp) in forms.items():
            runs(on)
            g = R.buf(n_emb, fill=start)
            _lib.check(lib.snerf_tgrid_encode_bwd(C.byref(desc), C.byref(co), P(tr), P(tm), sp, C.c_int64(B), P(gout), P(g), st()), "tgrid_encode_bwd")
            R.add(f"bwd/{name}{tag}", "gtable", g, start)
            fx = R.buf(n_emb, fill=0, dtype=torch.int64)
            _lib.check(lib.snerf_tgrid_encode_bwd_fx(C.byref(desc), C.byref(co), P(tr), P(tm), sp, C.c_int64(B), P(gout), P(fx), st()), "tgrid_encode_bwd_fx")
            R.add(f"fx/{name}{tag}", "gtable", _fx_result(R, fx, n_emb, start), start)
        runs(True)
        g = R.buf(n_emb, fill=start)
        for lo, hi in ((0, 1), (1, L)):  # two complementary level ranges into one buffer
            _lib.check(lib.snerf_tgrid_encode_bwd_levels(C.byref(desc), C.byref(co_pts), None, P(times), spr, C.c_int64(B), P(gout), P(g), lo, hi, st()), "tgrid_encode_bwd_levels")
        R.add(f"levels{tag}", "gtable", g, start)
        if D == 3 and geo["grid_C"] % 2 == 0:
            for key, (sh, lc) in TG_TILINGS.items():
                co = co_rays if (rays and key == "a") else co_pts
                tb = TiledTableBackward(enc, B, tile_rows_log2=sh, first_tiled_level=lc)
                assert tb.plan.tile_rows_log2 == sh and tb.plan.first_tiled_level == lc
                R.guard_tile_base(tb)
                g = R.buf(n_emb, fill=start)
                tb.bin(co, times, spr, gout)
                tb.coarse_levels(co, times, spr, gout, g)
                tb.scatter(gout, g)
                R.add(f"tiled/{key}{tag}", "gtable", g, start)
    R.assert_guards()
    assert torch.equal(emb.cpu(), torch.from_numpy(d["emb"])) and torch.equal(gout.cpu(), torch.from_numpy(d["gout"]))  # inputs are read only
    expect = {"fwd/" + f for f in forms} | {"fwd_dydx/out", "fwd_dydx/dy_dx", "input_bwd"}
    for start in starts:
        tag = f"@{start:g}"
        expect |= {f"{k}/{f}{tag}" for f in forms for k in ("bwd", "fx")} | {"levels" + tag}
        if D == 3 and geo["grid_C"] % 2 == 0:
            expect |= {f"tiled/{key}{tag}" for key in TG_TILINGS}
    assert set(R.got) == expect, set(R.got) ^ expect
    return R.got


def _expected_tgrid_route_count(d, n_starts):
    geo = d["geo"]
    forms = 2 + (geo["D"] == 3) + 2 * (d["case"].get("mode") == "rays")
    return forms + 3 + n_starts * (2 * forms + 1 + (2 if geo["D"] == 3 and geo["grid_C"] % 2 == 0 else 0))


# ------------------------------------------------------------------------------------------------------------------------------------
# static grid: every route
# ------------------------------------------------------------------------------------------------------------------------------------
def _hash_routes(d, starts):
    from soccernerfs_amd import _lib, ops
    from soccernerfs_amd.tcnn_compat import Encoding, TiledHashTableBackward

    lib = _lib.lib()
    geo = d["geo"]
    B, D, F, L = d["B"], geo["D"], geo["F"], geo["L"]
    cfg = {k: v for k, v in d["case"]["cfg"].items() if k != "D"}
    enc = Encoding(D, {"otype": "HashGrid", **cfg})
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(d["table"]).reshape(-1))
    enc = enc.to(DEV)
    table, desc = enc.params.detach(), enc.desc
    n_tab = table.numel()
    x, gout = _dev(d["x"]), _dev(d["gout"])
    R = Routes()
    st, P = ops._stream, (lambda t: ops._ptr(t) if t is not None else None)

    out = R.buf(B * L * F)
    _lib.check(lib.snerf_hashgrid_encode_fwd(C.byref(desc), P(table), P(x), C.c_int64(B), P(out), st()), "hashgrid_encode_fwd")
    R.add("fwd", "out", out)
    for start in starts:
        tag = f"@{start:g}"
        gt = R.buf(n_tab, fill=start)
        _lib.check(lib.snerf_hashgrid_encode_bwd(C.byref(desc), None, P(x), C.c_int64(B), P(gout), P(gt), None, st()), "hashgrid_encode_bwd")
        R.add("bwd/table_only" + tag, "gtable", gt, start)
        gx = R.buf(B * D, fill=start)
        _lib.check(lib.snerf_hashgrid_encode_bwd(C.byref(desc), P(table), P(x), C.c_int64(B), P(gout), None, P(gx), st()), "hashgrid_encode_bwd")
        R.add("bwd/x_only" + tag, "gx", gx, start)
        gt, gx = R.buf(n_tab, fill=start), R.buf(B * D, fill=start)
        _lib.check(lib.snerf_hashgrid_encode_bwd(C.byref(desc), P(table), P(x), C.c_int64(B), P(gout), P(gt), P(gx), st()), "hashgrid_encode_bwd")
        R.add("bwd/both.table" + tag, "gtable", gt, start)
        R.add("bwd/both.x" + tag, "gx", gx, start)
        ft, fxx = R.buf(n_tab, fill=0, dtype=torch.int64), R.buf(B * D, fill=0, dtype=torch.int64)
        _lib.check(lib.snerf_hashgrid_encode_bwd_fx(C.byref(desc), P(table), P(x), C.c_int64(B), P(gout), P(ft), P(fxx), st()), "hashgrid_encode_bwd_fx")
        R.add("fx/table" + tag, "gtable", _fx_result(R, ft, n_tab, start), start)
        R.add("fx/x" + tag, "gx", _fx_result(R, fxx, B * D, start), start)
        gt, gx = R.buf(n_tab, fill=start), R.buf(B * D, fill=start)
        for lo, hi in ((0, 1), (1, L)):
            _lib.check(lib.snerf_hashgrid_encode_bwd_levels(C.byref(desc), P(table), P(x), C.c_int64(B), P(gout), P(gt), P(gx), lo, hi, st()), "hashgrid_encode_bwd_levels")
        R.add("levels.table" + tag, "gtable", gt, start)
        R.add("levels.x" + tag, "gx", gx, start)
        if D == 3:
            for key, (sh, lc) in HT_TILINGS.items():
                tb = TiledHashTableBackward(enc, B, tile_rows_log2=sh, first_tiled_level=lc)
                assert tb.plan.tile_rows_log2 == sh and tb.plan.first_tiled_level == lc
                R.guard_tile_base(tb)
                gt = R.buf(n_tab, fill=start)
                tb.bin(x, gout)
                tb.coarse_levels(x, gout, gt)
                tb.scatter(x, gout, gt)
                R.add(f"tiled/{key}{tag}", "gtable", gt, start)
    # the autograd wrappers: Encoding.forward (table and coordinates) and ops.hashgrid_encode (coordinates only)
    enc.params.grad = None
    xg = x.clone().requires_grad_(True)
    o = enc(xg)
    o.backward(gout)
    R.add("autograd/Encoding.out", "out", o)
    R.add("autograd/Encoding.table", "gtable", enc.params.grad)
    R.add("autograd/Encoding.x", "gx", xg.grad)
    xg = x.clone().requires_grad_(True)
    o = ops.hashgrid_encode(xg, table, desc)
    o.backward(gout)
    R.add("autograd/ops.out", "out", o)
    R.add("autograd/ops.x", "gx", xg.grad)
    R.assert_guards()
    assert torch.equal(table.cpu(), torch.from_numpy(d["table"]).reshape(-1)) and torch.equal(x.cpu(), torch.from_numpy(d["x"]))
    expect = {"fwd", "autograd/Encoding.out", "autograd/Encoding.table", "autograd/Encoding.x", "autograd/ops.out", "autograd/ops.x"}
    for start in starts:
        tag = f"@{start:g}"
        expect |= {n + tag for n in ("bwd/table_only", "bwd/x_only", "bwd/both.table", "bwd/both.x", "fx/table", "fx/x", "levels.table", "levels.x")}
        if D == 3:
            expect |= {f"tiled/{key}{tag}" for key in HT_TILINGS}
    assert set(R.got) == expect, set(R.got) ^ expect
    return R.got


# ------------------------------------------------------------------------------------------------------------------------------------
# part A
# ------------------------------------------------------------------------------------------------------------------------------------
def _assert_exact(cid, got, ref):
    bad = []
    for name in sorted(got):
        kind, have, start = got[name]
        want = (ref[kind] + start).astype(np.float32).astype(np.float64).reshape(-1)   # exact on the lattice: the rounding changes nothing
        assert have.shape == want.shape, (name, have.shape, want.shape)
        diff = np.abs(have - want)
        n = int((have != want).sum())
        print(f"{cid} {name}: {n} differing / max |diff| {float(diff.max()) if diff.size else 0.0:.3e}")
        if n or not torch.equal(torch.from_numpy(have), torch.from_numpy(want)):
            bad.append((name, n, float(diff.max())))
    assert not bad, bad


@pytest.mark.parametrize("cid", [c["case_id"] for c in TR.TGRID_LATTICE])
def test_every_temporal_grid_route_is_exact_on_a_lattice(cid, monkeypatch):
    d, ref = TR.case_and_reference(cid)
    got = _tgrid_routes(d, monkeypatch, (0.0, TR.START))
    assert len(got) == _expected_tgrid_route_count(d, 2)
    _assert_exact(cid, got, ref)
    # out-of-range samples read nothing and receive nothing, in every forward form
    outside = np.repeat(~ref["inside"], d["geo"]["L"] * d["geo"]["C"])
    assert outside.any() and all(not have[outside].any() for kind, have, _ in got.values() if kind == "out")


@pytest.mark.parametrize("cid", [c["case_id"] for c in TR.HASH_LATTICE])
def test_every_static_grid_route_is_exact_on_a_lattice(cid):
    d, ref = TR.case_and_reference(cid)
    _assert_exact(cid, _hash_routes(d, (0.0, TR.START)), ref)


# ------------------------------------------------------------------------------------------------------------------------------------
# part B
# ------------------------------------------------------------------------------------------------------------------------------------
def _assert_within(cid, got, ref, bounds):
    """bounds: kind -> (k for u A, n array or None) ... see the module docstring"""
    bad = []
    for name in sorted(got):
        kind, have, start = got[name]
        assert start == 0.0
        want, A = ref[kind].reshape(-1), ref["A_" + kind].reshape(-1)
        bound = bounds(kind, name.startswith("fx/")).reshape(-1)
        err = np.abs(have - want)
        assert have.shape == want.shape and np.isfinite(have).all(), name
        dead = A == 0
        zero_ok = not have[dead].any()
        worst = int(np.argmax(err - bound))
        print(f"{cid} {name}: max err {float(err.max()):.3e}, worst element {float(err[worst]):.3e} / {float(bound[worst]):.3e}, max err / (u A) "
              f"{float((err[~dead] / (TR.U * A[~dead])).max()) if (~dead).any() else 0.0:.2f}, {int(dead.sum())} elements with A = 0 {'all zero' if zero_ok else 'NOT ZERO'}")
        if not zero_ok or not (err <= bound).all():
            bad.append((name, float(err[worst]), float(bound[worst]), int((err > bound).sum())))
    assert not bad, bad


@pytest.mark.parametrize("cid", [c["case_id"] for c in TR.TGRID_BOUNDARY])
def test_temporal_grid_routes_at_cell_boundaries_against_float64(cid, monkeypatch):
    d, ref = TR.case_and_reference(cid)
    geo = d["geo"]
    got = _tgrid_routes(d, monkeypatch, (0.0,))
    assert len(got) == _expected_tgrid_route_count(d, 1)

    def bounds(kind, fixed_point):
        if kind == "gtable":
            return TR.table_bound(ref["A_gtable"], ref["n_gtable"], TR.K_TG_TERM, fixed_point)
        k = {"out": TR.K_TG_OUT, "dy_dx": TR.K_TG_DYDX, "gx": TR.k_tg_gx(geo["L"], geo["C"])}[kind]
        return k * TR.U * ref["A_" + kind]

    _assert_within(cid, got, ref, bounds)
    outside = ~ref["inside"]
    assert outside.any()
    for kind, width in (("dy_dx", geo["L"] * geo["D"] * geo["C"]), ("gx", geo["D"])):
        for name, (k, have, _) in got.items():
            if k == kind:
                assert not have.reshape(d["B"], width)[outside].any(), name  # exactly 0 for out-of-range samples


@pytest.mark.parametrize("cid", [c["case_id"] for c in TR.HASH_BOUNDARY])
def test_static_grid_routes_at_cell_boundaries_against_float64(cid):
    d, ref = TR.case_and_reference(cid)
    geo = d["geo"]
    got = _hash_routes(d, (0.0,))

    def bounds(kind, fixed_point):
        if kind == "gtable":
            return TR.table_bound(ref["A_gtable"], ref["n_gtable"], TR.K_HT_TERM, fixed_point)
        if kind == "gx":
            k = TR.k_ht_gx(geo["L"], geo["F"]) + (1 if fixed_point else 0)
            return k * TR.U * ref["A_gx"] + (ref["n_gx"] * 2.0 ** -51 if fixed_point else 0.0)
        return TR.K_HT_OUT * TR.U * ref["A_out"]

    _assert_within(cid, got, ref, bounds)

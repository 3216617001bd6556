"""GPU: the owner-computes tile passes' fused Adam (snerf_tgrid_bwd_tiles_adam, snerf_hashgrid_bwd_tiles_adam) against the ORACLES' autograd in float64.

tests/test_gpu_tgrid_tiles.py and tests/test_gpu_hashgrid.py compare the fused form with the unfused HIP sequence; here the table gradient comes from
autograd through oracle/tgrid_oracle.encode / oracle/hashgrid_oracle.encode on the same positions, times and gout, the temporal-TV sign term of the OLD
table is added, and tests/optim_reference.py's float64 Adam is applied.  Bounds are FACTOR (5) x the float32 oracle's deviation from the float64 one for
m, v and p (profiles/r16_optim_deviations.json, "tiles"), deviations max |got - want| / max |want|.

The positions are well placed (optim_reference.well_placed: no grid position within 8 float32 ulps of an integer), so every evaluation order agrees on the
cells and no corner weight is exactly 0.  One step from a NON-zero state (m random, v >= 1e-8: no element has to be left out), with the TV term and without;
one step from ZERO state at step 1, where m and v are compared everywhere and p only where the float64 gradient's magnitude exceeds 100 x the float32 oracle's
largest absolute gradient error -- below that the sign Adam's first step follows is not determined in float32 -- with the share of touched entries left out
under 1 % (tests/test_optim_reference_cpu.py checks that the float32 oracle alone stays under that cap).

Touched entries: from zero state, m_out != 0 exactly where the float64 gradient is non-zero.  From the non-zero state an entry counts as touched by the
kernel when m_out differs from the float32 decay b1 * m_in; that set lies inside the float64 gradient's, and what is missing from it has (1 - b1) |g| below
one float32 ulp of b1 * m_in, where the float32 sum cannot show the gradient at all."""
import ctypes as C

import pytest
import torch

from tests import optim_reference as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_INTS = 8
BOUNDS = OR.load_bounds()["tiles"]
CASES = OR.tile_cases()


class _Buf:
    """A table-shaped float buffer with 64 sentinel floats behind it."""

    def __init__(self, src):
        n = src.numel()
        self.buf = torch.full((n + 64,), -71234.5, dtype=torch.float32, device=DEV)
        self.t = self.buf[:n].view(src.shape)
        self.t.copy_(src)

    def intact(self):
        return bool((self.buf[self.t.numel():] == -71234.5).all())


def _guard_tile_base(tb):
    n = tb.plan.n_tiles + 1
    buf = torch.full((n + GUARD_INTS,), -77, dtype=torch.int32, device=DEV)
    buf[:n] = 0
    tb.tile_base = buf[:n]
    return buf


def _fused_step(c, d, tv, state):
    """The product's sequence for one table: (TV sign from the old table) -> bin -> coarse levels -> fused tile pass with Adam."""
    from soccernerfs_amd import _lib, ops

    step = 3 if state == "rand" else 1
    zeros = torch.zeros(d["shape"])
    p, m, v, g = _Buf(d["table"]), _Buf(d["m"] if state == "rand" else zeros), _Buf(d["v"] if state == "rand" else zeros), _Buf(zeros)
    gout = d["gout"].to(DEV).contiguous()
    x = d["x"].to(DEV).contiguous()
    if c["kind"] == "tgrid":
        from soccernerfs_amd.temporal_grid import TemporalGridEncoder, TiledTableBackward

        enc = TemporalGridEncoder(**c["kw"]).to(DEV)
        assert tuple(enc.embeddings.shape) == tuple(d["shape"]) and enc.offsets.tolist() == d["offsets"]
        tb = TiledTableBackward(enc, d["B"], tile_rows_log2=c["sh"], first_tiled_level=c["lc"])
        assert tb.plan.first_tiled_level == c["lc"] and tb.plan.tile_rows_log2 == c["sh"]
        guard = _guard_tile_base(tb)
        co, times = ops.coords_from_points(x), d["times"].to(DEV)
        srow = None
        if tv:
            rows, gc = d["shape"]
            srow, part = torch.zeros(rows, device=DEV), torch.zeros(64, 16, device=DEV)
            _lib.check(_lib.lib().snerf_tgrid_tv_sign(ops._ptr(p.t), C.c_int64(rows), gc, d["tv_cols"][0], d["tv_cols"][1], OR.TV_WEIGHT, ops._ptr(part), 64,
                                                      ops._ptr(srow), ops._stream()), "tgrid_tv_sign")
        tb.bin(co, times, c["S"], gout)
        tb.coarse_levels(co, times, c["S"], gout, g.t)
        tb.scatter_adam(gout, g.t, p.t, m.t, v.t, OR.LR, step, c["eps"], tv_cols=d["tv_cols"] if tv else None, srow=srow)
    else:
        from soccernerfs_amd.tcnn_compat import Encoding, TiledHashTableBackward

        enc = Encoding(3, {"otype": "HashGrid", **c["cfg"]}).to(DEV)
        assert enc.params.numel() == d["shape"][0] * d["shape"][1]
        tb = TiledHashTableBackward(enc, d["B"], tile_rows_log2=c["sh"], first_tiled_level=c["lc"])
        assert tb.plan.first_tiled_level == c["lc"] and tb.plan.tile_rows_log2 == c["sh"]
        guard = _guard_tile_base(tb)
        tb.bin(x, gout)
        tb.coarse_levels(x, gout, g.t.view(-1))
        tb.scatter_adam(x, gout, g.t.view(-1), p.t.view(-1), m.t.view(-1), v.t.view(-1), OR.LR, step, c["eps"])
    torch.cuda.synchronize()
    assert bool((guard[-GUARD_INTS:] == -77).all()), guard[-GUARD_INTS:].tolist()  # the passes own tile_base[n_tiles + 1] and not a word more
    assert 0 < int(tb.tile_base[tb.plan.n_tiles]) <= tb.plan.record_capacity
    assert all(b.intact() for b in (p, m, v, g))
    assert float(g.t.abs().max()) == 0.0  # the coarse levels' gradient was read AND cleared
    return {"p_out": p.t.cpu(), "m": m.t.cpu(), "v": v.t.cpu()}


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["case_id"])
def test_fused_tile_adam_against_the_oracle_autograd(c):
    d = OR.make_tile_case(c)
    b1 = torch.tensor(OR.BETA1, dtype=torch.float32)
    bad = []
    for tv, state in OR.tile_variants(c):
        key = OR.tile_key(tv, state)
        rec = BOUNDS[c["case_id"]][key]
        ref = OR.tile_step(d, torch.float64, tv, state)
        got = _fused_step(c, d, tv, state)
        touched = ref["grad"] != 0
        assert int(touched.sum()) == rec["touched"]
        if state == "zero":
            keep = OR.resolved_mask(ref["grad"], rec["grad_abs_err32"]) | ~touched
            left_out = float((touched & ~keep).sum()) / int(touched.sum())
            print(f"{c['case_id']} {key} left_out_share {left_out:.5f} / {OR.UNRESOLVED_CAP}")
            assert left_out < OR.UNRESOLVED_CAP
            assert torch.equal(got["m"] != 0, touched)  # exactly the entries the float64 gradient touches
        else:
            keep = torch.ones_like(touched)
            decay = b1 * d["m"]
            changed = got["m"] != decay
            assert not bool((changed & ~touched).any())
            missing = touched & ~changed
            swallowed = (1.0 - OR.BETA1) * ref["grad"].abs() <= 2.0 ** -23 * decay.double().abs()
            print(f"{c['case_id']} {key} touched {int(touched.sum())} changed {int(changed.sum())} below_one_ulp_of_decay {int(missing.sum())}")
            assert not bool((missing & ~swallowed).any())
        devs = {"m": OR.rel_dev(got["m"], ref["m"]), "v": OR.rel_dev(got["v"], ref["v"]), "p_out": OR.rel_dev_where(got["p_out"], ref["p_out"], keep)}
        for k, dev in devs.items():
            bound = OR.FACTOR * rec[f"dev32_{k}"]
            print(f"{c['case_id']} {key} {k} {dev:.3e} / {bound:.3e}")
            if not dev <= bound:
                bad.append((key, k, dev, bound))
        assert float((got["p_out"] - d["table"]).abs().max()) > 1e-3  # the table did move
    assert not bad, bad

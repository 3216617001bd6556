"""GPU: snerf_tgrid_density_fwd (csrc/tgrid_density.hip), the proposal density of a temporal-grid field as one launch.

1. Bit-identity with the pair it replaces -- snerf_tgrid_encode_fwd (per-ray times) + snerf_mlp_fwd (aux = trunc_exp) -- by torch.equal, over the
   lattice of tests/tgrid_density_cases.py: S in {1, 31, 32, 33, 96, 256} x R in {1, 3, 133} on four tables (L = 5, C = 2, temporal_dim 8 / 32,
   both preset growth factors, a dense and a hashed level each), rays that leave the box, times exactly 0, exactly 1, on an interior knot and
   mid-interval.  Sentinel rows behind the density buffer must survive, the sentinel in its live rows must not.
2. On four of those cases the density is also compared with the float64 restatement (tests/table_reference.py's encoder + the net in float64).
   The bound is 5 x the deviation of the same restatement run in float32, measured on the CPU without the code under test
   (tools/measure_tgrid_density_deviations.py -> profiles/r29_tgrid_density_deviations.json); every element counts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import tgrid_density_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, TAIL = -7.0, 64

with open(os.path.join(ROOT, "profiles", "r29_tgrid_density_deviations.json")) as _f:
    YARDSTICK = json.load(_f)["cases"]

_ENC = {}


def _table(table):
    """-> (encoder on the device holding the case's table, the net's descriptor, its weights on the device); built once per table"""
    from soccernerfs_amd import _lib
    from soccernerfs_amd.temporal_grid import TemporalGridEncoder

    if table not in _ENC:
        geo, emb, W = TC.table_and_net(table)
        enc = TemporalGridEncoder(**TC.encoder_kwargs(table))
        assert enc.offsets.tolist() == geo["offsets"]
        with torch.no_grad():
            enc.embeddings.copy_(torch.from_numpy(emb))
        net = _lib.MlpDesc()
        net.d_in, net.hidden, net.n_hidden, net.d_out, net.hidden_act, net.out_act, net.operands = TC.L * TC.C, TC.HIDDEN, 1, 1, 1, 0, 0
        _ENC[table] = (enc.to(DEV), net, torch.from_numpy(W).to(DEV))
    return _ENC[table]


def _run(table, S, R):
    """-> (fused density with its tail, the pair's density, the pair's features)"""
    from soccernerfs_amd import _lib, ops

    enc, net, W = _table(table)
    lib, p = _lib.lib(), ops._ptr
    o, d, e, t = (torch.from_numpy(a).to(DEV).contiguous() for a in TC.rays(table, S, R))
    N = R * S
    co = ops.coords_from_rays(o, d, t, e, TC.AABB, False)
    assert lib.snerf_tgrid_density_fwd_supported(C.byref(enc.desc), C.byref(net)) == 1
    fused = torch.full((N + TAIL,), SENTINEL, device=DEV)
    _lib.check(lib.snerf_tgrid_density_fwd(C.byref(enc.desc), p(enc.embeddings), C.byref(co), p(t), S, C.c_int64(N), C.byref(net), p(W), p(fused), ops._stream()),
               "tgrid_density_fwd")
    feat = torch.full((N, enc.output_dim), SENTINEL, device=DEV)
    raw, dens = torch.full((N, 1), SENTINEL, device=DEV), torch.full((N,), SENTINEL, device=DEV)
    _lib.check(lib.snerf_tgrid_encode_fwd(C.byref(enc.desc), p(enc.embeddings), C.byref(co), None, p(t), S, C.c_int64(N), p(feat), ops._stream()), "tgrid_encode_fwd")
    _lib.check(lib.snerf_mlp_fwd(C.byref(net), p(W), p(feat), enc.output_dim, C.c_int64(N), p(raw), 1, 0, p(dens), ops._stream()), "mlp_fwd")
    return fused, dens, feat


@pytest.mark.parametrize("R", TC.RAYS)
@pytest.mark.parametrize("table", sorted(TC.TABLES))
def test_fused_density_is_bit_identical_to_encode_plus_mlp(table, R):
    out_of_range = live_b = 0
    for S in TC.SAMPLES:
        fused, dens, feat = _run(table, S, R)
        N = R * S
        assert bool((fused[N:] == SENTINEL).all()), (S, "wrote behind the N densities")
        assert bool((fused[:N] != SENTINEL).all()) and bool(torch.isfinite(fused[:N]).all()), S
        assert torch.equal(fused[:N], dens), (S, float((fused[:N].double() - dens.double()).abs().max()))
        dead = (feat == 0).all(dim=1)
        out_of_range += int(dead.sum())
        live_b += int((~dead).sum())
        assert bool((fused[:N][dead] == 1.0).all())  # features 0, net still evaluated: exp(0)
    assert out_of_range > 0 and live_b > 0, "mis-built: the lattice needs samples inside and outside the box"


def test_time_slots_of_the_lattice():
    """What the lattice promises about its times, checked on the inputs: exactly 0, exactly 1, an interior knot (one live column: the b column's
    weight is 0) and a mid-interval time all occur among the one-ray cases."""
    from tests import table_reference as TR

    seen = set()
    for S in TC.SAMPLES:
        t = TC.rays("t8_r64", S, 1)[3]
        _, w = TR.temporal_slots(t, TC.C, 8)
        seen.add((float(t[0]), bool((w[0, :, 1] == 0).all())))
    assert seen == {(0.0, True), (1.0, True), (0.5, True), (float(np.float32(0.37)), False)}


@pytest.mark.parametrize("case", TC.F64_CASES, ids=[TC.case_key(*c) for c in TC.F64_CASES])
def test_fused_density_against_the_float64_restatement(case):
    table, S, R = case
    key = TC.case_key(table, S, R)
    assert key in YARDSTICK, f"{key}: no yardstick in profiles/r29_tgrid_density_deviations.json"
    want, feat64 = TC.restate(table, S, R, np.float64)
    fused, _, feat = _run(table, S, R)
    got = fused[:R * S].cpu().numpy()
    assert want.shape == got.shape
    # the kernel and the restatement agree on which samples are out of range (all-zero features)
    assert np.array_equal((feat.cpu().numpy() == 0).all(axis=1), (feat64 == 0).all(axis=1))
    dev, bound = TC.relative_deviation(got, want), 5.0 * YARDSTICK[key]["deviation"]
    print(f"{key}: deviation from float64 {dev:.3e}, float32 restatement {YARDSTICK[key]['deviation']:.3e}, bound {bound:.3e}")
    assert dev <= bound, (key, dev, bound)

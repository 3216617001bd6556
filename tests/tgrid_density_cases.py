"""Inputs and the float64 restatement for snerf_tgrid_density_fwd (csrc/tgrid_density.hip): shared by tests/test_gpu_tgrid_density.py and
tools/measure_tgrid_density_deviations.py.  numpy only; the table encoder is tests/table_reference.py's, the net (L*C -> 16 -> 1, ReLU, no
bias, exp on the output) is restated here as the k-ordered chain the kernels run.

The lattice: S in SAMPLES x R in RAYS for each table of TABLES -- L = 5, C = 2, base resolution 16, temporal_dim 8 and 32, the preset's two
growth factors (max_res 64 and 256) and log2_hashmap_size 14, which leaves the levels of resolution <= 24 dense (25^3 = 15625 rows) and hashes
the finer ones.  Rays start inside the box [-1,1]^3 and run to t = 3, so the far samples of every ray are out of range; a ray's time is
exactly 0, exactly 1, an interior knot of the time table or a mid-interval value, by (ray + position of S in SAMPLES) mod 4, so that the
one-ray cases cover all four between them."""
import functools

import numpy as np

from tests import table_reference as TR

F32 = np.float32
SAMPLES = (1, 31, 32, 33, 96, 256)
RAYS = (1, 3, 133)
LOG2_HASHMAP = 14
TABLES = {"t8_r64": dict(temporal_dim=8, max_res=64), "t8_r256": dict(temporal_dim=8, max_res=256),
          "t32_r64": dict(temporal_dim=32, max_res=64), "t32_r256": dict(temporal_dim=32, max_res=256)}
L, C, H, HIDDEN = 5, 2, 16, 16
AABB = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]
# the four cases that are also compared with the float64 restatement: (table, S, R)
F64_CASES = (("t8_r64", 33, 3), ("t8_r256", 31, 133), ("t32_r64", 256, 1), ("t32_r256", 96, 3))


def growth(max_res: int) -> float:
    """TemporalHashMLPDensityField's per-level scale (nerfplayer_nerfacto_field.py:83)"""
    return float(np.exp((np.log(max_res) - np.log(H)) / (L - 1)))


def encoder_kwargs(table: str) -> dict:
    cfg = TABLES[table]
    return dict(input_dim=3, temporal_dim=cfg["temporal_dim"], num_levels=L, level_dim=C, per_level_scale=growth(cfg["max_res"]), base_resolution=H,
                log2_hashmap_size=LOG2_HASHMAP)


@functools.lru_cache(maxsize=None)
def table_and_net(table: str):
    """-> (geometry, embeddings [rows, C + T] in [-1/2, 1/2), W = [L*C x 16 | 16 x 1] in [-0.8, 0.8), input-major as snerf_mlp_fwd reads it)"""
    geo = TR.tgrid_geometry(**encoder_kwargs(table))
    assert any(lv["hashed"] for lv in geo["levels"]) and not all(lv["hashed"] for lv in geo["levels"]), "mis-built: needs a dense and a hashed level"
    rng = np.random.default_rng(sorted(TABLES).index(table) + 100)
    emb = rng.random((geo["offsets"][-1], geo["grid_C"])).astype(F32) - F32(0.5)
    W = ((rng.random(L * C * HIDDEN + HIDDEN) * 2 - 1) * 0.8).astype(F32)
    return geo, emb, W


def rays(table: str, S: int, R: int):
    """-> origins [R,3], dirs [R,3], ebins [R,S+1], times [R] (float32)"""
    T = TABLES[table]["temporal_dim"]
    rng = np.random.default_rng(1000 * S + R)
    o = ((rng.random((R, 3)) * 2 - 1) * 0.6).astype(F32)
    d = rng.random((R, 3)) * 2 - 1
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    # clustered edges, as after proposal resampling: runs of samples inside one cell, then jumps; the last edge is 3 (outside the box for every ray)
    e = np.sort(rng.random((R, S + 1)) ** 3 * 3.0, axis=1).astype(F32)
    e[:, -1] = 3.0
    n = T - 2
    assert n % 2 == 0
    kinds = (F32(0.37), F32(0.0), F32(1.0), F32(0.5))  # mid-interval, the two ends, an interior knot (0.5 * n is an integer: n is even)
    t = np.array([kinds[(r + SAMPLES.index(S)) % 4] for r in range(R)], F32)
    return o, d, e, t


def restate(table: str, S: int, R: int, dtype=np.float64):
    """The density [R * S] of a case in `dtype`: tests/table_reference.py's encoder, then the net as a k-ordered chain and exp."""
    geo, emb, W = table_and_net(table)
    o, d, e, t = rays(table, S, R)
    x = TR.ray_x(o, d, e, AABB[0], AABB[1])
    B = R * S
    feat = TR.tgrid_encode(geo, x, np.repeat(t, S), emb, np.zeros((B, L * C), F32), dtype=dtype)["out"].reshape(B, L * C).astype(dtype)
    W0, WO = W[:L * C * HIDDEN].reshape(L * C, HIDDEN).astype(dtype), W[L * C * HIDDEN:].astype(dtype)
    h = np.zeros((B, HIDDEN), dtype)
    for k in range(L * C):
        h = h + feat[:, k:k + 1] * W0[k][None, :]
    h = np.maximum(h, dtype(0))
    y = np.zeros(B, dtype)
    for k in range(HIDDEN):
        y = y + h[:, k] * WO[k]
    return np.exp(y), feat


def relative_deviation(got, want64) -> float:
    """max over ALL elements of |got - want| / |want| (a density is positive)"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    return float(np.max(np.abs(got - want64) / np.abs(want64)))


def case_key(table: str, S: int, R: int) -> str:
    return f"{table}-S{S}-R{R}"

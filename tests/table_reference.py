"""Float64 restatement of the two table encoders -- the temporal hash grid (csrc/tgrid.hip, csrc/tgrid_tiles.hip) and the static hash grid
(csrc/hashgrid.hip, csrc/hashgrid_tiles.hip) -- for tests/test_table_reference_cpu.py and tests/test_gpu_table_lattice.py.  numpy only;
independent of oracle/*_oracle.py (which the CPU test uses as a cross-check) and of the library.

What is float32 here, because it is the documented input of everything after it: a level's scale, the position `pos` inside the level
(temporal grid: x * scale rounded, then + 0.5 or + 0 rounded; static grid: one rounding, fma(scale, x, 0.5)), hence the cell floor(pos) and
the in-cell fraction pos - floor(pos) (exact); the time row value v = fl32(t * n); and, in ray mode, the sample position x with the
operations and order of tg_ray_x.  The coordinate derivative is discontinuous across cells, so a reference that chose its own cell could not
judge it.  Everything after that -- 1 - fraction, the corner weights, the time weights (r + 1) - v and v - r, every product and every sum --
is evaluated in `dtype` (float64: the reference; float32: the restatement whose agreement with it on the lattice cases is the exactness
condition of the GPU test).

Every result comes with, per element, A = the sum of |terms| and n = the number of non-zero terms, a term being one product that is added
into the element: corner weight x time weight x table value for an output, corner weight x time weight x upstream gradient for a table
entry, and so on.  The GPU test derives its part-B bounds from A and n; the CPU test derives the lattice's exactness condition from A and
the granule (the largest power of two that divides every term)."""
import functools

import numpy as np

F32 = np.float32
M32 = 0xFFFFFFFF
PRIMES = (1, 2654435761, 805459861)


def exp2f(v):
    """Correctly rounded float32 exp2 of a float32."""
    return F32(2.0 ** float(F32(v)))


# ------------------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------------------
def _strides(resolution_step, rows, D, hash_allowed):
    """The dense-or-hashed decision and the per-axis multipliers: the running stride is multiplied by the step per axis while it is <= rows; a
    stride that ends above rows means a hashed level where hashing is allowed, otherwise the axes behind the overflow do not contribute."""
    stride = 1
    for _ in range(D):
        if stride > rows:
            break
        stride = stride * resolution_step
    hashed = hash_allowed and stride > rows
    mult, st = [], 1
    for k in range(3):
        if k >= D:
            mult.append(0)
            continue
        mult.append(PRIMES[k] if hashed else (st if st <= rows else 0))
        if st <= rows:
            st = st * resolution_step
    return hashed, mult


def tgrid_geometry(temporal_dim=64, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2.0, base_resolution=16, log2_hashmap_size=19,
                   desired_resolution=None, gridtype="hash", align_corners=False):
    """The temporal grid's descriptor fields (constructor arithmetic of TemporalGridEncoder) and, from them, each level as tg_level derives it."""
    if desired_resolution is not None:
        per_level_scale = float(np.exp2(np.log2(float(desired_resolution) / base_resolution) / (num_levels - 1)))
    offsets, off = [], 0
    for i in range(num_levels):
        res = int(np.ceil(base_resolution * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (res if align_corners else res + 1) ** input_dim)
        offsets.append(off)
        off += int(np.ceil(n / 8) * 8)
    offsets.append(off)
    S = F32(np.log2(per_level_scale))  # the descriptor's float field
    levels = []
    for l in range(num_levels):
        rows = offsets[l + 1] - offsets[l]
        scale = F32(F32(exp2f(F32(l) * S) * F32(base_resolution)) - F32(1.0))
        resolution = int(np.ceil(scale)) + 1
        hashed, mult = _strides(resolution if align_corners else resolution + 1, rows, input_dim, gridtype == "hash")
        levels.append(dict(off0=offsets[l], rows=rows, scale=scale, resolution=resolution, hashed=hashed, mult=mult))
    return dict(kind="tgrid", D=input_dim, C=level_dim, T=temporal_dim, L=num_levels, grid_C=level_dim + temporal_dim, offsets=offsets, S=S,
                align_corners=bool(align_corners), per_level_scale=per_level_scale, levels=levels)


def hash_geometry(n_levels, n_features_per_level, base_resolution, per_level_scale, log2_hashmap_size, D=3):
    """The static grid's layout as snerf_hashgrid_layout computes it on the host, and each level as ht_level derives it."""
    log2_pls = F32(np.log2(np.float64(F32(per_level_scale))))  # log2f of the float argument
    offsets, levels = [0], []
    for l in range(n_levels):
        scale = F32(F32(exp2f(F32(l) * log2_pls) * F32(base_resolution)) - F32(1.0))
        res = int(np.ceil(scale)) + 1
        params = 1
        for _ in range(D):
            params *= res
            if params > M32 // 2:
                params = M32 // 2
                break
        params = min((params + 7) // 8 * 8, 1 << log2_hashmap_size)
        hashed, mult = _strides(res, params, D, True)
        levels.append(dict(off0=offsets[-1], rows=params, scale=scale, resolution=res, hashed=hashed, mult=mult))
        offsets.append(offsets[-1] + params)
    return dict(kind="hash", D=D, F=n_features_per_level, L=n_levels, offsets=offsets, levels=levels)


# ------------------------------------------------------------------------------------------------------------------------------------
# cell, rows, time slot, ray positions
# ------------------------------------------------------------------------------------------------------------------------------------
def tg_pos(x32, scale, align_corners):
    """float32 pos of the temporal grid: two roundings."""
    x32 = np.asarray(x32, F32)
    return (x32 * F32(scale)).astype(F32) + F32(0.0 if align_corners else 0.5)


def ht_pos(x32, scale):
    """float32 pos of the static grid: one rounding (the product of two floats is exact in float64; adding 0.5 there does not round before
    the float32 rounding can see it unless the product is below 2^-29, where the result is 0.5 either way)."""
    return (np.asarray(x32, F32).astype(np.float64) * np.float64(F32(scale)) + 0.5).astype(F32)


def cell_of(pos32):
    """-> (cell as uint32 values in uint64, in-cell fraction float32; exact).  Negative cells wrap through the cast, as (uint32)(int)floorf."""
    f = np.floor(pos32)
    return (f.astype(np.int64) & M32).astype(np.uint64), (pos32 - f).astype(F32)


def corner_rows(lv, cell, idx):
    """Row inside the level of corner idx (bit d: the far side of axis d) of the cells [B, D]: uint32 wrap-around products, XOR (hashed) or sum
    (dense), modulo rows."""
    index = np.zeros(cell.shape[0], np.uint64)
    for d in range(cell.shape[1]):
        c = (cell[:, d] + np.uint64((idx >> d) & 1)) & np.uint64(M32)
        term = (c * np.uint64(lv["mult"][d])) & np.uint64(M32)
        index = (index ^ term) if lv["hashed"] else ((index + term) & np.uint64(M32))
    return (index % np.uint64(lv["rows"])).astype(np.int64)


def temporal_slots(t32, C, T, dtype=np.float64):
    """Closed form of get_temporal_index for times [N] in [0, 1] -> (col [N, C, 2], w [N, C, 2]): per channel the a column and weight, then the
    b column and weight.  v = fl32(t * n), n = T - 2; r = floor(v), r = n at t == 1; channel p = r mod C blends its occupant ((r + 1) - v) with
    the entering column C + r (v - r); every other channel reads its occupant with weight 1.  A weight of exactly 1 leaves the b column dead
    (its weight is 0 by the same arithmetic)."""
    t32 = np.asarray(t32, F32)
    n = T - 2
    v = (t32 * F32(n)).astype(F32)
    r = v.astype(np.int64)
    r[t32 == 1] = n
    q = np.arange(C)[None, :]
    rr = r[:, None]
    occ = np.where(rr > q, C + q + C * ((rr - 1 - q) // C), q)
    blend = q == (rr % C)
    vd, rd = v.astype(dtype)[:, None], rr.astype(dtype)
    col = np.stack([occ, np.where(blend, C + rr, 0)], axis=-1)
    w = np.stack([np.where(blend, (rd + dtype(1)) - vd, dtype(1)), np.where(blend, vd - rd, dtype(0))], axis=-1).astype(dtype)
    return col, w


def temporal_row_index(t32, C, T):
    """The reference-shaped explicit rows [N, 4 C] float32: (w_a, col_a, w_b, col_b) per channel."""
    col, w = temporal_slots(t32, C, T, np.float32)
    out = np.zeros((len(col), 4 * C), F32)
    out[:, 0::4], out[:, 1::4], out[:, 2::4], out[:, 3::4] = w[:, :, 0], col[:, :, 0], w[:, :, 1], col[:, :, 1]
    return out


def ray_x(origins, dirs, ebins, aabb_min, aabb_max):
    """Sample positions [R * S, 3] of rays in float32 with tg_ray_x's operations in its order: pos = o + (d * (e0 + e1)) / 2, x = (pos - lo) /
    (hi - lo)."""
    o, d, e = np.asarray(origins, F32), np.asarray(dirs, F32), np.asarray(ebins, F32)
    lo, hi = np.asarray(aabb_min, F32), np.asarray(aabb_max, F32)
    mid = (e[:, :-1] + e[:, 1:]).astype(F32)                                   # [R, S]
    prod = (d[:, None, :] * mid[:, :, None]).astype(F32)
    pos = (o[:, None, :] + (prod / F32(2.0)).astype(F32)).astype(F32)
    x = ((pos - lo).astype(F32) / (hi - lo).astype(F32)).astype(F32)
    return x.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# the two encoders
# ------------------------------------------------------------------------------------------------------------------------------------
class _Acc:
    """value, A = sum |terms| and n = number of non-zero terms of an array of sums"""

    def __init__(self, shape, dtype):
        self.v, self.A, self.n = np.zeros(shape, dtype), np.zeros(shape, np.float64), np.zeros(shape, np.int64)

    def add(self, term, sl=(), at=None):
        """into the view [sl] elementwise, or (at: index arrays, possibly with repeats) scattered"""
        mag, nz = np.abs(term).astype(np.float64), (term != 0).astype(np.int64)
        if at is None:
            self.v[sl] += term
            self.A[sl] += mag
            self.n[sl] += nz
        else:
            np.add.at(self.v, at, term)
            np.add.at(self.A, at, mag)
            np.add.at(self.n, at, nz)


def _corner_factors(fr, D, idx, dtype):
    """[B, D]: the factor of each axis of corner idx: fraction on the far side, 1 - fraction on the near side"""
    one = dtype(1)
    return np.stack([fr[:, d] if (idx >> d) & 1 else one - fr[:, d] for d in range(D)], axis=1)


def _weight(fac, skip=None):
    """product of the axis factors in axis order (without axis `skip`)"""
    w = np.ones(fac.shape[0], fac.dtype)
    for d in range(fac.shape[1]):
        if d != skip:
            w = w * fac[:, d]
    return w


def tgrid_encode(geo, x32, t32, emb, gout, dtype=np.float64):
    """x32 [B, D] float32, t32 [B] float32 in [0, 1] (one per sample), emb [rows, C + T], gout [B, L * C] ->
    dict of out [B, L, C], dy_dx [B, L, D, C], gtable [rows, C + T], gx [B, D], each with its A_* and n_*; cells [L][B, D] and
    pos [L][B, D] (float32) for the boundary bookkeeping.  A sample with a coordinate outside [0, 1] reads nothing and receives nothing."""
    x32 = np.asarray(x32, F32)
    B, D = x32.shape
    C, T, L = geo["C"], geo["T"], geo["L"]
    emb, g = np.asarray(emb).astype(dtype), np.asarray(gout).astype(dtype).reshape(B, L, C)
    inside = ~((x32 < 0) | (x32 > 1)).any(axis=1)
    col, wt = temporal_slots(t32, C, T, dtype)
    out, dydx = _Acc((B, L, C), dtype), _Acc((B, L, D, C), dtype)
    gtab, gx = _Acc(emb.shape, dtype), _Acc((B, D), dtype)
    cells, poss = [], []
    for l, lv in enumerate(geo["levels"]):
        pos = tg_pos(x32, lv["scale"], geo["align_corners"])
        cell, fr32 = cell_of(pos)
        cells.append(cell)
        poss.append(pos)
        fr, scale = fr32.astype(dtype), dtype(lv["scale"])
        for idx in range(1 << D):
            fac = _corner_factors(fr, D, idx, dtype)
            w = _weight(fac)
            row = lv["off0"] + corner_rows(lv, cell, idx)
            for ab in (0, 1):
                live = inside[:, None] & (wt[:, :, ab] != 0)                       # [B, C]
                val = np.where(live, emb[row[:, None], col[:, :, ab]] * wt[:, :, ab], dtype(0))
                out.add(w[:, None] * val, sl=(slice(None), l))
                for gd in range(D):
                    wo = scale * _weight(fac, skip=gd)
                    dydx.add((wo if (idx >> gd) & 1 else -wo)[:, None] * val, sl=(slice(None), l, gd))
                tg = np.where(live, w[:, None] * (g[:, l] * wt[:, :, ab]), dtype(0))
                gtab.add(tg, at=(np.broadcast_to(row[:, None], tg.shape), col[:, :, ab]))
    for l in range(L):
        for ch in range(C):
            gx.add(g[:, l, ch][:, None] * dydx.v[:, l, :, ch])
    # a coordinate-gradient term is one product of the chain, not one (level, channel) sum: A and n follow the dy_dx terms
    gx.A = (np.abs(g).astype(np.float64)[:, :, None, :] * dydx.A).sum(axis=(1, 3))
    gx.n = ((g != 0)[:, :, None, :] * dydx.n).sum(axis=(1, 3))
    res = {}
    for name, a in (("out", out), ("dy_dx", dydx), ("gtable", gtab), ("gx", gx)):
        res[name], res["A_" + name], res["n_" + name] = a.v, a.A, a.n
    res["inside"], res["cells"], res["pos"] = inside, cells, poss
    return res


def hash_encode(geo, x32, table, gout, dtype=np.float64):
    """x32 [B, D] float32 (no bounds check: a coordinate below 0 wraps through the uint32 cast), table [rows, F], gout [B, L * F] ->
    dict of out [B, L, F], gtable [rows, F], gx [B, D] with A_* and n_*; cells and pos per level."""
    x32 = np.asarray(x32, F32)
    B, D = x32.shape
    F, L = geo["F"], geo["L"]
    table, g = np.asarray(table).astype(dtype).reshape(-1, F), np.asarray(gout).astype(dtype).reshape(B, L, F)
    out, gtab, gx = _Acc((B, L, F), dtype), _Acc(table.shape, dtype), _Acc((B, D), dtype)
    cells, poss = [], []
    fcol = np.broadcast_to(np.arange(F)[None, :], (B, F))
    for l, lv in enumerate(geo["levels"]):
        pos = ht_pos(x32, lv["scale"])
        cell, fr32 = cell_of(pos)
        cells.append(cell)
        poss.append(pos)
        fr, scale = fr32.astype(dtype), dtype(lv["scale"])
        for idx in range(1 << D):
            fac = _corner_factors(fr, D, idx, dtype)
            w = _weight(fac)
            row = lv["off0"] + corner_rows(lv, cell, idx)
            out.add(w[:, None] * table[row], sl=(slice(None), l))
            gtab.add(w[:, None] * g[:, l], at=(np.broadcast_to(row[:, None], (B, F)), fcol))
            for gd in range(D):
                wo = _weight(fac, skip=gd)
                tx = scale * ((wo if (idx >> gd) & 1 else -wo)[:, None] * (table[row] * g[:, l]))   # [B, F]
                gx.v[:, gd] += tx.sum(axis=1)
                gx.A[:, gd] += np.abs(tx).astype(np.float64).sum(axis=1)
                gx.n[:, gd] += (tx != 0).sum(axis=1)
    res = {}
    for name, a in (("out", out), ("gtable", gtab), ("gx", gx)):
        res[name], res["A_" + name], res["n_" + name] = a.v, a.A, a.n
    res["cells"], res["pos"] = cells, poss
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# exactness bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------------
def low_bit_exponent(v):
    """exponent of the lowest set bit of every non-zero float64 in v (an int array; zeros are left out)"""
    v = np.asarray(v, np.float64).ravel()
    v = v[v != 0]
    m, e = np.frexp(v)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((M & -M).astype(np.float64)).astype(np.int64)
    return e - 53 + tz


def granule(*arrays):
    """the largest power of two that divides every non-zero value of the arrays"""
    return 2.0 ** min(int(low_bit_exponent(a).min()) for a in arrays if np.any(np.asarray(a) != 0))


# ------------------------------------------------------------------------------------------------------------------------------------
# part A: the lattice cases.  per_level_scale 2 and a power-of-two or small integer base: integer scales; coordinates multiples of 1/8 (1/16 in
# the ray cases), times multiples of 1/(4 n), table values multiples of 1/4 in [-1, 1], integer upstream gradients in [-4, 4].
# ------------------------------------------------------------------------------------------------------------------------------------
TGRID_LATTICE = [
    dict(case_id="t_c2_hash", kw=dict(temporal_dim=6, level_dim=2, num_levels=4, log2_hashmap_size=10, base_resolution=4), mode="points", seed=11),
    dict(case_id="t_c4_rays", kw=dict(temporal_dim=10, level_dim=4, num_levels=3, log2_hashmap_size=11, base_resolution=4), mode="rays", extent=1, seed=12),
    dict(case_id="t_c1_tiled", kw=dict(temporal_dim=3, level_dim=1, num_levels=3, log2_hashmap_size=8, base_resolution=4, gridtype="tiled"), mode="points", seed=13),
    dict(case_id="t_c8_rays", kw=dict(temporal_dim=18, level_dim=8, num_levels=3, log2_hashmap_size=9, base_resolution=2), mode="rays", extent=2, seed=14),
    dict(case_id="t_all_dense", kw=dict(temporal_dim=4, level_dim=2, num_levels=3, log2_hashmap_size=19, base_resolution=2), mode="points", seed=15),
    dict(case_id="t_align", kw=dict(temporal_dim=6, level_dim=2, num_levels=4, log2_hashmap_size=10, base_resolution=4, align_corners=True), mode="points", seed=16),
    dict(case_id="t_d2", kw=dict(temporal_dim=4, level_dim=2, num_levels=3, log2_hashmap_size=8, base_resolution=4, input_dim=2), mode="points", seed=17),
]
for _c in TGRID_LATTICE:
    _c["kw"].setdefault("per_level_scale", 2.0)

HASH_LATTICE = [
    dict(case_id="h_f2", cfg=dict(n_levels=4, n_features_per_level=2, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=10), seed=21),
    dict(case_id="h_f4_all_dense", cfg=dict(n_levels=3, n_features_per_level=4, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=12), seed=22),
    dict(case_id="h_f1_d2", cfg=dict(n_levels=4, n_features_per_level=1, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=8, D=2), seed=23),
    dict(case_id="h_f8", cfg=dict(n_levels=4, n_features_per_level=8, base_resolution=2, per_level_scale=2.0, log2_hashmap_size=9), seed=24),
    dict(case_id="h_f1_base3", cfg=dict(n_levels=4, n_features_per_level=1, base_resolution=3, per_level_scale=2.0, log2_hashmap_size=11), seed=25),
    dict(case_id="h_f2_all_hashed", cfg=dict(n_levels=2, n_features_per_level=2, base_resolution=8, per_level_scale=2.0, log2_hashmap_size=8), seed=26),
]

LATTICE_B = 1500          # not a multiple of 256 (a workgroup) or of 32 (TG_RUN)
RAYS, SAMPLES = 41, 37    # ray cases: B = 1517; S = 37 is two ragged segments (19 + 18)
START = 3.0               # what an accumulating buffer holds before the route runs, in its second check


def _values(rng, shape):
    """multiples of 1/4 in [-1, 1], a fifth of them exactly zero"""
    v = rng.integers(-4, 5, shape).astype(F32) / F32(4)
    v[rng.random(shape) < 0.2] = 0
    return v


def _gout(rng, B, L, C):
    """integers in [-4, 4]; some samples all zero, some (sample, level) pairs all zero"""
    g = rng.integers(-4, 5, (B, L, C)).astype(F32)
    g[rng.random(B) < 0.05] = 0
    g[rng.random((B, L)) < 0.1] = 0
    g[5:9] = 0
    g[11, 0] = 0
    return g.reshape(B, L * C)


def make_tgrid_lattice_case(case):
    rng = np.random.default_rng(case["seed"])
    geo = tgrid_geometry(**case["kw"])
    D, C, T, L = geo["D"], geo["C"], geo["T"], geo["L"]
    n = T - 2
    d = dict(case=case, geo=geo)
    if case["mode"] == "rays":
        R, S = RAYS, SAMPLES
        ext = float(case["extent"])
        lo = np.array([-0.5, 0.0, -1.0], F32) if ext == 2 else np.array([0.0, 0.0, 0.0], F32)
        step = 0.5 if ext == 2 else 0.25          # edges are multiples of it: x is a multiple of 1/16 either way
        o = (lo + rng.integers(2, 7, (R, 3)).astype(F32) / F32(8) * F32(ext)).astype(F32)
        dirs_pool = np.array([0, 0, 0, 0.5, -0.5, 0.5, -0.5, 1, -1], F32)
        dirs = rng.choice(dirs_pool, (R, 3))
        # a ray rests (consecutive samples in one cell: zero-width bins) except on one stretch where every bin advances by a step
        inc = np.zeros((R, S + 1), F32)
        for r in range(R):
            a, m = int(rng.integers(1, S - 4)), int(rng.integers(0, 4))
            inc[r, a:a + m] = step
        inc[:, 0] = rng.integers(0, 2, R).astype(F32) * F32(step)
        edges = np.cumsum(inc, axis=1).astype(F32)
        o[0], dirs[0] = lo, 0                      # a ray that sits on the corner (0, 0, 0) ...
        o[1], dirs[1] = lo + F32(ext), 0           # ... and one on (1, 1, 1)
        t = (rng.integers(0, 4 * n + 1, R).astype(F32) / F32(4 * n)).astype(F32)
        t[2:n + 3] = np.arange(n + 1, dtype=F32) / F32(n)  # every knot, 0 and 1 among them
        t[1] = 1.0                                 # (1, 1, 1) at t == 1
        d.update(R=R, S=S, spr=S, origins=o, dirs=dirs, ebins=edges, aabb=[lo.tolist(), (lo + F32(ext)).tolist()], times=t)
        x = ray_x(o, dirs, edges, lo, lo + F32(ext))
        B = R * S
        t_sample = np.repeat(t, S)
    else:
        B = LATTICE_B
        x = (rng.integers(0, 9, (B, D)).astype(F32) / F32(8)).astype(F32)
        out = np.flatnonzero(rng.random(B) < 0.15)                              # a share of samples leaves [0, 1] on one axis
        x[out, rng.integers(0, D, len(out))] = rng.choice(np.array([-0.125, 1.125, 1.25], F32), len(out))
        x[0], x[1] = 1.0, 0.0
        x[2] = 0.5
        x[2, 0] = 1.0
        x[3] = 0.5
        x[3, -1] = 0.0
        t = (rng.integers(0, 4 * n + 1, B).astype(F32) / F32(4 * n)).astype(F32)
        t[4:n + 5] = np.arange(n + 1, dtype=F32) / F32(n)  # every knot, 0 and 1 among them
        t[0] = 1.0                                 # (1, ..., 1) at t == 1
        d.update(spr=1, times=t)
        t_sample = t
    emb = _values(rng, (geo["offsets"][-1], geo["grid_C"]))
    d.update(B=B, x=x, t_sample=t_sample, emb=emb, gout=_gout(rng, B, L, C), trow=temporal_row_index(t_sample, C, T))
    return d


def make_hash_lattice_case(case):
    rng = np.random.default_rng(case["seed"])
    geo = hash_geometry(**case["cfg"])
    B, D = LATTICE_B, geo["D"]
    x = (rng.integers(-2, 11, (B, D)).astype(F32) / F32(8)).astype(F32)         # -1/4 .. 5/4: no bounds check, the wrap-around is under test
    x[0], x[1], x[2] = 1.0, 0.0, -0.25
    x[3] = 0.5
    x[3, 0] = 1.0
    table = _values(rng, (geo["offsets"][-1], geo["F"]))
    return dict(case=case, geo=geo, B=B, x=x, table=table, gout=_gout(rng, B, geo["L"], geo["F"]))


def exactness(ref, names, start=START):
    """For the sums `names` of a reference result: the granule of all their terms' sums' building blocks and the largest (A + start) / granule.
    Every term and every partial sum of an element is a multiple of the granule and below A + start in magnitude, so with the ratio below 2^24
    every partial sum in any order is a float32."""
    out = {}
    for k in names:
        gr = granule(ref[k], ref["A_" + k])
        out[k] = (gr, float((ref["A_" + k].max() + start) / gr))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# part B: cell boundaries at non-dyadic scales
# ------------------------------------------------------------------------------------------------------------------------------------
TGRID_BOUNDARY = [
    dict(case_id="tb_1p5", kw=dict(temporal_dim=8, level_dim=2, num_levels=4, log2_hashmap_size=10, base_resolution=4, per_level_scale=1.5), seed=31),
    dict(case_id="tb_1p447", kw=dict(temporal_dim=6, level_dim=4, num_levels=4, log2_hashmap_size=11, base_resolution=5, per_level_scale=1.4472692), seed=32),
    dict(case_id="tb_desired", kw=dict(temporal_dim=10, level_dim=2, num_levels=5, log2_hashmap_size=10, base_resolution=4, desired_resolution=50), seed=33),
    dict(case_id="tb_align", kw=dict(temporal_dim=6, level_dim=1, num_levels=3, log2_hashmap_size=9, base_resolution=4, per_level_scale=1.5, align_corners=True), seed=34),
]
HASH_BOUNDARY = [
    dict(case_id="hb_1p5", cfg=dict(n_levels=4, n_features_per_level=2, base_resolution=4, per_level_scale=1.5, log2_hashmap_size=10), seed=41),
    dict(case_id="hb_1p447", cfg=dict(n_levels=5, n_features_per_level=4, base_resolution=5, per_level_scale=1.4472692, log2_hashmap_size=11), seed=42),
    dict(case_id="hb_1p447_f1", cfg=dict(n_levels=4, n_features_per_level=1, base_resolution=16, per_level_scale=1.4472692, log2_hashmap_size=12), seed=43),
]
N_RANDOM = 300


def boundary_points(geo, rng, lo=0.0, hi=1.0):
    """For each level and axis: x = fl32(k / scale) and fl32((k - 0.5) / scale) with their two float32 neighbours (a triple that shares its other
    coordinates), k over the first, middle and last cells and the powers of two (where pos changes binade: the two rounding rules part there).  Then (1, .., 1), (0, .., 0) and N_RANDOM random points.  All inside [lo, hi].
    -> (points [B, D] float32, triples [(first index, level, axis)])."""
    D = geo["D"]
    pts, triples = [], []
    for l, lv in enumerate(geo["levels"]):
        s = float(lv["scale"])
        last = int(np.ceil(s))
        for k in sorted({0, 1, 2, last // 2, last // 2 + 1, last - 1, last, last + 1} | {1 << j for j in range(2, 7) if (1 << j) <= last + 1}):
            for c in (k / s, (k - 0.5) / s):
                c = F32(c)
                three = (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf)))
                if not all(lo <= float(v) <= hi for v in three):
                    continue
                for axis in range(D):
                    p = rng.random(D).astype(F32) * F32(hi - lo) + F32(lo)
                    triples.append((len(pts), l, axis))
                    for v in three:
                        q = p.copy()
                        q[axis] = v
                        pts.append(q)
    # points at which the temporal grid's two roundings and the static grid's one rounding of pos fall into different cells, searched among the
    # neighbours of every cell boundary of the level (they are rare): a few per level, each on one axis
    if not geo.get("align_corners"):
        for lv in geo["levels"]:
            s = float(lv["scale"])
            cand = np.array([(k - 0.5) / s for k in range(0, int(np.ceil(s)) + 2)], F32)
            cand = np.concatenate([np.nextafter(cand, F32(-np.inf)), cand, np.nextafter(cand, F32(np.inf))])
            cand = cand[(cand >= lo) & (cand <= hi)]
            cand = cand[np.floor(tg_pos(cand, lv["scale"], False)) != np.floor(ht_pos(cand, lv["scale"]))][:4]
            for i, v in enumerate(cand):
                p = rng.random(D).astype(F32) * F32(hi - lo) + F32(lo)
                p[i % D] = v
                pts.append(p)
    pts.append(np.ones(D, F32))
    pts.append(np.zeros(D, F32))
    rnd = rng.random((N_RANDOM, D)).astype(F32) * F32(hi - lo) + F32(lo)
    return np.clip(np.concatenate([np.stack(pts), rnd]).astype(F32), F32(lo), F32(hi)), triples


def _random_table(rng, geo, width):
    """uniform in [-1/2, 1/2): neighbouring cells differ by O(1), their derivative by O(scale) -- against rounding bounds of O(1e-6)"""
    return rng.random((geo["offsets"][-1], width)).astype(F32) - F32(0.5)


def make_tgrid_boundary_case(case):
    rng = np.random.default_rng(case["seed"])
    geo = tgrid_geometry(**case["kw"])
    C, T, L = geo["C"], geo["T"], geo["L"]
    n = T - 2
    x, triples = boundary_points(geo, rng)
    B = len(x)
    first_random = B - N_RANDOM
    x[first_random:B:17, 0] = F32(1.0) + F32(0.03)      # a few out-of-range samples among the random points
    x[first_random + 3:B:23, -1] = F32(-0.02)
    t = rng.random(B).astype(F32)
    for i, _, _ in triples:                              # a triple shares its time: its members differ in one coordinate only
        t[i:i + 3] = t[i]
    t[first_random:first_random + n + 1] = np.arange(n + 1, dtype=F32) / F32(n)   # every knot
    gout = rng.random((B, L * C)).astype(F32) - F32(0.5)
    for i, _, _ in triples:                              # ... and its upstream gradient
        gout[i:i + 3] = gout[i]
    return dict(case=case, geo=geo, B=B, x=x, triples=triples, spr=1, times=t, t_sample=t, emb=_random_table(rng, geo, geo["grid_C"]),
                gout=gout, trow=temporal_row_index(t, C, T))


def make_hash_boundary_case(case):
    rng = np.random.default_rng(case["seed"])
    geo = hash_geometry(**case["cfg"])
    x, triples = boundary_points(geo, rng, lo=-0.25, hi=1.25)
    B = len(x)
    gout = rng.random((B, geo["L"] * geo["F"])).astype(F32) - F32(0.5)
    for i, _, _ in triples:                              # a triple shares its upstream gradient: its members differ in one coordinate only
        gout[i:i + 3] = gout[i]
    return dict(case=case, geo=geo, B=B, x=x, triples=triples, table=_random_table(rng, geo, geo["F"]), gout=gout)


def rounding_decided(geo, x32):
    """(point, level, axis) triples [B, L, D] whose cell is decided by the float32 rounding of pos: floor of the exact x * scale + offset differs
    from floor of the kernel's float32 pos.  The reference follows the float32 pos, so none of them has to be excluded from a comparison; they
    are what part B is about."""
    x32 = np.asarray(x32, F32)
    out = np.zeros((x32.shape[0], geo["L"], x32.shape[1]), bool)
    for l, lv in enumerate(geo["levels"]):
        off = 0.0 if geo.get("align_corners") else 0.5
        exact = x32.astype(np.float64) * np.float64(lv["scale"]) + off        # exact: 48-bit product, the sum fits float64 for these magnitudes
        pos = tg_pos(x32, lv["scale"], geo["align_corners"]) if geo["kind"] == "tgrid" else ht_pos(x32, lv["scale"])
        out[:, l] = np.floor(exact) != np.floor(pos.astype(np.float64))
    return out


def rules_differ(geo, x32):
    """[B, L, D]: where the two-rounding pos (temporal grid) and the one-rounding pos (static grid) of the same x and scale fall into different
    cells -- the points at which compiling one encoder's cell with the other's contraction rule shows."""
    x32 = np.asarray(x32, F32)
    out = np.zeros((x32.shape[0], geo["L"], x32.shape[1]), bool)
    if geo.get("align_corners"):
        return out
    for l, lv in enumerate(geo["levels"]):
        out[:, l] = np.floor(tg_pos(x32, lv["scale"], False)) != np.floor(ht_pos(x32, lv["scale"]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# part B bounds: k roundings on a term's way through a kernel, counted from the kernel text (u = 2^-24; a rounding of a factor or a product
# moves the term by at most u |term|, a rounding of a partial sum by at most u x the sum of |terms|, so |error| <= k u A to first order; every
# count below is an upper bound -- not every factor rounds -- which covers the second-order part)
# ------------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
# temporal grid, forward value (tgrid_kernel<false> and tgrid_runs_kernel<false>, the same arithmetic): time weight (r + 1) - v or v - r: 1; three
# 1 - fraction: 3; w = f0 * f1 * f2: 2; value * time weight: 1; w * that: 1; eight corner adds: 8 (the first adds to 0); the pair sum of the a | b
# lanes: 1
K_TG_OUT = 1 + 3 + 2 + 1 + 1 + 8 + 1
# dy_dx: time weight 1; two 1 - fraction: 2; scale * f * f: 2; value * time weight: 1; wo * that: 1; eight corner adds: 8; the pair sum: 1
K_TG_DYDX = 1 + 2 + 2 + 1 + 1 + 8 + 1
# a table-gradient term w * (g * wt): time weight 1; 1 - fraction 3; w 2; g * wt 1; w * that 1
K_TG_TERM = 1 + 3 + 2 + 1 + 1
# static grid, forward value: 1 - fraction 3; w 2; eight fused multiply-adds 8 (without contraction: a product and seven adds)
K_HT_OUT = 3 + 2 + 8
# a table-gradient term w * g: 1 - fraction 3; w 2; the product 1
K_HT_TERM = 3 + 2 + 1


def k_tg_gx(L, C):
    """snerf_tgrid_input_bwd on the kernel's dy_dx: the dy_dx chain, g * dy_dx, L C sequential adds"""
    return K_TG_DYDX + 1 + L * C


def k_ht_gx(L, F):
    """hashgrid_kernel's coordinate gradient: table * g 1; the butterfly over the F feature lanes log2 F; two 1 - fraction 2; wo 1; wo * dot 1; four
    corner adds per lane 4; the butterfly over the two x-corner lanes 1; * scale 1; one atomic add per level into the buffer L"""
    return 1 + int(np.log2(F)) + 2 + 1 + 1 + 4 + 1 + 1 + L


def table_bound(A, n, k_term, fixed_point=False):
    """per table entry: the term's own roundings, n - 1 adds among the n terms in whatever order (atomics, registers of a run, a tile's LDS image) and
    one add into what the buffer held; the fixed-point routes convert every addend with an absolute error of 2^-51 and round once more on the way
    back to float"""
    k = k_term + n + (1 if fixed_point else 0)
    return k * U * A + (n * 2.0 ** -51 if fixed_point else 0.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# cases by id, built once (tests share them and leave them unchanged)
# ------------------------------------------------------------------------------------------------------------------------------------
_MAKERS = {}
for _list, _make in ((TGRID_LATTICE, make_tgrid_lattice_case), (HASH_LATTICE, make_hash_lattice_case), (TGRID_BOUNDARY, make_tgrid_boundary_case),
                     (HASH_BOUNDARY, make_hash_boundary_case)):
    for _c in _list:
        _MAKERS[_c["case_id"]] = (_c, _make)


@functools.lru_cache(maxsize=None)
def case_and_reference(case_id):
    """-> (the case's data, its float64 reference)"""
    c, make = _MAKERS[case_id]
    d = make(c)
    if d["geo"]["kind"] == "tgrid":
        return d, tgrid_encode(d["geo"], d["x"], d["t_sample"], d["emb"], d["gout"])
    return d, hash_encode(d["geo"], d["x"], d["table"], d["gout"])

"""The fused gather-to-MLP kernels (csrc/field_fused.hip + field_fused_static.hip, proposal_fused.hip, proposal_bwd.hip) and the plane gather they
are compared with (csrc/kplanes.hip: snerf_kplanes_gather_fwd, with the in-kernel ray-sample coordinates of kplanes_common.hpp) against EXACT
float64 answers: the composition of tests/mlp_reference.py (the nets) with the plane lattice of tests/test_gpu_kplanes.py (the gather and scatter).

The restatement (all of it plain torch, float64 unless a dtype is passed)
  coordinates   mode 0: the points.  mode 1 (include/snerf.h, snerf_coords): tmid = (e[s] + e[s+1]) / 2, pos = o + d tmid,
                q = (pos - aabb_min) / (aabb_max - aabb_min), p = 2 q - 1 with `rescale`, else q; t = 2 time - 1; three-coordinate sets have no time.
  plane value   align_corners = True, border padding: pix = clamp((x + 1) / 2 (size - 1), 0, size - 1), corners floor and floor + 1, a corner
                beyond the last texel adds nothing; value = sum of the four texels times the products of the axis weights.
  features      product over a scale's planes (XY XZ XT YZ YT ZT; XY XZ YZ for three coordinates and for the frozen-time view of a
                four-coordinate buffer), concatenated or summed over the scales.
  nets          mlp_reference.restate: the proposal level 8 -> 64 -> 1 with trunc_exp on its only column; the field 32 n_scales -> 128 -> 16, density
                exp(h[:, 15]), then 15 -> 64 -> 64 -> 3 (Sigmoid) on h[:, :15].
  backward      gX and the weight gradients from restate; plane gradients by the product rule with LEAVE-ONE-OUT products over the other planes
                (an exactly-zero plane value does not hide the other planes' gradients), times the tap weights, summed per texel.

Exactness (asserted per case in float64 by `make`, which raises otherwise)
  (a) every coordinate, pixel position and tap weight is a multiple of 2^-8 of small magnitude (dyadic);
  (b) every plane value and feature is a float32 value and a fixed point of the operand rounding `rd` for bf16 AND fp16;
  (c) every hidden activation is a fixed point of that rounding, (d) and so is h[:, :15] of the field (restate's ("round", ...) trace records);
  (e) every accumulation sums multiples of one power of two u with sum |terms| / u < 2^24: the layer products and every weight-gradient element
      (restate's ("acc", ...) records), and every texel's gradient over all samples (`plane_grads(..., absolute=True)`);
  (f) the exp head's incoming gradient is float32(t / exp(clamp(z))) with t from mlp_reference.TARGETS, and the rounded gradient tile is exactly t.
So features, feat16, h, gX, the weight gradients and the plane gradients must come back with the bits of the float64 answer, whatever the order of
MFMA slots, waves, runs and atomics.  Density and rgb sit behind exp / Sigmoid and are exact only where the raw head output is exactly 0 (density 1,
rgb 1/2): the PLANTED rows, at least one eighth of every case.  Elsewhere they are bounded by 5 x the float32 restatement's deviation
(profiles/r25_fused_deviations.json, written by tools/measure_fused_deviations.py); the yardstick is taken over the case's rows plus 1024
further feature rows through the case's own nets (`_yard_feat`: a worst deviation over a handful of distinct values says nothing about float32).

Inputs
  resolutions   4 m + 1 per space axis, 3 on time: [5,5,5,3] and [9,9,9,3] (test_gpu_kplanes._LATTICE_RES) for the proposal levels and the summed
                gather; the field's scales take the multipliers of tests/test_gpu_field_fused.py, so 13 and 25 appear beside 2^k + 1 (pixel positions
                stay dyadic: 6 (x + 1), 12 (x + 1)).  aabb [-1,1]^3 and [-2,2]^3; dyadic origins, unnormalised directions, integer bin edges.
  "values"      samples on texel centres (space {-1, -1/2, 0, 1/2, 1}, time {-1, 0, 1}), texels from {1/2, 1, 2} with 3 % exact zeros: features
                are powers of two or 0.  One non-zero weight per unit in every layer that feeds a rounding (2^6 - 2^-6 is no bf16 value).
  "weights"     coordinates from {-1.25, -1 + k/8, 1.25}: fractional taps on every axis, clamped samples, 1.0 exactly on the last texel.  All
                planes 1.0 except ONE plane per case (`special`: a space plane in some cases, a time plane in others) holding integers 0..2:
                features are multiples of 1/32 up to 2.  TWO non-zero weights per first-layer unit (|sum| <= 4: eight bits), two of opposite sign
                per unit where a layer reads ReLU outputs (a difference within [-4, 4]).
  planted rows  every plane holds 1.0 in all channels of its centre texel and every 8th row (ray) sits there, so its features are all 1; every
                head column takes an even number of the units that are active on the all-ones input with alternating signs (`_balanced`), so its
                raw output is exactly 0 there while the units themselves are not.  Planted rays have direction 0 and are joined by their
                neighbour in the "same" cases, so consecutive rays hit the same texel.

Narrowings recorded: the "values" kind has one non-zero weight per unit (condition (c) with features from 2^-6 to 2^6); h[:, :15] of the "weights"
kind comes from pairs of opposite sign only (condition (d)); multipliers 3 and 6 give resolutions 13 and 25.

Importable on the CPU; reads nothing outside the repository."""
import functools
import math
import zlib
from collections import namedtuple

import torch

from tests import mlp_reference as R

F64 = torch.float64
GUARD_ROWS = 3
POISON = float("nan")  # what the time planes of a frozen-time case hold: no output may read it
POINT_N = (1, 31, 32, 33, 63, 64, 65, 127, 129, 1000, 4097)
RAY_SHAPES = ((1, 1), (5, 7), (37, 50), (3, 32), (2, 64), (129, 33))
FIELD_MS = ((1,), (1, 2), (1, 2, 4), (1, 2, 4, 8, 16), (1, 2, 3, 4, 6, 8))
VIEWS = ("4", "3", "frozen")
PLANT_EVERY = 8

# kernel: gather | dfwd | dbwd | field.  kind: values | weights.  view: 4 | 3 | frozen.  mode 0: N points; mode 1: R rays x S samples (N = R S).
# ms: the scales' multipliers; C / concat: the plane set (gather only; proposal 8 / summed, field 32 / concatenated).  relu: the proposal net's hidden
# activation.  special: which (scale, plane) of a "weights" case holds the integers.  same: rays in blocks on one point, direction 0.
# Not part of the content: keep (field outputs 0 none, 1 feat16 + h, 2 + feat32), order (the ordered entry point as well), nogx, ws0, gp0 (proposal backward).
Case = namedtuple("Case", "kernel kind view mode N R S rescale A ms C concat operands relu special same keep order nogx ws0 gp0")


def case_id(c):
    shape = f"N{c.N}" if c.mode == 0 else f"R{c.R}xS{c.S}-rs{c.rescale}" + ("-same" if c.same else "")
    tail = {"gather": f"C{c.C}{'cat' if c.concat else 'sum'}", "dfwd": f"relu{c.relu}", "field": f"keep{c.keep}" + ("-ord" if c.order else ""),
            "dbwd": f"relu{c.relu}" + ("-nogx" if c.nogx else "") + f"-ws{c.ws0:g}-gp{c.gp0:g}"}[c.kernel]
    return f"{c.kernel}-{c.kind}-v{c.view}-{shape}-A{c.A}-ms{'.'.join(map(str, c.ms))}-op{c.operands}-sp{c.special}-{tail}"


def content_key(c):
    return c._replace(keep=0, order=0, nogx=0, ws0=0.0, gp0=0.0)


# ------------------------------------------------------------------------------------------------ restatement
def resolutions(ms, n_coords):
    return [([4 * m + 1] * 3 + [3])[:n_coords] for m in ms]


def coordinates(co, n_coords, dtype=F64):
    """[N, n_coords] sample coordinates in grid_sample's [-1, 1] convention."""
    if co["mode"] == 0:
        return co["pts"].to(dtype)
    o, d, eb = co["o"].to(dtype), co["d"].to(dtype), co["eb"].to(dtype)
    tmid = (eb[:, :-1] + eb[:, 1:]) / 2
    pos = o[:, None, :] + d[:, None, :] * tmid[..., None]
    lo, hi = torch.tensor(co["aabb"][0], dtype=dtype), torch.tensor(co["aabb"][1], dtype=dtype)
    q = (pos - lo) / (hi - lo)
    p = q * 2 - 1 if co["rescale"] else q
    if n_coords == 4:
        t = (co["t"].to(dtype) * 2 - 1)[:, None, None].expand(p.shape[0], p.shape[1], 1)
        p = torch.cat([p, t], dim=-1)
    return p.reshape(-1, n_coords)


def axis_taps(x, size):
    """(i0, i1, w0, w1) along one axis: align_corners = True, border padding; the corner beyond the last texel carries weight 0."""
    pix = ((x + 1) / 2 * (size - 1)).clamp(0, size - 1)
    f0 = torch.floor(pix)
    inside = f0 + 1 <= size - 1
    w1 = torch.where(inside, pix - f0, torch.zeros_like(pix))
    w0 = (f0 + 1) - pix
    i0 = f0.long()
    return i0, torch.where(inside, i0 + 1, i0), w0, w1


def _corners(tx, ty, W):
    (x0, x1, wx0, wx1), (y0, y1, wy0, wy1) = tx, ty
    return ((y0 * W + x0, wx0 * wy0), (y0 * W + x1, wx1 * wy0), (y1 * W + x0, wx0 * wy1), (y1 * W + x1, wx1 * wy1))


def plane_list(ps, view):
    """[(plane index in the buffer, (a, b))] of the planes a view reads."""
    if view == "frozen":
        return [(q, ps.combs[q]) for q in (0, 1, 3)]
    return list(enumerate(ps.combs))


def gather(ps, planes, p, view):
    """-> features [N, out_dim], and per scale the list of (plane index, values [N, C], corners) the backward needs."""
    outs, parts = [], []
    for s, reso in enumerate(ps.resolutions):
        vals = []
        for q, (a, b) in plane_list(ps, view):
            H, W = ps.shapes[s][q]
            flat = ps.plane_view(s, q, planes).reshape(H * W, ps.C)
            cs = _corners(axis_taps(p[:, a], reso[a]), axis_taps(p[:, b], reso[b]), W)
            v = sum(flat[idx] * w[:, None] for idx, w in cs)
            vals.append((q, v, cs))
        prod = vals[0][1]
        for _, v, _ in vals[1:]:
            prod = prod * v
        outs.append(prod)
        parts.append(vals)
    return (torch.cat(outs, dim=-1) if ps.concat else sum(outs)), parts


def plane_grads(ps, planes, p, view, gfeat, absolute=False):
    """Gradient of sum(gfeat * features) with respect to the flat plane buffer: the product rule with leave-one-out products, written out.
    absolute: the sum of |terms| per texel instead, and the unit of all terms (condition (e))."""
    _, parts = gather(ps, planes, p, view)
    out = torch.zeros(ps.numel, dtype=planes.dtype)
    terms = []
    for s, vals in enumerate(parts):
        g = gfeat[:, s * ps.C:(s + 1) * ps.C] if ps.concat else gfeat
        for k, (q, _, cs) in enumerate(vals):
            loo = torch.ones_like(g)
            for k2, (_, v2, _) in enumerate(vals):
                if k2 != k:
                    loo = loo * v2
            H, W = ps.shapes[s][q]
            dst = ps.plane_view(s, q, out).reshape(H * W, ps.C)
            for idx, w in cs:
                t = g * loo * w[:, None]
                if absolute:
                    t = t.abs()
                    terms.append(t[t != 0])
                dst.index_add_(0, idx, t)
    if absolute:
        return out, R.unit(torch.cat(terms)) if terms and sum(t.numel() for t in terms) else 1.0
    return out


def proposal(feat, Ws, relu, operands, gdens=None, dtype=F64, trace=None):
    """8 -> 64 -> 1, density = trunc_exp(z): restate's z, aux (the density) and, with gdens, g_out, gX, gW."""
    return R.restate(feat.to(dtype), Ws, relu, 0, operands, None, 0, gdens, dtype=dtype, trace=trace)


def field(feat, Wsig, Wcol, operands, dtype=F64, trace=None):
    """-> h [N, 16], density = exp(h[:, 15]), rgb = Sigmoid net on h[:, :15], and the hidden layers' record."""
    s = R.restate(feat.to(dtype), Wsig, 1, 0, operands, aux_col=15, dtype=dtype, trace=trace)
    h = s["z"]
    if trace is not None:
        trace.append(("round", "h[:, :15]", int((R.rd(h[:, :15], 1) != h[:, :15]).sum() + (R.rd(h[:, :15], 2) != h[:, :15]).sum())))
    c = R.restate(h[:, :15], Wcol, 1, 1, operands, dtype=dtype, trace=trace)
    return {"h": h, "density": s["aux"], "rgb": c["Y"], "z_rgb": c["z"]}


# ------------------------------------------------------------------------------------------------ inputs
def _plane_set(c):
    from soccernerfs_amd.plane_set import PlaneSet

    return PlaneSet(c.C, resolutions(c.ms, 3 if c.view == "3" else 4), concat=bool(c.concat), generator=torch.Generator().manual_seed(1))


def _special(c, ps):
    """(scale, plane index in the buffer) of the plane that holds the integers of a "weights" case; the view reads it."""
    pl = plane_list(ps, c.view)
    return (c.special // len(pl)) % len(c.ms), pl[c.special % len(pl)][0]


def _planes(c, ps, gen):
    buf = torch.ones(ps.numel, dtype=F64)
    if c.kind == "values":
        buf = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (ps.numel,), generator=gen)]
        buf[torch.rand(ps.numel, generator=gen) < 0.03] = 0.0
    else:
        s, q = _special(c, ps)
        v = ps.plane_view(s, q, buf)
        v.copy_(torch.randint(0, 3, tuple(v.shape), generator=gen).to(F64))
    for s in range(len(c.ms)):
        for q, (H, W) in enumerate(ps.shapes[s]):
            ps.plane_view(s, q, buf)[H // 2, W // 2, :] = 1.0  # the planted texel: odd sizes, so p = 0 is its centre
    if c.view == "frozen":
        for s in range(len(c.ms)):
            for q, comb in enumerate(ps.combs):
                if 3 in comb:
                    ps.plane_view(s, q, buf).fill_(POISON)
    return buf


def _grid_choices(c):
    if c.kind == "weights":
        sp = torch.tensor([-1.25] + [-1.0 + k / 8.0 for k in range(17)] + [1.25], dtype=F64)
        return sp, sp
    return torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=F64), torch.tensor([-1.0, 0.0, 1.0], dtype=F64)


def _points(c, N, n_coords, gen, plant=True):
    sp, tm = _grid_choices(c)
    pts = sp[torch.randint(0, len(sp), (N, n_coords), generator=gen)]
    if n_coords == 4:
        pts[:, 3] = tm[torch.randint(0, len(tm), (N,), generator=gen)]
    if plant:
        pts[::PLANT_EVERY] = 0.0
    return pts.contiguous()


def _rays(c, n_coords, gen):
    """Dyadic rays whose sample coordinates fall on the kind's grid: p moves by whole steps of g (1/8 or 1/2) per unit of e[s] + e[s+1]."""
    Rn, S, A = c.R, c.S, float(c.A)
    g = 0.125 if c.kind == "weights" else 0.5
    G = g * A if c.rescale else 2.0 * g * A               # the grain of pos that is a step g of p
    half = int(round(1.25 * A / G))
    o = G * torch.randint(-half, half + 1, (Rn, 3), generator=gen).to(F64)
    d = 2.0 * G * torch.randint(-1, 2, (Rn, 3), generator=gen).to(F64)
    inc = (torch.rand(Rn, S + 1, generator=gen) < min(1.0, 3.0 / S)).to(F64)
    eb = torch.cumsum(inc, dim=1)                         # integer edges, many bins of width 0, sums e[s] + e[s+1] odd and even
    sp, tm = _grid_choices(c)
    tm = tm[tm >= -1.0]                                   # frame times are not negative (snerf_ray_time_order compares their bits)
    t = (tm[torch.randint(0, len(tm), (Rn,), generator=gen)] + 1) / 2
    home = 0.0 if c.rescale else -A                       # the position whose coordinate is p = 0
    if c.same:  # blocks of three rays on one point: runs meet ray boundaries both ways
        d.zero_()
        o = o[torch.arange(Rn) // 3 * 3]
        t = t[torch.arange(Rn) // 3 * 3]
    planted = torch.arange(Rn) % PLANT_EVERY == 0
    if c.same:
        planted |= torch.arange(Rn) % PLANT_EVERY == 1
    o[planted], d[planted], t[planted] = home, 0.0, 0.5
    t[1::2] = t[0::2][:Rn // 2]                           # frame times tie in pairs (snerf_ray_time_order keeps tied rays in ray order)
    return {"mode": 1, "o": o, "d": d, "eb": eb, "t": t if n_coords == 4 else None, "rescale": int(c.rescale), "aabb": [[-A] * 3, [A] * 3]}


def _balanced(act, D, nnz, gen):
    """[H, D] head layer: per column `nnz` units of +-1, at least two and an even number of them active on the planted input `act` (equal
    magnitudes there) with alternating signs of their contribution, so the column's raw output is exactly 0 on the planted rows; the rest from the
    units that are 0 there, where there are any."""
    H = act.numel()
    mags = act.abs()
    nzv = mags[mags > 0]
    if nzv.numel() < 2:
        raise AssertionError("fewer than two units are active on the planted input")
    m = nzv.mode().values
    on, off = (mags == m).nonzero()[:, 0], (mags == 0).nonzero()[:, 0]
    W = torch.zeros(H, D, dtype=F64)
    for j in range(D):
        k = min(nnz if off.numel() == 0 else nnz // 2, on.numel()) // 2 * 2
        pick = on[(torch.arange(k) * max(on.numel() // k, 1) + 5 * j) % on.numel()]
        if pick.unique().numel() != k:
            pick = on[torch.randperm(on.numel(), generator=gen)[:k]]
        W[pick, j] = torch.tensor([1.0, -1.0] * (k // 2), dtype=F64) * torch.sign(act[pick])
        rest = min(nnz - k, off.numel())
        if rest:
            W[off[torch.randperm(off.numel(), generator=gen)[:rest]], j] = R._signs((rest,), gen)
    return W


def _pair_layer(K, M, gen, mul=3):
    """[K, M]: +1 and -1 per column, on rows (mul u) and (mul u + K / 2) mod K: a difference of two ReLU outputs."""
    W = torch.zeros(K, M, dtype=F64)
    u = torch.arange(M)
    s = R._signs((M,), gen)
    W[(mul * u) % K, u] = s
    W[(mul * u + K // 2) % K, u] = -s
    return W


def _scale_column(W, col, z, limit):
    zmax = float(z.abs().max())
    if zmax > limit:
        W[:, col] *= 2.0 ** -math.ceil(math.log2(zmax / limit))


def _proposal_net(c, feat, gen):
    nnz = 2 if c.kind == "weights" else 1
    W0 = R._circulant(8, 64, nnz, gen)
    hid = torch.ones(1, 8, dtype=F64) @ W0
    Wo = _balanced((torch.relu(hid) if c.relu else hid)[0], 1, 16, gen)
    _scale_column(Wo, 0, R.restate(feat, [W0, Wo], c.relu, 0, c.operands)["z"], 16.0)
    return [W0, Wo]


def _field_nets(c, feat, gen):
    K0 = feat.shape[1]
    two = c.kind == "weights"
    W0 = R._circulant(K0, 128, 2 if two else 1, gen, mul=7)
    hid = torch.relu(torch.ones(1, K0, dtype=F64) @ W0)
    W1 = torch.zeros(128, 16, dtype=F64)
    W1[:, :15] = _pair_layer(128, 15, gen, mul=7) if two else R._circulant(128, 15, 1, gen, mul=7)
    W1[:, 15:] = _balanced(hid[0], 1, 16, gen)
    h = R.restate(feat, [W0, W1], 1, 0, c.operands)["z"]
    _scale_column(W1, 15, h[:, 15], 16.0)
    C0 = R._circulant(15, 64, 1, gen, mul=7)
    C1 = _pair_layer(64, 64, gen) if two else R._circulant(64, 64, 1, gen)
    h1 = (hid @ W1)[:, :15]
    a1 = torch.relu(torch.relu(h1 @ C0) @ C1)
    C2 = _balanced(a1[0], 3, 4, gen)
    z = R.restate(h[:, :15], [C0, C1, C2], 1, 0, c.operands)["z"]
    for col in range(3):
        _scale_column(C2, col, z[:, col], 4.0)
    return [W0, W1], [C0, C1, C2]


def _dyadic(t, what, cid, bits=8, limit=64.0):
    t = t[~torch.isnan(t)]
    if not bool(((t * 2.0 ** bits) == torch.floor(t * 2.0 ** bits)).all()) or float(t.abs().max()) > limit:
        raise AssertionError(f"{cid}: {what} is not a multiple of 2^-{bits} within +-{limit}")


def _fixed_points(t, what, cid):
    if not (torch.equal(t.float().double(), t) and torch.equal(R.rd(t, 1), t) and torch.equal(R.rd(t, 2), t)):
        raise AssertionError(f"{cid}: {what} is not exact in float32 and a fixed point of the bf16 and fp16 operand roundings")


def _seed(c):
    return zlib.crc32(case_id(content_key(c)).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def _make(c):
    cid = case_id(c)
    gen = torch.Generator().manual_seed(_seed(c))
    ps = _plane_set(c)
    n_coords = 3 if c.view in ("3", "frozen") else 4
    planes = _planes(c, ps, gen)
    co = {"mode": 0, "pts": _points(c, c.N, n_coords, gen)} if c.mode == 0 else _rays(c, n_coords, gen)
    N = c.N if c.mode == 0 else c.R * c.S
    p = coordinates(co, n_coords)
    m = {"ps": ps, "planes": planes, "co": co, "N": N, "n_coords": n_coords, "p": p}
    # (a)
    _dyadic(p, "a coordinate", cid)
    for s, reso in enumerate(ps.resolutions):
        for k in range(n_coords):
            _, _, w0, w1 = axis_taps(p[:, k], reso[k])
            _dyadic(torch.cat([w0, w1, ((p[:, k] + 1) / 2 * (reso[k] - 1))]), "a pixel position or tap weight", cid, limit=256.0)
    feat, parts = gather(ps, planes, p, c.view)
    # (b)
    for vals in parts:
        for q, v, _ in vals:
            _fixed_points(v, f"a value of plane {q}", cid)
    if c.kernel != "gather" or c.concat:
        _fixed_points(feat, "a feature", cid)
    elif not torch.equal(feat.float().double(), feat):
        raise AssertionError(f"{cid}: a summed feature is not exact in float32")
    if bool(torch.isnan(feat).any()):
        raise AssertionError(f"{cid}: the poison reached a feature")
    m["feat"] = feat
    planted = (p == 0).all(1)
    if c.kernel != "gather" and not bool((feat[planted] == 1.0).all()):
        raise AssertionError(f"{cid}: a planted row's features are not all 1")
    m["planted"] = planted
    if int(planted.sum()) * 8 < N:
        raise AssertionError(f"{cid}: {int(planted.sum())} of {N} rows are planted, fewer than one eighth")
    if c.kernel == "gather":
        return m
    ygen = torch.Generator().manual_seed(_seed(c) + 1)
    if c.kernel in ("dfwd", "dbwd"):
        Ws = _proposal_net(c, feat, gen)
        trace = []
        T = torch.tensor(R.TARGETS, dtype=F64)[torch.randint(0, 3, (N,), generator=gen)]
        z = proposal(feat, Ws, c.relu, c.operands)["z"][:, 0]
        gdens = (T / torch.exp(z.clamp(-15.0, 15.0))).float()
        ref = proposal(feat, Ws, c.relu, c.operands, gdens, trace=trace)
        R.check_trace(trace, cid)
        if not torch.equal(ref["g_out"][:, 0], T):  # (f)
            raise AssertionError(f"{cid}: the rounded gradient tile is not the dyadic target")
        if bool(ref["z"][planted].any()):
            raise AssertionError(f"{cid}: a planted row's raw density output is not 0")
        gp = plane_grads(ps, planes, p, c.view, ref["gX"])
        ab, u = plane_grads(ps, planes, p, c.view, ref["gX"], absolute=True)
        if not float(ab[~torch.isnan(ab)].max()) / u < 2.0 ** 24:  # (e), per texel over all samples
            raise AssertionError(f"{cid}: a texel's gradient sums {float(ab.max()) / u:.3g} units")
        for name, t in (("gX", ref["gX"]), ("gW", ref["gW"]), ("plane gradient", gp[~torch.isnan(gp)])):
            if not torch.equal(t.float().double(), t):
                raise AssertionError(f"{cid}: {name} is not a float32 value")
        m.update(Ws=Ws, W=torch.cat([w.reshape(-1) for w in Ws]), gdens=gdens, T=T, ref=ref, gp=gp, trace=trace)
        m["yard"] = lambda dtype: proposal(torch.cat([feat, _yard_feat(c, m, ygen)]), Ws, c.relu, c.operands, dtype=dtype)["aux"]
        return m
    Wsig, Wcol = _field_nets(c, feat, gen)
    trace = []
    ref = field(feat, Wsig, Wcol, c.operands, trace=trace)
    R.check_trace(trace, cid)
    if bool(ref["h"][planted, 15].any()) or bool(ref["z_rgb"][planted].any()):
        raise AssertionError(f"{cid}: a planted row's raw head outputs are not 0")
    if not torch.equal(ref["h"].float().double(), ref["h"]):
        raise AssertionError(f"{cid}: h is not a float32 value")
    m.update(Wsig=Wsig, Wcol=Wcol, Wsig_flat=torch.cat([w.reshape(-1) for w in Wsig]), Wcol_flat=torch.cat([w.reshape(-1) for w in Wcol]), ref=ref, trace=trace)
    m["yard"] = lambda dtype: field(torch.cat([feat, _yard_feat(c, m, ygen)]), Wsig, Wcol, c.operands, dtype=dtype)
    return m


def _yard_feat(c, m, gen):
    """1024 further feature rows for the float32 yardstick of the bounded head outputs: every channel drawn on its own from the values the case's
    kind can produce (multiples of 1/32 up to 2; powers of two from 2^-6 to 2^6, or 0).  A case's own rows reach few distinct raw head outputs (a
    handful in the "weights" kind, one where N = 1), and the worst float32 deviation over a handful of draws is whatever those draws give
    (mlp_reference.mlp_forward_cases): the yardstick is taken over the case's rows AND these, through the case's own nets and operand type."""
    gen.manual_seed(_seed(c) + 1)
    K = m["feat"].shape[1]
    if c.kind == "weights":
        return torch.randint(0, 65, (1024, K), generator=gen).to(F64) / 32.0
    f = 2.0 ** torch.randint(-6, 7, (1024, K), generator=gen).to(F64)
    f[torch.rand(1024, K, generator=gen) < 0.03] = 0.0
    return f


def make(c):
    """Inputs (float64; what the kernels receive after .float()) and the float64 answer of a case.  Raises where a condition (a) - (f) fails."""
    return _make(content_key(c))


def _density_deviation(a, b):
    ok = (b.log().abs() <= 32.0)  # a yardstick row may leave the range the case's own rows were scaled into: float32's exp stays finite here
    return R.deviation(a[ok], b[ok])


def deviations(c):
    """{output: worst elementwise relative deviation of the float32 restatement from the float64 one} of the bounded head outputs."""
    m = make(c)
    a, b = m["yard"](torch.float32), m["yard"](F64)
    if c.kernel == "field":
        return {"density": _density_deviation(a["density"], b["density"]), "rgb": R.deviation(a["rgb"], b["rgb"])}
    return {"density": _density_deviation(a, b)}


def needs_bound(c):
    return c.kernel in ("dfwd", "field")


# ------------------------------------------------------------------------------------------------ the lattice
def _case(kernel, kind, view, k, *, N=0, R_=0, S=0, rescale=1, same=0, ms=(1,), C=8, concat=0, operands=1, relu=1, keep=0, order=0, nogx=0, ws0=0.0, gp0=0.0):
    return Case(kernel, kind, view, 0 if N else 1, N, R_, S, rescale, (1, 2)[(k // 2) % 2], tuple(ms), C, concat, operands, relu, k, same, keep, order, nogx, ws0, gp0)


def _shapes():
    """The row shapes every kernel meets: the point counts, the ray shapes under both `rescale` values, and the same-texel rays."""
    out = [dict(N=n) for n in POINT_N]
    out += [dict(R_=r, S=s, rescale=rs) for r, s in RAY_SHAPES for rs in (1, 0)]
    out.append(dict(R_=12, S=5, rescale=1, same=1))
    return out


# Pruning rule: the product of the axes (24 row shapes x 2 kinds x 3 views x 2 operand types x 2 aabb x scale sets x options) is tens of thousands
# of cases.  Every kernel meets EVERY row shape once; along the row shapes the other axes rotate with the running index k at strides chosen so
# that, per kernel, every value of every axis occurs and every (view, kind), (view, operands) and (kind, aabb) pair occurs: kind = k % 2,
# aabb = (k // 2) % 2, view = (k // 2) % 3, operands = (k // 6) % 2 + 1 (the gather's C = 8 summed / 32 concatenated likewise), `special` = k
# (which walks the special plane through the space and time planes of every scale), and the kernel's own options at strides 3, 4 and 5.  The
# ordered field forward needs whole 32-sample tiles and four coordinates: the ray shapes with S % 32 == 0 take view "4" and run both entry points.
# tests/test_fused_reference_cpu.py checks the coverage claims.
def gather_cases():
    return [_case("gather", ("values", "weights")[k % 2], VIEWS[(k // 2) % 3], k, **sh, ms=(1, 2), C=(8, 32)[(k // 6) % 2], concat=(k // 6) % 2)
            for k, sh in enumerate(_shapes())]


def density_fwd_cases():
    return [_case("dfwd", ("values", "weights")[k % 2], VIEWS[(k // 2) % 3], k, **sh, ms=((1,), (2,))[(k // 4) % 2], operands=(k // 6) % 2 + 1, relu=int(k % 5 != 2))
            for k, sh in enumerate(_shapes())]


def density_bwd_cases():
    """One level per launch (the only view the kernel takes is "4": `SUPPORT`)."""
    return [_case("dbwd", ("values", "weights")[k % 2], "4", k, **sh, ms=((1,), (2,))[(k // 4) % 2], operands=(k // 6) % 2 + 1, relu=int(k % 5 != 2),
                  nogx=int(k % 3 == 1), ws0=0.25 * (k % 4 == 2), gp0=0.5 * (k % 5 == 3)) for k, sh in enumerate(_shapes())]


def density_bwd_pairs():
    """Both levels in one launch and in swapped order: they differ in resolution, N and coordinate mode (and kind); operands alike, as the ABI asks."""
    out = []
    for op in (1, 2):
        a = _case("dbwd", "weights", "4", 3 + op, N=1000, ms=(1,), operands=op, relu=1, gp0=0.5 * (op == 2))
        b = _case("dbwd", "values", "4", 6 + op, R_=37, S=50, rescale=0, ms=(2,), operands=op, relu=int(op == 1), nogx=int(op == 2), ws0=0.25 * (op == 1))
        d = _case("dbwd", "weights", "4", 8 + op, R_=12, S=5, rescale=1, same=1, ms=(2,), operands=op, relu=1)
        e = _case("dbwd", "values", "4", 10 + op, N=129, ms=(1,), operands=op, relu=1)
        out += [(a, b), (b, a), (d, e), (e, d)]
    return out


def field_cases():
    out = []
    for k, sh in enumerate(_shapes()):
        whole = sh.get("S", 0) % 32 == 0 and "S" in sh
        out.append(_case("field", ("values", "weights")[k % 2], "4" if whole else VIEWS[(k // 2) % 3], k, **sh, ms=FIELD_MS[k % 5], C=32, concat=1,
                         operands=(k // 6) % 2 + 1, keep=(k // 2) % 3, order=int(whole)))
    out.append(_case("field", "weights", "4", 31, R_=5, S=96, rescale=1, ms=FIELD_MS[4], C=32, concat=1, operands=2, keep=2, order=1))
    out.append(_case("field", "values", "4", 34, R_=37, S=32, rescale=0, ms=FIELD_MS[1], C=32, concat=1, operands=1, keep=1, order=1))
    out.append(_case("field", "values", "frozen", 32, N=257, ms=FIELD_MS[3], C=32, concat=1, operands=2, keep=2))
    out.append(_case("field", "weights", "3", 33, N=257, ms=FIELD_MS[4], C=32, concat=1, operands=1, keep=1))
    return out


def all_cases():
    """Every case once (a level of the two-level launches appears in two of them)."""
    return list(dict.fromkeys(gather_cases() + density_fwd_cases() + density_bwd_cases() + [c for pr in density_bwd_pairs() for c in pr] + field_cases()))


# What the `_supported` entry points answer per (kernel, view); snerf_kplanes_gather_fwd has none and takes every view.  tests/test_gpu_fused_lattice.py
# asserts each answer, runs the accepted pairs and asserts the refusal of the others.
SUPPORT = {("gather", "4"): 1, ("gather", "3"): 1, ("gather", "frozen"): 1, ("dfwd", "4"): 1, ("dfwd", "3"): 1, ("dfwd", "frozen"): 1,
           ("dbwd", "4"): 1, ("dbwd", "3"): 0, ("dbwd", "frozen"): 0, ("field", "4"): 1, ("field", "3"): 1, ("field", "frozen"): 1,
           ("field_ordered", "4"): 1, ("field_ordered", "3"): 0, ("field_ordered", "frozen"): 0}

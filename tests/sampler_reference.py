"""References and seeded input families for the ray samplers of csrc/ray_ops.hip (spaced_bins_kernel, resample_kernel behind
snerf_pdf_resample and snerf_weights_fwd, weights_bwd_kernel).  A plain helper module (like tests/per_ray_reference.py): numpy only, independent
of oracle/ and of the package; no fixtures, no collection hooks.

Every function takes the working type `ft`.  With ft = float32 it is a RESTATEMENT: each operation between the inputs and the result is one
correctly rounded IEEE float32 operation, in the order the reference program writes them (NS/model_components/ray_samplers.py:79-126, 238-246
SpacedSampler; :302-351 PDFSampler with include_original=False; :584 the annealing power; NS/cameras/rays.py:127-149 get_weights), with

  * torch.linspace as ATen's symmetric halves: step = (end - start) / (steps - 1); start + step * i below steps / 2, end - step * (steps - i - 1)
    from there on;
  * cumsum as ATen's CPU kernel forms it for float32: a float64 running sum, rounded to float32 per element;
  * the sum of the padded weights as cumsum(w)[-1] (the project's documented deviation from torch.sum's association order);
  * searchsorted(cdf, u, side="right") written as the count of cdf entries <= u, so the tie rule is borrowed from nowhere;
  * u built as the kernel documents it: linspace(0, 1 - 1 / nb, nb) with the end formed in the working type, + rand / nb or + 1 / (2 nb).

Where anneal == 1 and the weights are given nothing else happens between the inputs and `inds` / `sbins`, so a kernel that does the same is EQUAL
to the restatement on every element -- provided the float32 cumsum does not depend on the order of summation, which `prefix_sums_off_midpoints`
asserts per case as a property of the inputs.  powf (annealing) and expf (get_weights) are the host libm's here: those routes are bounded, not
pinned.  With ft = float64 the same functions are the plain float64 reference (cumsum is then a plain float64 cumsum).
"""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = float(np.finfo(np.float32).max)

# ---------------------------------------------------------------------------------------------------------------------------------------
# the lattice (tests/test_gpu_sampler_lattice.py runs it on the GPU; tests/test_sampler_reference_cpu.py measures E32 over it)
# ---------------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320)  # Sp and S: both sides of every multiple of 64, the limit
RAY_COUNTS = (1, 2, 3, 4, 5, 133)
PRODUCTION_PAIRS = ((256, 128), (128, 64))            # (Sp, S)
FIXTURE_PAIRS = ((256, 128), (128, 64), (96, 48), (13, 7))
POW2_S = (1, 3, 7, 63, 127, 255)                      # S + 1 a power of two: family X with u formed in the kernel
SMALL, LARGE = (1, 2, 3), (255, 256, 257, 319, 320)


def resample_pairs():
    """(Sp, S, R) of the PDF stage.  Pruning rule: the full 17 x 17 grid is cut to, per count c at position k of COUNTS, the partners
    {1, 3, 320, c itself, the next count, the count seven places on (cyclically)}: every Sp and every S thereby meets a small partner (1, 3), a large
    one (320), its own size and two sizes on other sides of other multiples of 64 -- as Sp with those S, and (the rule is applied to both
    orders) as S with those Sp.  The production and the fixtures' pairs are added.  R is dealt round-robin from RAY_COUNTS, so every R meets
    every residue of the pair list."""
    n = len(COUNTS)
    pairs = []
    for k, c in enumerate(COUNTS):
        for p in (1, 3, 320, c, COUNTS[(k + 1) % n], COUNTS[(k + 7) % n]):
            for pair in ((c, p), (p, c)):
                if pair not in pairs:
                    pairs.append(pair)
    for pair in PRODUCTION_PAIRS + FIXTURE_PAIRS:
        if pair not in pairs:
            pairs.append(pair)
    return [(sp, s, RAY_COUNTS[k % len(RAY_COUNTS)]) for k, (sp, s) in enumerate(pairs)]


def spaced_cases():
    """(S, R) of spaced_bins: every count with two ray counts, plus R * (S + 1) a multiple of the 256-thread workgroup (S = 63, R = 4 and
    S = 255, R = 5) and one short of / past it (S = 64, R = 4: 260; S = 2, R = 85: 255)."""
    out = [(s, RAY_COUNTS[k % 6]) for k, s in enumerate(COUNTS)] + [(s, RAY_COUNTS[(k + 3) % 6]) for k, s in enumerate(COUNTS)]
    out += [(63, 4), (255, 5), (64, 4), (2, 85), (7, 133), (48, 5)]
    return sorted(set(out))


WEIGHT_CASES = tuple((s, RAY_COUNTS[(k + 2) % 6]) for k, s in enumerate(COUNTS)) + ((64, 133), (320, 133), (37, 5))  # (S, R): the weights entry points


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(ord(ch) for ch in k) if isinstance(k, str) else int(k))) % (2**31 - 1)
    return np.random.default_rng(seed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) SpacedSampler, (b) PDFSampler, get_weights and its gradient -- in the working type ft
# ---------------------------------------------------------------------------------------------------------------------------------------
def linspace(start, end, steps, ft=f32):
    """ATen's linspace (RangeFactories: symmetric halves keep both ends exact), one rounding per operation."""
    start, end = ft(start), ft(end)
    if steps == 1:
        return np.array([start], dtype=ft)
    with np.errstate(all="ignore"):
        step = ft((end - start) / ft(steps - 1))
        i = np.arange(steps)
        lo = start + step * i.astype(ft)
        hi = end - step * (steps - i - 1).astype(ft)
    return np.where(i < steps // 2, lo, hi).astype(ft)


def cumsum(x, ft=f32):
    """Along the last axis: a float64 running sum rounded to ft per element."""
    return np.cumsum(np.asarray(x, dtype=f64), axis=-1).astype(ft)


def spacing_fn(x, kind, ft=f32):
    x = np.asarray(x, dtype=ft)
    if kind == "uniform":
        return x
    with np.errstate(all="ignore"):
        return np.where(x < ft(1), x / ft(2), ft(1) - ft(1) / (ft(2) * x)).astype(ft)  # :242


def spacing_fn_inv(x, kind, ft=f32):
    x = np.asarray(x, dtype=ft)
    if kind == "uniform":
        return x
    with np.errstate(all="ignore"):
        return np.where(x < ft(0.5), ft(2) * x, ft(1) / (ft(2) - ft(2) * x)).astype(ft)  # :243


def to_euclidean(bins, nears, fars, kind="uniform", ft=f32):
    """:114-116: fn_inv(x * fn(far) + (1 - x) * fn(near)); nears, fars [R]."""
    x = np.asarray(bins, dtype=ft)
    sn = spacing_fn(np.asarray(nears, dtype=ft).reshape(-1, 1), kind, ft)
    sf = spacing_fn(np.asarray(fars, dtype=ft).reshape(-1, 1), kind, ft)
    return spacing_fn_inv(x * sf + (ft(1) - x) * sn, kind, ft)


def spaced_bins(R, S, t_rand=None, ft=f32):
    """:101-112.  t_rand None (eval), [R, 1] (single jitter) or [R, S + 1]."""
    b = linspace(0, 1, S + 1, ft)[None, :]
    if t_rand is None:
        return np.broadcast_to(b, (R, S + 1)).copy()
    t = np.asarray(t_rand, dtype=ft)
    centers = (b[:, 1:] + b[:, :-1]) / ft(2)
    upper = np.concatenate([centers, b[:, -1:]], -1)
    lower = np.concatenate([b[:, :1], centers], -1)
    return (lower + (upper - lower) * t).astype(ft)


def pdf_u(R, S, rand=None, ft=f32):
    """:316-327 as the kernel documents it.  rand None (eval: bin centres), [R, 1] or [R, S + 1]."""
    nb = S + 1
    u = linspace(0, ft(1) - ft(1) / ft(nb), nb, ft)[None, :]
    if rand is None:
        return np.broadcast_to(u + ft(1) / ft(2 * nb), (R, nb)).astype(ft).copy()
    return (u + np.asarray(rand, dtype=ft) / ft(nb)).astype(ft)


def count_le(edges, q):
    """searchsorted(edges, q, side="right") on sorted rows: the number of edges <= q.  edges [R, E], q [R, Q] -> int64 [R, Q]."""
    out = np.empty(q.shape, dtype=np.int64)
    for r0 in range(0, q.shape[0], 16):  # blocks of rays: the [16, Q, E] comparison stays small
        out[r0:r0 + 16] = (edges[r0:r0 + 16, None, :] <= q[r0:r0 + 16, :, None]).sum(-1)
    return out


def pdf_cdf(weights, anneal=1.0, histogram_padding=0.01, eps=1e-5, ft=f32):
    """:584, :302-312 -> cdf [R, Sp + 1]."""
    w = np.asarray(weights, dtype=ft)
    Sp = w.shape[-1]
    with np.errstate(all="ignore"):
        if anneal != 1.0:
            w = np.power(w, ft(anneal)).astype(ft)
        w = w + ft(histogram_padding)
        s = cumsum(w, ft)[:, -1:]
        padding = np.maximum(ft(eps) - s, ft(0))
        w = w + padding / ft(Sp)
        pdf = (w / (s + padding)).astype(ft)
        cdf = np.minimum(ft(1), cumsum(pdf, ft))
    return np.concatenate([np.zeros_like(cdf[:, :1]), cdf], -1).astype(ft)


def pdf_sample(weights, sbins_prev, u, nears=None, fars=None, kind="uniform", anneal=1.0, histogram_padding=0.01, eps=1e-5, ft=f32):
    """:302-351.  Returns {"cdf", "inds", "sbins", "ebins" (None without nears / fars)}."""
    cdf = pdf_cdf(weights, anneal, histogram_padding, eps, ft)
    u = np.ascontiguousarray(u, dtype=ft)
    bins = np.asarray(sbins_prev, dtype=ft)
    Sp = bins.shape[-1] - 1
    inds = count_le(cdf, u)
    below, above = np.clip(inds - 1, 0, Sp), np.clip(inds, 0, Sp)
    take = lambda a, i: np.take_along_axis(a, i, -1)
    c0, c1, b0, b1 = take(cdf, below), take(cdf, above), take(bins, below), take(bins, above)
    with np.errstate(all="ignore"):
        t = ((u - c0) / (c1 - c0)).astype(ft)
        t = np.where(np.isnan(t), ft(0), np.clip(t, ft(-FLT_MAX) if ft is f32 else -np.inf, ft(FLT_MAX)))  # nan_to_num: +-inf -> +-FLT_MAX
        t = np.clip(t, ft(0), ft(1)).astype(ft)
        sb = (b0 + t * (b1 - b0)).astype(ft)
    eb = None if nears is None else to_euclidean(sb, nears, fars, kind, ft)
    return {"cdf": cdf, "inds": inds, "sbins": sb, "ebins": eb}


def get_weights(density, ebins, ft=f32):
    """rays.py:127-149: w = (1 - exp(-delta sigma)) exp(-exclusive cumsum(delta sigma)), nan_to_num."""
    e, d = np.asarray(ebins, dtype=ft), np.asarray(density, dtype=ft)
    with np.errstate(all="ignore"):
        dd = ((e[:, 1:] - e[:, :-1]) * d).astype(ft)
        excl = np.concatenate([np.zeros_like(dd[:, :1]), cumsum(dd[:, :-1], ft)], -1)
        w = ((ft(1) - np.exp(-dd)) * np.exp(-excl)).astype(ft)
    return np.nan_to_num(w, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(ft)


def get_weights_grad(density, ebins, grad_weights, ft=f32):
    """d/d sigma_k of sum_i g_i w_i on finite inputs: delta_k (g_k T_k exp(-dd_k) - sum_{i > k} g_i w_i).  (tests/per_ray_reference.py has
    get_weights and this gradient only inside ray_train_ref, through autograd; tests/test_sampler_reference_cpu.py holds both float64 versions
    to that autograd formula.)"""
    e, d, g = (np.asarray(a, dtype=ft) for a in (ebins, density, grad_weights))
    delta = e[:, 1:] - e[:, :-1]
    dd = (delta * d).astype(ft)
    excl = np.concatenate([np.zeros_like(dd[:, :1]), cumsum(dd[:, :-1], ft)], -1)
    T, ek = np.exp(-excl).astype(ft), np.exp(-dd).astype(ft)
    gw = (g * ((ft(1) - ek) * T)).astype(ft)
    incl = cumsum(gw[:, ::-1], ft)[:, ::-1]
    suffix = np.concatenate([incl[:, 1:], np.zeros_like(incl[:, :1])], -1)
    return (delta * (g * T * ek - suffix)).astype(ft)


def deviation(got, want):
    """max |got - want| over the largest |want| of the case (tests/per_ray_reference.py: deviation)."""
    got, want = np.asarray(got, dtype=f64), np.asarray(want, dtype=f64)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    return diff / scale if scale > 0 else diff


# ---------------------------------------------------------------------------------------------------------------------------------------
# criteria of the inexact routes (family A), every element
# ---------------------------------------------------------------------------------------------------------------------------------------
def index_within(inds, cdf64, u, tau):
    """Elementwise: cdf64[ind - 1] - tau <= u < cdf64[ind] + tau, the ends as searchsorted has them (ind = 0: nothing below; ind = Sp + 1:
    nothing above)."""
    R = cdf64.shape[0]
    low = np.concatenate([np.full((R, 1), -np.inf), cdf64], -1)   # low[ind] = cdf64[ind - 1]
    high = np.concatenate([cdf64, np.full((R, 1), np.inf)], -1)   # high[ind] = cdf64[ind]
    u = np.asarray(u, dtype=f64)
    inds = np.asarray(inds)
    ok_range = (inds >= 0) & (inds <= cdf64.shape[1])
    i = np.clip(inds, 0, cdf64.shape[1])
    return ok_range & (np.take_along_axis(low, i, -1) - tau <= u) & (u < np.take_along_axis(high, i, -1) + tau)


def bins_inside(inds, sbins, sbins_prev):
    """Elementwise: bins_prev[ind - 1] <= sbins <= bins_prev[ind] for the given indices (clamped as the sampler clamps them)."""
    b = np.asarray(sbins_prev, dtype=f64)
    Sp = b.shape[1] - 1
    lo = np.take_along_axis(b, np.clip(np.asarray(inds) - 1, 0, Sp), -1)
    hi = np.take_along_axis(b, np.clip(np.asarray(inds), 0, Sp), -1)
    s = np.asarray(sbins, dtype=f64)
    return (lo <= s) & (s <= hi)


def u_back(sbins, sbins_prev, cdf64):
    """The float64 piecewise-linear cdf evaluated at sbins (the well-conditioned direction: it must give u back)."""
    b, s = np.asarray(sbins_prev, dtype=f64), np.asarray(sbins, dtype=f64)
    Sp = b.shape[1] - 1
    j = np.clip(count_le(b, s) - 1, 0, Sp - 1)
    take = lambda a, i: np.take_along_axis(a, i, -1)
    b0, b1, c0, c1 = take(b, j), take(b, j + 1), take(cdf64, j), take(cdf64, j + 1)
    return c0 + (s - b0) / (b1 - b0) * (c1 - c0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d) input families.  A case: R, Sp, S, weights [R, Sp] (or density + ebins_prev), sbins_prev [R, Sp + 1], nears, fars [R],
# histogram_padding, eps, anneal, and ONE of u [R, S + 1] (u_mode 0) / rand [R, S + 1] or [R, 1] (u_mode 1) / neither (u_mode 2).
# ---------------------------------------------------------------------------------------------------------------------------------------
def case_u(case, ft=f32):
    """The u of a case in the working type."""
    if case.get("u") is not None:
        return np.asarray(case["u"], dtype=ft)
    return pdf_u(case["R"], case["S"], case.get("rand"), ft)


def case_weights(case, ft=f32):
    if case.get("density") is not None:
        return get_weights(case["density"], case["ebins_prev"], ft)
    return np.asarray(case["weights"], dtype=ft)


def reference(case, kind="uniform", ft=f32):
    return pdf_sample(case_weights(case, ft), case["sbins_prev"], case_u(case, ft), case["nears"], case["fars"], kind, case["anneal"],
                      case["histogram_padding"], case["eps"], ft)


def _dyadic_near_far(R, rng):
    near = rng.integers(0, 5, R) / 8.0             # 0 .. 0.5 in eighths
    far = near + rng.integers(8, 33, R) / 4.0      # + 2 .. 8 in quarters
    return near.astype(f32), far.astype(f32)


def _exact_weights(R, Sp, p, rng):
    """Integer weights k in units of 2^-10 so that k + p is a power of two per element and sum(k + p) is a power of two per row.
    p = 0: k in {0, 1, 2, 4} (zero weights are zero-width pdf bins), sum = the largest power of two <= max(Sp, 1), built from 4s and split
    at random into 2 + 2 and 1 + 1 over zero elements.  p in {1, 2, 4}: k in {0, p}, so k + p in {p, 2 p}, with Sp + #{k = p} a power of two."""
    k = np.zeros((R, Sp), dtype=np.int64)
    for r in range(R):
        if p == 0:
            T = 1 << int(np.floor(np.log2(max(Sp, 1))))
            row = [4] * (T // 4) + ([T % 4] if T % 4 else [])       # T = 1, 2: a single 1 or 2
            room = Sp - len(row)
            while room > 0 and rng.random() < 0.8:
                big = [i for i, v in enumerate(row) if v > 1]
                if not big:
                    break
                i = big[rng.integers(len(big))]
                row[i] //= 2
                row.append(row[i])
                room -= 1
            row += [0] * (Sp - len(row))
            k[r] = rng.permutation(np.array(row))
        else:
            total = 1 << int(np.ceil(np.log2(Sp)))                     # the power of two in [Sp, 2 Sp)
            k[r, rng.permutation(Sp)[: total - Sp]] = p
    return k


def exact_case(R, Sp, S, p=0, u_mode=0, rand_cols=None, seed=0):
    """Family X: every intermediate is the same number in float32 and float64 (assert_exact checks it).  Weights k 2^-10, histogram_padding
    p 2^-10 (_exact_weights); sbins_prev sorted j / 1024 with repeated edges; near, far dyadic.  u_mode 0: per ray u holds 0, 1, 1.25 (above the last cdf
    entry, which the clamp holds at 1), cdf knots, repeated knots (zero-width pdf bins, p = 0), midpoints and eighths of bins, in a per-ray rotation so that
    short rows see all of them across rays.  u_mode 1 / 2 need S + 1 a power of two: rand is q / 64 with exact zeros (u on the strata edges)."""
    rng = _rng("exact", R, Sp, S, p, u_mode, rand_cols or 0, seed)
    k = _exact_weights(R, Sp, p, rng)
    tot = (k + p).sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros((R, 1)), np.cumsum((k + p) / tot, -1)], -1)
    j = np.sort(rng.integers(0, 1025, (R, Sp + 1)), -1)
    rep = rng.random((R, Sp + 1)) < 0.15
    rep[:, 0] = False
    for c in range(1, Sp + 1):  # repeated edges: a copy of the left neighbour keeps the row sorted only if applied left to right and re-sorted
        j[:, c] = np.where(rep[:, c], j[:, c - 1], j[:, c])
    j = np.sort(j, -1)
    near, far = _dyadic_near_far(R, rng)
    case = {"family": "X", "R": R, "Sp": Sp, "S": S, "weights": (k / 1024.0).astype(f32), "sbins_prev": (j / 1024.0).astype(f32), "nears": near, "fars": far,
            "histogram_padding": p / 1024.0, "eps": 1e-5, "anneal": 1.0, "u": None, "rand": None, "u_mode": u_mode, "_cdf": cdf}
    nb = S + 1
    if u_mode == 0:
        u = np.empty((R, nb))
        for r in range(R):
            width = cdf[r, 1:] - cdf[r, :-1]
            full = np.flatnonzero(width > 0)
            empty = np.flatnonzero(width == 0)
            vals = [0.0, 1.0, 1.25]
            n_more = max(nb, 6)
            for m in range(n_more):
                what = m % 4
                i = full[rng.integers(len(full))]
                if what == 0:
                    vals.append(cdf[r, rng.integers(0, Sp + 1)])                     # a knot
                elif what == 1 and len(empty):
                    vals.append(cdf[r, empty[rng.integers(len(empty))]])            # a repeated knot
                elif what == 2:
                    vals.append(cdf[r, i] + width[i] / 2)                            # a midpoint
                else:
                    vals.append(cdf[r, i] + width[i] * rng.integers(1, 8) / 8.0)     # an eighth of a bin
            vals = np.roll(np.array(vals[:nb]), -r) if nb >= 6 else np.roll(np.array(vals), -r)[:nb]  # short rows: all kinds across rays
            u[r] = vals
        case["u"] = u.astype(f32)
        assert np.array_equal(case["u"].astype(f64), u)
    elif u_mode == 1:
        assert nb & (nb - 1) == 0
        q = rng.integers(0, 64, (R, rand_cols)) * (rng.random((R, rand_cols)) < 0.7)
        case["rand"] = (q / 64.0).astype(f32)
    else:
        assert nb & (nb - 1) == 0
    return case


def assert_exact(case):
    """Family X's preconditions, in float64: every partial sum of the padded weights and of the pdf, the pdf, cdf, t and sbins are fixed points of
    float32 rounding, i.e. the float32 restatement and the float64 reference are the same numbers.  Returns (u on a knot, zero-width pdf bins)
    as shares."""
    fixed = lambda a: np.array_equal(np.asarray(a, dtype=f64).astype(f32).astype(f64), np.asarray(a, dtype=f64))
    w = case["weights"].astype(f64) + f64(f32(case["histogram_padding"]))
    assert fixed(f32(case["histogram_padding"])) and float(f32(case["histogram_padding"])) == case["histogram_padding"]
    sums = np.cumsum(w, -1)
    assert fixed(w) and fixed(sums)
    tot = sums[:, -1:]
    assert np.all(np.log2(tot) == np.round(np.log2(tot))) and np.all(tot > case["eps"])  # a power of two: the division is exact; no eps padding
    pdf = w / tot
    assert fixed(pdf) and fixed(np.cumsum(pdf, -1)) and np.all(np.cumsum(pdf, -1)[:, -1] == 1.0)
    r32, r64 = reference(case, "uniform", f32), reference(case, "uniform", f64)
    assert np.array_equal(r64["cdf"], case["_cdf"])
    u64 = case_u(case, f64)
    assert np.array_equal(case_u(case, f32).astype(f64), u64)
    # (with u formed in the kernel sbins needs all 24 bits, so its product with `far` is exact for explicit u only)
    for name in ("cdf", "sbins") + (("ebins",) if case["u_mode"] == 0 else ()):
        assert fixed(r64[name]) and np.array_equal(r32[name].astype(f64), r64[name]), name
    assert np.array_equal(r32["inds"], r64["inds"])
    on_knot = (u64[:, :, None] == r64["cdf"][:, None, :]).any(-1)
    return float(on_knot.mean()), float((pdf == 0).mean())


def midpoint_distance(x):
    """Elementwise relative distance of the float64 array x from the nearest float32 rounding midpoint (exact zeros: inf)."""
    x = np.asarray(x, dtype=f64)
    y = x.astype(f32)
    with np.errstate(all="ignore"):
        up = (y.astype(f64) + np.nextafter(y, f32(np.inf)).astype(f64)) / 2
        dn = (y.astype(f64) + np.nextafter(y, f32(-np.inf)).astype(f64)) / 2
        d = np.minimum(np.abs(x - up), np.abs(x - dn)) / np.abs(x)
    return np.where(x == 0, np.inf, d)


GUARD_REL = 1e-12


def sums_order_independent(terms):
    """Per row of the non-negative float32 terms [R, n]: is the float32 rounding of every float64 prefix sum the same in ANY order of summation?
    Either (1) every subset sum is exact in float64 -- each term is a multiple of the smallest ulp g among the non-zero terms, and
    sum / g < 2^53 -- so every order arrives at the same float64 number (a prefix sum that IS a float32 midpoint, which sums of a few float32
    terms often are, then rounds to even in every order); or (2) no float64 prefix sum lies within 1e-12 relative of a float32 rounding
    midpoint, while re-associating at most 320 non-negative terms moves a float64 sum by under 320 x 2^-53 = 3.6e-14 relative."""
    t = np.asarray(terms, dtype=f32)
    assert np.all(t >= 0)
    with np.errstate(all="ignore"):
        g = np.minimum.accumulate(np.where(t > 0, np.spacing(t), f32(np.inf)).astype(f64), -1)  # per prefix: it sums its own terms only
        sums = np.cumsum(t.astype(f64), -1)
        exact = (sums == 0) | (sums / g < 2.0 ** 53)
    return (exact | (midpoint_distance(sums) > GUARD_REL)).all(-1)


def prefix_sums_off_midpoints(case):
    """The float32 cdf of the case does not depend on the order of summation (sums_order_independent, for the padded weights and for the
    pdf): a property of the inputs alone."""
    w = case_weights(case, f32)
    assert case["anneal"] == 1.0
    w = (w + f32(case["histogram_padding"])).astype(f32)
    s = cumsum(w)[:, -1:]
    padding = np.maximum(f32(case["eps"]) - s, f32(0))
    with np.errstate(all="ignore"):
        pdf = ((w + padding / f32(w.shape[1])) / (s + padding)).astype(f32)
    return bool(np.all(sums_order_independent(w)) and np.all(sums_order_independent(pdf)))


def _densities(R, S, rng, floor=0.0):
    d = rng.random((R, S)) ** 4 * 60 + floor
    if S > 1 and floor == 0.0:
        d = np.where(rng.random((R, S)) < 0.3, 0.0, d)  # exact zeros
    return d.astype(f32)


def pipeline_case(R, Sp, S, u_mode=1, rand_cols=None, seed=0):
    """Family P: spaced_bins with uniform jitter -> euclidean bins -> random densities with 30 % exact zeros -> get_weights -> resample with the
    default histogram_padding and eps and uniform draws.  Re-seeded until prefix_sums_off_midpoints holds (never relaxed)."""
    for attempt in range(64):
        rng = _rng("pipeline", R, Sp, S, u_mode, rand_cols or 0, seed, attempt)
        near = (rng.random(R) * 0.5 + 0.05).astype(f32)
        far = (near + 2.0 + rng.random(R) * 4.0).astype(f32)
        sb = spaced_bins(R, Sp, rng.random((R, Sp + 1)).astype(f32))
        eb = to_euclidean(sb, near, far)
        w = get_weights(_densities(R, Sp, rng), eb)
        case = {"family": "P", "R": R, "Sp": Sp, "S": S, "weights": w, "sbins_prev": sb, "nears": near, "fars": far, "histogram_padding": 0.01, "eps": 1e-5,
                "anneal": 1.0, "u": None, "rand": None, "u_mode": u_mode}
        if u_mode == 0:
            case["u"] = pdf_u(R, S, rng.random((R, S + 1)).astype(f32))
        elif u_mode == 1:
            case["rand"] = rng.random((R, rand_cols)).astype(f32)
        if prefix_sums_off_midpoints(case):
            return case
    raise AssertionError("no case off the rounding midpoints in 64 seeds")


DEGENERATE = ("all_zero", "single", "extremes", "equal_edges", "huge_eps")


def degenerate_case(which, R, Sp, S, seed=0):
    """Family Z.  all_zero: weights 0 with histogram_padding 0 (the eps padding is the whole pdf); single: one non-zero weight per ray
    (histogram_padding 0: every other pdf bin has zero width); extremes: 1e-30 and 1e30 in one row; equal_edges: sbins_prev with every edge equal;
    huge_eps: eps = 1e30 over ordinary weights (the padding branch with non-zero weights)."""
    for attempt in range(64):
        rng = _rng("degenerate", which, R, Sp, S, seed, attempt)
        near = (rng.random(R) * 0.5 + 0.05).astype(f32)
        far = (near + 2.0 + rng.random(R) * 4.0).astype(f32)
        sb = spaced_bins(R, Sp, rng.random((R, Sp + 1)).astype(f32))
        w = (rng.random((R, Sp)) ** 3).astype(f32)
        pad, eps = 0.01, 1e-5
        if which == "all_zero":
            w, pad = np.zeros((R, Sp), dtype=f32), 0.0
        elif which == "single":
            w, pad = np.zeros((R, Sp), dtype=f32), 0.0
            w[np.arange(R), rng.integers(0, Sp, R)] = (rng.random(R) + 0.1).astype(f32)
        elif which == "extremes":
            w[:, rng.integers(0, Sp)] = 1e-30
            if Sp > 1:
                cols = rng.permutation(Sp)[:2]
                w[:, cols[0]], w[:, cols[1]] = 1e-30, 1e30
            if R > 1:
                pad = 0.0 if seed % 2 else 0.01
        elif which == "equal_edges":
            sb = np.repeat(rng.random((R, 1)).astype(f32), Sp + 1, -1)
        elif which == "huge_eps":
            eps = 1e30
        else:
            raise ValueError(which)
        case = {"family": "Z", "which": which, "R": R, "Sp": Sp, "S": S, "weights": w, "sbins_prev": np.ascontiguousarray(sb), "nears": near, "fars": far,
                "histogram_padding": pad, "eps": eps, "anneal": 1.0, "u": None, "rand": rng.random((R, S + 1)).astype(f32), "u_mode": 1}
        if prefix_sums_off_midpoints(case):
            return case
    raise AssertionError("no case off the rounding midpoints in 64 seeds")


def inexact_case(route, R, Sp, S, seed=0):
    """Family A.  route "anneal0.37" / "anneal0.9": given weights under the annealing power; "fused": density + ebins_prev (get_weights in the
    kernel), anneal 1; "fused_anneal": both.  Densities are bounded away from 0 (for delta sigma < ~1e-6 the reference's own 1 - exp(-x) is
    rounding noise, which the power then amplifies in any implementation) and the previous level's bins are jittered by the middle half of a
    stratum only, so that no bin is narrow: the slope of the cdf over sbins, which carries the rounding of sbins into u_back, stays moderate.
    u is sorted (stratified draws)."""
    rng = _rng("inexact", route, R, Sp, S, seed)
    near = (rng.random(R) * 0.5 + 0.05).astype(f32)
    far = (near + 2.0 + rng.random(R) * 2.0).astype(f32)
    sb = spaced_bins(R, Sp, (0.25 + 0.5 * rng.random((R, Sp + 1))).astype(f32))
    eb = to_euclidean(sb, near, far)
    dens = (rng.random((R, Sp)) * 2.0 + 0.5).astype(f32)
    case = {"family": "A", "route": route, "R": R, "Sp": Sp, "S": S, "sbins_prev": sb, "nears": near, "fars": far, "histogram_padding": 0.01, "eps": 1e-5,
            "anneal": {"anneal0.37": 0.37, "anneal0.9": 0.9, "fused": 1.0, "fused_anneal": 0.37}[route], "u": pdf_u(R, S, rng.random((R, S + 1)).astype(f32)),
            "rand": None, "u_mode": 0}
    if route.startswith("fused"):
        case["density"], case["ebins_prev"], case["weights"] = dens, eb, None
    else:
        case["weights"] = get_weights(dens, eb)
    return case


INEXACT_ROUTES = ("anneal0.37", "anneal0.9", "fused", "fused_anneal")
INEXACT_SHAPES = ((1, 1, 1), (3, 2, 2), (64, 63, 3), (65, 64, 5), (128, 64, 133), (129, 65, 4), (256, 128, 133), (257, 320, 5), (320, 319, 3),
                  (319, 1, 2), (192, 193, 1), (13, 7, 5))  # (Sp, S, R)


def weights_case(R, S, seed=0):
    """The weights entry points: densities with exact zeros over jittered bins, and an upstream gradient."""
    rng = _rng("weights", R, S, seed)
    near = (rng.random(R) * 0.5 + 0.05).astype(f32)
    far = (near + 2.0 + rng.random(R) * 4.0).astype(f32)
    eb = to_euclidean(spaced_bins(R, S, rng.random((R, S + 1)).astype(f32)), near, far)
    return {"R": R, "S": S, "density": _densities(R, S, rng), "ebins": np.ascontiguousarray(eb), "grad_weights": (rng.random((R, S)) - 0.3).astype(f32)}


def prefill_like(want, *key):
    """What an accumulating call finds in its gradient buffer: uniform in +-half the largest reference gradient (float32)."""
    scale = float(np.abs(want).max()) or 1.0
    return ((_rng("prefill", *key).random(want.shape) - 0.5) * scale).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# E32: the float32 restatement against the float64 reference, per bounded quantity, maximised over the lattice
# ---------------------------------------------------------------------------------------------------------------------------------------
def inexact_cases():
    return [inexact_case(route, R, Sp, S) for route in INEXACT_ROUTES for Sp, S, R in INEXACT_SHAPES]


def measure_e32():
    """{quantity: (worst deviation, where)} of the float32 restatement from the float64 reference, each in units of the case's largest |want|:
    resample.cdf and resample.u_back (the float64 cdf at the float32 restatement's sbins, against u) over family A, resample.weights_out over its
    fused routes, weights_fwd.weights and weights_bwd.g_density over WEIGHT_CASES."""
    worst = {}

    def note(name, got, want, where):
        d = deviation(got, want)
        if name not in worst or d > worst[name][0]:
            worst[name] = (d, where)

    for case in inexact_cases():
        where = f"{case['route']} Sp={case['Sp']} S={case['S']} R={case['R']}"
        r32, r64 = reference(case, "uniform", f32), reference(case, "uniform", f64)
        note("resample.cdf", r32["cdf"], r64["cdf"], where)
        note("resample.u_back", u_back(r32["sbins"], case["sbins_prev"], r64["cdf"]), case_u(case, f64), where)
        if case.get("density") is not None:
            note("resample.weights_out", case_weights(case, f32), case_weights(case, f64), where)
    for S, R in WEIGHT_CASES:
        c = weights_case(R, S)
        where = f"S={S} R={R}"
        note("weights_fwd.weights", get_weights(c["density"], c["ebins"], f32), get_weights(c["density"], c["ebins"], f64), where)
        note("weights_bwd.g_density", get_weights_grad(c["density"], c["ebins"], c["grad_weights"], f32),
             get_weights_grad(c["density"], c["ebins"], c["grad_weights"], f64), where)
    return worst


MARGIN = 5.0  # the margin of r10 and r16 for expf / powf against the host libm and a wave-order sum against a sequential one
# quantity: E32 (measured by measure_e32, rounded up to two digits; tests/test_sampler_reference_cpu.py holds the table to its measurement and
# to profiles/r30_sampler_reference_e32.json)                    -> bound = MARGIN * E32
E32 = {
    "resample.cdf": 2.0e-07,                                      # tau = 1.0e-06
    "resample.u_back": 2.1e-07,                                   # recorded only: u_back is held to tau
    "resample.weights_out": 3.8e-06,                              # 1.9e-05 (1 - exp(-x) at x ~ 1e-2 over 319 samples)
    "weights_fwd.weights": 2.2e-07,                               # 1.1e-06
    "weights_bwd.g_density": 4.7e-07,                             # 2.35e-06
}
TAU = MARGIN * E32["resample.cdf"]

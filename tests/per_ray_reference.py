"""Float64 references and seeded input families for the per-ray kernels of csrc/render_loss.hip (compositing, distortion, interlevel, both
depth losses, the one-launch ray_train kernel).  A plain helper module (like tests/_measure.py): no fixtures, no collection hooks.

The references are written from the formulas in render_loss.hip's header comments and oracle/kplanes_oracle.py.  Inputs are float32 CPU
tensors (what the kernels read); every reference computes in float64 EXCEPT where the result is an integer decision or rests on a cancellation
that the kernel's own roundings decide:

  * the median index uses torch.cumsum of the float32 weights on the CPU (ATen: a double accumulator rounded per element, which
    wave_scan_f64 reproduces) and then "first index with >= 0.5";
  * the interlevel reference takes cy = [0, cumsum(w_prop)] the same way, forms w_outer = cy[hi + 1] - cy[lo] with ONE float32 rounding, and
    computes everything after that in float64.  Plain float64 is the wrong yardstick there: where w_outer is small the float32 cancellation
    in cy[hi + 1] - cy[lo], amplified by 1 / (w + 1e-7), moves the gradient by a large share of its largest element
    (tests/test_per_ray_reference_cpu.py measures both).

searchsorted(..., right) is restated as "count of edges <= query", so the tie rule is not borrowed from the code under test or from torch.
"""
import math

import torch

from oracle import kplanes_oracle as KO

EPS32 = float(torch.tensor(1.0e-7, dtype=torch.float32))  # the 1.0e-7f the kernels (and the float32 oracle) add
MARGIN = 1.0e-6  # outside family (d) no depth midpoint lies this close to D - sigma or D + sigma

# ---------------------------------------------------------------------------------------------------------------------------------------
# the lattice (tests/test_gpu_per_ray_lattice.py runs it on the GPU; tests/test_per_ray_reference_cpu.py measures E32 over it)
# ---------------------------------------------------------------------------------------------------------------------------------------
SAMPLE_COUNTS = (1, 2, 7, 48, 63, 64, 65, 96, 128, 129, 256, 257, 319, 320)
RAY_COUNTS = (1, 2, 3, 4, 5, 133)
# every S with an R that is not a multiple of four; every R with at least three S
LATTICE = ((1, 1), (1, 5), (2, 3), (2, 4), (7, 2), (7, 133), (48, 133), (48, 3), (63, 1), (63, 5), (64, 133), (64, 2), (65, 3), (65, 4),
           (96, 5), (96, 133), (128, 2), (128, 1), (129, 3), (129, 4), (256, 5), (256, 133), (257, 2), (257, 1), (319, 3), (319, 4),
           (320, 133), (320, 5))  # (S, R)
PRODUCTION_PAIRS = ((64, 256), (64, 128), (48, 256), (48, 128), (48, 96))
EDGE_PAIRS = ((1, 1), (1, 7), (7, 1), (7, 256), (63, 65), (65, 129), (257, 319), (320, 320), (320, 1))
INTERLEVEL_PAIRS = PRODUCTION_PAIRS + EDGE_PAIRS  # (S nerf, Sp proposal)
INTERLEVEL_RAYS = (133, 5, 3, 1, 2, 4)  # dealt round-robin over the pairs
RENDER_FAMILY_CASES = ((65, 5, 129, "b"), (48, 133, 96, "b"), (7, 3, 256, "c"), (320, 2, 1, "c"))  # (S, R, Sp, family): the renderers off family (a)


def interlevel_cases():
    """(S, Sp, R, family, weight mode) of every interlevel case.  Family (c) -- nerf edges drawn independently of the proposal -- applies where
    the nerf level is the coarser one or the proposal has a single bin."""
    out = []
    for k, (S, Sp) in enumerate(INTERLEVEL_PAIRS):
        R = INTERLEVEL_RAYS[k % len(INTERLEVEL_RAYS)]
        fams = ["a", "b"] + (["c"] if (S < Sp or Sp == 1) else [])
        for fam in fams:
            for mode in ("natural", "scaled"):
                out.append((S, Sp, R, fam, mode))
    return out


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(ord(ch) for ch in k) if isinstance(k, str) else int(k))) % (2**31 - 1)
    return torch.Generator().manual_seed(seed)


def _densities(R, S, gen):
    d = torch.rand(R, S, generator=gen) ** 4 * 60
    if S > 1:  # some exact zeros; a single sample is never zeroed
        d = torch.where(torch.rand(R, S, generator=gen) < 0.1, torch.zeros(()), d)
    return d


def _get_weights(deltas, dens):
    """KO.get_weights; a single sample has no transmittance in front of it (the oracle's concatenation is written for S > 1)."""
    return KO.get_weights(deltas, dens) if deltas.shape[1] > 1 else 1 - torch.exp(-deltas * dens)


# ---------------------------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------------------------
def pipeline_case(R, S, Sp, family="a", seed=0):
    """Families (a), (b), (c): a proposal level (Sp bins) and a nerf level (S bins) of R rays as the sampling pipeline shapes them.
    (a) proposal bins from KO.spaced_bins, nerf bins from KO.pdf_sample of the proposal weights, weights from KO.get_weights of random
    densities with some exact zeros; (b) = (a) with about a third of the nerf edges moved onto the nearest proposal edge and re-sorted
    (zero-width nerf bins occur); (c) nerf edges drawn uniformly, independent of the proposal (wide or single-bin envelopes)."""
    gen = _gen("pipeline", R, S, Sp, family, seed)
    rnd = lambda *sh: torch.rand(*sh, generator=gen)
    tp = KO.spaced_bins(R, Sp, rnd(R, Sp + 1)).contiguous()
    near = rnd(R, 1) * 0.5 + 0.05
    far = near + 2.0 + rnd(R, 1) * 4.0
    ebp = near + tp * (far - near)
    wp = _get_weights(ebp[:, 1:] - ebp[:, :-1], _densities(R, Sp, gen))
    if family == "c":
        c = torch.sort(rnd(R, S + 1), -1).values
    else:
        c = torch.sort(KO.pdf_sample(wp, tp, KO.pdf_u(R, S, rnd(R, S + 1)))[0], -1).values
    if family == "b":
        nearest = torch.gather(tp, -1, (c[:, :, None] - tp[:, None, :]).abs().argmin(-1))
        every_third = (torch.arange(S + 1)[None, :] + torch.arange(R)[:, None]) % 3 == 0  # a third even on a two-edge ray set
        c = torch.sort(torch.where(every_third | (rnd(R, S + 1) < 0.05), nearest, c), -1).values
    c = c.contiguous()
    eb = (near + c * (far - near)).contiguous()
    dens = _densities(R, S, gen)
    w = _get_weights(eb[:, 1:] - eb[:, :-1], dens)
    return {"R": R, "S": S, "Sp": Sp, "p_bins": tp, "w_prop": wp.contiguous(), "c_bins": c, "ebins": eb, "density": dens.contiguous(),
            "weights": w.contiguous(), "rgb": rnd(R, S, 3), "bg": rnd(R, 3), "target": rnd(R, 3)}


def scaled_nerf_weights(case, seed=0):
    """Nerf weights that straddle the proposal envelope: the float64 w_outer times a factor from [0.25, 0.75) or [1.25, 1.75), so that clipped
    and unclipped intervals both occur and w - w_outer is never a near-cancellation by construction."""
    gen = _gen("scaled", case["R"], case["S"], case["Sp"], seed)
    lo, hi = envelopes(case["c_bins"], case["p_bins"])
    cy = torch.cat([torch.zeros(case["R"], 1, dtype=torch.float64), torch.cumsum(case["w_prop"].double(), -1)], -1)
    wo = torch.gather(cy, -1, hi + 1) - torch.gather(cy, -1, lo)
    f = torch.rand(case["R"], case["S"], generator=gen) * 0.5 + 0.25 + (torch.rand(case["R"], case["S"], generator=gen) < 0.5).float()
    return (wo * f.double()).float().contiguous()


def tied_share(case):
    """Share of the nerf edges that equal a proposal edge exactly."""
    return float((case["c_bins"][:, :, None] == case["p_bins"][:, None, :]).any(-1).float().mean())


def envelope_width(case):
    """Mean number of proposal bins under one nerf interval."""
    lo, hi = envelopes(case["c_bins"], case["p_bins"])
    return float((hi - lo + 1).float().mean())


def exact_render_case(S):
    """Family (d) for the renderers: nine rays of dyadic weights -- cumulative sums that hit 0.5 exactly (at the first sample, inside a lane's
    block, at the last sample, across index 63/64), an all-zero ray, a ray whose total stays below 0.5, and accumulation above 1."""
    R = 9
    gen = _gen("exact_render", S)
    w = torch.zeros(R, S)
    w[0] = torch.tensor([2.0 ** -(i + 1) if i < 100 else 0.0 for i in range(S)])  # 0.5 at once
    w[1, : min(S, 2)] = 0.25                                   # 0.5 exactly at index 1
    #   2: all zero -> S - 1
    w[3] = 0.25 / S if S > 1 else 0.25                         # total below 0.5 -> S - 1
    w[4, : min(S, 3)] = 0.75                                   # accumulation above 1
    w[5, : min(S, 4)] = 0.125                                  # 0.5 exactly at index 3
    w[6, S - 1] = 0.5                                          # 0.5 exactly at the last sample
    if S > 64:
        w[7, 63], w[7, 64] = 0.25, 0.25                        # 0.5 exactly at index 64
    else:
        w[7, 0], w[7, S - 1] = 0.25, 0.25
    w[8, S // 2] = 0.5 - 2.0 ** -25                            # one ulp below 0.5 ...
    w[8, S - 1] = 2.0 ** -25 if S // 2 != S - 1 else w[8, S - 1]  # ... reached exactly at the last sample
    eb = torch.cumsum(torch.rand(R, S + 1, generator=gen) * 0.05 + 1e-3, -1)
    return {"R": R, "S": S, "weights": w.contiguous(), "rgb": torch.rand(R, S, 3, generator=gen), "ebins": eb.contiguous(),
            "bg": torch.rand(R, 3, generator=gen), "target": torch.rand(R, 3, generator=gen)}


def depth_case(R, S, seed=0, sigma=0.05):
    """Depth-loss inputs on family (a): termination depths inside, before and behind the sampled range, exact zeros and negatives (the D <= 0
    gate), direction norms, predicted depths.  Midpoints closer than MARGIN to D - sigma or D + sigma (for D and for D * directions_norm) are
    avoided by re-drawing D; depth_margin() is the check."""
    case = pipeline_case(R, S, max(S, 2), "a", seed + 17)
    gen = _gen("depth", R, S, seed)
    eb = case["ebins"]
    dn = (1.0 + torch.rand(R, generator=gen) * 0.4).contiguous()
    lo, hi = eb[:, 0], eb[:, -1]
    for attempt in range(64):
        D = lo - 0.3 + torch.rand(R, generator=gen) * (hi - lo + 0.6)
        kind = torch.arange(R) % 7
        D = torch.where(kind == 3, torch.zeros(()), D)
        D = torch.where(kind == 5, -D.abs() - 0.1, D)
        case.update(termination_depth=D.contiguous(), directions_norm=dn, predicted_depth=(D.abs() + torch.rand(R, generator=gen) - 0.5).contiguous(),
                    sigma=float(sigma))
        if depth_margin(case) > MARGIN:
            return case
    raise AssertionError("no termination depths off the window edges in 64 draws")


def depth_margin(case):
    """Smallest distance of any sample midpoint from a URF window edge D - sigma, D + sigma (D as given and D * directions_norm), in float64."""
    t = (case["ebins"][:, :-1].double() + case["ebins"][:, 1:].double()) / 2
    best = math.inf
    for D in (case["termination_depth"].double(), case["termination_depth"].double() * case["directions_norm"].double()):
        for edge in (D - case["sigma"], D + case["sigma"]):
            best = min(best, float((t - edge[:, None]).abs().min()))
    return best


def exact_depth_case(S):
    """Family (d) for the depth losses: bin edges, D and sigma on a dyadic grid, so that midpoints EQUAL D - sigma and D + sigma in float32 and
    float64 alike (pins <= against <), plus D = 0 and D < 0 rays.  directions_norm is a power of two: D * directions_norm stays exact."""
    R = 6
    gen = _gen("exact_depth", S)
    sigma = 0.25
    eb = (1.0 + torch.arange(S + 1, dtype=torch.float32) / 16.0)[None].repeat(R, 1).contiguous()  # midpoints 1 + (2 i + 1) / 32
    mid = lambda i: 1.0 + (2 * i + 1) / 32.0
    a, b = S // 3, (2 * S) // 3
    D = torch.tensor([mid(a) - sigma, mid(b) + sigma, mid(S // 2), 0.0, -1.0, mid(0) + sigma])  # row 0: t == D + sigma; rows 1, 5: t == D - sigma
    w = (torch.rand(R, S, generator=gen) * 0.3 + 0.2).contiguous()
    return {"R": R, "S": S, "ebins": eb, "weights": w, "termination_depth": D.contiguous(), "directions_norm": torch.full((R,), 0.5),
            "predicted_depth": (D.abs() + 0.125).contiguous(), "sigma": sigma}


def edge_hits(case):
    """Number of midpoints that equal D + sigma and D - sigma exactly (float32 arithmetic, as the kernel does it)."""
    t = (case["ebins"][:, :-1] + case["ebins"][:, 1:]) / 2
    D = case["termination_depth"][:, None]
    on = D > 0
    return int(((t == D + case["sigma"]) & on).sum()), int(((t == D - case["sigma"]) & on).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
def _background(rgb64, bg, bg_mode):
    if bg_mode == 0:
        return bg.double()
    if bg_mode == 1:
        return rgb64[:, -1]
    return bg.double().reshape(1, 3)


def median_index_ref(weights):
    """First index whose float32 running sum reaches 0.5, S - 1 when none does."""
    S = weights.shape[1]
    hit = torch.cumsum(weights, -1) >= 0.5
    first = torch.where(hit, torch.arange(S)[None], torch.full((1, 1), S)).min(-1).values
    return first.clamp_max(S - 1)


def render_ref(weights, rgb, ebins, bg, bg_mode, training):
    """rgb [R,3], accumulation [R], depth_expected [R] (unclipped) in float64; median_index, depth_median and median_rgb exactly as float32
    holds them (a gather, one float32 midpoint, nan_to_num / clamp)."""
    c32 = rgb if training else torch.nan_to_num(rgb)
    w, c = weights.double(), c32.double()
    acc = w.sum(-1)
    out = (w[..., None] * c).sum(-2) + _background(c, bg, bg_mode) * (1.0 - acc[:, None])
    if not training:
        out = out.clamp(0.0, 1.0)
    steps = (ebins[:, :-1].double() + ebins[:, 1:].double()) / 2
    idx = median_index_ref(weights)
    steps32 = (ebins[:, :-1] + ebins[:, 1:]) / 2.0
    mrgb = torch.gather(c32, 1, idx[:, None, None].expand(-1, 1, 3))[:, 0]
    if not training:
        mrgb = mrgb.clamp(0.0, 1.0)
    return {"rgb": out, "accumulation": acc, "depth_expected": (w * steps).sum(-1) / (acc + 1e-10), "median_index": idx,
            "depth_median": torch.gather(steps32, 1, idx[:, None])[:, 0], "median_rgb": mrgb}


def render_bwd_ref(weights, rgb, bg, bg_mode, g_rgb_out, g_acc=None, prefill_w=None):
    """d/d weights and d/d rgb of rgb_out = sum_s w_s rgb_s + bg (1 - sum_s w_s) and acc = sum_s w_s (bg modes 0 and 2: the background is a
    constant); prefill_w is what g_weights held before an accumulating call."""
    assert bg_mode in (0, 2)
    c, go = rgb.double(), g_rgb_out.double()
    b = _background(c, bg, bg_mode)
    gw = ((c - b[:, None, :]) * go[:, None, :]).sum(-1)
    if g_acc is not None:
        gw = gw + g_acc.double()[:, None]
    if prefill_w is not None:
        gw = gw + prefill_w.double()
    return gw, go[:, None, :] * weights.double()[..., None]


def render_mse_bwd_ref(weights, rgb, bg, bg_mode, rgb_out, target, go_scale):
    """The render backward fed with go_scale * (rgb_out - target), and the per-ray squared error."""
    d = rgb_out.double() - target.double()
    gw, grgb = render_bwd_ref(weights, rgb, bg, bg_mode, d * go_scale)
    return gw, grgb, (d * d).sum(-1)


def distortion_ref(weights, sbins, grad_scale=1.0, prefill=None):
    """L_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i); dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i (t_{i+1} - t_i)."""
    w, t = weights.double(), sbins.double()
    m = (t[:, 1:] + t[:, :-1]) / 2
    dt = t[:, 1:] - t[:, :-1]
    inner = ((m[:, :, None] - m[:, None, :]).abs() * w[:, None, :]).sum(-1)
    value = (w * inner).sum(-1) + (w * w * dt).sum(-1) / 3
    g = (2 * inner + 2 * w * dt / 3) * grad_scale
    return value, (g if prefill is None else g + prefill.double())


def envelopes(c_bins, p_bins):
    """lo_i = clamp(#{k < Sp: tp_k <= c_i} - 1, 0, Sp - 1), hi_i = clamp(#{k in 1..Sp: tp_k <= c_{i+1}}, 0, Sp - 1): searchsorted(..., right)
    written as a count of edges."""
    Sp = p_bins.shape[1] - 1
    lo = (p_bins[:, None, :-1] <= c_bins[:, :-1, None]).sum(-1) - 1
    hi = (p_bins[:, None, 1:] <= c_bins[:, 1:, None]).sum(-1)
    return lo.clamp(0, Sp - 1), hi.clamp(0, Sp - 1)


def interlevel_ref(c_bins, w_nerf, p_bins, w_prop, grad_scale=1.0, plain_float64=False):
    """Per-ray sum_i max(w_i - w_outer_i, 0)^2 / (w_i + 1e-7) and its gradient w.r.t. w_prop, w_outer_i = cy[hi_i + 1] - cy[lo_i].  The
    emulation (default) rounds cy and the difference to float32 as the kernel does; plain_float64 is the naive yardstick, kept to measure how
    wrong it is."""
    R, Sp = w_prop.shape
    lo, hi = envelopes(c_bins, p_bins)
    if plain_float64:
        cy = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(w_prop.double(), -1)], -1)
        wo = torch.gather(cy, -1, hi + 1) - torch.gather(cy, -1, lo)
    else:
        cy = torch.cat([torch.zeros(R, 1), torch.cumsum(w_prop, -1)], -1)  # float32: double accumulator, rounded per element
        wo = (torch.gather(cy, -1, hi + 1) - torch.gather(cy, -1, lo)).double()  # one float32 rounding
    w = w_nerf.double()
    d = (w - wo).clamp_min(0.0)
    value = (d * d / (w + EPS32)).sum(-1)
    gi = -2.0 * d / (w + EPS32)
    j = torch.arange(Sp)[None, None, :]
    inside = (lo[:, :, None] <= j) & (j <= hi[:, :, None])
    return value, (gi[:, :, None] * inside).sum(1) * grad_scale


def _depth_D(case, use_norm):
    D = case["termination_depth"].double()
    return D * case["directions_norm"].double() if use_norm else D


def ds_nerf_depth_ref(case, use_norm, grad_scale=1.0, prefill=None):
    """loss_r = [D_r > 0] sum_s -log(w_s + 1e-7) exp(-(t_s - D_r)^2 / (2 sigma)) (e_{s+1} - e_s) and grad_scale * d loss_r / d w."""
    D = _depth_D(case, use_norm)
    e, w = case["ebins"].double(), case["weights"].double()
    t = (e[:, :-1] + e[:, 1:]) / 2
    k = torch.exp(-((t - D[:, None]) ** 2) / (2 * case["sigma"])) * (e[:, 1:] - e[:, :-1])
    on = (D > 0).double()
    value = (-torch.log(w + EPS32) * k).sum(-1) * on
    g = -k / (w + EPS32) * on[:, None] * grad_scale
    return value, (g if prefill is None else g + prefill.double())


def urf_depth_ref(case, use_norm, grad_scale=1.0, prefill=None):
    """loss_r = [D_r > 0] ((D_r - d_r)^2 + sum_{|t_s - D_r| <= sigma} (w_s - N(t_s - D_r; 0, sigma / 3))^2 + sum_{t_s < D_r - sigma} w_s^2),
    grad_scale * d loss_r / d w and grad_scale * d loss_r / d d_r."""
    D = _depth_D(case, use_norm)
    sigma = case["sigma"]
    e, w, pred = case["ebins"].double(), case["weights"].double(), case["predicted_depth"].double()
    t = (e[:, :-1] + e[:, 1:]) / 2
    # x = t - D with the float32 roundings of the midpoint, of D * directions_norm and of the difference (IEEE operations the kernel and the
    # reference program share): at sigma = 0.01 the exponent x^2 / (2 (sigma / 3)^2) turns a 1e-7 rounding of x into 1e-4 of the pdf, and
    # plain float64 then misses fixture G8b's own float32 gradient by 1.5e-5 of an element.  The window comparisons stay in float64.
    t32 = (case["ebins"][:, :-1] + case["ebins"][:, 1:]) / 2.0
    D32 = case["termination_depth"] * case["directions_norm"] if use_norm else case["termination_depth"]
    x = (t32 - D32[:, None]).double()
    sd = sigma / 3.0
    pdf = torch.exp(-(x * x) / (2 * sd * sd) - math.log(sd) - 0.5 * math.log(2 * math.pi))
    near = (t <= D[:, None] + sigma) & (t >= D[:, None] - sigma)
    front = t < D[:, None] - sigma
    zero = torch.zeros((), dtype=torch.float64)
    term = torch.where(near, (w - pdf) ** 2, torch.where(front, w * w, zero))
    g = torch.where(near, 2 * (w - pdf), torch.where(front, 2 * w, zero))
    on = (D > 0).double()
    value = (term.sum(-1) + (D - pred) ** 2) * on
    g = g * on[:, None] * grad_scale
    return value, (g if prefill is None else g + prefill.double()), -2.0 * (D - pred) * on * grad_scale


def ray_train_ref(case, go_scale, dist_scale, bg_mode=0):
    """The nerf level's per-ray training work in float64 on finite inputs: weights from get_weights, rgb_out, accumulation, the per-ray
    distortion value, the per-ray squared error, and g_density, g_weights, g_rgb = d/d density, d/d weights, d/d rgb of
    go_scale / 2 * sum (rgb_out - target)^2 + dist_scale * sum_r distortion_r  by autograd."""
    dens = case["density"].double().requires_grad_(True)
    e = case["ebins"].double()
    dd = (e[:, 1:] - e[:, :-1]) * dens
    excl = torch.cumsum(dd, -1) - dd
    w = (1 - torch.exp(-dd)) * torch.exp(-excl)
    w.retain_grad()
    c = case["rgb"].double().requires_grad_(True)
    acc = w.sum(-1)
    out = (w[..., None] * c).sum(-2) + _background(c, case["bg"], bg_mode) * (1 - acc[:, None])
    t = case["c_bins"].double()
    m = (t[:, 1:] + t[:, :-1]) / 2
    inner = ((m[:, :, None] - m[:, None, :]).abs() * w[:, None, :]).sum(-1)
    dist = (w * inner).sum(-1) + (w * w * (t[:, 1:] - t[:, :-1])).sum(-1) / 3
    d = out - case["target"].double()
    (go_scale / 2 * (d * d).sum() + dist_scale * dist.sum()).backward()
    return {"weights": w.detach(), "rgb_out": out.detach(), "acc": acc.detach(), "dist_rays": dist.detach(), "sqerr": (d * d).sum(-1).detach(),
            "g_density": dens.grad, "g_weights": w.grad, "g_rgb": c.grad}


# ---------------------------------------------------------------------------------------------------------------------------------------
# deviation metric shared by the E32 measurement and the GPU bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
def deviation(got, want):
    """max |got - want| over the largest |want| of the case; where want is identically zero the absolute figure (which must then be zero)."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.numel() == 0:
        return 0.0
    diff = float((got - want).abs().max())
    scale = float(want.abs().max())
    return diff / scale if scale > 0 else diff


def prefill_like(want, *key):
    """What an accumulating call finds in its gradient buffer: uniform in +-half the largest reference gradient (float32)."""
    scale = float(want.abs().max()) or 1.0
    return ((torch.rand(want.shape, generator=_gen("prefill", *key)) - 0.5) * scale).float().contiguous()


def upstream(case, *key):
    """Upstream gradients of the render backward (g_rgb_out [R,3], g_acc [R]) and an rgb_out for the MSE-folded one."""
    gen = _gen("upstream", case["R"], case["S"], *key)
    R = case["R"]
    return torch.rand(R, 3, generator=gen) - 0.5, torch.rand(R, generator=gen), torch.rand(R, 3, generator=gen)


DEPTH_SIGMAS = (0.05, 0.2, 0.01)


def lattice_depth_case(k):
    """Depth-loss inputs of the k-th lattice entry."""
    S, R = LATTICE[k]
    return depth_case(R, S, seed=k, sigma=DEPTH_SIGMAS[k % 3])


def with_nonfinite_rgb(case):
    """Eval-mode inputs with NaN and +-inf colours: rays 0, 3, 6, ... carry +inf / -inf / NaN in channels 0 / 1 / 2 of a few samples (one sign
    per channel, so nothing cancels), rays 1, 4, 7, ... a last sample of (NaN, +inf, -inf).  Weights are halved (exactly): 1 - accumulation stays
    well above zero, so FLT_MAX * (1 - accumulation) has the same sign in float32 and float64."""
    out = dict(case)
    R, S = case["R"], case["S"]
    rgb = case["rgb"].clone()
    for r in range(0, R, 3):
        for i in sorted({0, S // 2, S - 1} if r % 2 == 0 else {S // 3}):
            rgb[r, i] = torch.tensor([float("inf"), float("-inf"), float("nan")])
    for r in range(1, R, 3):
        rgb[r, S - 1] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    out["rgb"], out["weights"] = rgb.contiguous(), (case["weights"] * 0.5).contiguous()
    return out

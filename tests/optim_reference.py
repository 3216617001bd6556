"""Reference side of the optimiser-sweep tests (tests/test_optim_reference_cpu.py, test_gpu_optim_lattice.py, test_gpu_tile_adam_oracle.py) --
test infrastructure.

Everything here is plain torch on the CPU, dtype-parametric: run in float64 it is the reference of a comparison, run in float32 it is the
yardstick (a bound is FACTOR x the float32 restatement's deviation from the float64 one on the same inputs, relative to the output's largest
magnitude; measured once by tools/measure_optim_deviations.py into profiles/r16_optim_deviations.json, which the GPU tests read).

Regularisers: the K-Planes plane losses (NS/model_components/losses.py:356-452) restated for a plane set in reference layout (a list over
scales of [1,C,H,W] tensors, six per scale for a space-time set, three for a static one); the gradient is autograd of the restated values.
oracle/kplanes_oracle.py hard-codes the six-plane indices, so it is the cross-check of the six-plane cases only.

Adam: the formula of csrc/optim.hip's comment,
    g_total = g * grad_scale + c_tv d(tv) + c_smooth d(smooth) + c_l1 d(l1)       (a non-finite element counts as 0 and is counted as dropped)
    m = b1 m + (1 - b1) g_total;  v = b2 v + (1 - b2) g_total^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
Every scalar is the float32 value the C ABI receives, taken as a double: BETA1 = float(float32(0.9)), BETA2 = float(float32(0.999)), and
1 - beta is then exact in both precisions.  torch.optim.Adam given the decimal 0.999 forms 1 - 0.999 in double, 1.29e-5 (relative) away:
a property of the float ABI, pinned by test_optim_reference_cpu.py::test_abi_beta_deviation_is_pinned."""
import itertools
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVIATIONS = os.path.join(ROOT, "profiles", "r16_optim_deviations.json")
FACTOR = 5.0  # bound = FACTOR x the float32 restatement's deviation: the project's standing rule
U32 = 2.0 ** -24  # float32 unit roundoff


def f32(x) -> float:
    """The float32 value a C ABI `float` argument receives, as a double."""
    return float(np.float32(x))


BETA1, BETA2 = f32(0.9), f32(0.999)
LR = 1e-2
PRESET_COEFS = (0.0002, 0.001, 0.0001)  # space_tv, time_smoothness, sparse_transients of the k-planes preset (method_configs.py:530-541)
COEFS = {"preset": PRESET_COEFS, "big": (0.3, 0.7, 1.1), "zero": (0.0, 0.0, 0.0), "tv": (0.3, 0.0, 0.0), "smooth": (0.0, 0.7, 0.0),
         "l1": (0.0, 0.0, 1.1), "no_tv": (0.0, 0.7, 1.1)}
STATES = {"zero1": ("zero", 1), "rand3": ("rand", 3), "rand30000": ("rand", 30000)}


def load_bounds():
    with open(DEVIATIONS) as f:
        return json.load(f)


def rel_dev(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0; any error against an all-zero reference is inf)."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if want.numel() == 0:
        return 0.0
    err = float((got - want).abs().max())
    if err == 0.0:
        return 0.0
    scale = float(want.abs().max())
    return float("inf") if scale == 0.0 else err / scale


def rel_dev_where(got, want, mask) -> float:
    """rel_dev over the elements of `mask`, still relative to the WHOLE reference's largest magnitude."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if not bool(mask.any()):
        return 0.0
    err = float((got - want)[mask].abs().max())
    return 0.0 if err == 0.0 else err / float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------------
# plane-set layout (flat, channel-last: soccernerfs_amd/plane_set.py) written out independently of the package
# ------------------------------------------------------------------------------------------------------------------------------------
def resolutions(base, mult):
    """One [x, y, z(, t)] list per scale: the spatial axes are multiplied, the time axis is not."""
    return [[int(r) * int(k) if a < 3 else int(r) for a, r in enumerate(base)] for k in mult]


def plane_layout(C, res):
    """[(scale, plane, offset, H, W, has_time)] in memory order; plane p pairs the axes (a, b) of combinations(range(n_coords), 2), W = res[a], H = res[b]."""
    out, off = [], 0
    for s, reso in enumerate(res):
        for p, (a, b) in enumerate(itertools.combinations(range(len(reso)), 2)):
            H, W = reso[b], reso[a]
            out.append((s, p, off, H, W, len(reso) == 4 and b == 3))
            off += H * W * C
    return out, off


def to_grids(flat, C, res):
    """Flat channel-last buffer -> reference layout: list over scales of [1,C,H,W] tensors (views where possible; differentiable)."""
    layout, _ = plane_layout(C, res)
    grids = [[] for _ in res]
    for s, _, off, H, W, _ in layout:
        grids[s].append(flat[off: off + H * W * C].view(H, W, C).permute(2, 0, 1)[None])
    return grids


# ------------------------------------------------------------------------------------------------------------------------------------
# regularisers
# ------------------------------------------------------------------------------------------------------------------------------------
def _mean_sq(d):
    return (d * d).mean()


def _tv(t, along_h: bool):
    """Mean squared first difference along the last axis (always) plus, on a space-only plane, along the one before it."""
    out = _mean_sq(t[..., :, 1:] - t[..., :, :-1])
    if along_h:
        out = out + _mean_sq(t[..., 1:, :] - t[..., :-1, :])
    return out


def _smoothness(t):
    """Mean squared second difference along H (time)."""
    return _mean_sq(t[..., 2:, :] - 2 * t[..., 1:-1, :] + t[..., :-2, :])


def regularizers(grids):
    """(space_tv, time_smoothness, sparse_transients) of a plane set in reference layout.  Three planes per scale: all spatial, no time
    terms (exact zeros).  Six: planes 0, 1, 3 are spatial; 2, 4, 5 hold time along H and take the 1-D TV, the smoothness and the L1 term."""
    dt = grids[0][0].dtype
    tv, sm, l1 = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)
    for planes in grids:
        assert len(planes) in (3, 6)
        time_ids = () if len(planes) == 3 else (2, 4, 5)
        for i, t in enumerate(planes):
            tv = tv + _tv(t, along_h=i not in time_ids)
            if i in time_ids:
                sm = sm + _smoothness(t)
                l1 = l1 + (1 - t).abs().mean()
    return tv, sm, l1


def reg_values_and_grad(flat, C, res, coefs):
    """Values (3, unscaled) and the gradient of c_tv tv + c_smooth smooth + c_l1 l1 with respect to the flat buffer, in flat's dtype."""
    x = flat.detach().clone().requires_grad_(True)
    vals = regularizers(to_grids(x, C, res))
    total = sum(f32(c) * v for c, v in zip(coefs, vals))
    if total.requires_grad:
        (g,) = torch.autograd.grad(total, x)
    else:
        g = torch.zeros_like(x)
    return torch.stack([v.detach() for v in vals]), g


# ------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------------
def adam(p, g_total, m, v, step, lr=LR, b1=BETA1, b2=BETA2, eps=1e-12):
    """One step in p's dtype; scalars are doubles (float32-valued where they cross the C ABI).  Returns p, m, v, dropped."""
    lr, eps = f32(lr), f32(eps)
    finite = torch.isfinite(g_total)
    g = torch.where(finite, g_total, torch.zeros_like(g_total))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * (g * g)
    step_size = f32(lr / (1.0 - b1 ** step))          # the kernels receive both constants rounded to float
    inv_sqrt_bc2 = f32(1.0 / np.sqrt(1.0 - b2 ** step))
    p = p - step_size * (m / (v.sqrt() * inv_sqrt_bc2 + eps))
    return p, m, v, int((~finite).sum())


def planes_step(d, dtype, coefs=None, b1=BETA1, b2=BETA2):
    """The fused sweep on a case's data (make_case): dict of p_out, m, v, reg_grad, values, g_total, dropped."""
    c = d["case"]
    coefs = COEFS[c["coefs"]] if coefs is None else coefs
    p, g, m, v = (d[k].to(dtype) for k in ("p", "g", "m", "v"))
    vals, rg = reg_values_and_grad(p, c["C"], d["res"], coefs)
    g_total = g * c["grad_scale"] + rg
    po, mo, vo, dropped = adam(p, g_total, m, v, d["step"], b1=b1, b2=b2)
    return {"p_out": po, "m": mo, "v": vo, "reg_grad": rg, "values": vals, "g_total": g_total, "dropped": dropped}


# ------------------------------------------------------------------------------------------------------------------------------------
# the case lattice
# ------------------------------------------------------------------------------------------------------------------------------------
def _case(C, base, mult, params, grad, coefs, state, grad_scale=1.0, zero_grad=1):
    return dict(C=C, base=tuple(base), mult=tuple(mult), params=params, grad=grad, coefs=coefs, state=state, grad_scale=float(grad_scale),
                zero_grad=int(zero_grad))


# C in {8,16,32} x 1/2/3 scales x n_coords 4/3 x parameter families x gradient families x coefficient sets x state/step x grad_scale x
# zero_grad: every value of every axis occurs; no full product.  Resolutions: [2,2,2,3] every spatial texel is a border texel and time has
# exactly one second difference; [3,5,4,4] H - 2 = 2, so each of the stencil branches h, h-1, h-2 holds for some rows and fails for others;
# [5,3,2,7] C=8 whole planes smaller than a 256-lane workgroup; [20,12,9,7] x (1,2) C=32 planes over many workgroups, sizes no multiple of
# 1024 floats; [16,16,16,100] the preset's time resolution.  grad "zero": the regularisers are the only gradient.
PLANE_CASES = [
    _case(8, (2, 2, 2, 3), (1,), "random", "dense", "big", "zero1"),
    _case(16, (2, 2, 2, 3), (1,), "random", "zero", "big", "rand3", zero_grad=0),
    _case(32, (2, 2, 2, 3), (1, 2), "quarter_one", "half_zero", "preset", "rand30000", grad_scale=0.5),
    _case(8, (2, 2, 2, 3), (1,), "random", "zero", "smooth", "zero1"),
    _case(32, (2, 2, 2, 3), (1, 2, 4), "random", "zero", "tv", "zero1"),
    _case(16, (2, 2, 2, 3), (1, 2), "time_one", "zero", "preset", "zero1"),
    _case(8, (3, 5, 4, 4), (1,), "random", "zero", "big", "zero1"),
    _case(16, (3, 5, 4, 4), (1, 2), "random", "dense", "preset", "rand3", grad_scale=0.5, zero_grad=0),
    _case(32, (3, 5, 4, 4), (1, 2, 4), "random", "zero", "smooth", "rand3"),
    _case(8, (3, 5, 4, 4), (1, 2, 4), "quarter_one", "zero", "l1", "zero1"),
    _case(16, (3, 5, 4, 4), (1,), "random", "zero", "tv", "rand30000", zero_grad=0),
    _case(32, (3, 5, 4, 4), (1,), "time_one", "dense", "preset", "zero1"),
    _case(8, (3, 5, 4, 4), (1, 2), "constant", "zero", "big", "zero1"),
    _case(16, (3, 5, 4, 4), (1,), "random", "wide", "big", "rand3"),
    _case(16, (3, 5, 4, 4), (1, 2), "random", "zero", "l1", "rand3"),
    _case(8, (3, 5, 4, 4), (1,), "random", "dense", "big", "rand30000", grad_scale=0.5, zero_grad=0),
    _case(32, (3, 5, 4, 4), (1, 2), "quarter_one", "zero", "big", "zero1"),
    _case(8, (5, 3, 2, 7), (1,), "random", "dense", "big", "rand3", grad_scale=0.5),
    _case(8, (5, 3, 2, 7), (1,), "random", "zero", "preset", "zero1"),
    _case(8, (5, 3, 2, 7), (1, 2), "quarter_one", "half_zero", "big", "rand30000", zero_grad=0),
    _case(8, (5, 3, 2, 7), (1,), "random", "dense", "zero", "rand3"),
    _case(8, (5, 3, 2, 7), (1,), "random", "zero", "zero", "zero1"),
    _case(32, (20, 12, 9, 7), (1, 2), "random", "dense", "preset", "rand3", grad_scale=0.5),
    _case(32, (20, 12, 9, 7), (1, 2), "random", "zero", "big", "zero1"),
    _case(32, (20, 12, 9, 7), (1, 2), "quarter_one", "half_zero", "big", "rand30000", zero_grad=0),
    _case(32, (20, 12, 9, 7), (1, 2), "time_one", "wide", "preset", "zero1"),
    _case(16, (16, 16, 16, 100), (1,), "random", "zero", "big", "zero1"),
    _case(16, (16, 16, 16, 100), (1,), "time_one", "dense", "preset", "rand30000", grad_scale=0.5),
    _case(8, (16, 16, 16, 100), (1,), "random", "half_zero", "smooth", "rand3", zero_grad=0),
    # static scenes: three planes per scale, all spatial; the time coefficients must do nothing
    _case(8, (2, 2, 2), (1,), "random", "zero", "big", "zero1"),
    _case(16, (2, 2, 2), (1, 2), "random", "dense", "preset", "rand3", grad_scale=0.5, zero_grad=0),
    _case(32, (2, 2, 2), (1, 2, 4), "random", "half_zero", "tv", "rand30000"),
    _case(8, (5, 3, 4), (1,), "random", "zero", "big", "zero1"),
    _case(16, (5, 3, 4), (1, 2, 4), "random", "dense", "big", "rand3", grad_scale=0.5),
    _case(32, (5, 3, 4), (1,), "constant", "zero", "big", "zero1"),
    _case(8, (5, 3, 4), (1, 2), "random", "wide", "zero", "rand30000"),
    _case(32, (20, 12, 9), (1, 2), "random", "zero", "big", "zero1"),
    _case(32, (20, 12, 9), (1, 2), "random", "dense", "preset", "rand3", grad_scale=0.5),
    _case(16, (20, 12, 9), (1, 2), "random", "half_zero", "tv", "rand30000", zero_grad=0),
    _case(8, (20, 12, 9), (1, 2), "random", "dense", "no_tv", "rand3"),
]
for _i, _c in enumerate(PLANE_CASES):
    _c["seed"] = 100 + _i


def case_id(c) -> str:
    return (f"C{c['C']}-{'x'.join(map(str, c['base']))}-m{''.join(map(str, c['mult']))}-{c['params']}-g_{c['grad']}-c_{c['coefs']}-{c['state']}"
            f"-gs{c['grad_scale']:g}-zg{c['zero_grad']}")


for _c in PLANE_CASES:
    _c["case_id"] = case_id(_c)
assert len({c["case_id"] for c in PLANE_CASES}) == len(PLANE_CASES)
# the three cases that also run shard ranges and planted non-finite gradients: a static set, one smaller than a workgroup, a multi-scale one
RANGE_CASE_IDS = [PLANE_CASES[37]["case_id"], PLANE_CASES[17]["case_id"], PLANE_CASES[22]["case_id"]]


def signed_magnitudes(n, gen, kind):
    """float32 gradients whose magnitudes are exactly 0 or within [1e-12, 1e3] (g * g then never underflows in float32)."""
    if kind == "zero":
        return torch.zeros(n)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    if kind == "wide":
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 15.0 - 12.0)
    else:
        mag = torch.rand(n, generator=gen, dtype=torch.float64) * 0.5
    g = (sign * mag.clamp(1e-12, 1e3)).float()
    if kind == "half_zero":
        g = torch.where(torch.rand(n, generator=gen) < 0.5, torch.zeros(n), g)
    mag32 = g.abs()
    assert bool(((mag32 == 0) | ((mag32 >= f32(1e-12)) & (mag32 <= 1e3))).all())
    return g


def random_state(n, gen, kind):
    if kind == "zero":
        return torch.zeros(n), torch.zeros(n)
    return (torch.rand(n, generator=gen) - 0.5) * 0.1, torch.rand(n, generator=gen) * 0.01 + 1e-8


def make_case(c):
    """float32 inputs of a lattice case (exactly what the kernels are given): flat p, g, m, v, the resolutions and the step."""
    gen = torch.Generator().manual_seed(c["seed"])
    res = resolutions(c["base"], c["mult"])
    layout, n = plane_layout(c["C"], res)
    p = torch.rand(n, generator=gen) * 2.0
    if c["params"] == "constant":
        p = torch.full((n,), 0.75)
    for _, _, off, H, W, has_time in layout:
        if not has_time:
            continue
        seg = p[off: off + H * W * c["C"]]
        if c["params"] == "time_one":
            seg.fill_(1.0)
        elif c["params"] == "quarter_one":
            seg[torch.rand(seg.numel(), generator=gen) < 0.25] = 1.0
    g = signed_magnitudes(n, gen, c["grad"])
    kind, step = STATES[c["state"]]
    m, v = random_state(n, gen, kind)
    acc = torch.rand(n, generator=gen) - 0.5  # what snerf_plane_reg's accumulate mode (overwrite = 0) adds onto
    return {"case": c, "res": res, "layout": layout, "n": n, "p": p, "g": g, "m": m, "v": v, "acc": acc, "step": step}


def value_summation_bound(n_blocks: int, n_slots: int) -> float:
    """Relative float32 bound of the kernel's summation tree for one loss value (every term is >= 0, so the bound is relative to the sum):
    3 adds inside a float4's sum of squares, 1 add of a lane's second term, 6 butterfly levels of a wavefront, 3 adds over a workgroup's
    four wavefronts, ceil(n_blocks / n_slots) - 1 atomic adds into a slot; the slots are summed in float64 by the test.  A chain of L
    roundings on the way of every term gives |error| <= L u / (1 - L u) x sum."""
    L = 3 + 1 + 6 + 3 + max(0, -(-n_blocks // n_slots) - 1)
    return L * U32 / (1.0 - L * U32)


def n_workgroups(C, layout) -> int:
    return sum((H * W * (C // 4) + 255) // 256 for _, _, _, H, W, _ in layout)


# ------------------------------------------------------------------------------------------------------------------------------------
# flat Adam (snerf_adam_step) and Adam with the temporal-TV columns (snerf_adam_step_tv)
# ------------------------------------------------------------------------------------------------------------------------------------
FLAT_NS = (1, 2, 3, 4, 5, 255, 1023, 1024, 1025, 4099)  # n % 4 in every phase; n < 4: only the scalar tail runs
FLAT_EPS = (1e-12, 1e-15, 1e-6)                           # the fields', the camera optimiser's, the hash table's
FLAT_FAMILIES = [  # (grad, state, grad_scale): with FLAT_NS and FLAT_EPS every value of every axis occurs
    ("dense", "zero1", 1.0), ("dense", "rand3", 0.5), ("half_zero", "rand30000", 1.0), ("zero", "rand3", 1.0), ("wide", "rand3", 1.0),
    ("zero", "zero1", 1.0), ("wide", "zero1", 0.5), ("half_zero", "rand3", 1.0), ("dense", "rand30000", 1.0), ("wide", "rand30000", 1.0),
]
FLAT_CASES = [dict(n=n, eps=FLAT_EPS[i % 3], grad=f[0], state=f[1], grad_scale=f[2], in_place=int(i % 2 == 0), seed=300 + i,
                   case_id=f"n{n}-eps{FLAT_EPS[i % 3]:g}-g_{f[0]}-{f[1]}-gs{f[2]:g}-{'inplace' if i % 2 == 0 else 'pingpong'}")
              for i, (n, f) in enumerate(zip(FLAT_NS, FLAT_FAMILIES))]
FLAT_CASES += [dict(n=n, eps=FLAT_EPS[(i + 1) % 3], grad=f[0], state=f[1], grad_scale=f[2], in_place=int(i % 2 == 1), seed=320 + i,
                    case_id=f"n{n}-eps{FLAT_EPS[(i + 1) % 3]:g}-g_{f[0]}-{f[1]}-gs{f[2]:g}-{'inplace' if i % 2 == 1 else 'pingpong'}")
               for i, (n, f) in enumerate(zip(FLAT_NS, FLAT_FAMILIES[3:] + FLAT_FAMILIES[:3]))]


def make_flat_case(c):
    gen = torch.Generator().manual_seed(c["seed"])
    n = c["n"]
    p = torch.rand(n, generator=gen) * 2.0 - 1.0
    g = signed_magnitudes(n, gen, c["grad"])
    kind, step = STATES[c["state"]]
    m, v = random_state(n, gen, kind)
    return {"case": c, "p": p, "g": g, "m": m, "v": v, "step": step}


def flat_step(d, dtype):
    c = d["case"]
    p, g, m, v = (d[k].to(dtype) for k in ("p", "g", "m", "v"))
    po, mo, vo, dropped = adam(p, g * c["grad_scale"], m, v, d["step"], eps=c["eps"])
    return {"p_out": po, "m": mo, "v": vo, "dropped": dropped}


# a float4 straddles a row end whenever grid_C % 4 != 0; the column pairs include (0, grid_C - 1) and a pair inside one float4
TV_CASES = [dict(rows=r, grid_C=gc, cols=cols, state=st, grad=gr, grad_scale=gs, seed=400 + i,
                 case_id=f"rows{r}-C{gc}-cols{cols[0]}_{cols[1]}-g_{gr}-{st}-gs{gs:g}")
            for i, (r, gc, cols, st, gr, gs) in enumerate([
                (8, 4, (0, 3), "zero1", "dense", 1.0), (24, 4, (2, 1), "rand3", "zero", 1.0),
                (8, 6, (0, 5), "rand3", "dense", 0.5), (24, 6, (4, 5), "rand30000", "half_zero", 1.0),
                (8, 34, (0, 33), "rand30000", "zero", 1.0), (24, 34, (33, 32), "zero1", "wide", 1.0),
                (8, 66, (1, 2), "rand3", "half_zero", 1.0), (24, 66, (0, 65), "rand3", "dense", 0.5)])]


def make_tv_case(c):
    gen = torch.Generator().manual_seed(c["seed"])
    n = c["rows"] * c["grid_C"]
    p = torch.rand(n, generator=gen) * 2.0 - 1.0
    g = signed_magnitudes(n, gen, c["grad"])
    kind, step = STATES[c["state"]]
    m, v = random_state(n, gen, kind)
    # what tgrid_tv_sign_kernel writes: weight * sign(E[r,a] - E[r,b]) / rows, from the OLD table (some rows exactly 0)
    E = p.view(c["rows"], c["grid_C"])
    srow = 0.37 * torch.sign(E[:, c["cols"][0]] - E[:, c["cols"][1]]) / c["rows"]
    srow[::5] = 0.0
    return {"case": c, "p": p, "g": g, "m": m, "v": v, "srow": srow.float(), "step": step}


def tv_step(d, dtype):
    c = d["case"]
    p, g, m, v = (d[k].to(dtype) for k in ("p", "g", "m", "v"))
    gt = (g * c["grad_scale"]).view(c["rows"], c["grid_C"]).clone()
    gt[:, c["cols"][0]] += d["srow"].to(dtype)
    gt[:, c["cols"][1]] -= d["srow"].to(dtype)
    po, mo, vo, dropped = adam(p, gt.reshape(-1), m, v, d["step"])
    return {"p_out": po, "m": mo, "v": vo, "dropped": dropped}


# ------------------------------------------------------------------------------------------------------------------------------------
# the tile passes' fused Adam (snerf_tgrid_bwd_tiles_adam, snerf_hashgrid_bwd_tiles_adam) against the oracles' autograd
# ------------------------------------------------------------------------------------------------------------------------------------
TV_WEIGHT = 0.1
GRAD_RESOLVED = 100.0  # zero-state step: p is compared where |float64 gradient| > GRAD_RESOLVED x the float32 oracle's largest absolute gradient error
UNRESOLVED_CAP = 0.01  # ... and the share of touched entries left out stays under this


def tile_cases():
    """Two temporal-grid configurations of tests/test_gpu_tgrid_tiles.py::CASES (every level tiled with small tiles: tile boundaries inside dense
    levels whose row count is no multiple of the tile; first_tiled_level = 1) and one hash grid of tests/test_gpu_hashgrid.py (5 levels, F = 8)."""
    from tests.test_gpu_tgrid_tiles import CASES

    return [dict(case_id="tgrid-every_level_tiled", kind="tgrid", kw=CASES[3][0], sh=CASES[3][1], lc=CASES[3][2], R=129, S=37, eps=1e-12, seed=501),
            dict(case_id="tgrid-first_tiled_level_1", kind="tgrid", kw=CASES[4][0], sh=CASES[4][1], lc=CASES[4][2], R=129, S=37, eps=1e-12, seed=502),
            dict(case_id="hashgrid-L5-F8", kind="hashgrid", sh=3, lc=1, B=1237, eps=1e-6, seed=503,
                 cfg=dict(n_levels=5, n_features_per_level=8, base_resolution=5, per_level_scale=1.5, log2_hashmap_size=9))]


def _level_scales(c):
    if c["kind"] == "hashgrid":
        from oracle import hashgrid_oracle as HG

        g = c["cfg"]
        return [float(s) for s in HG.level_geometry(g["n_levels"], g["base_resolution"], g["per_level_scale"], g["log2_hashmap_size"])[0]]
    from oracle import tgrid_oracle as TO

    kw = c["kw"]
    base = kw.get("base_resolution", 16)
    log2_scale = float(np.log2(TO.resolve_scale(kw["num_levels"], base, kw.get("per_level_scale", 2.0), kw.get("desired_resolution"))))
    return [float(np.float32(np.exp2(np.float32(l * log2_scale))) * np.float32(base) - np.float32(1.0)) for l in range(kw["num_levels"])]


def well_placed(x, scales):
    """Points whose grid position x * scale + 0.5 is, at every level, further than 8 float32 ulps from an integer: every float32 evaluation order
    and the float64 one then agree on the cell, and no corner weight is exactly 0 -- so the set of touched table entries is the same for all."""
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for s in scales:
        pos = x.double() * s + 0.5
        ok &= ((pos - pos.round()).abs() > 8 * 2.0 ** -23 * pos.abs().clamp(min=1.0)).all(dim=-1)
    return ok


def make_tile_case(c):
    """float32 inputs: positions in [0,1]^3 (well placed, see above), one time per ray, gout of size 1e-3 (no engineered cancellation), the old
    table, a non-zero optimiser state (m random, v >= 1e-8: a well-conditioned denominator everywhere) and the TV column pair."""
    gen = torch.Generator().manual_seed(c["seed"])
    B = c["B"] if c["kind"] == "hashgrid" else c["R"] * c["S"]
    cand = torch.rand(2 * B, 3, generator=gen)
    x = cand[well_placed(cand, _level_scales(c))][:B].contiguous()
    assert x.shape[0] == B
    d = {"case": c, "B": B, "x": x}
    if c["kind"] == "tgrid":
        from oracle import tgrid_oracle as TO

        kw = c["kw"]
        base = kw.get("base_resolution", 16)
        scale = TO.resolve_scale(kw["num_levels"], base, kw.get("per_level_scale", 2.0), kw.get("desired_resolution"))
        offs = TO.level_offsets(kw["num_levels"], base, scale, kw["log2_hashmap_size"], kw["input_dim"])
        times = torch.rand(c["R"], generator=gen)
        times[0], times[1] = 0.0, 1.0
        table = TO.channel_table(kw["temporal_dim"], kw["level_dim"])
        d.update(times=times, offsets=offs, log2_scale=float(np.log2(scale)), base_res=base, level_dim=kw["level_dim"], chan=table,
                 trow=TO.temporal_index(times.repeat_interleave(c["S"]), table), shape=(offs[-1], kw["level_dim"] + kw["temporal_dim"]),
                 out_dim=kw["num_levels"] * kw["level_dim"], tv_cols=tuple(int(q) for q in table["index_ab"][7 % table["index_ab"].shape[0]]))
    else:
        from oracle import hashgrid_oracle as HG

        g = c["cfg"]
        rows = HG.level_geometry(g["n_levels"], g["base_resolution"], g["per_level_scale"], g["log2_hashmap_size"])[2][-1]
        d.update(shape=(rows, g["n_features_per_level"]), out_dim=g["n_levels"] * g["n_features_per_level"], tv_cols=None)
    n = d["shape"][0] * d["shape"][1]
    # random sign, magnitude uniform in [0.5e-3, 1.5e-3): as randn * 1e-3 without its mass near 0, which (times a small corner weight) is what leaves a
    # gradient below float32's resolution; no cancellation is engineered
    sign = torch.where(torch.rand(B, d["out_dim"], generator=gen) < 0.5, -1.0, 1.0)
    d["gout"] = sign * (torch.rand(B, d["out_dim"], generator=gen) + 0.5) * 1e-3
    d["table"] = ((torch.rand(n, generator=gen) - 0.5) * 0.2).view(d["shape"])
    d["m"] = ((torch.rand(n, generator=gen) - 0.5) * 1e-3).view(d["shape"])
    d["v"] = (torch.rand(n, generator=gen) * 1e-6 + 1e-8).view(d["shape"])
    return d


def tile_gradient(d, dtype, tv: bool):
    """d loss / d table by autograd through the oracle's encode on the case's positions, times and gout, plus the temporal-TV term
    TV_WEIGHT * mean |E[:, a] - E[:, b]| of the OLD table when tv."""
    c = d["case"]
    table = d["table"].to(dtype).clone().requires_grad_(True)
    if c["kind"] == "tgrid":
        from oracle import tgrid_oracle as TO

        out = TO.encode(d["x"].to(dtype), d["trow"].to(dtype), table, d["offsets"], d["log2_scale"], d["base_res"], 0, d["level_dim"])
    else:
        from oracle import hashgrid_oracle as HG

        g = c["cfg"]
        out = HG.encode(d["x"].to(dtype), table, g["n_levels"], g["n_features_per_level"], g["base_resolution"], g["per_level_scale"], g["log2_hashmap_size"])
    loss = (out * d["gout"].to(dtype)).sum()
    if tv:
        a, b = d["tv_cols"]
        loss = loss + f32(TV_WEIGHT) * (table[:, a] - table[:, b]).abs().mean()
    (grad,) = torch.autograd.grad(loss, table)
    return grad


def tile_step(d, dtype, tv: bool, state: str):
    """One Adam step of the whole table: state "rand" (the case's m, v; step 3) or "zero" (step 1)."""
    step = 3 if state == "rand" else 1
    grad = tile_gradient(d, dtype, tv)
    m = d["m"].to(dtype) if state == "rand" else torch.zeros(d["shape"], dtype=dtype)
    v = d["v"].to(dtype) if state == "rand" else torch.zeros(d["shape"], dtype=dtype)
    po, mo, vo, dropped = adam(d["table"].to(dtype), grad, m, v, step, eps=d["case"]["eps"])
    assert dropped == 0
    return {"p_out": po, "m": mo, "v": vo, "grad": grad, "step": step}


def tile_variants(c):
    return [(tv, st) for tv in ((False, True) if c["kind"] == "tgrid" else (False,)) for st in ("rand", "zero")]


def tile_key(tv, state):
    return f"{'tv' if tv else 'no_tv'}-{state}"


def resolved_mask(g64, grad_abs_err32):
    """Entries whose first Adam step (a move of lr along the gradient's sign) is determined in float32."""
    return g64.abs() > GRAD_RESOLVED * grad_abs_err32


def tile_deviations(d, tv, state):
    """The float32 oracle's deviation from the float64 one for one variant of a tile case: what tools/measure_optim_deviations.py records."""
    r64, r32 = tile_step(d, torch.float64, tv, state), tile_step(d, torch.float32, tv, state)
    touched = r64["grad"] != 0
    err = float((r32["grad"].double() - r64["grad"]).abs().max())
    rec = {"step": r64["step"], "touched": int(touched.sum()), "grad_abs_err32": err, "same_touched_set_in_float32": bool(((r32["grad"] != 0) == touched).all()),
           "dev32_m": rel_dev(r32["m"], r64["m"]), "dev32_v": rel_dev(r32["v"], r64["v"])}
    if state == "zero":
        keep = resolved_mask(r64["grad"], err) | ~touched
        rec["dev32_p_out"] = rel_dev_where(r32["p_out"], r64["p_out"], keep)
        rec["unresolved_share"] = float((touched & ~keep).sum()) / max(1, int(touched.sum()))
    else:
        rec["dev32_p_out"] = rel_dev(r32["p_out"], r64["p_out"])
    return rec

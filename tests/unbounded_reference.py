"""Reference side of the unbounded-scene tests (tests/test_unbounded_cpu.py, tests/test_gpu_unbounded.py) -- test infrastructure.

A torch restatement, in float64 (the reference of a comparison) or float32 (the expected bits of an equality, or the yardstick of a bound), of
what snerf_coords.contract = 1 computes: the sample positions of a ray, SceneContraction(order=inf), the fields' halving, the contraction's
Jacobian transposed with this project's tie rule (the FIRST axis that attains the maximum), and the near / far collider.  It is tied to
oracle.kplanes_oracle.scene_contraction_inf, to the `contracted` array recorded from the reference (tests/golden/g6c_contraction.npz) and to
float64 autograd by tests/test_unbounded_cpu.py.

Two generators:
  * coordinate_rounds(R, S, n_coords, seed): dyadic rays for the EQUALITY tests.  Every ray carries one planted sample whose position is a
    chosen dyadic point of a category (inside the unit cube, on its face, outside with each axis and sign largest, two-axis ties, m = 2^k up to
    1024).  A shape with fewer rays than categories gets several ray sets ("rounds") -- a (1, 1) shape holds ONE sample, so its case is one launch per planted point;
    the generator asserts that the rounds of a case together hold every category, at the planted float32 positions.
  * gradient_case(...): random rays for the coordinate-gradient test, with the share of samples inside the stated margins asserted.
Bounds are pose_reference.FACTOR x the float32 restatement's deviation from the float64 one (tools/measure_unbounded_deviations.py ->
profiles/r27_unbounded_deviations.json)."""
import json
import os

import torch

from oracle import kplanes_oracle as KO
from tests import pose_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVIATIONS = os.path.join(ROOT, "profiles", "r27_unbounded_deviations.json")
FACTOR = PR.FACTOR
RAY_SHAPES = ((1, 1), (5, 7), (3, 32), (2, 64), (129, 33))  # fused_reference.RAY_SHAPES without (37, 50): the shapes the issue names
TIE_MARGIN = 1e-3    # |pos_a| - |pos_b| of the two largest axes, relative to m: closer, and float32 may pick the other axis as the largest
FACE_MARGIN = 1e-3   # |m - 1|: closer, and float32 may take the other branch of the contraction
KEEP_SHARE = 7.0 / 8.0


def load_bounds():
    with open(DEVIATIONS) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------------------------------
# the arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def positions(o, d, ebins):
    """Frustums.get_positions: o + (d * (e[s] + e[s+1])) / 2, [R,S,3], in the dtype of the inputs and in that operation order."""
    mid = ebins[:, :-1] + ebins[:, 1:]
    return o[:, None, :] + (d[:, None, :] * mid[:, :, None]) / 2


def contract_half(pos):
    """SceneContraction(order=inf) and the halving: m = max_k |pos_k|; where(m < 1, pos, (2 - 1/m) * (pos / m)) / 2.  m == 1 takes the second
    branch.  Written out (not a call into the package or the oracle), operation by operation as the kernel evaluates it."""
    m = pos.abs().max(dim=-1, keepdim=True).values
    y = torch.where(m < 1, pos, (2 - 1 / m) * (pos / m))
    return y / 2


def points(o, d, ebins, times, n_coords=4):
    """The coordinates the planes see at contract = 1, [R*S, n_coords]: contract_half(positions) and t = 2 * time - 1."""
    p = contract_half(positions(o, d, ebins))
    R, S = p.shape[:2]
    if n_coords == 3:
        return p.reshape(-1, 3)
    t = times.reshape(R, 1, 1) * 2 - 1
    return torch.cat([p, t.expand(R, S, 1)], dim=-1).reshape(-1, 4)


def contract_half_vjp(pos, g):
    """g = d L / d p (p = contract_half(pos)), [...,3] -> d L / d pos: the Jacobian transposed.  Inside: g / 2.  Outside, with j the FIRST index
    whose |pos_j| equals m: (a g_k + [k == j] b sum_i pos_i g_i) / 2, a = 2/m - 1/m^2, b = (-2/m^2 + 2/m^3) sign(pos_j)."""
    ab = pos.abs()
    m = ab.max(dim=-1, keepdim=True).values
    j = (ab == m).to(torch.int64).argmax(dim=-1, keepdim=True)  # argmax of a 0/1 tensor: the first maximal index
    onehot = torch.zeros_like(pos).scatter_(-1, j, 1.0)
    sign = torch.where(torch.gather(pos, -1, j) < 0, -torch.ones_like(m), torch.ones_like(m))
    a = 2 / m - 1 / (m * m)
    b = (-2 / (m * m) + 2 / (m * m * m)) * sign
    dot = (pos * g).sum(-1, keepdim=True)
    out = (a * g + onehot * b * dot) / 2
    return torch.where(m < 1, g / 2, out)


def near_far(R, near_plane, far_plane, training, dtype=torch.float32):
    """NearFarCollider (scene_colliders.py:170-188): near_plane in training, 0 otherwise; far_plane.  [R,1] each."""
    ones = torch.ones(R, 1, dtype=dtype)
    return ones * (near_plane if training else 0.0), ones * far_plane


# ------------------------------------------------------------------------------------------------------------------------------------
# equality cases: dyadic rays with planted categories
# ------------------------------------------------------------------------------------------------------------------------------------
def planted_points():
    """[(category, position)]: dyadic positions, one or more per category."""
    out = [("inside", (0.25, -0.5, 0.125)), ("inside", (0.0, 0.0, 0.0)),
           ("face", (1.0, 0.5, -0.25)), ("face", (-0.5, -1.0, 0.75)), ("face", (0.25, 0.125, 1.0))]
    for k in range(3):
        for s in (1.0, -1.0):
            p = [0.5, -0.25, 0.75]
            p[k] = 1.5 * s
            out.append((f"outside-axis{k}{'+' if s > 0 else '-'}", tuple(p)))
    out += [("tie", (2.0, 2.0, 0.5)), ("tie", (-3.0, 0.25, 3.0)), ("tie", (0.5, -1.5, -1.5)), ("tie", (1.0, -1.0, 0.5))]
    for k in range(1, 11):
        p = [0.375 * (k % 4), -1.25, 0.5 * k]
        p[k % 3] = float(2 ** k) * (1.0 if k % 2 else -1.0)
        out.append((f"pow2-{k}", tuple(p)))
    return out


CATEGORIES = sorted({c for c, _ in planted_points()})
_DIRS = (1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.0, 2.0, -2.0)


def coordinate_rounds(R, S, n_coords=4, seed=0):
    """A case of the equality tests: a list of ray sets of shape (R, S), float32 on the CPU, each a dict(origins, dirs, ebins, times, planted)
    with planted = [(ray, sample, category)].  Bin edges e[s] = s / 4 (sample centres (2 s + 1) / 8), directions from a small dyadic set and
    origins chosen so that sample r % S of ray r IS the planted position: every value is dyadic and every product and sum below is exact in
    float32.  Asserts that the case holds every category, checked on the float32 positions themselves."""
    gen = torch.Generator().manual_seed(9000 + 131 * R + S + seed)
    pl = planted_points()
    n_rounds = max(1, -(-len(pl) // R))
    rounds, seen = [], set()
    eb = (torch.arange(S + 1, dtype=torch.float32) / 4).expand(R, S + 1).contiguous()
    centre = (2 * torch.arange(S, dtype=torch.float32) + 1) / 8
    for k in range(n_rounds):
        d = torch.tensor(_DIRS)[torch.randint(0, len(_DIRS), (R, 3), generator=gen)]
        o = torch.zeros(R, 3)
        planted = []
        for r in range(R):
            cat, P = pl[(k * R + r) % len(pl)]
            s = r % S
            o[r] = torch.tensor(P) - d[r] * centre[s]
            planted.append((r, s, cat))
        times = torch.randint(0, 9, (R,), generator=gen).float() / 8  # dyadic: 2 t - 1 is exact
        pos = positions(o, d, eb)
        for r, s, cat in planted:
            P = torch.tensor(pl[(k * R + r) % len(pl)][1])
            assert torch.equal(pos[r, s], P), f"({R},{S}) round {k}: planted sample ({r},{s}) is {pos[r, s].tolist()}, not {P.tolist()}"
            _assert_category(cat, pos[r, s])
            seen.add(cat)
        assert torch.equal(pos.double(), positions(o.double(), d.double(), eb.double())), "the dyadic positions are not exact in float32"
        rounds.append(dict(origins=o, dirs=d, ebins=eb, times=times, planted=planted))
    assert seen == set(CATEGORIES), f"({R},{S}): categories missing from the case: {sorted(set(CATEGORIES) - seen)}"
    return rounds


def _assert_category(cat, p):
    ab = p.abs()
    m = float(ab.max())
    if cat == "inside":
        assert m < 1
    elif cat == "face":
        assert m == 1.0
    elif cat.startswith("outside-axis"):
        k, s = int(cat[12]), cat[13]
        assert m > 1 and int(ab.argmax()) == k and (float(p[k]) > 0) == (s == "+") and int((ab == m).sum()) == 1
    elif cat == "tie":
        assert int((ab == m).sum()) == 2 and m >= 1
    else:
        k = int(cat.split("-")[1])
        assert m == float(2 ** k)


def expected_points(rs, n_coords=4):
    """The float32 points of a ray set, computed on the CPU through the PACKAGE's SceneContraction module (spatial_distortions.py): the
    independent side of the equality.  [R*S, n_coords]."""
    from soccernerfs_amd.spatial_distortions import SceneContraction

    pos = rs["origins"][:, None, :] + (rs["dirs"][:, None, :] * (rs["ebins"][:, :-1] + rs["ebins"][:, 1:])[:, :, None]) / 2
    p = SceneContraction(order=float("inf"))(pos) / 2
    R, S = p.shape[:2]
    if n_coords == 3:
        return p.reshape(-1, 3).contiguous()
    t = rs["times"].reshape(R, 1, 1) * 2 - 1
    return torch.cat([p, t.expand(R, S, 1)], dim=-1).reshape(-1, 4).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------
# gradient cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _gcase(R, S, C, mult, base, seed):
    return dict(R=R, S=S, C=C, mult=tuple(mult), base=tuple(base), concat=int(len(mult) > 1), seed=seed, mode=1, N=R * S, rescale=1)


# R in {1, 5} x S in {1, 7, 64, 65}; C 8 and 32; one and two scales; six and three planes
GRAD_CASES = [
    _gcase(1, 1, 8, (1,), (12, 10, 8, 3), 1), _gcase(1, 7, 32, (1, 2), (8, 8, 8, 4), 2), _gcase(1, 64, 8, (1, 2), (9, 7, 5), 3),
    _gcase(1, 65, 32, (1,), (16, 12, 9), 4), _gcase(5, 1, 32, (1, 2), (6, 5, 4), 5), _gcase(5, 7, 8, (1,), (10, 9, 8), 6),
    _gcase(5, 64, 32, (1, 2), (8, 6, 7, 3), 24), _gcase(5, 65, 8, (1, 2), (12, 12, 12, 4), 37), _gcase(5, 64, 8, (1,), (24, 24, 24, 4), 20),
    _gcase(5, 65, 32, (1, 2), (16, 16, 16, 4), 10),
]


def grad_case_id(c):
    return f"R{c['R']}-S{c['S']}-C{c['C']}-s{len(c['mult'])}-nc{len(c['base'])}-res" + "x".join(map(str, c["base"]))


def make_gradient_case(c):
    """Planes, upstream gradient and rays (float32, CPU).  Each ray starts inside the unit cube and leaves it: its samples are spread from the
    origin to 2^u (u uniform in [0, 5]) along the ray, so that inside and outside samples with every axis largest occur (asserted over the case
    set by the CPU test; a one-sample case cannot hold them all)."""
    gen = torch.Generator().manual_seed(7700 + c["seed"])
    d = PR.make_coords_case(dict(c, seed=500 + c["seed"]))
    R, S = c["R"], c["S"]
    d["origins"] = torch.rand(R, 3, generator=gen) * 1.2 - 0.6
    d["dirs"] = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    far = 2.0 ** (torch.rand(R, 1, generator=gen) * 5)
    d["ebins"] = torch.sort(torch.rand(R, S + 1, generator=gen), dim=-1).values ** 2 * far
    d["times"] = torch.rand(R, generator=gen)
    return d


def grad_points(c, d, dtype):
    return points(d["origins"].to(dtype), d["dirs"].to(dtype), d["ebins"].to(dtype), d["times"].to(dtype), len(c["base"]))


def grad_reference(c, d, dtype):
    """(grad_pts [N,nc], grad_origins [R,3], grad_dirs [R,3]) in `dtype`: autograd through the interpolation for d / d p, then the restated
    Jacobian and the sums over the ray's samples (bin edges constant)."""
    pts = grad_points(c, d, dtype).detach().requires_grad_(True)
    planes = [[p.to(dtype) for p in g] for g in d["planes"]]
    out = PR.interpolate(pts, planes, d["combs"], bool(c["concat"]))
    (out * d["gout"].to(dtype)).sum().backward()
    gp = pts.grad.detach()
    R, S = c["R"], c["S"]
    pos = positions(d["origins"].to(dtype), d["dirs"].to(dtype), d["ebins"].to(dtype))
    h = contract_half_vjp(pos, gp[:, :3].reshape(R, S, 3))
    e = d["ebins"].to(dtype)
    tmid = ((e[:, :-1] + e[:, 1:]) / 2)[:, :, None]
    return gp, h.sum(1), (tmid * h).sum(1)


def level_ray_gradient(o, d, ebins, times, planes, combs, concat, gfeat, dtype):
    """(grad_origins, grad_dirs) [R,3] of one sampling level in `dtype`, for a given upstream feature gradient gfeat [R*S, W]: autograd
    through the interpolation at the contracted points, the restated Jacobian, the sums over the ray (bin edges constant).  planes: list over
    scales of the reference-layout planes; six or three per scale (combs)."""
    o, d, ebins, times = (x.to(dtype) for x in (o, d, ebins, times))
    nc = 4 if len(combs) == 6 else 3
    pts = points(o, d, ebins, times, nc).detach().requires_grad_(True)
    out = PR.interpolate(pts, [[p.to(dtype) for p in g] for g in planes], combs, concat)
    (out * gfeat.to(dtype)).sum().backward()
    R, S = ebins.shape[0], ebins.shape[1] - 1
    h = contract_half_vjp(positions(o, d, ebins), pts.grad[:, :3].reshape(R, S, 3))
    tmid = ((ebins[:, :-1] + ebins[:, 1:]) / 2)[:, :, None]
    return h.sum(1), (tmid * h).sum(1)


def grad_comparable(c, d):
    """bool [N]: samples outside every margin -- TIE_MARGIN (relative gap of the two largest |pos_k|), FACE_MARGIN (|m - 1|) and
    pose_reference.LATTICE_MARGIN texels from every lattice line of every scale.  Evaluated in float64."""
    pos = positions(d["origins"].double(), d["dirs"].double(), d["ebins"].double()).reshape(-1, 3)
    ab = pos.abs().sort(dim=-1, descending=True).values
    m = ab[:, 0]
    ok = ((ab[:, 0] - ab[:, 1]) > TIE_MARGIN * m.clamp(min=1e-30)) | (m < 1 - FACE_MARGIN)  # a tie inside the cube changes nothing
    ok &= (m - 1).abs() > FACE_MARGIN
    pts = grad_points(c, d, torch.float64)
    for reso in d["reso"]:
        for k, W in enumerate(reso):
            if W == 1:
                continue
            u = (pts[:, k] + 1) / 2 * (W - 1)
            ok &= ~(((u - torch.round(u)).abs() < PR.LATTICE_MARGIN) & (u > -PR.LATTICE_MARGIN) & (u < W - 1 + PR.LATTICE_MARGIN))
    return ok


def grad_rays_comparable(c, d):
    """bool [R]: rays all of whose samples are comparable (a ray sum holds every sample of the ray).  The seeds of GRAD_CASES are chosen so
    that this is every ray of every case (tests/test_unbounded_cpu.py asserts it): no sample is left out of the ray comparison."""
    return grad_comparable(c, d).reshape(c["R"], c["S"]).all(dim=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# three training steps of the unbounded model, restated (the yardstick of the trainer comparison)
# ------------------------------------------------------------------------------------------------------------------------------------
STEP_E = dict(base_res=(16, 16, 16, 4), multiscale=(1, 2), feat_dim=32, prop_res=((24, 24, 24, 4), (32, 32, 32, 4)), prop_feat=8, sigma_hidden=128,
              color_hidden=64, aabb_scale=1.5, seed=5)
STEP_SAMPLES = ((64, 32), 16)
STEP_NEAR, STEP_FAR, STEP_R = 0.05, 24.0, 256
STEP_TOLERANCES = {"rgb": 1e-6, "loss": 1e-6, "param": 3e-7}  # the bounded comparison's (tests/test_gpu_view_dependent.py): the floor of a bound


def step_rays(R, seed, S=STEP_SAMPLES):
    """(rays, target, rng) on the CPU.  Half of the rays start inside the unit cube; the others start outside the sphere of radius sqrt(3)
    around it and point away from the origin: they never meet the cube."""
    gen = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 0.9
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    away = torch.nn.functional.normalize(torch.randn(R // 2, 3, generator=gen), dim=-1)
    o[R // 2:] = away * (1.8 + 2.0 * torch.rand(R // 2, 1, generator=gen))
    d[R // 2:] = torch.nn.functional.normalize(away + 0.3 * (torch.rand(R // 2, 3, generator=gen) * 2 - 1), dim=-1)  # |offset| <= 0.52 < 1
    assert bool(((o[R // 2:] * d[R // 2:]).sum(-1) > 0).all()) and float(o[R // 2:].norm(dim=-1).min()) > 1.74  # > sqrt(3): outside, leaving
    t, target = torch.rand(R, 1, generator=gen), torch.rand(R, 3, generator=gen)
    (S0, S1), S2 = S
    rng = {"t_rand": torch.rand(R, S0 + 1, generator=gen), "u": [torch.rand(R, S1 + 1, generator=gen), torch.rand(R, S2 + 1, generator=gen)],
           "bg": torch.rand(R, 3, generator=gen)}
    return {"origins": o, "directions": d, "times": t}, target, rng


def forward_unbounded(P, rays, rng, num_proposal_samples, num_nerf_samples, anneal, near, far):
    """KO.kplanes_forward's statements (training) for bounded = False: NearFarCollider constants, the piecewise spacing, and every field fed
    contract_half(positions) -- through the oracle's field functions on the box [-1, 1]^3, whose normalisation is then the identity (the
    density field's [0, 1] quirk undone by 2 p - 1 first, as tests/test_oracle_golden.py does for the reference's recording)."""
    o, d, times = rays["origins"], rays["directions"], rays["times"]
    R = o.shape[0]
    unit = torch.tensor([[-1.0] * 3, [1.0] * 3], dtype=o.dtype)
    nears, fars = torch.full((R, 1), near, dtype=o.dtype), torch.full((R, 1), far, dtype=o.dtype)
    levels = list(num_proposal_samples) + [num_nerf_samples]
    weights_list, sdist_list = [], []
    weights = bins = None
    for li, S in enumerate(levels):
        if li == 0:
            bins = KO.spaced_bins(R, S, rng["t_rand"])
        else:
            bins, _, _ = KO.pdf_sample(torch.pow(weights, anneal), bins, KO.pdf_u(R, S, rng["u"][li - 1]))
        eucl = KO.spacing_to_euclidean(bins, nears, fars, kind="piecewise")
        starts, ends = eucl[:, :-1], eucl[:, 1:]
        p = contract_half(KO.sample_positions(o, d, starts, ends))
        if li < len(levels) - 1:
            dens = KO.density_field_forward(2 * p - 1, times, unit, P["prop_grids"][li], P["prop_sigma"][li])
            weights = KO.get_weights(ends - starts, dens)
            weights_list.append(weights)
            sdist_list.append(bins)
    density, rgb = KO.field_forward(p, times, unit, P["field_grids"], P["field_sigma"], P["field_color"])
    weights = KO.get_weights(ends - starts, density)
    weights_list.append(weights)
    sdist_list.append(bins)
    return {"rgb": KO.render_rgb(rgb, weights, rng["bg"], True), "weights_list": weights_list, "sdist_list": sdist_list}


def three_steps(dtype, steps=3, lr=1e-2, warm_up_end=1, max_steps=1000):
    """`steps` training steps (forward, the loss dict, autograd, Adam with eps 1e-12 on every tensor, the trainer test's schedule) in `dtype`
    on the CPU.  Returns {"rgb": [per step], "loss": [per step {term: value}], "params": [final tensors]}."""
    P = PR._cast(KO.make_kplanes_params(**STEP_E), dtype)
    leaves = KO.all_param_tensors(P)
    for x in leaves:
        x.requires_grad_(True)
    m, v = [torch.zeros_like(x) for x in leaves], [torch.zeros_like(x) for x in leaves]
    out = {"rgb": [], "loss": [], "params": None}
    for step in range(steps):
        rays, target, rng = PR._cast(list(step_rays(STEP_R, 20 + step)), dtype)
        f = forward_unbounded(P, rays, rng, STEP_SAMPLES[0], STEP_SAMPLES[1], KO.anneal_value(step, 1000, 10.0), STEP_NEAR, STEP_FAR)
        ld = KO.kplanes_loss_dict(P, f, target)
        for x in leaves:
            x.grad = None
        sum(ld.values()).backward()
        out["rgb"].append(f["rgb"].detach().clone())
        out["loss"].append({k: float(val.detach()) for k, val in ld.items()})
        with torch.no_grad():
            for x, mm, vv in zip(leaves, m, v):
                KO.adam_step(x, x.grad, mm, vv, step + 1, lr * KO.cosine_lr_factor(step, warm_up_end, max_steps, 0.0))
    out["params"] = [x.detach().clone() for x in leaves]
    return out


def three_steps_deviation():
    """float32 against float64 restatement of the three steps: {"rgb": max abs, "loss": max relative over the terms, "param": max relative L2
    over the tensors}."""
    a, b = three_steps(torch.float32), three_steps(torch.float64)
    rgb = max(float((x.double() - y).abs().max()) for x, y in zip(a["rgb"], b["rgb"]))
    loss = max(abs(x[k] - y[k]) / abs(y[k]) for x, y in zip(a["loss"], b["loss"]) for k in y if abs(y[k]) > 1e-9)
    param = max(float((x.double() - y).norm() / (y.norm() + 1e-30)) for x, y in zip(a["params"], b["params"]))
    return {"rgb": rgb, "loss": loss, "param": param}

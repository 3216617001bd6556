"""Reference side of the camera-optimiser tests (tests/test_pose_cpu.py, test_gpu_kplanes_coords.py, test_gpu_pose.py) -- test infrastructure.

Everything here is a torch restatement that runs in float64 (the reference of a comparison) or in float32 (the yardstick: a bound is 5 x the
float32 restatement's deviation from the float64 one on the same inputs, relative to the output's largest magnitude; measured once on the CPU
by tools/measure_pose_deviations.py into profiles/r15_pose_deviations.json, which the GPU tests read).  The chain is composed from
oracle/kplanes_oracle.py's functions; the pose algebra (Rodrigues' formula with the reference's floor on the angle, pose composition) is written
in its own form and pinned against values recorded from the reference (tests/golden/g19_pose.npz).

ONE difference from the reference's autograd, on purpose (include/snerf.h): nears / fars -- and with them every bin edge --
are DETACHED from the rays (detach_bins=True), because the kernels hold the bin edges constant.  detach_bins=False is the reference's full
gradient, used only to record how large the omitted term is."""
import itertools
import json
import os

import numpy as np
import torch

from oracle import kplanes_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVIATIONS = os.path.join(ROOT, "profiles", "r15_pose_deviations.json")
FACTOR = 5.0  # bound = FACTOR x the float32 restatement's deviation (the factor of the kernels whose arithmetic order differs from torch's)


def load_bounds():
    with open(DEVIATIONS) as f:
        return json.load(f)


def rel_dev(got, want) -> float:
    """max |got - want| / max |want| (0 / 0 = 0)."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    return 0.0 if err == 0.0 else err / max(scale, 1e-300)


# ------------------------------------------------------------------------------------------------------------------------------------
# pose algebra
# ------------------------------------------------------------------------------------------------------------------------------------
def pose_delta_transform(delta):
    """The rigid transform a pose row stands for (what NS/cameras/lie_groups.py:23-58 computes; pinned by tests/golden/g19_pose.npz): delta
    [b,6] = (shift, axis vector w) -> [b,3,4] = [Rot(w) | shift].  Rodrigues' formula written with cross products,
        Rot(w) = I + a [w]x + b (w w^T - |w|^2 I),   a = sin(th) / th,   b = (1 - cos(th)) / th^2,
    where th = sqrt(max(|w|^2, 1e-4)): below that floor the reference's angle is held at 0.01 while the axis vector keeps its length, so the
    result is not exactly a rotation there, and a and b do not depend on w."""
    shift, w = delta[:, :3], delta[:, 3:]
    sq = (w * w).sum(-1)
    th = torch.sqrt(torch.clamp(sq, min=1e-4))
    a, b = torch.sin(th) / th, (1.0 - torch.cos(th)) / (th * th)
    eye = torch.eye(3, dtype=delta.dtype)
    # column j of [w]x is w x e_j
    cross = torch.stack([torch.linalg.cross(w, eye[j].expand_as(w), dim=-1) for j in range(3)], dim=-1)
    second = w[:, :, None] * w[:, None, :] - sq[:, None, None] * eye
    rot = eye + a[:, None, None] * cross + b[:, None, None] * second
    return torch.cat([rot, shift[:, :, None]], dim=-1)


def compose_poses(left, right):
    """[Ra | ta] followed on the right by [Rb | tb], for [...,3,4] poses: [Ra Rb | ta + Ra tb] (what NS/utils/poses.py:53-67 returns)."""
    rot = torch.einsum("...ij,...jk->...ik", left[..., :, :3], right[..., :, :3])
    pos = left[..., :, 3] + torch.einsum("...ij,...j->...i", left[..., :, :3], right[..., :, 3])
    return torch.cat([rot, pos[..., None]], dim=-1)


def adjusted_c2w(c2w, adj, groups=None):
    """The whole table with its pose rows applied on the right, as NS/cameras/cameras.py:707-708 applies them: camera m takes row groups[m]."""
    rows = adj if groups is None else adj[groups]
    return compose_poses(c2w, pose_delta_transform(rows))


def rays_from_directions(v, cam, c2w_adj):
    """Camera-space directions v [R,3] of rays of cameras cam [R] -> world origins and normalised directions (cameras.py:704-717)."""
    m = c2w_adj[cam]
    w = (v[:, None, :] * m[:, :3, :3]).sum(-1)
    n = torch.clamp(torch.linalg.norm(w, dim=-1, keepdim=True), min=float(np.finfo(np.float64).eps * 4))
    return m[:, :3, 3], w / n


# ------------------------------------------------------------------------------------------------------------------------------------
# coordinate gradient of the plane gather
# ------------------------------------------------------------------------------------------------------------------------------------
def _case(C, mult, concat, base, mode, R=0, S=0, rescale=1, N=0, seed=0):
    return dict(C=C, mult=tuple(mult), concat=int(concat), base=tuple(base), mode=mode, R=R, S=S, rescale=int(rescale),
                N=N if mode == 0 else R * S, seed=seed)


# C in {8,16,32} x scales in {1,2,5} x concat/sum x n_coords 3/4 x rescale 0/1 x S in {1,31,32,64,320} x R in {1,3,65,130}, resolutions from 1
# and 2 up to 64: every value of every axis occurs, in both coordinate modes; no full product (each case costs a float64 autograd on the CPU)
COORDS_CASES = [
    _case(8, (1,), 0, (24, 24, 24, 4), 1, R=65, S=64, rescale=0, seed=1),            # a proposal level's shape
    _case(8, (1,), 0, (32, 32, 32, 4), 1, R=3, S=320, rescale=0, seed=2),
    _case(8, (1,), 0, (16, 12, 9, 3), 1, R=130, S=320, rescale=1, seed=3),           # the largest: 41600 samples
    _case(32, (1, 2, 4, 8, 16), 1, (4, 4, 4, 2), 1, R=65, S=64, rescale=1, seed=4),  # the field's shape, resolutions up to 64
    _case(32, (1, 2), 1, (16, 16, 16, 4), 1, R=130, S=31, rescale=1, seed=5),
    _case(16, (1, 2), 1, (5, 7, 3, 2), 1, R=3, S=32, rescale=1, seed=6),
    _case(16, (1, 2, 3, 4, 5), 0, (3, 2, 5, 1), 1, R=130, S=1, rescale=1, seed=7),   # a time axis of resolution 1
    _case(8, (1, 2), 1, (9, 6, 2), 1, R=65, S=32, rescale=1, seed=8),                # static scene, three planes
    _case(32, (1,), 0, (1, 8, 8), 1, R=1, S=1, rescale=0, seed=31),                   # one sample; an x axis of resolution 1
    _case(16, (1, 2, 4, 8, 16), 1, (4, 3, 2), 1, R=1, S=320, rescale=0, seed=10),
    _case(32, (1, 2, 4, 8, 16), 0, (2, 2, 2, 2), 1, R=3, S=31, rescale=1, seed=11),
    _case(16, (1, 2), 0, (8, 8, 8, 4), 1, R=65, S=1, rescale=0, seed=12),
    _case(8, (1,), 0, (6, 6, 6, 2), 0, N=1, seed=13),
    _case(8, (1, 2), 1, (12, 10, 8, 3), 0, N=4030, seed=14),
    _case(16, (1, 2, 4, 8, 16), 1, (4, 4, 4, 3), 0, N=2080, seed=15),
    _case(32, (1,), 1, (7, 5, 3), 0, N=3, seed=16),
    _case(32, (1, 2), 0, (32, 24, 17, 7), 0, N=4160, seed=17),
    _case(16, (1,), 0, (9, 9, 9), 0, N=129, seed=18),                                # not a multiple of a wavefront's block of samples
    _case(8, (1, 2, 4, 8, 16), 0, (4, 4, 4), 0, N=257, seed=29),
    _case(32, (1, 2, 4, 8, 16), 1, (4, 4, 4, 1), 0, N=67, seed=20),
]
AABB = ((-1.5, -1.0, -0.5), (1.5, 2.0, 1.0))  # deliberately not a cube: one scale factor per axis
LATTICE_MARGIN = 1e-4  # texels: closer to an integer (or a clamp end) than this, the bilinear slope may be taken from the neighbouring cell
OUTSIDE_MARGIN = 1e-4  # normalised units beyond +-1 from where a coordinate's gradient must be exactly 0


def case_id(c) -> str:
    return (f"C{c['C']}-s{len(c['mult'])}-{'cat' if c['concat'] else 'sum'}-nc{len(c['base'])}-" +
            (f"rays-R{c['R']}-S{c['S']}-rs{c['rescale']}" if c["mode"] == 1 else f"pts-N{c['N']}") + "-res" + "x".join(map(str, c["base"])))


def case_resolutions(c):
    nc = len(c["base"])
    return [[r * m for r in c["base"][:3]] + list(c["base"][3:]) for m in c["mult"]] if nc == 4 else [[r * m for r in c["base"]] for m in c["mult"]]


def make_coords_case(c):
    """Inputs of one case, float32 on the CPU: planes in the reference layout (list over scales of [1,C,H,W], time planes random too), the
    upstream gradient, and the points [N,nc] in [-1.25, 1.25] (mode 0) or rays whose samples partly leave the box (mode 1)."""
    gen = torch.Generator().manual_seed(1000 + c["seed"])
    nc = len(c["base"])
    combs = list(itertools.combinations(range(nc), 2))
    reso = case_resolutions(c)
    planes = [[torch.rand(1, c["C"], r[b], r[a], generator=gen) * 0.8 + 0.2 for (a, b) in combs] for r in reso]
    N = c["N"]
    out_w = c["C"] * len(reso) if c["concat"] else c["C"]
    d = {"planes": planes, "gout": torch.randn(N, out_w, generator=gen), "reso": reso, "combs": combs}
    if c["mode"] == 0:
        d["pts"] = torch.rand(N, nc, generator=gen) * 2.5 - 1.25
    else:
        R, S = c["R"], c["S"]
        lo, hi = torch.tensor(AABB[0]), torch.tensor(AABB[1])
        d["origins"] = lo + (hi - lo) * (torch.rand(R, 3, generator=gen) * 1.1 - 0.05)
        d["dirs"] = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
        d["times"] = torch.rand(R, generator=gen) * 1.2 - 0.1
        d["ebins"] = torch.sort(torch.rand(R, S + 1, generator=gen) * 2.5, dim=-1).values
    return d


def case_points(c, d, dtype):
    """The [-1,1] coordinates the planes see, [N,nc], in `dtype`: the points themselves, or Frustums.get_positions +
    SceneBox.get_normalized_positions + the rescale and the time map of the fields (oracle functions)."""
    if c["mode"] == 0:
        return d["pts"].to(dtype)
    o, dr, e, t = (d[k].to(dtype) for k in ("origins", "dirs", "ebins", "times"))
    aabb = torch.tensor(AABB, dtype=dtype)
    pos = KO.sample_positions(o, dr, e[:, :-1], e[:, 1:])
    p = KO.normalize_positions(pos, aabb)
    if c["rescale"]:
        p = p * 2.0 - 1.0
    if len(c["base"]) == 3:
        return p.reshape(-1, 3)
    tt = (t * 2) - 1
    return torch.cat([p, tt[:, None, None].expand(p.shape[0], p.shape[1], 1)], dim=-1).reshape(-1, 4)


def interpolate(pts, planes, combs, concat):
    """interpolate_kplanes (kplanes_field.py:77-126) for 6 or 3 planes: the oracle's bilinear_plane, product over planes, concat / sum."""
    outs = []
    for grids in planes:
        prod = 1.0
        for ci, comb in enumerate(combs):
            prod = prod * KO.bilinear_plane(grids[ci], pts[:, list(comb)])
        outs.append(prod)
    return torch.cat(outs, dim=-1) if concat else sum(outs)


def coords_gradient(c, d, dtype):
    """autograd's d(sum gout . interpolate(pts)) / d pts, [N,nc], evaluated in `dtype`."""
    pts = case_points(c, d, dtype).detach().requires_grad_(True)
    planes = [[p.to(dtype) for p in g] for g in d["planes"]]
    out = interpolate(pts, planes, d["combs"], bool(c["concat"]))
    (out * d["gout"].to(dtype)).sum().backward()
    return pts.grad.detach()


def comparable_samples(c, d):
    """bool [N]: samples whose float64 unnormalised coordinate is more than LATTICE_MARGIN texels from every integer and clamp end on every
    axis of every scale -- elsewhere float32 and float64 may take different bilinear cells, whose slopes differ.  An axis of resolution 1 has
    the unnormalised coordinate 0 for every input and the slope 0 on both sides: it excludes nothing."""
    pts = case_points(c, d, torch.float64)
    ok = torch.ones(pts.shape[0], dtype=torch.bool)
    for reso in d["reso"]:
        for k, W in enumerate(reso):
            if W == 1:
                continue
            u = (pts[:, k] + 1) / 2 * (W - 1)
            near = ((u - torch.round(u)).abs() < LATTICE_MARGIN) & (u > -LATTICE_MARGIN) & (u < W - 1 + LATTICE_MARGIN)
            ok &= ~near
    return ok


def outside_axes(c, d):
    """bool [N,nc]: coordinates beyond +-(1 + OUTSIDE_MARGIN) -- clipped at every scale, so their gradient must be exactly 0."""
    return case_points(c, d, torch.float64).abs() > 1 + OUTSIDE_MARGIN


def ray_sums(c, d, grad_pts):
    """float64 reduction of a [N,nc] per-point gradient to the rays: (g_origins, g_dirs, bound) with bound [R,3] the recursive-summation
    error bound (S + 4) 2^-24 k sum_s |term| of float32 sums (Higham, gamma_n ~ n u; +4 for the scale and the bin-centre roundings)."""
    R, S = c["R"], c["S"]
    g = grad_pts.double().reshape(R, S, -1)[:, :, :3]
    e = d["ebins"].double()
    tmid = ((e[:, :-1] + e[:, 1:]) / 2)[:, :, None]
    k = (2.0 if c["rescale"] else 1.0) / (torch.tensor(AABB[1]).double() - torch.tensor(AABB[0]).double())
    u = (S + 4) * 2.0 ** -24
    go, gd = k * g.sum(1), k * (tmid * g).sum(1)
    return go, gd, (u * k * g.abs().sum(1), u * k * (tmid * g).abs().sum(1))


# ------------------------------------------------------------------------------------------------------------------------------------
# pose backward of the ray generation
# ------------------------------------------------------------------------------------------------------------------------------------
POSE_TABLES = ("perspective", "perspective_lens", "fisheye", "equirectangular", "mixed")
POSE_R, POSE_M = 257, 5


def make_pose_table(kind: str, seed: int = 0):
    """A table of POSE_M cameras on a ring looking at the origin, POSE_R random pixels, random ray gradients; numpy float64 / int64."""
    rs = np.random.RandomState(4200 + seed + POSE_TABLES.index(kind))
    M, R, H, W = POSE_M, POSE_R, 48, 64
    c2w = np.zeros((M, 3, 4))
    for m in range(M):
        ang = 2 * np.pi * m / M + 0.3
        pos = np.array([3.0 * np.cos(ang), 3.0 * np.sin(ang), 0.8 + 0.2 * m])
        back = pos / np.linalg.norm(pos)  # the camera looks along -z
        right = np.cross(np.array([0.0, 0.0, 1.0]), back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        c2w[m, :, 0], c2w[m, :, 1], c2w[m, :, 2], c2w[m, :, 3] = right, up, back, pos
    c2w = c2w.astype(np.float32).astype(np.float64)
    types = {"perspective": [1] * M, "perspective_lens": [1] * M, "fisheye": [2] * M, "equirectangular": [3] * M, "mixed": [1, 2, 3, 1, 2]}[kind]
    types = np.array(types, np.int32)
    fx = np.where(types == 1, 70.0, np.where(types == 2, 40.0, float(W))) + rs.rand(M)
    fy = np.where(types == 1, 70.0, np.where(types == 2, 40.0, float(H))) + rs.rand(M)
    fx, fy = fx.astype(np.float32).astype(np.float64), fy.astype(np.float32).astype(np.float64)
    cx, cy = np.full(M, W / 2 + 0.25), np.full(M, H / 2 - 0.25)
    dist = None
    if kind in ("perspective_lens", "mixed"):
        dist = (rs.rand(M, 6) - 0.5) * np.array([0.1, 0.02, 0.0, 0.0, 0.004, 0.004])
        dist = dist.astype(np.float32).astype(np.float64)
    idx = np.stack([rs.randint(0, M, R), rs.randint(0, H, R), rs.randint(0, W, R)], -1).astype(np.int64)
    return dict(kind=kind, M=M, R=R, c2w=c2w, fx=fx, fy=fy, cx=cx, cy=cy, types=types, distortion=dist, indices=idx,
                g_o=rs.randn(R, 3).astype(np.float32).astype(np.float64), g_d=rs.randn(R, 3).astype(np.float32).astype(np.float64))


def pose_adjustments(G: int, seed: int, above_clamp: bool):
    """[G,6] float32: |w| ~ 3e-3 (|w|^2 < 1e-4: the clamp is active) or ~ 0.2 (above it)."""
    gen = torch.Generator().manual_seed(77 + seed)
    a = torch.randn(G, 6, generator=gen)
    a[:, :3] *= 0.05
    a[:, 3:] *= 0.12 if above_clamp else 0.002
    return a


POSE_GROUPS = {"identity": None, "two_groups": [0, 1, 0, 1, 1]}


def camera_space_directions(t):
    """float64 camera-space directions [R,3] of the table's rays (tests/camera_types_reference.py: lens and camera types), a constant of the pose."""
    from tests import camera_types_reference as CT

    out = CT.generate_rays(t["indices"], t["fx"], t["fy"], t["cx"], t["cy"], t["c2w"], distortion=t["distortion"], camera_type=t["types"])
    kinds = t["types"][t["indices"][:, 0]]
    return CT.camera_directions(out["coords"], kinds)[0]


def pose_gradient(t, adj, groups, dtype):
    """autograd of raygen -> sum(g_o . o + g_d . d) with respect to the pose rows, in `dtype`: [G,6]."""
    v = torch.from_numpy(camera_space_directions(t)).to(dtype)
    adj = adj.to(dtype).clone().requires_grad_(True)
    g = None if groups is None else torch.as_tensor(groups, dtype=torch.long)
    c2w = adjusted_c2w(torch.from_numpy(t["c2w"]).to(dtype), adj, g)
    o, d = rays_from_directions(v, torch.from_numpy(t["indices"][:, 0]), c2w)
    ((torch.from_numpy(t["g_o"]).to(dtype) * o).sum() + (torch.from_numpy(t["g_d"]).to(dtype) * d).sum()).backward()
    return adj.grad.detach()


# ------------------------------------------------------------------------------------------------------------------------------------
# three joint training steps: the field's Adam and the poses' Adam
# ------------------------------------------------------------------------------------------------------------------------------------
# the smallest trainer-parity shape (tests/test_gpu_trainer.py::test_three_training_steps_match_oracle)
STEP_E = dict(base_res=(16, 16, 16, 4), multiscale=(1, 2), feat_dim=32, prop_res=((24, 24, 24, 4), (32, 32, 32, 4)), prop_feat=8,
              sigma_hidden=128, color_hidden=64, aabb_scale=1.5, seed=5)
STEP_R, STEP_S, STEP_M, STEP_HW = 40, ((64, 32), 16), 5, (24, 32)
STEP_GROUPS = [0, 1, 1, 2, 0]


def step_cameras():
    """STEP_M pinhole cameras around the box, float32 tensors: c2w [M,3,4], fx, fy, cx, cy, times [M]."""
    t = make_pose_table("perspective", seed=9)
    H, W = STEP_HW
    f32 = lambda a: torch.from_numpy(np.asarray(a)).float()
    return dict(c2w=f32(t["c2w"]), fx=torch.full((STEP_M,), 30.0), fy=torch.full((STEP_M,), 30.0), cx=torch.full((STEP_M,), W / 2.0),
                cy=torch.full((STEP_M,), H / 2.0), times=torch.linspace(0.1, 0.9, STEP_M))


def step_draws(step: int):
    """The batch of training step `step`: pixel indices, targets and the samplers' uniform draws (float32, CPU)."""
    gen = torch.Generator().manual_seed(500 + step)
    R, (S0, S1), S2 = STEP_R, STEP_S[0], STEP_S[1]
    H, W = STEP_HW
    idx = torch.stack([torch.randint(0, STEP_M, (R,), generator=gen), torch.randint(0, H, (R,), generator=gen),
                       torch.randint(0, W, (R,), generator=gen)], -1)
    return dict(indices=idx, target=torch.rand(R, 3, generator=gen),
                rng={"t_rand": torch.rand(R, S0 + 1, generator=gen), "u": [torch.rand(R, S1 + 1, generator=gen), torch.rand(R, S2 + 1, generator=gen)],
                     "bg": torch.rand(R, 3, generator=gen)})


def forward_detached(P, rays, rng, num_proposal_samples, num_nerf_samples, anneal, detach_bins=True):
    """KO.kplanes_forward's statements (training, proposal networks with gradients) with nears / fars detached from the rays."""
    aabb = P["aabb"]
    o, d, times = rays["origins"], rays["directions"], rays["times"]
    R = o.shape[0]
    nears, fars = KO.intersect_aabb(o, d, aabb, 0.0, True)
    if detach_bins:
        nears, fars = nears.detach(), fars.detach()
    levels = list(num_proposal_samples) + [num_nerf_samples]
    weights_list, sdist_list = [], []
    weights = bins = None
    for li, S in enumerate(levels):
        if li == 0:
            bins = KO.spaced_bins(R, S, rng["t_rand"])
        else:
            bins, _, _ = KO.pdf_sample(torch.pow(weights, anneal), bins, KO.pdf_u(R, S, rng["u"][li - 1]))
        eucl = KO.spacing_to_euclidean(bins, nears, fars)
        starts, ends = eucl[:, :-1], eucl[:, 1:]
        pos = KO.sample_positions(o, d, starts, ends)
        if li < len(levels) - 1:
            dens = KO.density_field_forward(pos, times, aabb, P["prop_grids"][li], P["prop_sigma"][li])
            weights = KO.get_weights(ends - starts, dens)
            weights_list.append(weights)
            sdist_list.append(bins)
    density, rgb = KO.field_forward(pos, times, aabb, P["field_grids"], P["field_sigma"], P["field_color"])
    weights = KO.get_weights(ends - starts, density)
    weights_list.append(weights)
    sdist_list.append(bins)
    return {"rgb": KO.render_rgb(rgb, weights, rng["bg"], True), "weights_list": weights_list, "sdist_list": sdist_list}


def _cast(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: _cast(v, dtype) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_cast(v, dtype) for v in x]
    return x


def three_steps(dtype, n_steps: int = 3, detach_bins: bool = True, groups=STEP_GROUPS):
    """n_steps joint steps in `dtype` on the CPU: rays from the adjusted pinhole table (KO.generate_rays_pinhole), the detached-bin forward,
    KO.kplanes_loss_dict, autograd, the field's Adam (lr 1e-2 with the cosine warm-up ending at step 2, as the parity test) and
    torch.optim.Adam(lr=6e-4, eps=1e-15) on the pose rows.  Returns per step: ray_grads (origins, directions), grad_pose, pose_adjustment."""
    P = _cast(KO.make_kplanes_params(**STEP_E), dtype)
    leaves = KO.all_param_tensors(P)
    for x in leaves:
        x.requires_grad_(True)
    ms, vs = [torch.zeros_like(x) for x in leaves], [torch.zeros_like(x) for x in leaves]
    cams = _cast(step_cameras(), dtype)
    g = None if groups is None else torch.as_tensor(groups, dtype=torch.long)
    G = STEP_M if groups is None else int(max(groups)) + 1
    adj = torch.zeros(G, 6, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([adj], lr=6e-4, eps=1e-15)
    out = []
    for step in range(n_steps):
        b = _cast(step_draws(step), dtype)
        c2w = adjusted_c2w(cams["c2w"], adj, g)
        rays = KO.generate_rays_pinhole(b["indices"], cams["fx"], cams["fy"], cams["cx"], cams["cy"], c2w, cams["times"])
        o, d = rays["origins"], rays["directions"]
        o.retain_grad()
        d.retain_grad()
        fwd = forward_detached(P, {"origins": o, "directions": d, "times": rays["times"]}, b["rng"], STEP_S[0], STEP_S[1],
                               KO.anneal_value(step, 1000, 10.0), detach_bins)
        loss = sum(KO.kplanes_loss_dict(P, fwd, b["target"]).values())
        for x in leaves:
            x.grad = None
        opt.zero_grad()
        loss.backward()
        rec = {"g_origins": o.grad.detach().clone(), "g_directions": d.grad.detach().clone(), "grad_pose": adj.grad.detach().clone()}
        lr = 1e-2 * KO.cosine_lr_factor(step, 2, 30000, 0.0)
        with torch.no_grad():
            for x, m, v in zip(leaves, ms, vs):
                KO.adam_step(x, x.grad if x.grad is not None else torch.zeros_like(x), m, v, step + 1, lr)
        opt.step()
        rec["pose_adjustment"] = adj.detach().clone()
        out.append(rec)
    return out

"""The K-Planes training step with frozen time planes, restated from oracle.kplanes_oracle's own pieces.

`oracle.kplanes_oracle.kplanes_forward` has no `freeze_time_planes`; its pieces do (`density_field_forward` / `field_forward` hand the flag to
`interpolate_kplanes`, NS/fields/kplanes_field.py:95-99).  `forward` below is that function's training path with the flag passed through,
`loss_dict` is `kplanes_loss_dict` without the four time terms (NS/models/kplanes.py:438), and `adam_on_touched` steps only tensors that
received a gradient, as torch.optim.Adam skips parameters whose `.grad` is None.  With the flag off the two reproduce `kplanes_forward` +
`kplanes_loss_dict` bit for bit (tests/test_static_planes_cpu.py), so the flag is the only thing the GPU test adds to that reference.

One deliberate difference from the reference model under the flag, written down in DESIGN.md 4.14: the reference's `space_tv_loss` still walks
all six planes and takes the time planes' 1-D total variation along their space axis.  Frozen planes are constant there (they are the ones they
were initialised to) so the term is exactly zero in value and in gradient; the fused trainer sweeps the three space planes only, and so does
`loss_dict(freeze_time_planes=True)`.
"""
from typing import Dict, Sequence

import torch

from oracle import kplanes_oracle as KO

TIME_TERMS = ("time_smoothness_loss", "sparse_transients_loss", "time_smoothness_proposal_loss", "sparse_transients_proposal_loss")

# the shape and draws of tests/test_gpu_trainer.py::test_three_training_steps_match_oracle
THREE_STEPS = dict(base_res=(16, 16, 16, 4), multiscale=(1, 2), feat_dim=32, prop_res=((24, 24, 24, 4), (32, 32, 32, 4)), prop_feat=8,
                   sigma_hidden=128, color_hidden=64, aabb_scale=1.5, seed=5)
THREE_STEPS_RAYS, THREE_STEPS_SAMPLES, THREE_STEPS_SEED, THREE_STEPS_WARM_UP = 40, ((64, 32), 16), 77, 2


def draw_batch(gen: torch.Generator, R: int) -> Dict:
    """One step's rays, target and uniform draws, in the order that test draws them."""
    o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
    times = torch.rand(R, 1, generator=gen)
    target = torch.rand(R, 3, generator=gen)
    rng = {"t_rand": torch.rand(R, 65, generator=gen), "u": [torch.rand(R, 33, generator=gen), torch.rand(R, 17, generator=gen)],
           "bg": torch.rand(R, 3, generator=gen)}
    return {"rays": {"origins": o, "directions": d, "times": times}, "target": target, "rng": rng}


def forward(params: Dict, rays: Dict, rng: Dict, num_proposal_samples: Sequence[int], num_nerf_samples: int, anneal: float,
            freeze_time_planes: bool = False) -> Dict:
    """KO.kplanes_forward (training, proposal gradients on, near plane 0) with freeze_time_planes handed to both field forwards."""
    aabb = params["aabb"]
    o, d, times = rays["origins"], rays["directions"], rays["times"]
    R = o.shape[0]
    frozen = {"freeze_time_planes": True} if freeze_time_planes else {}
    nears, fars = KO.intersect_aabb(o, d, aabb, 0.0, True)
    levels = list(num_proposal_samples) + [num_nerf_samples]
    weights_list, sdist_list = [], []
    weights = bins = None
    for li, S in enumerate(levels):
        if li == 0:
            bins = KO.spaced_bins(R, S, rng["t_rand"]).to(o.device)
        else:
            u = KO.pdf_u(R, S, rng["u"][li - 1]).to(o.device)
            bins, _, _ = KO.pdf_sample(torch.pow(weights, anneal), bins, u)
        eucl = KO.spacing_to_euclidean(bins, nears, fars)
        starts, ends = eucl[:, :-1], eucl[:, 1:]
        pos = KO.sample_positions(o, d, starts, ends)
        if li < len(levels) - 1:
            dens = KO.density_field_forward(pos, times, aabb, params["prop_grids"][li], params["prop_sigma"][li], **frozen)
            weights = KO.get_weights(ends - starts, dens)
            weights_list.append(weights)
            sdist_list.append(bins)
    density, rgb = KO.field_forward(pos, times, aabb, params["field_grids"], params["field_sigma"], params["field_color"], **frozen)
    weights = KO.get_weights(ends - starts, density)
    weights_list.append(weights)
    sdist_list.append(bins)
    return {"rgb": KO.render_rgb(rgb, weights, rng["bg"], True), "weights_list": weights_list, "sdist_list": sdist_list}


def space_tv_space_planes(ms_grids):
    """KO.space_tv_loss over the space planes alone (see the module docstring)."""
    total = 0.0
    for grids in ms_grids:
        for gi in KO.SPACE_PLANES:
            total = total + KO.plane_tv(grids[gi])
    return total


def loss_dict(params: Dict, out: Dict, target: torch.Tensor, freeze_time_planes: bool = False, coef: Dict = KO.DEFAULT_LOSS_COEF) -> Dict:
    """KO.kplanes_loss_dict (training); with the flag: without the four time terms, the space TV over the space planes."""
    if not freeze_time_planes:
        return KO.kplanes_loss_dict(params, out, target, coef)
    ld = {"rgb_loss": torch.mean((target - out["rgb"]) ** 2),
          "distortion_loss": KO.distortion_loss(out["weights_list"][-1], out["sdist_list"][-1]),
          "interlevel_loss": KO.interlevel_loss(out["weights_list"], out["sdist_list"]),
          "space_tv_loss": space_tv_space_planes(params["field_grids"]),
          "space_tv_proposal_loss": space_tv_space_planes(params["prop_grids"])}
    return {k: v * coef[k] for k, v in ld.items()}


def adam_on_touched(leaves, ms, vs, step: int, lr: float) -> int:
    """KO.adam_step on every leaf that received a gradient; the others keep value and moments.  Returns how many were stepped."""
    n = 0
    with torch.no_grad():
        for x, m, v in zip(leaves, ms, vs):
            if x.grad is not None:
                KO.adam_step(x, x.grad, m, v, step, lr)
                n += 1
    return n


def time_plane_leaves(params: Dict):
    return [g[p] for g in list(params["field_grids"]) + list(params["prop_grids"]) for p in KO.TIME_PLANES]

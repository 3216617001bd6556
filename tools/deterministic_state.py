"""Same bits before and after a host-side change: the three fused trainers in deterministic mode (small shapes of tests/test_gpu_determinism.py,
tests/test_gpu_nerfplayer_trainer.py and tests/test_gpu_nerfplayer_full_trainer.py; host-generated inputs, fixed TV rows, 16 train steps so that
steps with and without a proposal update occur), parameters and Adam moments saved per configuration; for the full NeRFPlayer trainer also
`launches` of every step, on the deterministic and on the float-atomic paths.  Dev tool.

    python tools/deterministic_state.py run TREE OUTDIR    # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/deterministic_state.py cmp OUTDIR_A OUTDIR_B   # torch.equal of every saved tensor, equality of the recorded step data; exit 1 on a difference
"""
import json
import os
import sys

import torch


def compare(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        if f.endswith(".pt"):
            x, y = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
            eq = {k: bool(torch.equal(x[k], y[k])) for k in x}
            print(f, eq, "n =", x["params"].numel())
            bad += not all(eq.values())
    ia, ib = json.load(open(os.path.join(a, "info.json"))), json.load(open(os.path.join(b, "info.json")))
    for k in ia:
        same = ia[k] == ib[k]
        print("info", k, "SAME" if same else ("DIFF", ia[k], ib[k]), ia[k].get("updated"), ia[k].get("launches"))
        bad += not same
    print("VERDICT", "all equal" if bad == 0 else f"{bad} differ")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
STEPS = 16
g = lambda z: z.to(DEV).contiguous()
info = {}

def save(tag, tr):
    tr.synchronize()
    torch.save({"params": tr.params.cpu(), "exp_avg": tr.exp_avg.cpu(), "exp_avg_sq": tr.exp_avg_sq.cpu()}, os.path.join(out, tag + ".pt"))
    info[tag] = {"step": tr.step, "finite": bool(torch.isfinite(tr.params).all()), "absmean": float(tr.params.abs().mean()), "m_absmean": float(tr.exp_avg.abs().mean())}

# ---- K-Planes (SMALL of tests/test_gpu_determinism.py) ----
from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer
SMALL = dict(aabb_scale=1.5, spacetime_resolution=(16, 16, 16, 4), multiscale_res=(1, 2), feature_dim=32,
             proposal_resolutions=((24, 24, 24, 4), (32, 32, 32, 4)), proposal_feature_dim=8, num_proposal_samples_per_ray=(64, 32),
             num_nerf_samples_per_ray=16, warm_up_end=2)
def kp_inputs(R, steps, seed=3):
    gen = torch.Generator().manual_seed(seed)
    o_ = []
    for _ in range(steps):
        o = (torch.rand(R, 3, generator=gen) * 2 - 1) * 1.2
        d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1)
        rays = {"origins": o, "directions": d, "times": torch.rand(R, 1, generator=gen)}
        rng = {"t_rand": torch.rand(R, 65, generator=gen), "u": [torch.rand(R, 33, generator=gen), torch.rand(R, 17, generator=gen)], "bg": torch.rand(R, 3, generator=gen)}
        o_.append((rays, torch.rand(R, 3, generator=gen), rng))
    return o_
for tag, kw in (("kplanes_fp32", dict(mlp_operands="fp32")), ("kplanes_bf16", dict(mlp_operands="bf16")),
                ("kplanes_bf16_vd", dict(mlp_operands="bf16", disable_viewing_dependent=False)),
                ("kplanes_fp32_every2", dict(mlp_operands="fp32", proposal_warmup=1, proposal_update_every=3))):
    R = 512
    tr = KPlanesTrainer(KPlanesTrainConfig(**SMALL, deterministic=True, **kw), R, DEV)
    upd = []
    for rays, target, rng in kp_inputs(R, STEPS):
        before = tr._steps_since_update
        tr.train_step({k: g(v) for k, v in rays.items()}, g(target), {"t_rand": g(rng["t_rand"]), "u": [g(u) for u in rng["u"]], "bg": g(rng["bg"])})
        upd.append(int(tr._steps_since_update <= before))
    save(tag, tr)
    info[tag]["updated"] = upd
    del tr

# ---- NeRFPlayer-nerfacto (small shapes of tests/test_gpu_nerfplayer_trainer.py) ----
from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModelConfig
from soccernerfs_amd.nerfplayer_trainer import NerfplayerTrainer
PROP = [{"hidden_dim": 16, "temporal_dim": 8, "log2_hashmap_size": 10, "num_levels": 4, "max_res": 32},
        {"hidden_dim": 16, "temporal_dim": 8, "log2_hashmap_size": 10, "num_levels": 4, "max_res": 64}]
def np_batch(R, n_img, seed):
    gen = torch.Generator().manual_seed(seed)
    o = ((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.3).to(DEV)
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1).to(DEV)
    times = torch.rand(R, 1, generator=gen).to(DEV)
    cams = torch.randint(0, n_img, (R,), generator=gen).to(DEV)
    target = torch.rand(R, 3, generator=gen).to(DEV)
    rng = {"t_rand": torch.rand(R, 1, generator=gen).to(DEV), "u": [torch.rand(R, 1, generator=gen).to(DEV), torch.rand(R, 1, generator=gen).to(DEV)], "bg": torch.rand(R, 3, generator=gen).to(DEV)}
    return {"origins": o, "directions": d, "times": times}, cams, target, rng
for tag, kw, tv in (("nerfacto", {}, 1.0), ("nerfacto_async", dict(async_field_sweep=True), 1.0), ("nerfacto_async_notv", dict(async_field_sweep=True), 0.0),
                    ("nerfacto_bf16", dict(mlp_operands="bf16"), 1.0)):
    R, n_img = 128, 9
    cfg = NerfplayerNerfactoModelConfig(num_levels=6, log2_hashmap_size=12, temporal_dim=16, proposal_net_args_list=PROP, num_proposal_samples_per_ray=(64, 32),
                                        num_nerf_samples_per_ray=16)
    if tv != 1.0:
        cfg.temporal_tv_weight = tv
    tr = NerfplayerTrainer(cfg, R, n_img, aabb_scale=1.0, device=DEV, seed=5, deterministic=True, warm_up_end=4, **kw)
    with torch.no_grad():
        gg = torch.Generator().manual_seed(1)
        for name in ("field.table", "prop0.table", "prop1.table"):
            tr.views[name].copy_((torch.rand(tr.views[name].shape, generator=gg) * 2 - 1).to(DEV))
    tr.tv_rows = [2, 1, 3]
    upd = []
    for k in range(STEPS):
        rays, cams, target, rng = np_batch(R, n_img, 100 + k)
        before = tr._steps_since_update
        tr.train_step(rays, cams, target, rng)
        upd.append(int(tr._steps_since_update <= before))
    save(tag, tr)
    info[tag]["updated"] = upd
    info[tag]["loss"] = {k: float(v) for k, v in tr.loss_dict().items() if k != "temporal_tv_loss"}
    del tr

# ---- full NeRFPlayer (small shapes of tests/test_gpu_nerfplayer_full_trainer.py) ----
from soccernerfs_amd.nerfplayer import NerfplayerModelConfig
from soccernerfs_amd.nerfplayer_full_trainer import NerfplayerFullTrainer
def full_cfg(tv=1.0):
    return NerfplayerModelConfig(num_levels=16, log2_hashmap_size=12, temporal_dim=16, temporal_tv_weight=tv, proposal_net_args_list=PROP,
                                 num_proposal_samples_per_ray=(64, 32), num_nerf_samples_per_ray=16)
def full_batch(R, seed):
    gen = torch.Generator().manual_seed(seed)
    o = g((torch.rand(R, 3, generator=gen) * 2 - 1) * 0.3)
    d = g(torch.nn.functional.normalize(torch.rand(R, 3, generator=gen) * 2 - 1, dim=-1))
    times, target = g(torch.rand(R, 1, generator=gen)), g(torch.rand(R, 3, generator=gen))
    rng = {"t_rand": g(torch.rand(R, 1, generator=gen)), "u": [g(torch.rand(R, 1, generator=gen)), g(torch.rand(R, 1, generator=gen))], "bg": g(torch.rand(R, 3, generator=gen))}
    return {"origins": o, "directions": d, "times": times}, target, rng
for tag, kw, tv in (("full", {}, 1.0), ("full_async", dict(async_table_sweeps=True), 1.0), ("full_notv", dict(async_table_sweeps=True), 0.0), ("full_bf16", dict(mlp_operands="bf16"), 1.0)):
    R = 128
    tr = NerfplayerFullTrainer(full_cfg(tv), R, aabb_scale=1.0, device=DEV, seed=5, deterministic=True, warm_up_end=4, **kw)
    tr.tv_rows = [2, 1, 3, 0]
    upd, launches = [], []
    for k in range(STEPS):
        rays, target, rng = full_batch(R, 200 + k)
        before = tr._steps_since_update
        tr.train_step(rays, target, rng)
        upd.append(int(tr._steps_since_update <= before))
        launches.append(tr.launches)
    save(tag, tr)
    info[tag]["updated"], info[tag]["launches"] = upd, launches
    info[tag]["loss"] = {k: float(v) for k, v in tr.loss_dict().items() if k != "temporal_tv_loss"}
    del tr
# tr.launches on the float-atomic paths
for tag, kw in (("full_launches_default", {}), ("full_launches_async_tiled", dict(async_table_sweeps=True, tiled_table_backward=True)),
                ("full_launches_async_tiled_hash", dict(async_table_sweeps=True, tiled_table_backward=True, tiled_hash_backward=True)),
                ("full_launches_bf16_async_tiled", dict(async_table_sweeps=True, tiled_table_backward=True, mlp_operands="bf16"))):
    R = 128
    tr = NerfplayerFullTrainer(full_cfg(), R, aabb_scale=1.0, device=DEV, seed=5, warm_up_end=4, **kw)
    tr.tv_rows = [2, 1, 3, 0]
    ls = []
    for k in range(13):
        rays, target, rng = full_batch(R, 300 + k)
        tr.train_step(rays, target, rng)
        ls.append(tr.launches)
    tr.synchronize()
    info[tag] = {"launches": ls, "finite": bool(torch.isfinite(tr.params).all())}
    del tr
json.dump(info, open(os.path.join(out, "info.json"), "w"), indent=1)
print(json.dumps(info))

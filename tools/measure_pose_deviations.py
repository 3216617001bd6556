#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the camera-optimiser tests -> profiles/r15_pose_deviations.json.

For every case of tests/pose_reference.py the restatement is evaluated in float64 (the reference) and in float32 (the yardstick) with torch on
the CPU; the deviation of the second from the first, relative to the reference's largest magnitude, is written down with the case's seed and
shape.  The GPU tests bound the kernels by FACTOR (5) x these figures.  Also recorded -- a record, not a bound -- is how large the term is
that the kernels omit on purpose: the reference's autograd differentiates the collider's nears / fars with respect to the ray, the kernels
hold the bin edges constant (cosine and norm ratio between the two pose gradients at the three-step fixture)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pose_reference as PR  # noqa: E402


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {"factor": PR.FACTOR, "rule": "bound = factor x dev32, dev32 = max |float32 restatement - float64 restatement| / max |float64 restatement|",
           "coords": {}, "pose_apply": {}, "pose_bwd": {}, "three_steps": {}, "omitted_bin_edge_term": {}}
    for c in PR.COORDS_CASES:
        d = PR.make_coords_case(c)
        ok = PR.comparable_samples(c, d)
        g64, g32 = PR.coords_gradient(c, d, torch.float64), PR.coords_gradient(c, d, torch.float32)
        out["coords"][PR.case_id(c)] = {"seed": c["seed"], "N": c["N"], "excluded_share": 1.0 - float(ok.double().mean()),
                                        "dev32_grad_pts": PR.rel_dev(g32[ok], g64[ok]), "max_abs_ref": float(g64[ok].abs().max()) if ok.any() else 0.0}
        print(PR.case_id(c), out["coords"][PR.case_id(c)], flush=True)
    for kind in PR.POSE_TABLES:
        t = PR.make_pose_table(kind)
        for gname, groups in PR.POSE_GROUPS.items():
            G = PR.POSE_M if groups is None else max(groups) + 1
            for above in (False, True):
                adj = PR.pose_adjustments(G, 1, above)
                key = f"{kind}-{gname}-{'above' if above else 'below'}_clamp"
                g = None if groups is None else torch.as_tensor(groups)
                c64 = PR.adjusted_c2w(torch.from_numpy(t["c2w"]), adj.double(), g)
                c32 = PR.adjusted_c2w(torch.from_numpy(t["c2w"]).float(), adj, g)
                out["pose_apply"][key] = {"seed": 1, "M": PR.POSE_M, "G": G, "dev32_c2w": PR.rel_dev(c32, c64)}
                g64, g32 = PR.pose_gradient(t, adj, groups, torch.float64), PR.pose_gradient(t, adj, groups, torch.float32)
                out["pose_bwd"][key] = {"seed": 1, "R": PR.POSE_R, "M": PR.POSE_M, "G": G, "dev32_grad_pose": PR.rel_dev(g32, g64)}
                print(key, out["pose_apply"][key], out["pose_bwd"][key], flush=True)
    s64, s32 = PR.three_steps(torch.float64), PR.three_steps(torch.float32)
    out["three_steps"]["shape"] = {"E": {k: (list(v) if isinstance(v, tuple) else v) for k, v in PR.STEP_E.items()}, "R": PR.STEP_R, "S": [list(PR.STEP_S[0]), PR.STEP_S[1]],
                                   "M": PR.STEP_M, "groups": PR.STEP_GROUPS, "draw_seeds": "500 + step"}
    for i, (a, b) in enumerate(zip(s32, s64)):
        out["three_steps"][f"step{i + 1}"] = {f"dev32_{k}": PR.rel_dev(a[k], b[k]) for k in b}
        print("step", i + 1, out["three_steps"][f"step{i + 1}"], flush=True)
    full = PR.three_steps(torch.float64, detach_bins=False)
    for i, (a, b) in enumerate(zip(full, s64)):
        x, y = a["grad_pose"].reshape(-1), b["grad_pose"].reshape(-1)
        out["omitted_bin_edge_term"][f"step{i + 1}"] = {
            "cosine_full_vs_detached": float(torch.dot(x, y) / (x.norm() * y.norm())), "norm_ratio_detached_over_full": float(y.norm() / x.norm()),
            "note": "grad_pose of the reference's full autograd (nears / fars differentiated) against the detached-bin gradient the kernels form; float64; "
                    "from step 2 on the two runs' parameters have drifted apart, so only step 1 compares the same point"}
        print("omitted", i + 1, out["omitted_bin_edge_term"][f"step{i + 1}"], flush=True)
    with open(PR.DEVIATIONS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

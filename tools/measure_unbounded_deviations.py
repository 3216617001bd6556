#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the unbounded-scene tests -> profiles/r27_unbounded_deviations.json.

For every case of tests/unbounded_reference.GRAD_CASES the restated coordinate gradient at snerf_coords.contract = 1 (autograd through the
interpolation for d / d p, the contraction's Jacobian transposed, the sums over a ray's samples) is evaluated in float64 (the reference) and in
float32 (the yardstick) with torch on the CPU; the deviation of the second from the first, relative to the reference's largest magnitude over
the compared samples or rays, is written down with the case's seed and shape.  tests/test_gpu_unbounded.py bounds the kernel by FACTOR (5) x
these figures.  The three training steps of the restated unbounded model (tests/unbounded_reference.three_steps) are measured the same way:
they decide the bound of the trainer-against-model comparison where the far samples exceed the bounded comparison's tolerances.  Also recorded: the deviation of the float32 coordinates themselves from the float64 ones (a record: the GPU test compares the
coordinates by EQUALITY with the float32 expression, not against this figure)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pose_reference as PR  # noqa: E402
from tests import unbounded_reference as U  # noqa: E402


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {"factor": U.FACTOR, "rule": "bound = factor x dev32, dev32 = max |float32 restatement - float64 restatement| / max |float64 restatement|",
           "margins": {"tie_relative": U.TIE_MARGIN, "face": U.FACE_MARGIN, "lattice_texels": PR.LATTICE_MARGIN}, "coords_gradient": {}}
    for c in U.GRAD_CASES:
        d = U.make_gradient_case(c)
        ok, okr = U.grad_comparable(c, d), U.grad_rays_comparable(c, d)
        gp64, go64, gd64 = U.grad_reference(c, d, torch.float64)
        gp32, go32, gd32 = U.grad_reference(c, d, torch.float32)
        rec = {"seed": c["seed"], "N": c["N"], "kept_share": float(ok.double().mean()), "kept_rays": int(okr.sum()),
               "dev32_points": PR.rel_dev(U.grad_points(c, d, torch.float32), U.grad_points(c, d, torch.float64)),
               "dev32_grad_pts": PR.rel_dev(gp32[ok], gp64[ok]), "dev32_grad_origins": PR.rel_dev(go32[okr], go64[okr]),
               "dev32_grad_dirs": PR.rel_dev(gd32[okr], gd64[okr]), "max_abs_grad_pts": float(gp64[ok].abs().max()),
               "max_abs_grad_origins": float(go64[okr].abs().max()), "max_abs_grad_dirs": float(gd64[okr].abs().max())}
        out["coords_gradient"][U.grad_case_id(c)] = rec
        print(U.grad_case_id(c), rec, flush=True)
    # the trainer comparison: three steps of the restated unbounded model, float32 against float64 (tolerances: the bounded comparison's floor)
    out["three_steps"] = {"dev32": U.three_steps_deviation(), "floor": U.STEP_TOLERANCES, "rays": U.STEP_R, "near": U.STEP_NEAR, "far": U.STEP_FAR,
                          "rule": "bound = max(floor, factor x dev32): rgb absolute, loss terms relative, parameters relative L2 per tensor"}
    print("three_steps", out["three_steps"], flush=True)
    with open(U.DEVIATIONS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", U.DEVIATIONS)


if __name__ == "__main__":
    main()

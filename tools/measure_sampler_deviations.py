#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the sampler lattice's inexact routes -> profiles/r30_sampler_reference_e32.json.

With the weights given and anneal == 1 the ray samplers are pinned by equality (tests/sampler_reference.py).  Behind powf (annealing) and expf
(get_weights in the kernel, snerf_weights_fwd / snerf_weights_bwd) they are bounded: for every bounded quantity the float32 restatement is
evaluated against the float64 reference over the lattice's family A and weights cases, and the worst deviation, max |float32 - float64| over the
case's largest |float64|, is written down.  tests/test_gpu_sampler_lattice.py bounds the kernels by MARGIN (5) x the table
sampler_reference.E32, which tests/test_sampler_reference_cpu.py holds to this measurement; tau = 5 x E32 of the cdf is the allowance of the
index criterion and of u_back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sampler_reference as SR  # noqa: E402

PATH = os.path.join(ROOT, "profiles", "r30_sampler_reference_e32.json")


def measure():
    worst = SR.measure_e32()
    return {"metric": "max |float32 restatement - float64 reference| / max |float64 reference| per case, maximised over family A "
                      "(resample.*) and the weights cases (weights_*)",
            "margin": SR.MARGIN, "tau": SR.TAU,
            "E32": {k: float(f"{v[0]:.3e}") for k, v in worst.items()}, "where": {k: v[1] for k, v in worst.items()}}


def main():
    out = measure()
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in sorted(out["E32"].items()):
        print(f"E32 {k:28s} {v:.3e}   at {out['where'][k]}")
    print(f"-> {os.path.relpath(PATH, ROOT)}")


if __name__ == "__main__":
    main()

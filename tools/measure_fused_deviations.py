#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the fused lattice's inexact outputs -> profiles/r25_fused_deviations.json.

On the exact cases of tests/fused_reference.py everything up to the raw head outputs is the same number in every arithmetic; density (exp) and rgb
(Sigmoid) are not.  For every case of snerf_kplanes_density_fwd and of the field forward the restatement is evaluated in float64 (the reference)
and in float32 (the yardstick) with torch on the CPU, over the case's rows plus 1024 further feature rows through the case's own nets
(fused_reference._yard_feat), and the worst elementwise relative deviation max |a - b| / |b| is written down per output.
tests/test_gpu_fused_lattice.py bounds the kernels on the rows that are not planted, elementwise, by FACTOR (5) x these figures; on the planted
rows it asks for density 1.0 and rgb 0.5 exactly."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import fused_reference as F  # noqa: E402

FACTOR = 5


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cases = {}
    for c in F.all_cases():
        if F.needs_bound(c):
            cases[F.case_id(F.content_key(c))] = F.deviations(c)
    out = {"factor": FACTOR,
           "rule": "density, rgb on rows that are not planted: elementwise |kernel - float64| <= factor x dev32 x |float64|, dev32 = max over the "
                   "yardstick rows of |float32 restatement - float64 restatement| / |float64 restatement|",
           "cases": cases}
    path = os.path.join(ROOT, "profiles", "r25_fused_deviations.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    worst = max(max(v.values()) for v in cases.values())
    least = min(min(v.values()) for v in cases.values())
    print(f"{len(cases)} cases -> {os.path.relpath(path, ROOT)}; deviations between {least:.3e} and {worst:.3e}")


if __name__ == "__main__":
    main()

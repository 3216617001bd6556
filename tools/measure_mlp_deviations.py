#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the MLP lattice's inexact forward outputs -> profiles/r17_mlp_deviations.json.

On the exact cases of tests/mlp_reference.py the only outputs that are not exact are those behind a Sigmoid or an exp (Y of a Sigmoid output,
aux_out of the trunc_exp head, Y of a Sigmoid dense layer): the raw output z is the same number in every arithmetic, the activation is not.  For
every such case the restatement is evaluated in float64 (the reference) and in float32 (the yardstick) with torch on the CPU, and the worst
elementwise relative deviation max |a - b| / |b| is written down per output.  tests/test_gpu_mlp_lattice.py bounds the kernels, elementwise, by
FACTOR (5) x these figures.  The exact-fp32 kernels' backward cases with a head away from a raw output of 0 (mlp_reference.is_bounded_backward)
are in the file too: gX and gW, deviation max |a - b| / max |b| over the output, bounded in the same way."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mlp_reference as R  # noqa: E402

FACTOR = 5


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cases = {}
    for c in R.mlp_forward_cases() + R.dense_cases() + R.mlp_backward_cases():
        if R.needs_bound(c):
            cases[R.case_id(c)] = R.case_deviations(c)
    out = {"factor": FACTOR,
           "rule": "Y, aux (forward outputs): elementwise |kernel - float64| <= factor x dev32 x |float64|, dev32 = max over the case's elements of "
                   "|float32 restatement - float64 restatement| / |float64 restatement|",
           "rule_backward": "gX, gW (bounded backward cases of the exact-fp32 kernels): max |kernel - float64| / max |float64| over the output "
                            "<= factor x dev32, dev32 = the same figure of the float32 restatement",
           "cases": cases}
    path = os.path.join(ROOT, "profiles", "r17_mlp_deviations.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    worst = max(max(v.values()) for v in cases.values())
    least = min(min(v.values()) for v in cases.values())
    print(f"{len(cases)} cases -> {os.path.relpath(path, ROOT)}; deviations between {least:.3e} and {worst:.3e}")


if __name__ == "__main__":
    main()

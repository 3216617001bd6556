#!/usr/bin/env python3
"""The yardstick of tests/test_gpu_tgrid_density.py's float64 comparison, measured on the CPU without the code under test: for each of
tests/tgrid_density_cases.F64_CASES the float64 restatement of the fused proposal density (tests/table_reference.py's encoder, the net as a
k-ordered chain, exp) is run again in float32, and the largest relative deviation over all elements is written to
profiles/r29_tgrid_density_deviations.json.  The GPU test allows the kernel 5 x that per case.

    python tools/measure_tgrid_density_deviations.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tgrid_density_cases as TC  # noqa: E402


def main():
    out = {"what": "max over all elements of |float32 restatement - float64 restatement| / float64 restatement of the density; the GPU test's bound is 5 x this",
           "cases": {}}
    for table, S, R in TC.F64_CASES:
        d64, f64 = TC.restate(table, S, R, np.float64)
        d32, _ = TC.restate(table, S, R, np.float32)
        inside = int((np.abs(f64).sum(axis=1) != 0).sum())
        out["cases"][TC.case_key(table, S, R)] = {"elements": int(d64.size), "samples_in_range": inside, "density_min": float(d64.min()), "density_max": float(d64.max()),
                                                  "deviation": TC.relative_deviation(d32, d64)}
        print(TC.case_key(table, S, R), out["cases"][TC.case_key(table, S, R)])
    with open(os.path.join(ROOT, "profiles", "r29_tgrid_density_deviations.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

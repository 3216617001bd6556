#!/usr/bin/env python
"""CPU only: the float32 yardsticks of the optimiser-sweep tests -> profiles/r16_optim_deviations.json.

For every case of tests/optim_reference.py the restatement (plane regularisers by autograd, Adam by its formula) is evaluated in float64 (the
reference) and in float32 (the yardstick) with torch on the CPU; the deviation of the second from the first, max |a - b| / max |b|, is written
down per output.  The GPU tests bound the kernels by FACTOR (5) x these figures; where a figure is 0 the kernel must be exact.  Also recorded
-- a record, not a bound on the kernels -- is what the float ABI's betas change against decimal betas in one float64 step.  The tile passes'
fused Adam is measured the same way with the oracles' autograd (oracle/tgrid_oracle.py, oracle/hashgrid_oracle.py) as the restatement."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import optim_reference as OR  # noqa: E402


def abi_beta_change(d):
    """One float64 step with the decimal betas against one with the float-valued betas: relative change of v_out and of the update."""
    a, b = OR.planes_step(d, torch.float64, b1=0.9, b2=0.999), OR.planes_step(d, torch.float64)
    p = d["p"].double()
    return OR.rel_dev(a["v"], b["v"]), OR.rel_dev(a["p_out"] - p, b["p_out"] - p)


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {"factor": OR.FACTOR, "rule": "bound = factor x dev32, dev32 = max |float32 restatement - float64 restatement| / max |float64 restatement|; "
                                        "the three loss values add the float32 bound of the kernel's summation tree (tests/optim_reference.py: value_summation_bound)",
           "planes": {}, "flat": {}, "tv": {}, "tiles": {}, "abi_beta": {}}
    worst_v, worst_u = 0.0, 0.0
    for c in OR.PLANE_CASES:
        d = OR.make_case(c)
        r64, r32 = OR.planes_step(d, torch.float64), OR.planes_step(d, torch.float32)
        acc = d["acc"]
        rec = {"seed": c["seed"], "n": d["n"], "step": d["step"]}
        for k in ("p_out", "m", "v", "reg_grad"):
            rec[f"dev32_{k}"] = OR.rel_dev(r32[k], r64[k])
        rec["dev32_reg_grad_accumulated"] = OR.rel_dev(acc + r32["reg_grad"], acc.double() + r64["reg_grad"])
        rec["dev32_values"] = [OR.rel_dev(r32["values"][i], r64["values"][i]) for i in range(3)]
        rec["values"] = [float(x) for x in r64["values"]]
        dv, du = abi_beta_change(d)
        rec["abi_beta_rel_change_v"], rec["abi_beta_rel_change_update"] = dv, du
        worst_v, worst_u = max(worst_v, dv), max(worst_u, du)
        out["planes"][c["case_id"]] = rec
        print(c["case_id"], rec, flush=True)
    out["abi_beta"] = {"beta1": OR.BETA1, "beta2": OR.BETA2, "one_minus_beta2_float_abi": 1.0 - OR.BETA2, "one_minus_beta2_decimal": 1.0 - 0.999,
                       "rel_difference_one_minus_beta2": abs((1.0 - OR.BETA2) - (1.0 - 0.999)) / (1.0 - 0.999),
                       "max_rel_change_v": worst_v, "max_rel_change_update": worst_u,
                       "note": "one float64 step with betas (0.9, 0.999) against one with the float32-valued betas the C ABI receives, largest over the plane lattice"}
    print("abi_beta", out["abi_beta"], flush=True)
    for name, cases, make, step in (("flat", OR.FLAT_CASES, OR.make_flat_case, OR.flat_step), ("tv", OR.TV_CASES, OR.make_tv_case, OR.tv_step)):
        for c in cases:
            d = make(c)
            r64, r32 = step(d, torch.float64), step(d, torch.float32)
            rec = {"seed": c["seed"], "step": d["step"]}
            for k in ("p_out", "m", "v"):
                rec[f"dev32_{k}"] = OR.rel_dev(r32[k], r64[k])
            out[name][c["case_id"]] = rec
            print(c["case_id"], rec, flush=True)
    for c in OR.tile_cases():  # the tile passes' fused Adam: the float32 ORACLE (autograd through oracle/*_oracle.encode) against the float64 one
        d = OR.make_tile_case(c)
        rec = {"seed": c["seed"], "B": d["B"], "table_shape": list(d["shape"])}
        for tv, state in OR.tile_variants(c):
            rec[OR.tile_key(tv, state)] = OR.tile_deviations(d, tv, state)
        out["tiles"][c["case_id"]] = rec
        print(c["case_id"], rec, flush=True)
    with open(OR.DEVIATIONS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

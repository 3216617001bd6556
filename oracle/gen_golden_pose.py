#!/usr/bin/env python3
"""Writes the G19 pose fixture from the reference's own code (needs the reference tree; CPU only):

    python oracle/gen_golden_pose.py     # writes tests/golden/g19_pose.npz

Inputs and outputs of the reference's pose algebra, float64 on the CPU: exp_map_SO3xR3 (NS/cameras/lie_groups.py:23-58) of 64 seeded
tangent vectors -- 16 all zero or nearly so, 24 below the clamp (|w|^2 < 1e-4), 24 above it -- and pose_utils.multiply (NS/utils/poses.py:53-67)
of 64 seeded poses with those transforms on the right, as NS/cameras/cameras.py:707-708 composes them; and the multipliers of the
ExponentialDecayScheduler (NS/engine/schedulers.py:84-106) for the camera optimiser's configuration (lr 6e-4, max_steps 10000) with lr_final
None and 1e-5 at a few steps.  Arrays only; fixed member timestamps, so a rerun gives the same bytes."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._refimport import import_reference  # noqa: E402

SEED = 19


def main():
    import_reference()
    from nerfstudio.cameras.lie_groups import exp_map_SO3xR3
    from nerfstudio.engine.schedulers import ExponentialDecaySchedulerConfig
    from nerfstudio.utils import poses as pose_utils

    gen = torch.Generator().manual_seed(SEED)
    tv = torch.randn(64, 6, generator=gen, dtype=torch.float64)
    tv[:16] *= 0.0
    tv[8:16, 3:] = torch.randn(8, 3, generator=gen, dtype=torch.float64) * 1e-7
    tv[16:40, 3:] *= 0.003
    tv[40:, 3:] *= 0.4
    tv[:, :3] *= 0.2
    q, _ = torch.linalg.qr(torch.randn(64, 3, 3, generator=gen, dtype=torch.float64))
    poses = torch.cat([q, torch.randn(64, 3, 1, generator=gen, dtype=torch.float64)], -1)
    e = exp_map_SO3xR3(tv)
    out = {"tangent": tv.numpy(), "exp_map": e.numpy(), "poses": poses.numpy(), "composed": pose_utils.multiply(poses, e).numpy()}
    steps = np.array([0, 1, 100, 5000, 9999, 10000, 20000], np.int64)
    out["sched_steps"] = steps
    for name, lr_final in (("none", None), ("1e-5", 1e-5)):
        cfg = ExponentialDecaySchedulerConfig(max_steps=10000, lr_final=lr_final)
        opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=6e-4, eps=1e-15)
        sched = cfg.setup().get_scheduler(opt, 6e-4)
        lam = sched.lr_lambdas[0]
        out["sched_lr_" + name] = np.array([6e-4 * float(lam(int(s))) for s in steps], np.float64)
    buf = io.BytesIO()
    np.savez(buf, **out)
    src = zipfile.ZipFile(io.BytesIO(buf.getvalue()))
    path = os.path.join(ROOT, "tests", "golden", "g19_pose.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as dst:
        for info in src.infolist():
            zi = zipfile.ZipInfo(info.filename, date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            dst.writestr(zi, src.read(info.filename))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes the G17 lens fixture from the reference's own code (needs the reference tree; CPU only):

    python tools/gen_golden_lens.py     # writes tests/golden/g17_lens.npz

Four perspective cameras at 96 x 54 with OpenCV distortion rows (k1 k2 k3 k4 p1 p2): row 0 all zero, row 1 radial only, row 2 all six with a
tangential pair of opposite signs, row 3 a strong barrel.  The rays are those of the reference's Cameras(..., distortion_params=...)
(NS/cameras/cameras.py:505-741 with the undistortion of NS/cameras/camera_utils.py:298-401), float32 on the CPU:

  * the full frame of camera FRAME_CAMERA (5184 rays, row-major), then
  * N_RANDOM seeded random pixels of each camera (4 x 512 rays),

7232 rays in this order.  Stored: the inputs (fx, fy, cx, cy, width, height, camera_to_worlds, cam_times, distortion), the ray table
`indices` (camera, row, col) and per ray directions, pixel_area, directions_norm, times.  Origins are the translation columns of
camera_to_worlds and are not stored.  Arrays only.  The archive is written with fixed member timestamps, so a rerun gives the same bytes.
"""
import io
import math
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._refimport import import_reference  # noqa: E402

W, H = 96, 54
FRAME_CAMERA = 3
N_RANDOM = 512
SEED = 17
FX, FY = [60.0, 70.0, 45.0, 80.0], [62.0, 70.0, 47.0, 79.0]
CX, CY = [48.0, 47.3, 50.0, 48.0], [27.0, 26.5, 27.0, 28.2]
DISTORTION = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
              [-0.12, 0.03, 0.0, 0.0, 0.0, 0.0],
              [0.08, -0.02, 0.004, -0.001, 0.002, -0.0015],
              [-0.25, 0.08, -0.01, 0.0, 0.001, 0.0005]]
TIMES = [0.0, 0.3, 0.65, 1.0]


def pose(yaw, pitch, roll, t):
    """camera-to-world [3,4]: R = Rz(yaw) Rx(pitch) Ry(roll), translation t."""
    cz, sz, cx, sx, cy, sy = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    return np.concatenate([rz @ rx @ ry, np.asarray(t, np.float64)[:, None]], 1)


def make_inputs():
    c2w = np.stack([pose(0.3, 1.1, 0.05, (0.9, -1.2, 0.6)), pose(-0.7, 1.3, -0.1, (-1.1, -0.8, 0.45)), pose(1.9, 0.9, 0.2, (1.0, 0.7, 0.8)),
                    pose(2.8, 1.2, -0.03, (-0.4, 1.3, 0.5))]).astype(np.float32)
    rng = np.random.default_rng(SEED)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    parts = [np.stack([np.full(H * W, FRAME_CAMERA), ys.reshape(-1), xs.reshape(-1)], -1)]
    for c in range(4):
        parts.append(np.stack([np.full(N_RANDOM, c), rng.integers(0, H, N_RANDOM), rng.integers(0, W, N_RANDOM)], -1))
    f32 = lambda v: np.asarray(v, np.float32)
    return {"fx": f32(FX), "fy": f32(FY), "cx": f32(CX), "cy": f32(CY), "width": np.int64(W), "height": np.int64(H), "camera_to_worlds": c2w,
            "cam_times": f32(TIMES), "distortion": f32(DISTORTION), "indices": np.concatenate(parts).astype(np.int64)}


def save_npz_reproducibly(path, arrays):
    """np.savez_compressed's layout (one .npy member per array, deflate) with a fixed timestamp on every member."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import_reference()
    from nerfstudio.cameras.cameras import Cameras, CameraType

    res = make_inputs()
    t = torch.from_numpy
    cams = Cameras(camera_to_worlds=t(res["camera_to_worlds"]), fx=t(res["fx"]), fy=t(res["fy"]), cx=t(res["cx"]), cy=t(res["cy"]), width=W, height=H,
                   distortion_params=t(res["distortion"]), camera_type=CameraType.PERSPECTIVE, times=t(res["cam_times"]))
    idx = t(res["indices"])
    rb = cams.generate_rays(camera_indices=idx[:, 0:1], coords=idx[:, 1:3].float() + 0.5)
    frame = cams.generate_rays(camera_indices=FRAME_CAMERA)  # the meshgrid path (cameras.py:300-418) must agree with the table path
    n = H * W
    assert torch.equal(frame.directions.reshape(n, 3), rb.directions[:n]) and torch.equal(frame.pixel_area.reshape(n, 1), rb.pixel_area[:n])
    assert torch.equal(rb.origins, t(res["camera_to_worlds"])[idx[:, 0], :, 3])
    f = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    res.update({"directions": f(rb.directions), "pixel_area": f(rb.pixel_area), "directions_norm": f(rb.metadata["directions_norm"]), "times": f(rb.times)})
    out = os.path.join(ROOT, "tests", "golden", "g17_lens.npz")
    save_npz_reproducibly(out, res)
    for k, v in res.items():
        print(k, np.asarray(v).dtype, np.asarray(v).shape)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes the G18 camera-type fixture from the reference's own code (needs the reference tree; CPU only):

    python tools/gen_golden_camera_types.py     # writes tests/golden/g18_camera_types.npz

Three tables of four cameras at 96 x 54, on the poses, times and ray table of G17 (tools/gen_golden_lens.py):

  * A, fisheye (CameraType 2): fx = (40, 45, 36, 50), fy = (41, 45, 37, 49), G17's cx, cy, distortion = 0.25 x G17's rows (row 0 is zero);
  * B, equirectangular (3): fx = 48, fy = 54, cx = 48, cy = 27, and A's non-zero distortion rows, which must have no effect;
  * C, mixed: types (1, 2, 3, 2), A's intrinsics for cameras 0, 1 and 3, B's for camera 2, A's distortion rows.

The rays are those of the reference's Cameras(..., camera_type=...) (NS/cameras/cameras.py:505-741), float32 on the CPU: the full frame of
camera FRAME_CAMERA (5184 rays, row-major), then N_RANDOM seeded random pixels of each camera (4 x 512 rays), 7232 rays per table.  Stored:
the shared inputs (width, height, camera_to_worlds, cam_times, indices) and per table, under the prefixes a_, b_, c_: fx, fy, cx, cy,
distortion, camera_type and per ray directions, pixel_area, directions_norm, times.  Origins are the translation columns of camera_to_worlds
and are not stored.  Arrays only.  The archive is written with fixed member timestamps, so a rerun gives the same bytes.

The script fails rather than writes if the meshgrid path differs from the table path, if the reference's output holds a NaN (its fisheye
branch divides 0 by 0 at a pixel centre exactly on the principal point, theta == 0: these inputs must not go there), or if table B differs from
the same table generated without distortion rows.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_lens import CX, CY, DISTORTION, FRAME_CAMERA, H, W, make_inputs, save_npz_reproducibly  # noqa: E402
from oracle._refimport import import_reference  # noqa: E402

PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3
f32 = lambda v: np.asarray(v, np.float32)
LENS = f32(DISTORTION) * np.float32(0.25)
TABLE_A = {"fx": f32([40.0, 45.0, 36.0, 50.0]), "fy": f32([41.0, 45.0, 37.0, 49.0]), "cx": f32(CX), "cy": f32(CY), "distortion": LENS,
           "camera_type": np.full(4, FISHEYE, np.int32)}
TABLE_B = {"fx": f32([48.0] * 4), "fy": f32([54.0] * 4), "cx": f32([48.0] * 4), "cy": f32([27.0] * 4), "distortion": LENS,
           "camera_type": np.full(4, EQUIRECTANGULAR, np.int32)}
_pick = lambda k: np.where(np.arange(4) == 2, TABLE_B[k], TABLE_A[k])
TABLE_C = {"fx": _pick("fx"), "fy": _pick("fy"), "cx": _pick("cx"), "cy": _pick("cy"), "distortion": LENS,
           "camera_type": np.asarray([PERSPECTIVE, FISHEYE, EQUIRECTANGULAR, FISHEYE], np.int32)}


def reference_rays(Cameras, shared, tab, distortion=True):
    t = torch.from_numpy
    cams = Cameras(camera_to_worlds=t(shared["camera_to_worlds"]), fx=t(tab["fx"]), fy=t(tab["fy"]), cx=t(tab["cx"]), cy=t(tab["cy"]), width=W, height=H,
                   distortion_params=t(tab["distortion"]) if distortion else None, camera_type=t(tab["camera_type"]).long(), times=t(shared["cam_times"]))
    idx = t(shared["indices"])
    rb = cams.generate_rays(camera_indices=idx[:, 0:1], coords=idx[:, 1:3].float() + 0.5)
    frame = cams.generate_rays(camera_indices=FRAME_CAMERA)  # the meshgrid path (cameras.py:300-418) must agree with the table path
    n = H * W
    assert torch.equal(frame.directions.reshape(n, 3), rb.directions[:n]) and torch.equal(frame.pixel_area.reshape(n, 1), rb.pixel_area[:n])
    assert torch.equal(rb.origins, t(shared["camera_to_worlds"])[idx[:, 0], :, 3])
    f = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    out = {"directions": f(rb.directions), "pixel_area": f(rb.pixel_area), "directions_norm": f(rb.metadata["directions_norm"]), "times": f(rb.times)}
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{k}: the reference's output is not finite (theta == 0 on a fisheye pixel?)"
    return out


def main():
    import_reference()
    from nerfstudio.cameras.cameras import Cameras, CameraType

    assert (CameraType.PERSPECTIVE.value, CameraType.FISHEYE.value, CameraType.EQUIRECTANGULAR.value) == (PERSPECTIVE, FISHEYE, EQUIRECTANGULAR)
    g17 = make_inputs()
    shared = {k: g17[k] for k in ("width", "height", "camera_to_worlds", "cam_times", "indices")}
    assert not LENS[0].any() and LENS[1:].any(axis=1).all()
    res = dict(shared)
    for prefix, tab in (("a_", TABLE_A), ("b_", TABLE_B), ("c_", TABLE_C)):
        # theta == 0 needs a pixel centre (or its +1 neighbour) exactly on the principal point: a half-integer cx AND cy
        fish = tab["camera_type"] == FISHEYE
        assert not ((np.modf(tab["cx"][fish])[0] == 0.5) & (np.modf(tab["cy"][fish])[0] == 0.5)).any(), "a fisheye camera's principal point is a pixel centre"
        rays = reference_rays(Cameras, shared, tab)
        if prefix == "b_":
            plain = reference_rays(Cameras, shared, tab, distortion=False)
            assert all(np.array_equal(rays[k], plain[k]) for k in rays), "equirectangular rays must not depend on the distortion rows"
        res.update({prefix + k: v for k, v in {**tab, **rays}.items()})
    out = os.path.join(ROOT, "tests", "golden", "g18_camera_types.npz")
    save_npz_reproducibly(out, res)
    for k, v in res.items():
        print(k, np.asarray(v).dtype, np.asarray(v).shape)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes the G16 camera-path fixture from the reference's own code (needs the reference tree; CPU only):

    python tools/gen_golden_camera_path.py     # writes tests/golden/g16_camera_path.json and g16_camera_path.npz

g16_camera_path.json: a camera-path dict as the viewer exports it (render_height / render_width / camera_path[*].camera_to_world, fov,
render_time), four cameras on an arc around the scene at 96 x 54.
g16_camera_path.npz: what NS/cameras/camera_paths.py:116-176 get_path_from_json returns for it (fx, fy, cx, cy, width, height,
camera_to_worlds, times) and Cameras.generate_rays(camera_indices=RAY_CAMERA) of that result (origins, directions, times, pixel_area).

The focal-length helper lives in the viewer utilities (NS/viewer/server/utils.py:48-60), whose module imports four packages of the viewer's
transport that this environment does not have; they are registered as empty modules first -- nothing of them is called.
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._refimport import import_reference  # noqa: E402

RAY_CAMERA = 2


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera-to-world 4x4 (camera looks down -z, y up), row-major list of 16."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return [float(v) for v in m.reshape(-1)]


def make_path():
    cams = []
    for k, (az, fov, t) in enumerate(((-0.6, 50.0, 0.0), (-0.2, 47.5, 0.25), (0.3, 42.0, 0.6), (0.7, 35.0, 1.0))):
        eye = (3.2 * math.sin(az), -3.2 * math.cos(az), 1.1 + 0.15 * k)
        cams.append({"camera_to_world": look_at(eye, target=(0.1 * k, 0.0, 0.0)), "fov": fov, "aspect": 96 / 54, "render_time": t})
    return {"render_height": 54, "render_width": 96, "camera_type": "perspective", "fps": 24, "seconds": len(cams) / 24, "camera_path": cams}


def main():
    for name in ("zmq", "msgpack", "msgpack_numpy", "umsgpack"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import_reference()
    from nerfstudio.cameras.camera_paths import get_path_from_json

    path = make_path()
    cams = get_path_from_json(path)
    rb = cams.generate_rays(camera_indices=RAY_CAMERA)
    f = lambda t: np.asarray(t.detach().cpu().numpy())
    res = {
        "fx": f(cams.fx), "fy": f(cams.fy), "cx": f(cams.cx), "cy": f(cams.cy), "width": f(cams.width), "height": f(cams.height),
        "camera_to_worlds": f(cams.camera_to_worlds), "times": f(cams.times), "ray_camera": np.int64(RAY_CAMERA),
        "ray_origins": f(rb.origins), "ray_directions": f(rb.directions), "ray_times": f(rb.times), "ray_pixel_area": f(rb.pixel_area),
    }
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "g16_camera_path.json"), "w") as fh:
        json.dump(path, fh, indent=1)
    np.savez_compressed(os.path.join(gold, "g16_camera_path.npz"), **res)
    for k, v in res.items():
        print(k, v.dtype, v.shape)


if __name__ == "__main__":
    main()

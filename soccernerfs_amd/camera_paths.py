"""Camera paths as the viewer exports them and `ns-render --traj filename` reads them: NS/cameras/camera_paths.py:116-176
(get_path_from_json) with the focal-length rule of NS/viewer/server/utils.py:48-60.  Pure host code: no kernel is involved.

Perspective, fisheye and equirectangular paths (the viewer's render panel offers all three); a caller says which types it can generate rays
for, and the default is perspective only.  Interpolated / spiral paths (camera_paths.py:30-113) are not built."""
import json
import math
from typing import Any, Dict, Sequence, Union

import torch

from .cameras import Cameras, CameraType

ALL_CAMERA_TYPES = ("perspective", "fisheye", "equirectangular")


def three_js_perspective_camera_focal_length(fov: float, image_height: int) -> float:
    """Focal length in pixels of a three.js perspective camera with vertical field of view `fov` (degrees); NS/viewer/server/utils.py:48-60.
    Evaluated in double precision, as the reference does; Cameras stores it as float32."""
    if fov is None:
        return 50
    pp_h = image_height / 2.0
    return pp_h / math.tan(fov * (math.pi / 180.0) / 2.0)


def load_camera_path(path_or_dict: Union[str, Dict[str, Any]]) -> Dict[str, Any]:
    """A camera-path dict, or the JSON file that holds one (scripts/render.py:188-190)."""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    with open(path_or_dict, "r", encoding="utf-8") as f:
        return json.load(f)


def get_path_from_json(camera_path: Dict[str, Any], camera_types: Sequence[str] = ("perspective",)) -> Cameras:
    """The trajectory of a camera-path dict as a Cameras table (host tensors; `.to(device)` moves it).

    camera_types: the path types the caller can render.  A "fisheye" or "equirectangular" path raises NotImplementedError unless it is listed:
    a caller whose rays come from Cameras.generate_rays / KPlanesRenderer passes camera_types=ALL_CAMERA_TYPES.  Any other string is a
    perspective path, as in the reference (camera_paths.py:133-140).  An equirectangular path has fx = W / 2, fy = H and reads no fov; a fisheye
    path takes the three.js focal length from fov like a perspective one (:149-157).

    render_height / render_width give height, width, cx = W / 2, cy = H / 2; every entry of camera_path["camera_path"] gives
    camera_to_world (16 numbers, row-major 4x4, the first three rows are used) and fov (degrees) -> fx = fy.  `times` exists only if ALL
    entries carry render_time (camera_paths.py:159-163)."""
    image_height = camera_path["render_height"]
    image_width = camera_path["render_width"]
    camera_type = camera_path.get("camera_type", "perspective")
    if camera_type in ("fisheye", "equirectangular") and camera_type not in camera_types:
        raise NotImplementedError(f"camera_type {camera_type!r} is not among camera_types={tuple(camera_types)!r}: a caller that generates such rays "
                                  "passes camera_types=camera_paths.ALL_CAMERA_TYPES")
    kind = {"fisheye": CameraType.FISHEYE, "equirectangular": CameraType.EQUIRECTANGULAR}.get(camera_type, CameraType.PERSPECTIVE)
    entries = camera_path["camera_path"]
    c2ws, focals, fys = [], [], []
    for camera in entries:
        c2ws.append(torch.tensor(camera["camera_to_world"], dtype=torch.float32).view(4, 4)[:3])
        if kind == CameraType.EQUIRECTANGULAR:
            focals.append(image_width / 2)
            fys.append(image_height)
        else:
            focals.append(three_js_perspective_camera_focal_length(camera["fov"], image_height))
    times = torch.tensor([camera["render_time"] for camera in entries], dtype=torch.float32) if all("render_time" in c for c in entries) else None
    focal = torch.tensor(focals, dtype=torch.float64).to(torch.float32)  # one rounding of the double value
    fy = torch.tensor(fys, dtype=torch.float64).to(torch.float32) if kind == CameraType.EQUIRECTANGULAR else focal.clone()
    return Cameras(torch.stack(c2ws, dim=0), focal, fy, image_width / 2, image_height / 2, int(image_width), int(image_height), times, camera_type=kind)

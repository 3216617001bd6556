"""CPU: camera paths (soccernerfs_amd/camera_paths.py) against what the reference's get_path_from_json (NS/cameras/camera_paths.py:116-176)
returned for the same path dict (G16: tests/golden/g16_camera_path.json -> g16_camera_path.npz, written by tools/gen_golden_camera_path.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g16():
    with open(os.path.join(GOLD, "g16_camera_path.json")) as f:
        path = json.load(f)
    return path, np.load(os.path.join(GOLD, "g16_camera_path.npz"))


def test_path_matches_reference():
    from soccernerfs_amd.camera_paths import get_path_from_json

    path, g = _g16()
    cams = get_path_from_json(path)
    M = len(path["camera_path"])
    assert len(cams) == M == g["fx"].shape[0]
    assert cams.width == int(g["width"][0, 0]) == path["render_width"] and cams.height == int(g["height"][0, 0]) == path["render_height"]
    assert (g["width"] == cams.width).all() and (g["height"] == cams.height).all()
    for k in ("fx", "fy"):
        got, want = getattr(cams, k), torch.from_numpy(g[k]).reshape(-1)
        assert got.dtype == torch.float32 and want.dtype == torch.float64
        # the reference holds the focal length in float64; Cameras holds float32.  Rounding a double to the nearest float moves it by at most
        # half an ulp, so one fp32 ulp of the value bounds the difference whatever the rounding of tan() underneath (derived, not measured)
        ulp = torch.from_numpy(np.spacing(g[k].reshape(-1).astype(np.float32))).double()
        assert bool(((got.double() - want).abs() <= ulp).all()), (got, want)
    for k in ("cx", "cy"):
        assert torch.equal(getattr(cams, k), torch.from_numpy(g[k]).reshape(-1))
    assert torch.equal(cams.camera_to_worlds, torch.from_numpy(g["camera_to_worlds"]))
    assert cams.times is not None and torch.equal(cams.times, torch.from_numpy(g["times"]).reshape(-1))
    assert cams.cx[0] == cams.width / 2 and cams.cy[0] == cams.height / 2


def test_camera_to_world_uses_first_three_rows_row_major():
    from soccernerfs_amd.camera_paths import get_path_from_json

    path, _ = _g16()
    cams = get_path_from_json(path)
    for k, entry in enumerate(path["camera_path"]):
        want = torch.tensor(entry["camera_to_world"], dtype=torch.float32).view(4, 4)[:3]
        assert torch.equal(cams.camera_to_worlds[k], want)


def test_times_need_every_entry():
    from soccernerfs_amd.camera_paths import get_path_from_json

    path, _ = _g16()
    p = copy.deepcopy(path)
    del p["camera_path"][1]["render_time"]
    assert get_path_from_json(p).times is None
    assert get_path_from_json(path).times is not None


def test_default_type_is_perspective_and_others_raise():
    from soccernerfs_amd.camera_paths import get_path_from_json

    path, _ = _g16()
    p = copy.deepcopy(path)
    del p["camera_type"]
    assert len(get_path_from_json(p)) == len(path["camera_path"])
    for kind in ("fisheye", "equirectangular"):
        p = copy.deepcopy(path)
        p["camera_type"] = kind
        with pytest.raises(NotImplementedError):
            get_path_from_json(p)


def test_load_camera_path_reads_files_and_dicts(tmp_path):
    from soccernerfs_amd.camera_paths import load_camera_path

    path, _ = _g16()
    assert load_camera_path(path) is path
    fn = tmp_path / "path.json"
    fn.write_text(json.dumps(path))
    assert load_camera_path(str(fn)) == path

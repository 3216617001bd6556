"""CPU: the camera types' references and plumbing.  The float64 restatement (tests/camera_types_reference.py) against the reference's own float32
rays of fisheye, equirectangular and mixed tables (G18, tools/gen_golden_camera_types.py); the theta == 0 rule; the entries added to ABI 16
revision 2; CameraType and the camera-model table; camera paths, the dataparser and the sphere-uniform pixel draw on the host."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import _measure
from tests import camera_types_reference as CR
from tests import lens_reference as LR
from tests.conftest import GOLDEN, ROOT

NEW = ["snerf_raygen_cam", "snerf_raygen_frame_cam", "snerf_sample_pixels_sphere"]
SPHERE_SEED, SPHERE_H, SPHERE_BAND = 18, 54, 1e-4
_SCRATCH = os.path.dirname(_measure._OUT)


@pytest.fixture(scope="module")
def g18():
    z = np.load(os.path.join(GOLDEN, "g18_camera_types.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref64(g18):
    return {p: CR.generate_rays(**CR.table(g18, p)) for p in ("a_", "b_", "c_")}


def _group(g, p):
    return {k: g[p + k] for k in ("directions", "directions_norm", "pixel_area")}


def test_fixture_layout(g18):
    g = g18
    n = int(g["width"]) * int(g["height"])
    assert (int(g["width"]), int(g["height"])) == (96, 54) and g["indices"].shape == (n + 4 * 512, 3) == (7232, 3)
    assert (g["indices"][:n, 0] == 3).all()
    g17 = np.load(os.path.join(GOLDEN, "g17_lens.npz"), allow_pickle=False)
    for k in ("indices", "camera_to_worlds", "cam_times"):
        assert np.array_equal(g[k], g17[k]), k
    assert g["a_camera_type"].tolist() == [2] * 4 and g["b_camera_type"].tolist() == [3] * 4 and g["c_camera_type"].tolist() == [1, 2, 3, 2]
    assert g["a_fx"].tolist() == [40, 45, 36, 50] and g["a_fy"].tolist() == [41, 45, 37, 49]
    assert np.array_equal(g["a_cx"], g17["cx"]) and np.array_equal(g["a_cy"], g17["cy"])
    assert np.array_equal(g["a_distortion"], np.float32(0.25) * g17["distortion"]) and not g["a_distortion"][0].any()
    for k, v in (("fx", 48), ("fy", 54), ("cx", 48), ("cy", 27)):
        assert (g["b_" + k] == v).all()
        assert np.array_equal(g["c_" + k], np.where(np.arange(4) == 2, g["b_" + k], g["a_" + k])), k
    assert np.array_equal(g["b_distortion"], g["a_distortion"]) and np.array_equal(g["c_distortion"], g["a_distortion"])
    assert all(np.isfinite(g[p + k]).all() for p in ("a_", "b_", "c_") for k in ("directions", "pixel_area", "directions_norm", "times"))
    assert os.path.getsize(os.path.join(GOLDEN, "g18_camera_types.npz")) < 512 * 1024


def test_float64_restatement_against_the_reference_rays(g18, ref64):
    """E32, the largest deviation of the reference's float32 rays from the float64 restatement, per table and group: positive (the two are not
    the same numbers), of float32 size (the restatement is the same function), and recorded.  On the CPU that wrote G18: directions 2.3e-7
    (fisheye) / 2.7e-7 (equirectangular), norm 1.6e-7 / 1.9e-7, pixel area 1.6e-5 / 3.2e-5."""
    record = {}
    for p in ("a_", "b_", "c_"):
        r = ref64[p]
        e32 = LR.deviations(_group(g18, p), r)
        record[p[0]] = e32
        print(p, e32, "min fisheye theta", r["min_theta"])
        assert all(v > 0 for v in e32.values()), e32
        # float32 has eps 6e-8; the directions are unit vectors formed by ~10 roundings, the pixel area by a difference of neighbouring unit
        # vectors ~1/50 apart (amplification ~50 per factor): a wrong formula is off by 1e-2 or more
        assert e32["directions"] <= 1e-6 and e32["directions_norm"] <= 1e-6 and e32["pixel_area"] <= 1e-4, e32
        assert np.array_equal(g18[p + "times"].astype(np.float64), r["times"])
        assert np.array_equal(r["origins"], g18["camera_to_worlds"].astype(np.float64)[g18["indices"][:, 0], :, 3])
    assert ref64["a_"]["min_theta"] > 1e-3  # the fixture stays away from theta == 0, where the reference gives NaN
    try:
        os.makedirs(_SCRATCH, exist_ok=True)
        with open(os.path.join(_SCRATCH, "r13_camera_types_e32.json"), "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
    except OSError:
        pass
    # the type matters: the perspective directions of table A's pixels are far away
    t = CR.table(g18, "a_")
    pin = CR.generate_rays(**{**t, "camera_type": 1})
    assert np.abs(pin["directions"] - ref64["a_"]["directions"]).max() > 1e-1
    # the mixed table is its parts: camera 0 perspective through the lens, 1 and 3 from A, 2 from B
    c, cam = ref64["c_"], g18["indices"][:, 0]
    lens = LR.generate_rays(t["indices"], t["fx"], t["fy"], t["cx"], t["cy"], t["c2w"], t["times"], t["distortion"])
    for k in ("directions", "pixel_area", "directions_norm"):
        assert np.array_equal(c[k][cam == 0], lens[k][cam == 0]), k
        assert np.array_equal(c[k][(cam == 1) | (cam == 3)], ref64["a_"][k][(cam == 1) | (cam == 3)]), k
        assert np.array_equal(c[k][cam == 2], ref64["b_"][k][cam == 2]), k


def test_equirectangular_ignores_the_distortion_rows(g18, ref64):
    t = CR.table(g18, "b_")
    assert t["distortion"][1:].any(axis=1).all()
    plain = CR.generate_rays(**{**t, "distortion": None})
    for k in ("directions", "pixel_area", "directions_norm", "coords"):
        assert np.array_equal(plain[k], ref64["b_"][k]), k
    # ... and a fisheye table does not
    assert not np.array_equal(CR.generate_rays(**{**CR.table(g18, "a_"), "distortion": None})["directions"], ref64["a_"]["directions"])


def test_theta_zero_rule():
    """A pixel centre exactly on the principal point: the restatement has the kernel's branch, sin(theta) / theta := 1 -> (0, 0, -1); without the
    branch the expression is 0 * 0 / 0."""
    z = np.zeros(1)
    assert [float(v[0]) for v in CR.fisheye_direction(z, z)] == [0.0, 0.0, -1.0]
    with np.errstate(invalid="ignore"):
        assert np.isnan(z * np.sin(z) / z).all()  # what the reference's expression gives there
    c2w = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
    r = CR.generate_rays(np.array([[0, 7, 10], [0, 7, 9], [0, 6, 10]]), [9.0], [9.0], [10.5], [7.5], c2w, camera_type=CR.FISHEYE)
    assert r["min_theta"] == 0.0 and np.isfinite(r["directions"]).all() and np.isfinite(r["pixel_area"]).all()
    assert r["directions"][0].tolist() == [0.0, 0.0, -1.0] and r["pixel_area"][0, 0] > 0
    # rays 1 and 2 have the principal point as their +1 neighbour: their pixel area uses the branch too
    assert (r["pixel_area"] > 0).all()
    # the branch is continuous: theta = 1e-9 gives the same direction to 1e-18
    tiny = CR.fisheye_direction(np.array([1e-9]), z)
    assert abs(float(tiny[0][0]) - 1e-9) < 1e-18 and float(tiny[2][0]) == -1.0


def test_theta_is_clipped_at_the_float32_pi():
    x = np.array([4.0, 0.0, np.pi - 1e-3])
    dx, dy, dz = CR.fisheye_direction(x, np.array([0.0, -5.0, 0.0]))
    s = np.sin(CR.PI_CLIP)
    assert CR.PI_CLIP > np.pi and abs(s + 8.742278e-8) < 1e-13
    assert dx[0] == 4.0 * s / CR.PI_CLIP and dy[1] == -5.0 * s / CR.PI_CLIP and dz[0] == dz[1] == -np.cos(CR.PI_CLIP)
    assert abs(dx[2] - np.sin(x[2])) < 1e-15  # below the clip: x sin(x) / x


def test_new_entries_declared_exported_and_bound():
    from soccernerfs_amd import _lib

    raw = open(os.path.join(ROOT, "include", "snerf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", txt), s
        assert s in _lib.EXPORTS and hasattr(l, s), s
    assert l.snerf_raygen_cam.argtypes == [C.c_void_p, C.c_void_p] and l.snerf_raygen_frame_cam.argtypes == [C.c_void_p, C.c_void_p]
    assert l.snerf_sample_pixels_sphere.argtypes == l.snerf_sample_pixels_uniform.argtypes
    # no new revision: the entries are part of revision 2's surface
    assert int(re.search(r"#define\s+SNERF_ABI_REVISION\s+(\d+)", raw).group(1)) == _lib.ABI_REVISION == l.snerf_abi_revision() == 2
    assert int(re.search(r"#define\s+SNERF_ABI_VERSION\s+(\d+)", raw).group(1)) == _lib.ABI_VERSION == l.snerf_abi_version() == 16
    for name, value in (("PERSPECTIVE", 1), ("FISHEYE", 2), ("EQUIRECTANGULAR", 3)):
        assert int(re.search(r"#define\s+SNERF_CAMERA_" + name + r"\s+(\d+)", raw).group(1)) == value
    # the lens structs are prefixes of the new ones, field for field -- in the binding and in the header
    assert _lib.RaygenCamArgs._fields_[:len(_lib.RaygenLensArgs._fields_)] == _lib.RaygenLensArgs._fields_
    assert _lib.RaygenFrameCamArgs._fields_[:len(_lib.RaygenFrameLensArgs._fields_)] == _lib.RaygenFrameLensArgs._fields_
    assert _lib.RaygenCamArgs._fields_[len(_lib.RaygenLensArgs._fields_):] == [("camera_type", C.c_void_p), ("camera_type_stride", C.c_int32)]
    assert _lib.RaygenFrameCamArgs._fields_[len(_lib.RaygenFrameLensArgs._fields_):] == [("camera_type", C.c_int32), ("has_distortion", C.c_int32)]
    body = lambda name: re.sub(r"\s+", " ", re.search(r"typedef struct \{([^}]*)\} " + name + ";", txt).group(1)).strip()
    assert body("snerf_raygen_cam_args").startswith(body("snerf_raygen_lens_args"))
    assert body("snerf_raygen_frame_cam_args").startswith(body("snerf_raygen_frame_lens_args"))
    assert body("snerf_raygen_cam_args")[len(body("snerf_raygen_lens_args")):].strip() == "const int32_t* camera_type; int32_t camera_type_stride;"
    assert body("snerf_raygen_frame_cam_args")[len(body("snerf_raygen_frame_lens_args")):].strip() == "int32_t camera_type; int32_t has_distortion;"
    # snerf_raygen_lens_args: 152 + pointer + int32 = 164, padded to 168; + pointer, int32, padding to 8
    assert C.sizeof(_lib.RaygenLensArgs) == 168 and C.sizeof(_lib.RaygenCamArgs) == 168 + 8 + 4 + 4
    assert _lib.RaygenCamArgs.camera_type.offset == 168 and _lib.RaygenCamArgs.camera_type_stride.offset == 176
    assert _lib.RaygenCamArgs.distortion.offset == 152 and _lib.RaygenCamArgs.distortion_stride.offset == 160
    # snerf_raygen_frame_lens_args: 184 + 6 floats = 208; + two int32
    assert C.sizeof(_lib.RaygenFrameLensArgs) == 208 and C.sizeof(_lib.RaygenFrameCamArgs) == 208 + 8
    assert _lib.RaygenFrameCamArgs.camera_type.offset == 208 and _lib.RaygenFrameCamArgs.has_distortion.offset == 212


def test_new_entries_validate_their_arguments():
    """Null arguments, bad strides, a bad pixel range and a camera type outside 1..3 are refused on the host, before anything is launched."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    assert l.snerf_raygen_cam(None, None) < 0 and l.snerf_raygen_frame_cam(None, None) < 0
    a = _lib.RaygenCamArgs()
    a.R, a.camera_type_stride = 4, 2
    assert l.snerf_raygen_cam(C.byref(a), None) < 0 and b"camera_type_stride" in l.snerf_last_error()
    a.camera_type_stride, a.distortion_stride = 1, 5
    assert l.snerf_raygen_cam(C.byref(a), None) < 0 and b"distortion_stride" in l.snerf_last_error()
    a.distortion_stride = 0
    assert l.snerf_raygen_cam(C.byref(a), None) < 0 and b"null" in l.snerf_last_error()
    a.R = 0
    assert l.snerf_raygen_cam(C.byref(a), None) == 0  # nothing to do
    fa = _lib.RaygenFrameCamArgs()
    fa.W, fa.H, fa.p0, fa.p1 = 96, 54, 0, 10
    for bad in (0, 4, -1):
        fa.camera_type = bad
        assert l.snerf_raygen_frame_cam(C.byref(fa), None) < 0 and b"camera_type=%d" % bad in l.snerf_last_error()
    fa.camera_type, fa.p1 = 2, 96 * 54 + 1
    assert l.snerf_raygen_frame_cam(C.byref(fa), None) < 0 and b"pixel range" in l.snerf_last_error()
    fa.p1 = 10
    assert l.snerf_raygen_frame_cam(C.byref(fa), None) < 0 and b"null" in l.snerf_last_error()
    assert l.snerf_sample_pixels_sphere(None, 4, 1, 1, 1, None, None, None, None) < 0 and b"null" in l.snerf_last_error()
    assert l.snerf_sample_pixels_sphere(None, 4, 0, 1, 1, None, None, None, None) < 0


def test_camera_type_enum_and_model_table():
    from soccernerfs_amd.cameras import CAMERA_MODEL_TO_TYPE, CameraType

    assert [(t.name, t.value) for t in CameraType] == [("PERSPECTIVE", 1), ("FISHEYE", 2), ("EQUIRECTANGULAR", 3)]
    # NS/cameras/cameras.py:50-58, typed out
    want = {"SIMPLE_PINHOLE": "PERSPECTIVE", "PINHOLE": "PERSPECTIVE", "SIMPLE_RADIAL": "PERSPECTIVE", "RADIAL": "PERSPECTIVE", "OPENCV": "PERSPECTIVE",
            "OPENCV_FISHEYE": "FISHEYE", "EQUIRECTANGULAR": "EQUIRECTANGULAR"}
    assert {k: v.name for k, v in CAMERA_MODEL_TO_TYPE.items()} == want


def test_cameras_keep_the_type_and_flag_it_on_the_host(g18):
    from soccernerfs_amd.cameras import Cameras, CameraType

    g, t = g18, torch.from_numpy
    mk = lambda **kw: Cameras(t(g["camera_to_worlds"]), t(g["a_fx"]), t(g["a_fy"]), t(g["a_cx"]), t(g["a_cy"]), 96, 54, t(g["cam_times"]), **kw)
    plain = mk()
    assert plain.all_perspective is True and plain.camera_type.dtype == torch.int32 and plain.camera_type.tolist() == [1] * 4
    for given in (CameraType.FISHEYE, 2, torch.tensor([2, 2, 2, 2]), torch.tensor([[2], [2], [2], [2]]), torch.tensor(2)):
        cams = mk(camera_type=given)
        assert cams.all_perspective is False and cams.camera_type.dtype == torch.int32 and cams.camera_type.tolist() == [2] * 4
    mixed = mk(camera_type=t(g["c_camera_type"]), distortion_params=t(g["c_distortion"]))
    assert mixed.all_perspective is False and mixed.has_distortion is True and mixed.camera_type.tolist() == [1, 2, 3, 2]
    assert mk(camera_type=1).all_perspective is True and mk(camera_type=torch.ones(4, dtype=torch.int64)).all_perspective is True
    moved = mixed.to("cpu")
    assert moved.all_perspective is False and torch.equal(moved.camera_type, mixed.camera_type) and moved.has_distortion is True
    for bad in (0, 4, torch.tensor([1, 2, 3, 4]), torch.tensor([1, 2, 3]), 2.0, torch.tensor([2.0] * 4), "fisheye"):
        with pytest.raises(ValueError):
            mk(camera_type=bad)


def _g16():
    with open(os.path.join(GOLDEN, "g16_camera_path.json")) as f:
        path = json.load(f)
    return path, np.load(os.path.join(GOLDEN, "g16_camera_path.npz"))


def test_camera_paths_of_the_new_types():
    from soccernerfs_amd import camera_paths
    from soccernerfs_amd.camera_paths import ALL_CAMERA_TYPES, get_path_from_json

    path, g = _g16()
    assert ALL_CAMERA_TYPES == ("perspective", "fisheye", "equirectangular")
    base = get_path_from_json(path)
    assert base.all_perspective and torch.equal(get_path_from_json(path, camera_types=ALL_CAMERA_TYPES).fx, base.fx)
    W, H, M = path["render_width"], path["render_height"], len(path["camera_path"])
    for kind in ("fisheye", "equirectangular"):
        p = copy.deepcopy(path)
        p["camera_type"] = kind
        with pytest.raises(NotImplementedError, match="camera_types"):  # the plain call still refuses, and names the keyword
            get_path_from_json(p)
        with pytest.raises(NotImplementedError):
            get_path_from_json(p, camera_types=("perspective",))
        if kind == "equirectangular":
            for entry in p["camera_path"]:
                del entry["fov"]  # no fov is read (camera_paths.py:149-151)
        cams = get_path_from_json(p, camera_types=ALL_CAMERA_TYPES)
        assert len(cams) == M and (cams.width, cams.height) == (W, H) and cams.all_perspective is False
        assert torch.equal(cams.camera_to_worlds, base.camera_to_worlds) and torch.equal(cams.times, base.times)
        assert torch.equal(cams.cx, base.cx) and torch.equal(cams.cy, base.cy)
        if kind == "equirectangular":
            assert cams.camera_type.tolist() == [3] * M
            assert cams.fx.tolist() == [W / 2] * M and cams.fy.tolist() == [float(H)] * M and cams.fx.dtype == torch.float32
        else:
            assert cams.camera_type.tolist() == [2] * M
            assert torch.equal(cams.fx, base.fx) and torch.equal(cams.fy, base.fy)
            ulp = np.spacing(g["fx"].reshape(-1).astype(np.float32)).astype(np.float64)
            assert (np.abs(cams.fx.double().numpy() - g["fx"].reshape(-1)) <= ulp).all()  # G16's focal lengths (float64 there)
    # any other string is a perspective path, as in the reference (camera_paths.py:139-140)
    p = copy.deepcopy(path)
    p["camera_type"] = "something"
    assert get_path_from_json(p).all_perspective
    assert camera_paths.load_camera_path(path) is path


def test_dataparser_maps_the_camera_model(tmp_path):
    from soccernerfs_amd.dataparsers import BroadcaststyleDataParserConfig

    case = json.load(open(os.path.join(GOLDEN, "g14_dataparser.json")))[0]

    def parse(model, sub):
        d = tmp_path / sub
        d.mkdir()
        meta = json.loads(case["transforms"])
        assert "camera_model" not in meta
        if model is not None:
            meta["camera_model"] = model
        (d / "transforms.json").write_text(json.dumps(meta))
        for f in case["existing"]:
            (d / f).parent.mkdir(parents=True, exist_ok=True)
            (d / f).touch()
        return BroadcaststyleDataParserConfig(data=d, fps_downsample=case["fps_downsample"], **case.get("options", {})).setup().get_dataparser_outputs("train")

    base, fish, equi, ocv = parse(None, "base"), parse("OPENCV_FISHEYE", "fish"), parse("EQUIRECTANGULAR", "equi"), parse("OPENCV", "ocv")
    M = len(base.cameras)
    assert base.cameras.all_perspective and base.cameras.camera_type.tolist() == [1] * M and ocv.cameras.all_perspective
    assert fish.cameras.camera_type.tolist() == [2] * M and not fish.cameras.all_perspective
    assert equi.cameras.camera_type.tolist() == [3] * M
    for out in (fish, equi, ocv):
        for k in ("camera_to_worlds", "fx", "fy", "cx", "cy", "times", "ids", "distortion_params"):
            assert torch.equal(getattr(out.cameras, k), getattr(base.cameras, k)), k
        assert (out.cameras.width, out.cameras.height, out.cameras.has_distortion) == (base.cameras.width, base.cameras.height, base.cameras.has_distortion)
    with pytest.raises(NotImplementedError):
        parse("FULL_OPENCV_NOT_A_MODEL", "bad")


def _sphere_u():
    return torch.rand(4096, 3, generator=torch.Generator().manual_seed(SPHERE_SEED))


def sphere_band(u1):
    """Rows of u1 whose H * acos(1 - 2 u1) / pi in float64 lies within SPHERE_BAND of an integer: there float32 may floor to the neighbour."""
    v = CR.sphere_rows(u1.double().numpy(), SPHERE_H)
    return np.abs(v - np.round(v)) <= SPHERE_BAND, np.floor(v).astype(np.int64)


def test_sphere_draw_on_the_host():
    """The reference's float32 expression (pixel_samplers.py:259-265) against its float64 evaluation on the same u."""
    u = _sphere_u()
    M, H, W = 5, SPHERE_H, 96
    idx = torch.floor(torch.stack((u[:, 0], torch.acos(1 - 2 * u[:, 1]) / torch.pi, u[:, 2]), dim=-1) * torch.tensor([M, H, W])).long()
    band, rows64 = sphere_band(u[:, 1])
    print("rows in the band:", int(band.sum()))
    assert band.sum() <= 8  # the seed's condition
    assert np.array_equal(idx[:, 1].numpy()[~band], rows64[~band])
    assert (np.abs(idx[:, 1].numpy() - rows64) <= 1).all()
    assert int(idx[:, 1].max()) < H and int(idx[:, 1].min()) >= 0 and int(rows64.max()) < H
    assert torch.equal(idx[:, 0], torch.floor(u[:, 0] * M).long()) and torch.equal(idx[:, 2], torch.floor(u[:, 2] * W).long())
    # uniform on the sphere: the rows follow sin(phi) / 2, so the middle third of the image holds half the draws (cos(pi / 3) = 1 / 2) ...
    mid = ((rows64 >= H // 3) & (rows64 < 2 * H // 3)).mean()
    assert abs(mid - 0.5) < 4 * np.sqrt(0.25 / 4096)  # four standard deviations of a binomial share
    # ... where the uniform draw would put a third
    assert abs(mid - 1 / 3) > 0.1


def test_equirectangular_sampler_is_a_pixel_sampler():
    from soccernerfs_amd.pixel_samplers import EquirectangularPixelSampler, PixelSampler

    s = EquirectangularPixelSampler(num_rays_per_batch=64)
    assert isinstance(s, PixelSampler) and s.num_rays_per_batch == 64
    with pytest.raises(NotImplementedError):  # with a mask the reference falls back to the base method, which is not built here
        s.sample_method(8, 2, 4, 4, mask=torch.ones(2, 4, 4, 1), device="cpu")

"""CPU: the lens path's references and plumbing.  The float64 restatement (tests/lens_reference.py) against the reference's own float32 rays
(G17, tools/gen_golden_lens.py); the undistortion against the forward model, independent of the solver; ABI 16 revision 2; and what Cameras
keeps of the coefficients."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import lens_reference as LR
from tests.conftest import GOLDEN, ROOT

NEW = ["snerf_raygen_lens", "snerf_raygen_frame_lens"]


@pytest.fixture(scope="module")
def g17():
    z = np.load(os.path.join(GOLDEN, "g17_lens.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref64(g17):
    g = g17
    return LR.generate_rays(g["indices"], g["fx"], g["fy"], g["cx"], g["cy"], g["camera_to_worlds"], g["cam_times"], g["distortion"])


def test_fixture_layout(g17):
    g = g17
    n = int(g["width"]) * int(g["height"])
    assert (int(g["width"]), int(g["height"])) == (96, 54) and g["indices"].shape == (n + 4 * 512, 3) == (7232, 3)
    ys, xs = np.meshgrid(np.arange(54), np.arange(96), indexing="ij")
    assert (g["indices"][:n, 0] == 3).all() and (g["indices"][:n, 1] == ys.reshape(-1)).all() and (g["indices"][:n, 2] == xs.reshape(-1)).all()
    for c in range(4):
        assert (g["indices"][n + 512 * c:n + 512 * (c + 1), 0] == c).all()
    assert not g["distortion"][0].any() and g["distortion"][1:].any(axis=1).all()
    assert os.path.getsize(os.path.join(GOLDEN, "g17_lens.npz")) < 256 * 1024


def test_float64_reference_against_the_reference_rays(g17, ref64):
    """Every output of the float64 restatement within 1e-6 absolute (1e-4 relative for the pixel area) of the reference's float32 values, and
    the inputs stay a hundred times clear of the solver's gate."""
    g, r = g17, ref64
    assert r["min_denominator"] >= 0.1
    assert r["last_residual"] < 1e-12
    print("min |denominator|", r["min_denominator"], "last residual", r["last_residual"])
    assert np.abs(g["directions"].astype(np.float64) - r["directions"]).max() <= 1e-6
    assert np.abs(g["directions_norm"].astype(np.float64) - r["directions_norm"]).max() <= 1e-6
    assert (np.abs(g["pixel_area"].astype(np.float64) - r["pixel_area"]) / r["pixel_area"]).max() <= 1e-4
    assert np.array_equal(g["times"].astype(np.float64), r["times"])
    assert np.array_equal(r["origins"], g["camera_to_worlds"].astype(np.float64)[g["indices"][:, 0], :, 3])
    # the coefficients matter: the pinhole directions of the same pixels are 3e-2 .. 6e-2 away
    pin = LR.generate_rays(g["indices"], g["fx"], g["fy"], g["cx"], g["cy"], g["camera_to_worlds"])
    assert np.abs(pin["directions"] - r["directions"]).max() > 1e-2
    # ... and an all-zero row is the pinhole camera
    zero = g["indices"][:, 0] == 0
    assert np.array_equal(pin["directions"][zero], r["directions"][zero]) and np.array_equal(pin["pixel_area"][zero], r["pixel_area"][zero])


def test_undistortion_round_trip_through_the_forward_model(g17, ref64):
    """xd = x d + 2 p1 x y + p2 (r + 2 x^2) and its y twin, applied to the undistorted coordinates of all three pairs, return the pixel's
    normalised coordinates: checks the solver's fixed point without using the solver's residual."""
    g = g17
    want = LR.coord_stack(g["indices"], g["fx"], g["fy"], g["cx"], g["cy"])
    back = LR.distort(ref64["undistorted"], g["distortion"].astype(np.float64)[g["indices"][:, 0]][None])
    assert np.abs(back - want).max() <= 1e-12
    moved = np.abs(ref64["undistorted"] - want).max()
    assert moved > 1e-2, moved


def test_revision_2_agrees_between_header_library_and_binding():
    from soccernerfs_amd import _lib

    txt = open(os.path.join(ROOT, "include", "snerf.h")).read()
    l = _lib.lib()
    assert int(re.search(r"#define\s+SNERF_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION == l.snerf_abi_version() == 16
    assert int(re.search(r"#define\s+SNERF_ABI_REVISION\s+(\d+)", txt).group(1)) == _lib.ABI_REVISION == l.snerf_abi_revision() == 2


def test_lens_entries_declared_exported_and_bound():
    from soccernerfs_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snerf.h")).read(), flags=re.S)
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", txt), s
        assert s in _lib.EXPORTS and hasattr(l, s), s
        assert getattr(l, s).argtypes == [C.c_void_p, C.c_void_p], s
    fields = lambda cls: dict((f[0], f[1]) for f in cls._fields_)
    la, fa = fields(_lib.RaygenLensArgs), fields(_lib.RaygenFrameLensArgs)
    # the existing structs are prefixes of the new ones, field for field
    assert _lib.RaygenLensArgs._fields_[:len(_lib.RaygenArgs._fields_)] == _lib.RaygenArgs._fields_
    assert _lib.RaygenFrameLensArgs._fields_[:len(_lib.RaygenFrameArgs._fields_)] == _lib.RaygenFrameArgs._fields_
    assert la["distortion"] is C.c_void_p and la["distortion_stride"] is C.c_int32 and la["near_plane"] is C.c_float and la["R"] is C.c_int32
    assert fa["distortion"] is C.c_float * 6 and fa["fx"] is C.c_float and fa["W"] is C.c_int32 and fa["p0"] is C.c_int64
    # snerf_raygen_args: 7 pointers, 3 int32 + 7 floats, 7 pointers = 152; + pointer, int32, padding to 8
    assert C.sizeof(_lib.RaygenArgs) == 152 and C.sizeof(_lib.RaygenLensArgs) == 152 + 8 + 4 + 4
    assert _lib.RaygenLensArgs.distortion.offset == 152 and _lib.RaygenLensArgs.distortion_stride.offset == 160
    # snerf_raygen_frame_args is 184 bytes (tests/test_abi_revision_cpu.py) and stays; + 6 floats
    assert C.sizeof(_lib.RaygenFrameArgs) == 184 and C.sizeof(_lib.RaygenFrameLensArgs) == 184 + 24
    assert _lib.RaygenFrameLensArgs.distortion.offset == 184


def test_lens_entries_validate_their_arguments():
    """Null arguments, a negative ray count and a stride outside {0, 6} are refused on the host, before anything is launched."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    assert l.snerf_raygen_lens(None, None) != 0 and l.snerf_raygen_frame_lens(None, None) != 0
    a = _lib.RaygenLensArgs()
    a.R, a.distortion_stride = 4, 5
    assert l.snerf_raygen_lens(C.byref(a), None) != 0 and b"distortion_stride" in l.snerf_last_error()
    a.distortion_stride = 6
    assert l.snerf_raygen_lens(C.byref(a), None) != 0 and b"null" in l.snerf_last_error()
    a.R = -1
    assert l.snerf_raygen_lens(C.byref(a), None) != 0
    fa = _lib.RaygenFrameLensArgs()
    fa.W, fa.H, fa.p0, fa.p1 = 96, 54, 0, 96 * 54 + 1
    assert l.snerf_raygen_frame_lens(C.byref(fa), None) != 0 and b"pixel range" in l.snerf_last_error()
    fa.p1 = 10
    assert l.snerf_raygen_frame_lens(C.byref(fa), None) != 0 and b"null" in l.snerf_last_error()


def test_cameras_keep_the_coefficients_and_flag_them_on_the_host(g17):
    from soccernerfs_amd.cameras import Cameras

    g = g17
    t = torch.from_numpy
    mk = lambda dp: Cameras(t(g["camera_to_worlds"]), t(g["fx"]), t(g["fy"]), t(g["cx"]), t(g["cy"]), 96, 54, t(g["cam_times"]), distortion_params=dp)
    none, zero, lens = mk(None), mk(torch.zeros(4, 6)), mk(t(g["distortion"]))
    assert none.distortion_params is None and none.has_distortion is False
    assert zero.has_distortion is False and zero.distortion_params.shape == (4, 6)
    assert lens.has_distortion is True and torch.equal(lens.distortion_params, t(g["distortion"]))
    one = Cameras(t(g["camera_to_worlds"][1:2]), 70.0, 70.0, 47.3, 26.5, 96, 54, distortion_params=t(g["distortion"][1]))
    assert one.has_distortion is True and one.distortion_params.shape == (1, 6)
    assert mk(t(g["distortion"][2])).distortion_params.shape == (4, 6)  # one row for all cameras
    for cams in (none, zero, lens):
        moved = cams.to("cpu")
        assert moved.has_distortion is cams.has_distortion
        assert (moved.distortion_params is None) if cams.distortion_params is None else torch.equal(moved.distortion_params, cams.distortion_params)
    with pytest.raises(ValueError):
        mk(torch.zeros(3, 6))

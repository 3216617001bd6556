"""Float64 NumPy restatement of the reference's ray generation for its three camera types, for the tests of snerf_raygen_cam /
snerf_raygen_frame_cam: Cameras._generate_rays_from_coords (NS/cameras/cameras.py:596-741), every statement once.  The coordinate stack and
the undistortion are those of tests/lens_reference.py (which also owns deviations(), the three figures the tests bound); this module adds what
depends on the camera's type:

  * the undistortion is skipped for equirectangular cameras, even with a non-zero row (cameras.py:645-647);
  * PERSPECTIVE (:665-670) d = (x, y, -1);
  * FISHEYE (:672-683) theta = clip(sqrt(x^2 + y^2), 0, pi), d = (x sin(theta) / theta, y sin(theta) / theta, -cos(theta));
  * EQUIRECTANGULAR (:685-696) theta = -pi x, phi = pi (0.5 - y), d = (-sin(theta) sin(phi), cos(phi), -cos(theta) sin(phi)).

Two points where this is not the reference's text read in float64:

  * theta == 0.  The reference's x * sin(theta) / theta is 0 * 0 / 0 = NaN for a pixel centre exactly on the principal point.  The kernel
    returns the limit (0, 0, -1), sin(theta) / theta := 1; fisheye_direction has the same branch, on the same condition.
  * the clip.  torch.clip(theta, 0.0, math.pi) on a float32 tensor clips at float32(pi) = PI_CLIP, which lies 8.7e-8 ABOVE pi, so a clipped ray
    has sin(theta) = -8.7e-8, not 1.2e-16, and x sin(theta) / theta is of that order, not zero.  PI_CLIP is therefore an input constant of the
    computation, like an intrinsic, and is used as such here; clipping at float64 pi would be another function on the clipped rays (their
    pixel area, a difference of such directions, would differ by many orders of magnitude), not a more precise one.  The equirectangular
    branch multiplies by pi, where float32(pi) is an ordinary rounding of 3e-8 relative: float64 pi there.

generate_rays(dtype=np.float32) evaluates the same statements in float32 NumPy for a lens-free table: the float32 yardstick for a camera no
fixture holds.
"""
import numpy as np

from tests import lens_reference as LR

PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3
PI_CLIP = float(np.float32(np.pi))


def fisheye_direction(x, y):
    """cameras.py:676-683 on coordinates [...]: -> (dx, dy, dz)."""
    dt = x.dtype.type
    theta = np.clip(np.sqrt(x * x + y * y), dt(0.0), dt(PI_CLIP))
    s = np.sin(theta)
    zero = theta == 0  # the kernel's branch: sin(theta) / theta := 1
    safe = np.where(zero, dt(1.0), theta)
    return np.where(zero, x, x * s / safe), np.where(zero, y, y * s / safe), -np.cos(theta)


def equirectangular_direction(x, y):
    """cameras.py:691-696."""
    dt = x.dtype.type
    theta = -dt(np.pi) * x
    phi = dt(np.pi) * (dt(0.5) - y)
    return -np.sin(theta) * np.sin(phi), np.cos(phi), -np.cos(theta) * np.sin(phi)


def camera_directions(stack, kinds):
    """stack [3,R,2] undistorted coordinates, kinds int [R] -> camera-space directions [3,R,3] (cameras.py:663-700)."""
    bad = set(np.unique(kinds).tolist()) - {PERSPECTIVE, FISHEYE, EQUIRECTANGULAR}
    if bad:
        raise ValueError(f"Camera type {sorted(bad)[0]} not supported.")
    x, y = stack[..., 0], stack[..., 1]
    out = np.stack([x, y, -np.ones_like(x)], -1)
    for kind, fn in ((FISHEYE, fisheye_direction), (EQUIRECTANGULAR, equirectangular_direction)):
        m = kinds == kind
        if m.any():
            out[:, m] = np.stack(fn(x[:, m], y[:, m]), -1)
    return out


def coord_stack(indices, fx, fy, cx, cy, dtype=np.float64):
    """lens_reference.coord_stack (cameras.py:599-632) in `dtype`."""
    indices = np.asarray(indices, np.int64)
    c = indices[:, 0]
    y, x = indices[:, 1].astype(dtype) + dtype(0.5), indices[:, 2].astype(dtype) + dtype(0.5)
    fx, fy, cx, cy = (np.asarray(v, dtype)[c] for v in (fx, fy, cx, cy))
    one = dtype(1)
    return np.stack([np.stack([(x - cx) / fx, -(y - cy) / fy], -1), np.stack([(x - cx + one) / fx, -(y - cy) / fy], -1),
                     np.stack([(x - cx) / fx, -(y - cy + one) / fy], -1)], 0)


def generate_rays(indices, fx, fy, cx, cy, c2w, times=None, distortion=None, camera_type=None, dtype=np.float64):
    """indices int [R,3] (camera, row, col); fx, fy, cx, cy [M]; c2w [M,3,4]; times [M]; distortion None, [6] or [M,6]; camera_type None
    (perspective), an int or [M].  -> dict of `dtype` arrays: origins [R,3], directions [R,3], pixel_area [R,1], directions_norm [R,1], times
    [R,1] (if times is given), coords [3,R,2] (after the undistortion), and min_theta: the smallest fisheye theta of any pair (inf if none)."""
    indices = np.asarray(indices, np.int64)
    c = indices[:, 0]
    M = np.asarray(c2w).shape[0]
    kinds = np.broadcast_to(np.asarray(PERSPECTIVE if camera_type is None else camera_type, np.int64).reshape(-1), (M,))[c]
    stack = coord_stack(indices, fx, fy, cx, cy, dtype)
    if distortion is not None:
        assert dtype is np.float64, "the undistortion is restated in float64 only"
        assert np.array_equal(stack, LR.coord_stack(indices, fx, fy, cx, cy))
        k = np.asarray(distortion, np.float64)
        k = k[c] if k.ndim == 2 else np.broadcast_to(k, (len(c), 6))
        lens = kinds != EQUIRECTANGULAR  # "Do not apply distortion for equirectangular images"
        if lens.any():
            und, min_den, _ = LR.undistort(stack[:, lens], k[lens][None])
            assert min_den >= LR.MIN_DENOMINATOR, f"min |denominator| = {min_den}: too close to the solver's gate for a float32 comparison"
            stack = stack.copy()
            stack[:, lens] = und
    fish = kinds == FISHEYE
    min_theta = float(np.sqrt((stack[:, fish] ** 2).sum(-1)).min()) if fish.any() else np.inf
    m = np.asarray(c2w, dtype)[c]                                                 # [R,3,4]
    dirs = camera_directions(stack, kinds)                                        # [3,R,3]
    rot = dirs[..., None, :] * m[None, :, :3, :3]
    dirs = (rot[..., 0] + rot[..., 1]) + rot[..., 2]                              # cameras.py:712-714
    norm = np.maximum(np.sqrt((dirs[..., 0:1] * dirs[..., 0:1] + dirs[..., 1:2] * dirs[..., 1:2]) + dirs[..., 2:3] * dirs[..., 2:3]),
                      dtype(np.finfo(np.float64).eps * 4))                        # normalize_with_norm
    dirs = dirs / norm
    sq = lambda d: np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    dx, dy = sq(dirs[0] - dirs[1]), sq(dirs[0] - dirs[2])
    out = {"origins": m[:, :3, 3], "directions": dirs[0], "pixel_area": (dx * dy)[:, None], "directions_norm": norm[0], "coords": stack,
           "min_theta": min_theta}
    if times is not None:
        out["times"] = np.asarray(times, dtype)[c][:, None]
    return out


def table(g, prefix):
    """The arguments of generate_rays for table `prefix` ("a_", "b_", "c_") of the G18 fixture."""
    return dict(indices=g["indices"], fx=g[prefix + "fx"], fy=g[prefix + "fy"], cx=g[prefix + "cx"], cy=g[prefix + "cy"], c2w=g["camera_to_worlds"],
                times=g["cam_times"], distortion=g[prefix + "distortion"], camera_type=g[prefix + "camera_type"])


def sphere_rows(u1, height, dtype=np.float64):
    """The row of EquirectangularPixelSampler.sample_method (NS/data/pixel_samplers.py:259-265): H * acos(1 - 2 u1) / pi before the floor, in
    `dtype` with the reference's order of operations ((acos(1 - 2 u) / pi) * H)."""
    u1 = np.asarray(u1, dtype)
    return (np.arccos(dtype(1) - dtype(2) * u1) / dtype(np.pi)) * dtype(height)

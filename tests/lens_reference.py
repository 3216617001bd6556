"""Float64 NumPy restatement of the reference's ray generation through a lens, for the tests of snerf_raygen_lens / snerf_raygen_frame_lens:
Cameras._generate_rays_from_coords for perspective cameras with distortion_params (NS/cameras/cameras.py:596-741) and
radial_and_tangential_undistort with its residual and Jacobian (NS/cameras/camera_utils.py:298-401).  The same kind of helper as
tests/per_ray_reference.py: every statement of the reference once, in float64, so that the float32 reference (the G17 fixture) and the
kernels can both be measured against it.

Condition on the inputs.  The solver takes a step only where |denominator| > 1e-3; an input near that threshold could branch differently in
float32 and float64, and the comparison would then measure the branch, not the arithmetic.  generate_rays therefore ASSERTS that the smallest
|denominator| of any iteration, pair and ray is at least MIN_DENOMINATOR = 0.1, a hundred times the gate, and returns that minimum.  A camera
a test adds must satisfy this by the choice of its coefficients.
"""
import numpy as np

EPS = 1e-3
ITERATIONS = 10
MIN_DENOMINATOR = 0.1


def residual_and_jacobian(x, y, xd, yd, k):
    """camera_utils.py:298-360.  k [..., 6] = k1 k2 k3 k4 p1 p2."""
    k1, k2, k3, k4, p1, p2 = (k[..., i] for i in range(6))
    r = x * x + y * y
    d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    fx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
    fy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
    d_r = k1 + r * (2.0 * k2 + r * (3.0 * k3 + r * 4.0 * k4))
    d_x = 2.0 * x * d_r
    d_y = 2.0 * y * d_r
    fx_x = d + d_x * x + 2.0 * p1 * y + 6.0 * p2 * x
    fx_y = d_y * x + 2.0 * p1 * x + 2.0 * p2 * y
    fy_x = d_x * y + 2.0 * p2 * y + 2.0 * p1 * x
    fy_y = d + d_y * y + 2.0 * p2 * x + 6.0 * p1 * y
    return fx, fy, fx_x, fx_y, fy_x, fy_y


def undistort(coords, k):
    """camera_utils.py:363-401: coords [..., 2], k broadcastable to [..., 6] -> (undistorted [..., 2], min |denominator| over all iterations,
    max |residual| after the last step)."""
    coords, k = np.asarray(coords, np.float64), np.asarray(k, np.float64)
    xd, yd = coords[..., 0], coords[..., 1]
    x, y = xd.copy(), yd.copy()
    min_den = np.inf
    for _ in range(ITERATIONS):
        fx, fy, fx_x, fx_y, fy_x, fy_y = residual_and_jacobian(x, y, xd, yd, k)
        den = fy_x * fx_y - fx_x * fy_y
        xn = fx * fy_y - fy * fx_y
        yn = fy * fx_x - fx * fy_x
        ok = np.abs(den) > EPS
        safe = np.where(ok, den, 1.0)
        x = x + np.where(ok, xn / safe, 0.0)
        y = y + np.where(ok, yn / safe, 0.0)
        if den.size:
            min_den = min(min_den, float(np.abs(den).min()))
    fx, fy = residual_and_jacobian(x, y, xd, yd, k)[:2]
    res = float(max(np.abs(fx).max(), np.abs(fy).max())) if fx.size else 0.0
    return np.stack([x, y], -1), min_den, res


def distort(coords, k):
    """The forward model on its own (the comment of camera_utils.py:333-335): undistorted [..., 2] -> distorted [..., 2].  Written from the
    formula, not from the solver's residual, for the round-trip test."""
    coords, k = np.asarray(coords, np.float64), np.asarray(k, np.float64)
    x, y = coords[..., 0], coords[..., 1]
    k1, k2, k3, k4, p1, p2 = (k[..., i] for i in range(6))
    r = x ** 2 + y ** 2
    d = 1.0 + k1 * r + k2 * r ** 2 + k3 * r ** 3 + k4 * r ** 4
    xd = x * d + 2.0 * p1 * x * y + p2 * (r + 2.0 * x ** 2)
    yd = y * d + 2.0 * p2 * x * y + p1 * (r + 2.0 * y ** 2)
    return np.stack([xd, yd], -1)


def coord_stack(indices, fx, fy, cx, cy):
    """cameras.py:599-632: the normalised coordinates of the pixel centre and of its x + 1 and y + 1 neighbours, [3, R, 2]."""
    indices = np.asarray(indices, np.int64)
    c = indices[:, 0]
    y, x = indices[:, 1].astype(np.float64) + 0.5, indices[:, 2].astype(np.float64) + 0.5
    fx, fy, cx, cy = (np.asarray(v, np.float64)[c] for v in (fx, fy, cx, cy))
    coord = np.stack([(x - cx) / fx, -(y - cy) / fy], -1)
    coord_x = np.stack([(x - cx + 1) / fx, -(y - cy) / fy], -1)
    coord_y = np.stack([(x - cx) / fx, -(y - cy + 1) / fy], -1)
    return np.stack([coord, coord_x, coord_y], 0)


def generate_rays(indices, fx, fy, cx, cy, c2w, times=None, distortion=None, check_condition=True):
    """indices int [R,3] (camera, row, col); fx, fy, cx, cy [M]; c2w [M,3,4]; times [M]; distortion None, [6] or [M,6].
    -> dict of float64 arrays: origins [R,3], directions [R,3], pixel_area [R,1], directions_norm [R,1], times [R,1] (if times is given),
    undistorted [3,R,2], and the floats min_denominator, last_residual."""
    indices = np.asarray(indices, np.int64)
    c = indices[:, 0]
    stack = coord_stack(indices, fx, fy, cx, cy)
    min_den, res = np.inf, 0.0
    if distortion is not None:
        k = np.asarray(distortion, np.float64)
        k = k[c] if k.ndim == 2 else np.broadcast_to(k, (len(c), 6))
        stack, min_den, res = undistort(stack, k[None])
        if check_condition:
            assert min_den >= MIN_DENOMINATOR, f"min |denominator| = {min_den}: too close to the solver's gate {EPS} for a float32 comparison"
    m = np.asarray(c2w, np.float64)[c]                                           # [R,3,4]
    dirs = np.concatenate([stack, -np.ones(stack.shape[:-1] + (1,))], -1)         # [3,R,3]
    dirs = np.sum(dirs[..., None, :] * m[None, :, :3, :3], axis=-1)               # cameras.py:712-714
    norm = np.maximum(np.sqrt(np.sum(dirs * dirs, -1, keepdims=True)), np.finfo(np.float64).eps * 4)  # normalize_with_norm
    dirs = dirs / norm
    dx = np.sqrt(np.sum((dirs[0] - dirs[1]) ** 2, -1))
    dy = np.sqrt(np.sum((dirs[0] - dirs[2]) ** 2, -1))
    out = {"origins": m[:, :3, 3], "directions": dirs[0], "pixel_area": (dx * dy)[:, None], "directions_norm": norm[0], "undistorted": stack,
           "min_denominator": min_den, "last_residual": res}
    if times is not None:
        out["times"] = np.asarray(times, np.float64)[c][:, None]
    return out


def deviations(got, want):
    """The three figures the lens tests bound: directions max |got - want|; directions_norm and pixel_area max |got - want| / |want|."""
    g = {k: np.asarray(got[k], np.float64).reshape(np.asarray(want[k]).shape) for k in ("directions", "directions_norm", "pixel_area")}
    rel = lambda k: float((np.abs(g[k] - want[k]) / np.abs(want[k])).max())
    return {"directions": float(np.abs(g["directions"] - want["directions"]).max()), "directions_norm": rel("directions_norm"),
            "pixel_area": rel("pixel_area")}

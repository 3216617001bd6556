"""GPU: fisheye and equirectangular cameras (snerf_raygen_cam, snerf_raygen_frame_cam, snerf_sample_pixels_sphere and everything above them).

References.  tests/camera_types_reference.py is the reference's ray generation for its three camera types in float64; G18
(tools/gen_golden_camera_types.py) holds the reference's own float32 rays of three tables of four cameras on G17's poses and ray table:
A fisheye with lens rows, B equirectangular with the same (ineffective) rows, C mixed (1, 2, 3, 2).

Bounds (the convention of tests/test_gpu_lens.py).  E32 = the largest deviation of G18's float32 rays from the float64 restatement on the same
7232 rays, per table and output group: directions absolute, directions_norm and pixel_area relative.  A kernel may deviate by MARGIN = 5 times
E32: that lets the device's sinf / cosf / sqrtf round differently from the host's and still fails a wrong formula by orders of magnitude.  The
bound is computed from the fixture below, nothing is typed in.  Origins and times are copies and are compared exactly.  Every call through the
C ABI writes into buffers with GUARD sentinel rows behind each output, which must stay untouched, and every live row must have been written
(Outs of tests/test_gpu_lens.py).  The measured deviations go to r13_camera_types_deviations.json in the scratch directory of tests/_measure.py
(the copy of this file's run: profiles/r13_camera_types_deviations.json).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _measure
from tests import camera_types_reference as CR
from tests import lens_reference as LR
from tests.conftest import GOLDEN
from tests.test_camera_types_cpu import SPHERE_H, _sphere_u, sphere_band
from tests.test_gpu_lens import AABB, DEV, KEYS, MARGIN, SMALL, Outs, _raygen, _raygen_frame, _stream

pytestmark = pytest.mark.gpu
W, H = 96, 54
TABLES = ("a_", "b_", "c_")
TABLE_KEYS = ("fx", "fy", "cx", "cy", "distortion", "camera_type")
GROUPS = ("directions", "directions_norm", "pixel_area")
_RECORD = {}
_SCRATCH = os.path.dirname(_measure._OUT)  # where the suite's measured deviations go; not part of the repository


def _record(name, dev):
    _RECORD[name] = dev
    try:
        os.makedirs(_SCRATCH, exist_ok=True)
        with open(os.path.join(_SCRATCH, "r13_camera_types_deviations.json"), "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture(scope="module")
def g18():
    z = np.load(os.path.join(GOLDEN, "g18_camera_types.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _host(g, p):
    """Table `p` of the fixture under the key names of tests/test_gpu_lens.py."""
    return {**{k: g[p + k] for k in TABLE_KEYS}, **{k: g[k] for k in ("camera_to_worlds", "cam_times", "indices")}}


@pytest.fixture(scope="module")
def host(g18):
    return {p: _host(g18, p) for p in TABLES}


@pytest.fixture(scope="module")
def ref64(g18):
    return {p: CR.generate_rays(**CR.table(g18, p)) for p in TABLES}


@pytest.fixture(scope="module")
def bound(g18, ref64):
    out = {}
    for p in TABLES:
        e32 = LR.deviations({k: g18[p + k] for k in GROUPS}, ref64[p])
        _record(f"reference_float32_vs_float64.{p[0]}", e32)
        assert all(v > 0 for v in e32.values())
        out[p] = {k: MARGIN * v for k, v in e32.items()}
    return out


@pytest.fixture(scope="module")
def table(host):
    return {p: {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in host[p].items()} for p in TABLES}


def _raygen_cam(table, indices, distortion="table", camera_type="table", collide=True, training=False, near_plane=0.05):
    """snerf_raygen_cam through the C ABI.  distortion: "table" (the table's rows), None (NULL) or a [M,6] / [6] device tensor; camera_type:
    "table", None (NULL), or an int32 device tensor [M] (stride 1) / [1] (stride 0)."""
    from soccernerfs_amd import _lib

    distortion = table["distortion"] if isinstance(distortion, str) else distortion
    camera_type = table["camera_type"] if isinstance(camera_type, str) else camera_type
    n = indices.shape[0]
    o = Outs(n)
    a = _lib.RaygenCamArgs()
    a.indices = indices.data_ptr()
    a.fx, a.fy, a.cx, a.cy, a.c2w, a.cam_times = (table[k].data_ptr() for k in ("fx", "fy", "cx", "cy", "camera_to_worlds", "cam_times"))
    a.R, a.collide, a.training, a.near_plane = n, int(collide), int(training), near_plane
    for i in range(3):
        a.aabb_min[i], a.aabb_max[i] = AABB[0][i], AABB[1][i]
    o.fill(a, collide)
    if distortion is not None:
        a.distortion, a.distortion_stride = distortion.data_ptr(), 6 if distortion.dim() == 2 else 0
    if camera_type is not None:
        assert camera_type.dtype == torch.int32 and camera_type.numel() in (1, table["fx"].numel())
        a.camera_type, a.camera_type_stride = camera_type.data_ptr(), 1 if camera_type.numel() > 1 else 0
    _lib.check(_lib.lib().snerf_raygen_cam(C.byref(a), _stream()), "raygen_cam")
    return o.get()


def _raygen_frame_cam(g, k, p0, p1, camera_type, distortion, width=W, height=H):
    """snerf_raygen_frame_cam for camera k of the host table g; distortion: six floats or None (has_distortion = 0)."""
    from soccernerfs_amd import _lib

    o = Outs(p1 - p0)
    a = _lib.RaygenFrameCamArgs()
    a.fx, a.fy, a.cx, a.cy, a.time = (float(g[q][k]) for q in ("fx", "fy", "cx", "cy", "cam_times"))
    for i, v in enumerate(np.asarray(g["camera_to_worlds"][k]).reshape(-1).tolist()):
        a.c2w[i] = v
    a.W, a.H, a.p0, a.p1, a.near_plane = width, height, p0, p1, 0.05
    for i in range(3):
        a.aabb_min[i], a.aabb_max[i] = AABB[0][i], AABB[1][i]
    o.fill(a)
    a.camera_type, a.has_distortion = int(camera_type), int(distortion is not None)
    if distortion is not None:
        for i in range(6):
            a.distortion[i] = float(distortion[i])
    _lib.check(_lib.lib().snerf_raygen_frame_cam(C.byref(a), _stream()), "raygen_frame_cam")
    return o.get()


def _deviations(got, want, rows=slice(None)):
    return LR.deviations({k: got[k].cpu().numpy()[rows] for k in GROUPS}, {k: want[k][rows] for k in GROUPS})


def _check(label, got, ref, n, bound):
    """got: device outputs of the first n rays of a table; ref: the float64 reference of all its rays."""
    want = {k: v[:n] for k, v in ref.items() if isinstance(v, np.ndarray) and v.ndim == 2}
    dev = _deviations(got, want)
    _record(label, dev)
    print(label, {k: f"{v:.3e} (bound {bound[k]:.3e})" for k, v in dev.items()})
    assert np.array_equal(got["origins"].cpu().numpy().astype(np.float64), want["origins"]), "origins are copies of the translation column"
    assert np.array_equal(got["times"].cpu().numpy().astype(np.float64), want["times"]), "times are copies of the camera's time"
    bad = {k: (v, bound[k]) for k, v in dev.items() if not v <= bound[k]}
    assert not bad, f"{label}: deviation beyond {MARGIN} x the reference's own: {bad}"


def _same(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), k


# 1. the three tables against the float64 reference, over ragged ray counts
@pytest.mark.parametrize("n", [1, 255, 257, 7232])
@pytest.mark.parametrize("p", TABLES)
def test_raygen_cam_against_the_float64_reference(ref64, bound, table, p, n):
    got = _raygen_cam(table[p], table[p]["indices"][:n].contiguous())
    _check(f"raygen_cam.{p[0]}.R{n}", got, ref64[p], n, bound[p])


# 2. perspective types are the entries that exist, bit for bit
@pytest.mark.parametrize("rows", [True, False], ids=["lens_rows", "no_rows"])
def test_perspective_types_equal_the_existing_entries(table, rows):
    t = table["a_"]
    idx = t["indices"]
    ones, one = torch.ones(4, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    for collide in (True, False):
        for training in (True, False):
            want = _raygen(t, idx, distortion="table" if rows else None, collide=collide, training=training)
            assert set(want) == set(KEYS + (("nears", "fars") if collide else ()))
            for kind in (None, ones, one):
                got = _raygen_cam(t, idx, distortion="table" if rows else None, camera_type=kind, collide=collide, training=training)
                assert set(got) == set(want)
                _same(got, want)
    if rows:  # the rows do something on this table: the comparison above is not one of pinhole rays with themselves
        assert not torch.equal(want["directions"], _raygen(t, idx, distortion=None, collide=False)["directions"])


# 3. a mixed table is its parts
def test_mixed_table_is_its_parts(table):
    a, b, c = table["a_"], table["b_"], table["c_"]
    idx = c["indices"]
    cam = idx[:, 0]
    mixed = _raygen_cam(c, idx)
    lens = _raygen(a, idx, collide=True, training=False)  # camera 0: perspective with A's intrinsics (its row is the zero row, whatever)
    fish, equi = _raygen_cam(a, idx), _raygen_cam(b, idx)
    for k in mixed:
        assert torch.equal(mixed[k][cam == 0], lens[k][cam == 0]), k
        assert torch.equal(mixed[k][cam == 2], equi[k][cam == 2]), k
        for m in (1, 3):
            assert torch.equal(mixed[k][cam == m], fish[k][cam == m]), (k, m)
    assert int((cam == 0).sum()) == 512 and int((cam == 3).sum()) == 512 + W * H
    assert not torch.equal(mixed["directions"][cam == 2], fish["directions"][cam == 2])


# 4. equirectangular cameras ignore the lens
def test_equirectangular_ignores_the_lens(table):
    b = table["b_"]
    assert bool((b["distortion"][1:] != 0).any(dim=1).all())
    idx = b["indices"]
    with_rows = _raygen_cam(b, idx)
    _same(_raygen_cam(b, idx, distortion=torch.zeros(4, 6, device=DEV)), with_rows)
    _same(_raygen_cam(b, idx, distortion=None), with_rows)
    _same(_raygen_cam(b, idx, distortion=b["distortion"][3].contiguous(), camera_type=torch.full((1,), 3, dtype=torch.int32, device=DEV)), with_rows)


def _meshgrid(width, height, cam=0):
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([np.full(width * height, cam), ys.reshape(-1), xs.reshape(-1)], -1).astype(np.int64)


def _one_camera(g18, fx, fy, cx, cy, kind, k=3):
    f = lambda v: np.asarray([v], np.float32)
    host = {"fx": f(fx), "fy": f(fy), "cx": f(cx), "cy": f(cy), "camera_to_worlds": g18["camera_to_worlds"][k:k + 1], "cam_times": g18["cam_times"][k:k + 1],
            "camera_type": np.asarray([kind], np.int32)}
    return host, {k_: torch.from_numpy(v).to(DEV).contiguous() for k_, v in host.items()}


# 5. theta == 0: the one deliberate deviation from the reference
def test_fisheye_pixel_on_the_principal_point(g18, bound):
    w, h = 21, 15
    host, dev = _one_camera(g18, 12.0, 12.0, 10.5, 7.5, CR.FISHEYE)
    idx = _meshgrid(w, h)
    ref = CR.generate_rays(idx, host["fx"], host["fy"], host["cx"], host["cy"], host["camera_to_worlds"], host["cam_times"], camera_type=CR.FISHEYE)
    assert ref["min_theta"] == 0.0
    got = _raygen_cam(dev, torch.from_numpy(idx).to(DEV), distortion=None)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    r = 7 * w + 10  # pixel (row 7, column 10): its centre (10.5, 7.5) is the principal point
    axis = -host["camera_to_worlds"][0][:, 2].astype(np.float64)
    axis /= np.linalg.norm(axis)
    assert np.abs(got["directions"][r].cpu().numpy() - axis).max() <= bound["a_"]["directions"]
    assert float(got["pixel_area"][r]) > 0
    _check("raygen_cam.theta_zero_frame", got, ref, w * h, bound["a_"])
    _same(_raygen_frame_cam(host, 0, 0, w * h, CR.FISHEYE, None, w, h), got)


# 6. theta beyond pi is clipped
def test_fisheye_theta_clip(g18):
    """fx = fy = 8 at 96 x 54: |(x, y)| reaches 6.9, so most of the frame is clipped at theta = pi.  E32 is taken from a float32 NumPy evaluation
    of the same statements, since G18 does not hold this camera.  On the clipped rays the pixel area is rounding noise in ANY float32 evaluation,
    the reference's included (directions 1e-9 apart, formed by sums of O(1) terms), so that group's E32, and with it its bound, is of order 1e2 to
    1e3 for this frame by construction; the pixels whose three coordinate pairs all stay below pi are therefore bounded a second time on their
    own."""
    host, dev = _one_camera(g18, 8.0, 8.0, 48.0, 27.0, CR.FISHEYE)
    idx = _meshgrid(W, H)
    args = (idx, host["fx"], host["fy"], host["cx"], host["cy"], host["camera_to_worlds"], host["cam_times"])
    ref, f32 = CR.generate_rays(*args, camera_type=CR.FISHEYE), CR.generate_rays(*args, camera_type=CR.FISHEYE, dtype=np.float32)
    theta = np.sqrt((ref["coords"] ** 2).sum(-1))  # [3, R]
    assert (theta[0] > np.pi).sum() > 1000 and theta.max() > 6.0
    inside = (theta < np.pi - 1e-3).all(0)
    assert 100 < inside.sum() < W * H - 1000
    got = _raygen_cam(dev, torch.from_numpy(idx).to(DEV), distortion=None)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for label, rows in (("frame", slice(None)), ("below_pi", inside)):
        e32 = LR.deviations({k: f32[k][rows] for k in GROUPS}, {k: ref[k][rows] for k in GROUPS})
        dev_ = _deviations(got, ref, rows)
        _record(f"theta_clip.{label}.float32_numpy", e32)
        _record(f"theta_clip.{label}.raygen_cam", dev_)
        print(label, {k: f"{dev_[k]:.3e} (E32 {e32[k]:.3e})" for k in GROUPS})
        assert all(v > 0 for v in e32.values())
        bad = {k: (dev_[k], MARGIN * e32[k]) for k in GROUPS if not dev_[k] <= MARGIN * e32[k]}
        assert not bad, (label, bad)
    assert np.array_equal(got["times"].cpu().numpy().astype(np.float64), ref["times"])
    _same(_raygen_frame_cam(host, 0, 0, W * H, CR.FISHEYE, None), got)


# 7. the frame kernel against the table kernel
@pytest.mark.parametrize("p0,p1", [(0, 1), (95, 97), (4000, 5184), (0, 5184)])
@pytest.mark.parametrize("kind", [2, 3])
def test_raygen_frame_cam_equals_raygen_cam_on_the_meshgrid_table(host, table, kind, p0, p1):
    k = 3
    p = {2: "a_", 3: "b_"}[kind]
    idx = table[p]["indices"][:W * H]
    assert bool((idx[:, 0] == k).all())  # the fixture's first 5184 rays ARE camera 3's meshgrid table
    want = _raygen_cam(table[p], idx[p0:p1].contiguous(), collide=True, training=False)
    got = _raygen_frame_cam(host[p], k, p0, p1, kind, host[p]["distortion"][k])
    _same(got, want)
    # without a lens: has_distortion = 0 is the table entry with a NULL distortion
    _same(_raygen_frame_cam(host[p], k, p0, p1, kind, None), _raygen_cam(table[p], idx[p0:p1].contiguous(), distortion=None))
    # and a perspective camera is the frame entries that exist
    _same(_raygen_frame_cam(host[p], k, p0, p1, 1, host[p]["distortion"][k]), _raygen_frame(host[p], k, p0, p1, host[p]["distortion"][k]))
    _same(_raygen_frame_cam(host[p], k, p0, p1, 1, None), _raygen_frame(host[p], k, p0, p1, None))
    assert not torch.equal(got["directions"], _raygen_frame(host[p], k, p0, p1, None)["directions"])


# 8. the fused collider is the collider
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("p", TABLES)
def test_fused_collider_equals_aabb_collide(table, p, training):
    from soccernerfs_amd import ops

    got = _raygen_cam(table[p], table[p]["indices"], collide=True, training=training, near_plane=0.05)
    nears, fars = ops.aabb_collide(got["origins"].contiguous(), got["directions"].contiguous(), AABB, 0.05, training)
    assert torch.equal(got["nears"], nears) and torch.equal(got["fars"], fars)
    assert bool((got["fars"] > got["nears"]).all())


# 9. Cameras / RayGenerator / generate_rays(k)
def _cameras(g, **kw):
    from soccernerfs_amd.cameras import Cameras

    t = torch.from_numpy
    kw = {"distortion_params": t(g["distortion"]), "camera_type": t(g["camera_type"]), **kw}
    return Cameras(t(g["camera_to_worlds"]), t(g["fx"]), t(g["fy"]), t(g["cx"]), t(g["cy"]), W, H, t(g["cam_times"]), **kw).to(DEV)


def _bundle(rb):
    return {"origins": rb.origins, "directions": rb.directions, "pixel_area": rb.pixel_area, "directions_norm": rb.metadata["directions_norm"], "times": rb.times}


@pytest.mark.parametrize("p", TABLES)
def test_cameras_and_ray_generator_take_the_type(host, table, ref64, bound, p):
    from soccernerfs_amd.cameras import RayGenerator

    idx = table[p]["indices"]
    coords = idx[:, 1:3].float() + 0.5
    want = _raygen_cam(table[p], idx, collide=False)
    cams = _cameras(host[p])
    assert cams.all_perspective is False and cams.camera_type.is_cuda and cams.camera_type.dtype == torch.int32
    rb = cams.generate_rays(idx[:, 0:1], coords)
    _same(_bundle(rb), want, KEYS)
    _same(_bundle(RayGenerator(cams)(idx)), want, KEYS)
    _check(f"cameras.generate_rays.{p[0]}", _bundle(rb), ref64[p], idx.shape[0], bound[p])
    full = cams.generate_rays(3)  # a whole image by its camera number
    assert full.directions.shape == (H, W, 3) and torch.equal(full.directions.reshape(-1, 3), want["directions"][:W * H])
    assert torch.equal(full.pixel_area.reshape(-1, 1), want["pixel_area"][:W * H])
    # .to() carries the flag and the table
    back = cams.to("cpu").to(DEV)
    assert back.all_perspective is False and torch.equal(back.camera_type, cams.camera_type)
    _same(_bundle(back.generate_rays(idx[:, 0:1], coords)), want, KEYS)
    # disable_distortion drops the rows and keeps the type
    off = _bundle(cams.generate_rays(idx[:, 0:1], coords, disable_distortion=True))
    _same(off, _raygen_cam(table[p], idx, distortion=None, collide=False), KEYS)
    if p == "b_":
        _same(off, want, KEYS)
    else:
        assert not torch.equal(off["directions"], want["directions"])
        # the keyword is not ignored: a fisheye table's directions leave the same table's perspective directions by more than 1e-1 somewhere
        pin = _bundle(_cameras(host[p], camera_type=1).generate_rays(idx[:, 0:1], coords))
        _same(pin, _raygen(table[p], idx, collide=False), KEYS)
        assert float((rb.directions - pin["directions"]).abs().max()) > 1e-1


def test_generate_rays_refuses_an_unknown_type(host, table):
    from soccernerfs_amd import ops

    t = table["a_"]
    args = (t["indices"][:8].contiguous(), t["fx"], t["fy"], t["cx"], t["cy"], t["camera_to_worlds"], t["cam_times"])
    for bad in (0, 4, torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="not supported"):
            ops.generate_rays(*args, camera_type=bad)
    one = ops.generate_rays(*args, camera_type=2)
    _same(one, ops.generate_rays(*args, camera_type=t["camera_type"]), KEYS)


# 10. the sphere-uniform pixel draw
@pytest.mark.parametrize("R", [1, 257, 4096])
def test_sample_pixels_sphere(R):
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import EquirectangularPixelSampler

    M, Wd = 5, 96
    u_host = _sphere_u()[:R].contiguous()
    u = u_host.to(DEV)
    images = torch.randint(0, 256, (M, SPHERE_H, Wd, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    idx, target = ops.sample_pixels_sphere(u, M, SPHERE_H, Wd, images)
    uni, _ = ops.sample_pixels_uniform(u, M, SPHERE_H, Wd)
    assert idx.dtype == torch.int64 and idx.shape == (R, 3)
    assert torch.equal(idx[:, 0], uni[:, 0]) and torch.equal(idx[:, 2], uni[:, 2])
    band, rows64 = sphere_band(u_host[:, 1])
    rows = idx[:, 1].cpu().numpy()
    assert np.array_equal(rows[~band], rows64[~band]) and (np.abs(rows - rows64) <= 1).all() and rows.max() < SPHERE_H and rows.min() >= 0
    # uint8 -> float32 / 255 evaluated on the HOST, as the reference's dataset does (a correctly rounded division): the device library divides a
    # tensor by a scalar as a product with its reciprocal, which is one ulp off on some values and is not what the kernel restates
    want = images.cpu()[idx[:, 0].cpu(), idx[:, 1].cpu(), idx[:, 2].cpu()].float() / 255.0
    assert torch.equal(target.cpu(), want)
    only_idx, none = ops.sample_pixels_sphere(u, M, SPHERE_H, Wd)
    assert none is None and torch.equal(only_idx, idx)
    torch.manual_seed(77)
    drawn = torch.rand((R, 3), device=DEV)
    torch.manual_seed(77)
    got = EquirectangularPixelSampler(R).sample_method(R, M, SPHERE_H, Wd, device=DEV)
    assert torch.equal(got, ops.sample_pixels_sphere(drawn, M, SPHERE_H, Wd)[0])


# 11. the renderer
@pytest.fixture(scope="module")
def trained():
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    tr = KPlanesTrainer(KPlanesTrainConfig(**SMALL), 4096, DEV)
    gen = torch.Generator().manual_seed(3)
    d = lambda z: z.to(DEV).contiguous()
    for _ in range(4):
        rays = {"origins": d((torch.rand(4096, 3, generator=gen) * 2 - 1) * 1.2),
                "directions": d(torch.nn.functional.normalize(torch.rand(4096, 3, generator=gen) * 2 - 1, dim=-1)), "times": d(torch.rand(4096, 1, generator=gen))}
        tr.train_step(rays, d(torch.rand(4096, 3, generator=gen)))
    return tr


def _eval_path(tr, cams, k, anneal):
    """The eval path of tools/train_psnr.py: ops.generate_rays(camera_type=...) + forward(training=False), 4096 rays at a time."""
    from soccernerfs_amd import ops

    h, w = cams.height, cams.width
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
    rgb, acc, depth = torch.empty(h * w, 3, device=DEV), torch.empty(h * w, device=DEV), torch.empty(h * w, device=DEV)
    for i in range(0, h * w, tr.R):
        rays = ops.generate_rays(idx[i:i + tr.R].contiguous(), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, cams.times, aabb=tr.aabb,
                                 near_plane=tr.cfg.near_plane, training=False, distortion_params=cams.distortion_params if cams.has_distortion else None,
                                 camera_type=cams.camera_type)
        n = rays["origins"].shape[0]
        rgb[i:i + n] = tr.forward(rays, None, anneal, training=False)
        acc[i:i + n], depth[i:i + n] = tr.buf["acc"][:n], tr.buf["depth"][:n]
    return rgb.view(h, w, 3), acc.view(h, w, 1), depth.view(h, w, 1)


@pytest.mark.parametrize("case", ["equirectangular", "fisheye_lens"])
def test_render_frame_of_the_new_types_equals_the_eval_path(g18, host, trained, case):
    from soccernerfs_amd.cameras import Cameras
    from soccernerfs_amd.render import KPlanesRenderer

    tr, t = trained, torch.from_numpy
    if case == "equirectangular":  # 96 x 48 = 4608 rays = 4000 + 608
        mk = lambda kind: Cameras(t(g18["camera_to_worlds"]), 48.0, 48.0, 48.0, 24.0, 96, 48, t(g18["cam_times"]), camera_type=kind).to(DEV)
        cams, plain, k = mk(3), mk(1), 3
    else:                          # camera 3 of table A, through its lens row: 5184 = 4000 + 1184
        cams, plain, k = _cameras(host["a_"]), _cameras(host["a_"], camera_type=1), 3
    assert plain.all_perspective and not cams.all_perspective
    frames, pinhole = {}, {}
    for fused in (True, False):
        rn = KPlanesRenderer(tr, rays_per_chunk=4000, fused_tail=fused)
        assert rn.fused_tail == fused  # this shape supports the fused tail
        n0 = rn.launches
        frames[fused] = rn.render_frame(cams, k)
        per_frame = rn.launches - n0
        pinhole[fused] = rn.render_frame(plain, k)
        assert rn.launches - n0 == 2 * per_frame  # a frame of the new types issues as many launches as a perspective one
        anneal = rn.default_anneal()
    rgb, acc, depth = _eval_path(tr, cams, k, anneal)
    assert float(rgb.std()) > 0 and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all()) and bool(torch.isfinite(acc).all())
    for fused in (True, False):
        assert torch.equal(frames[fused]["rgb"], rgb), fused
        assert torch.equal(frames[fused]["accumulation"], acc), fused
        assert torch.equal(frames[fused]["depth"], depth), fused
        assert not torch.equal(frames[fused]["rgb"], pinhole[fused]["rgb"]), fused
    p_rgb, _, _ = _eval_path(tr, plain, k, anneal)
    assert torch.equal(pinhole[True]["rgb"], p_rgb)


def test_render_camera_path_of_the_new_types(g18, trained, tmp_path):
    from PIL import Image
    from soccernerfs_amd.camera_paths import get_path_from_json
    from soccernerfs_amd.render import KPlanesRenderer

    c2w = lambda k: np.concatenate([g18["camera_to_worlds"][k].astype(np.float64), [[0.0, 0.0, 0.0, 1.0]]], 0).reshape(-1).tolist()
    entries = [{"camera_to_world": c2w(k), "fov": 50.0, "aspect": 2.0, "render_time": float(g18["cam_times"][k])} for k in (1, 3)]
    path = {"render_width": 48, "render_height": 24, "camera_type": "equirectangular", "camera_path": entries, "fps": 24, "seconds": 1.0}
    rn = KPlanesRenderer(trained, rays_per_chunk=1000)
    files = rn.render_camera_path(path, str(tmp_path / "equi"))
    assert [os.path.basename(f) for f in files] == ["00000.png", "00001.png"]
    images = [np.asarray(Image.open(f)) for f in files]
    assert all(im.shape == (24, 48, 3) and im.dtype == np.uint8 for im in images) and not np.array_equal(images[0], images[1])
    # a perspective path: the bytes get_path_from_json(path) + render_frame give, as before
    persp = {**path, "camera_type": "perspective"}
    files_p = rn.render_camera_path(persp, str(tmp_path / "persp"))
    cams = get_path_from_json(persp).to(DEV)
    for k, f in enumerate(files_p):
        ref_file = tmp_path / f"ref_{k}.png"
        Image.fromarray(rn.to_uint8(rn.render_frame(cams, k)["rgb"]).cpu().numpy()).save(ref_file)
        assert open(f, "rb").read() == open(ref_file, "rb").read()
    assert not np.array_equal(np.asarray(Image.open(files_p[0])), images[0])


# 12. the synthetic dataset
def test_synthetic_dataset_with_a_camera_type():
    from soccernerfs_amd import synthetic
    from soccernerfs_amd.cameras import CameraType

    cams = synthetic.make_cameras(3, W, H)
    times = torch.tensor([0.0, 0.5])
    base = synthetic.render_dataset(cams, times, [0, 2], DEV, chunk_rows=20)
    assert "camera_type" not in base and "distortion" not in base
    fish = synthetic.render_dataset({**cams, "camera_type": 2}, times, [0, 2], DEV, chunk_rows=20)
    assert fish["camera_type"].dtype == torch.int32 and fish["camera_type"].tolist() == [2] * 4
    assert not torch.equal(fish["images"], base["images"])
    assert torch.equal(synthetic.render_dataset({**cams, "camera_type": CameraType.FISHEYE}, times, [0, 2], DEV, chunk_rows=20)["images"], fish["images"])
    per_cam = synthetic.render_dataset({**cams, "camera_type": torch.tensor([2, 1, 2])}, times, [0, 2], DEV, chunk_rows=20)
    assert torch.equal(per_cam["images"], fish["images"])
    persp = synthetic.render_dataset({**cams, "camera_type": 1}, times, [0, 2], DEV, chunk_rows=20)
    assert persp["camera_type"].tolist() == [1] * 4 and torch.equal(persp["images"], base["images"])
    for k in ("fx", "fy", "cx", "cy", "c2w", "times", "cam_id"):
        assert torch.equal(fish[k], base[k]), k
    with pytest.raises(ValueError):
        synthetic.render_dataset({**cams, "camera_type": 4}, times, [0, 2], DEV, chunk_rows=20)

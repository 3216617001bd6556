"""GPU: rays through the cameras' lens distortion (snerf_raygen_lens, snerf_raygen_frame_lens and everything above them).

References.  tests/lens_reference.py is the reference's ray generation with its undistortion in float64; G17 (tools/gen_golden_lens.py) holds the
reference's own float32 rays of four cameras (row 0 all zero, rows 1-3 lenses), the full frame of camera 3 plus 512 random pixels of each.

Bounds (the convention of tests/test_gpu_per_ray_lattice.py).  E32 = the largest deviation of G17's float32 rays from the float64 reference on
the same 7232 rays, per output group: directions absolute, directions_norm and pixel_area relative.  A kernel may deviate by MARGIN = 5 times
E32; the bound is computed from the fixture below, nothing is typed in.  (On the CPU that wrote G17: 1.3e-7, 1.5e-7, 1.9e-5.)  One figure per
group bounds every ray count; origins and times are copies and are compared exactly.  Every call through the C ABI writes into buffers with
GUARD sentinel rows behind each output, which must stay untouched, and every live row must have been written.  The measured deviations of the
reference and of the kernels go to r12_lens_deviations.json in the scratch directory of tests/_measure.py (the copy of this file's run:
profiles/r12_lens_deviations.json).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _measure
from tests import lens_reference as LR
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 5.0
GUARD = 4
DEAD, LIVE = -7777.0, 12345.678
AABB = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]
W, H = 96, 54
KEYS = ("origins", "directions", "pixel_area", "directions_norm", "times")
_RECORD = {}
_SCRATCH = os.path.dirname(_measure._OUT)  # where the suite's measured deviations go; not part of the repository


def _record(name, dev):
    _RECORD[name] = dev
    try:
        os.makedirs(_SCRATCH, exist_ok=True)
        with open(os.path.join(_SCRATCH, "r12_lens_deviations.json"), "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture(scope="module")
def g17():
    z = np.load(os.path.join(GOLDEN, "g17_lens.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _ref(g, distortion):
    return LR.generate_rays(g["indices"], g["fx"], g["fy"], g["cx"], g["cy"], g["camera_to_worlds"], g["cam_times"], distortion)


@pytest.fixture(scope="module")
def ref64(g17):
    return _ref(g17, g17["distortion"])


@pytest.fixture(scope="module")
def bound(g17, ref64):
    e32 = LR.deviations(g17, ref64)
    _record("reference_float32_vs_float64", e32)
    assert all(v > 0 for v in e32.values())
    return {k: MARGIN * v for k, v in e32.items()}


@pytest.fixture(scope="module")
def table(g17):
    return {k: torch.from_numpy(g17[k]).to(DEV).contiguous() for k in ("fx", "fy", "cx", "cy", "camera_to_worlds", "cam_times", "distortion", "indices")}


class Outs:
    """The outputs of one raygen call, each [n + GUARD, .]: live rows hold LIVE, the rows behind them DEAD."""
    SHAPES = {"origins": 3, "directions": 3, "pixel_area": 1, "directions_norm": 1, "times": 1, "nears": 1, "fars": 1}

    def __init__(self, n):
        self.n = n
        self.buf = {k: torch.full((n + GUARD, c), DEAD, device=DEV) for k, c in self.SHAPES.items()}
        for b in self.buf.values():
            b[:n] = LIVE

    def fill(self, a, collide=True):
        a.origins, a.dirs, a.pixel_area, a.dir_norm, a.times = (self.buf[k].data_ptr() for k in KEYS)
        if collide:
            a.nears, a.fars = self.buf["nears"].data_ptr(), self.buf["fars"].data_ptr()
        self.written = KEYS + (("nears", "fars") if collide else ())

    def get(self):
        torch.cuda.synchronize()
        out = {}
        for k, b in self.buf.items():
            assert bool((b[self.n:] == DEAD).all()), f"{k}: rows behind the last ray were written"
            if k in self.written:
                assert not bool((b[:self.n] == LIVE).any()), f"{k}: live elements were left unwritten"
                out[k] = b[:self.n]
            else:
                assert bool((b[:self.n] == LIVE).all()), f"{k}: written although not asked for"
        return out


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raygen(table, indices, distortion="table", collide=True, training=False, near_plane=0.05):
    """snerf_raygen (distortion None) or snerf_raygen_lens (a [M,6] or [6] device tensor; "table": the fixture's) through the C ABI."""
    from soccernerfs_amd import _lib

    distortion = table["distortion"] if isinstance(distortion, str) else distortion
    n = indices.shape[0]
    o = Outs(n)
    a = _lib.RaygenArgs() if distortion is None else _lib.RaygenLensArgs()
    a.indices = indices.data_ptr()
    a.fx, a.fy, a.cx, a.cy, a.c2w, a.cam_times = (table[k].data_ptr() for k in ("fx", "fy", "cx", "cy", "camera_to_worlds", "cam_times"))
    a.R, a.collide, a.training, a.near_plane = n, int(collide), int(training), near_plane
    for i in range(3):
        a.aabb_min[i], a.aabb_max[i] = AABB[0][i], AABB[1][i]
    o.fill(a, collide)
    if distortion is None:
        _lib.check(_lib.lib().snerf_raygen(C.byref(a), _stream()), "raygen")
    else:
        a.distortion, a.distortion_stride = distortion.data_ptr(), 6 if distortion.dim() == 2 else 0
        _lib.check(_lib.lib().snerf_raygen_lens(C.byref(a), _stream()), "raygen_lens")
    return o.get()


def _raygen_frame(g, k, p0, p1, distortion):
    """snerf_raygen_frame (distortion None) or snerf_raygen_frame_lens (six floats) for camera k of the fixture."""
    from soccernerfs_amd import _lib

    o = Outs(p1 - p0)
    a = _lib.RaygenFrameArgs() if distortion is None else _lib.RaygenFrameLensArgs()
    a.fx, a.fy, a.cx, a.cy, a.time = (float(g[q][k]) for q in ("fx", "fy", "cx", "cy", "cam_times"))
    for i, v in enumerate(g["camera_to_worlds"][k].reshape(-1).tolist()):
        a.c2w[i] = v
    a.W, a.H, a.p0, a.p1, a.near_plane = W, H, p0, p1, 0.05
    for i in range(3):
        a.aabb_min[i], a.aabb_max[i] = AABB[0][i], AABB[1][i]
    o.fill(a)
    if distortion is None:
        _lib.check(_lib.lib().snerf_raygen_frame(C.byref(a), _stream()), "raygen_frame")
    else:
        for i in range(6):
            a.distortion[i] = float(distortion[i])
        _lib.check(_lib.lib().snerf_raygen_frame_lens(C.byref(a), _stream()), "raygen_frame_lens")
    return o.get()


def _check(label, got, ref, n, bound):
    """got: device outputs of the first n rays of the fixture's table; ref: the float64 reference of all rays."""
    want = {k: v[:n] for k, v in ref.items() if isinstance(v, np.ndarray) and v.ndim == 2}
    dev = LR.deviations({k: got[k].cpu().numpy() for k in ("directions", "directions_norm", "pixel_area")}, want)
    _record(label, dev)
    print(label, {k: f"{v:.3e} (bound {bound[k]:.3e})" for k, v in dev.items()})
    assert np.array_equal(got["origins"].cpu().numpy().astype(np.float64), want["origins"]), "origins are copies of the translation column"
    assert np.array_equal(got["times"].cpu().numpy().astype(np.float64), want["times"]), "times are copies of the camera's time"
    bad = {k: (v, bound[k]) for k, v in dev.items() if not v <= bound[k]}
    assert not bad, f"{label}: deviation beyond {MARGIN} x the reference's own: {bad}"


# 5. per-camera rows against the float64 reference, over ragged ray counts
@pytest.mark.parametrize("n", [1, 255, 257, 7232])
def test_raygen_lens_against_the_float64_reference(g17, ref64, bound, table, n):
    got = _raygen(table, table["indices"][:n].contiguous())
    _check(f"raygen_lens.table.R{n}", got, ref64, n, bound)


# 6. one shared row: camera 2's, whose tangential pair has p1 != p2 and opposite signs
@pytest.mark.parametrize("n", [1, 255, 257, 7232])
def test_raygen_lens_shared_row(g17, bound, table, n):
    row = g17["distortion"][2]
    assert row[4] != row[5] and row[4] * row[5] < 0
    ref = _ref(g17, row)  # asserts min |denominator| >= 0.1 for this row on all four cameras
    got = _raygen(table, table["indices"][:n].contiguous(), distortion=table["distortion"][2].contiguous())
    _check(f"raygen_lens.shared_row.R{n}", got, ref, n, bound)
    # the same row written out per camera is the same computation
    per_cam = _raygen(table, table["indices"][:n].contiguous(), distortion=table["distortion"][2].expand(4, 6).contiguous())
    for k in per_cam:
        assert torch.equal(per_cam[k], got[k]), k


# 7. zero rows are the pinhole kernel, and the fused collider is the collider
@pytest.mark.parametrize("collide", [True, False], ids=["collider", "no_collider"])
def test_zero_rows_equal_the_pinhole_entry(table, collide):
    idx = table["indices"]
    lens = _raygen(table, idx, distortion=torch.zeros(4, 6, device=DEV), collide=collide, training=True)
    pin = _raygen(table, idx, distortion=None, collide=collide, training=True)
    assert set(lens) == set(pin) == set(KEYS + (("nears", "fars") if collide else ()))
    for k in pin:
        assert torch.equal(lens[k], pin[k]), k
    shared = _raygen(table, idx, distortion=torch.zeros(6, device=DEV), collide=collide, training=True)
    for k in pin:
        assert torch.equal(shared[k], pin[k]), k
    # camera 0 of the fixture's own table has the zero row
    mixed = _raygen(table, idx, collide=collide, training=True)
    cam0 = idx[:, 0] == 0
    assert int(cam0.sum()) == 512
    for k in pin:
        assert torch.equal(mixed[k][cam0], pin[k][cam0]), k
    assert not torch.equal(mixed["directions"][~cam0], pin["directions"][~cam0])


@pytest.mark.parametrize("training", [True, False])
def test_fused_collider_of_lens_rays_equals_aabb_collide(table, training):
    from soccernerfs_amd import ops

    got = _raygen(table, table["indices"], collide=True, training=training, near_plane=0.05)
    nears, fars = ops.aabb_collide(got["origins"].contiguous(), got["directions"].contiguous(), AABB, 0.05, training)
    assert torch.equal(got["nears"], nears) and torch.equal(got["fars"], fars)
    assert bool((got["fars"] > got["nears"]).all())


# 8. the frame kernel against the table kernel
@pytest.mark.parametrize("p0,p1", [(0, 1), (95, 97), (4000, 5184), (0, 5184)])
def test_raygen_frame_lens_equals_raygen_lens_on_the_meshgrid_table(g17, table, p0, p1):
    k = 3
    idx = table["indices"][:W * H]
    assert bool((idx[:, 0] == k).all())  # the fixture's first 5184 rays ARE camera 3's meshgrid table
    want = _raygen(table, idx[p0:p1].contiguous(), collide=True, training=False)
    got = _raygen_frame(g17, k, p0, p1, g17["distortion"][k])
    for key in want:
        assert torch.equal(got[key], want[key]), key
    # and with a zero row it is the pinhole frame kernel
    z, pin = _raygen_frame(g17, k, p0, p1, np.zeros(6)), _raygen_frame(g17, k, p0, p1, None)
    for key in pin:
        assert torch.equal(z[key], pin[key]), key
    assert not torch.equal(got["directions"], pin["directions"])


# 9. Cameras / RayGenerator
def _cameras(g, distortion):
    from soccernerfs_amd.cameras import Cameras

    t = torch.from_numpy
    return Cameras(t(g["camera_to_worlds"]), t(g["fx"]), t(g["fy"]), t(g["cx"]), t(g["cy"]), W, H, t(g["cam_times"]),
                   distortion_params=None if distortion is None else t(distortion)).to(DEV)


def test_cameras_and_ray_generator_take_the_lens_path(g17, table):
    from soccernerfs_amd.cameras import RayGenerator

    idx = table["indices"]
    want = _raygen(table, idx, collide=False)
    cams = _cameras(g17, g17["distortion"])
    assert cams.has_distortion and cams.distortion_params.is_cuda
    rb = cams.generate_rays(idx[:, 0:1], idx[:, 1:3].float() + 0.5)
    rg = RayGenerator(cams)(idx)
    for b in (rb, rg):
        assert torch.equal(b.origins, want["origins"]) and torch.equal(b.directions, want["directions"]) and torch.equal(b.times, want["times"])
        assert torch.equal(b.pixel_area, want["pixel_area"]) and torch.equal(b.metadata["directions_norm"], want["directions_norm"])
    # a whole image by its camera number
    full = cams.generate_rays(3)
    assert full.directions.shape == (H, W, 3) and torch.equal(full.directions.reshape(-1, 3), want["directions"][:W * H])
    # disable_distortion: the same table without coefficients
    plain = _cameras(g17, None)
    assert not plain.has_distortion
    off, pin = cams.generate_rays(idx[:, 0:1], idx[:, 1:3].float() + 0.5, disable_distortion=True), plain.generate_rays(idx[:, 0:1], idx[:, 1:3].float() + 0.5)
    want_pin = _raygen(table, idx, distortion=None, collide=False)
    for b in (off, pin):
        assert torch.equal(b.directions, want_pin["directions"]) and torch.equal(b.pixel_area, want_pin["pixel_area"])
        assert torch.equal(b.metadata["directions_norm"], want_pin["directions_norm"]) and torch.equal(b.origins, want_pin["origins"])
    # the coefficients are applied: camera 3's lens directions leave its pinhole directions by more than 1e-2 somewhere
    cam3 = idx[:, 0] == 3
    assert float((rb.directions[cam3] - pin.directions[cam3]).abs().max()) > 1e-2


def test_cameras_against_the_float64_reference(g17, ref64, bound, table):
    idx = table["indices"]
    rb = _cameras(g17, g17["distortion"]).generate_rays(idx[:, 0:1], idx[:, 1:3].float() + 0.5)
    got = {"origins": rb.origins, "directions": rb.directions, "pixel_area": rb.pixel_area, "directions_norm": rb.metadata["directions_norm"], "times": rb.times}
    _check("cameras.generate_rays", got, ref64, idx.shape[0], bound)


# 10. the renderer
SMALL = dict(aabb_scale=1.5, spacetime_resolution=(16, 16, 16, 4), multiscale_res=(1, 2), feature_dim=32,
             proposal_resolutions=((24, 24, 24, 4), (32, 32, 32, 4)), proposal_feature_dim=8, num_proposal_samples_per_ray=(64, 32),
             num_nerf_samples_per_ray=32, warm_up_end=2)


def test_render_frame_through_the_lens_equals_the_eval_path(g17):
    from soccernerfs_amd import ops
    from soccernerfs_amd.render import KPlanesRenderer
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    tr = KPlanesTrainer(KPlanesTrainConfig(**SMALL), 4096, DEV)
    gen = torch.Generator().manual_seed(3)
    d = lambda z: z.to(DEV).contiguous()
    for _ in range(4):
        rays = {"origins": d((torch.rand(4096, 3, generator=gen) * 2 - 1) * 1.2),
                "directions": d(torch.nn.functional.normalize(torch.rand(4096, 3, generator=gen) * 2 - 1, dim=-1)), "times": d(torch.rand(4096, 1, generator=gen))}
        tr.train_step(rays, d(torch.rand(4096, 3, generator=gen)))
    k = 3
    cams, plain = _cameras(g17, g17["distortion"]), _cameras(g17, None)
    frames, pinhole = {}, {}
    for fused in (True, False):
        rn = KPlanesRenderer(tr, rays_per_chunk=4000, fused_tail=fused)  # 5184 = 4000 + 1184
        assert rn.fused_tail == fused  # this shape supports the fused tail
        frames[fused], pinhole[fused] = rn.render_frame(cams, k), rn.render_frame(plain, k)
        zero_row = rn.render_frame(cams, 0)  # camera 0 of the lens table has the all-zero row: the pinhole entry
        assert torch.equal(zero_row["rgb"], rn.render_frame(plain, 0)["rgb"])
        anneal = rn.default_anneal()
    # the eval path of tools/train_psnr.py fed with lens rays
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    idx = torch.stack([torch.full_like(ys, k), ys, xs], -1).reshape(-1, 3)
    rgb, acc, depth = torch.empty(H * W, 3, device=DEV), torch.empty(H * W, device=DEV), torch.empty(H * W, device=DEV)
    for i in range(0, H * W, tr.R):
        rays = ops.generate_rays(idx[i:i + tr.R].contiguous(), cams.fx, cams.fy, cams.cx, cams.cy, cams.camera_to_worlds, cams.times, aabb=tr.aabb,
                                 near_plane=tr.cfg.near_plane, training=False, distortion_params=cams.distortion_params)
        n = rays["origins"].shape[0]
        rgb[i:i + n] = tr.forward(rays, None, anneal, training=False)
        acc[i:i + n], depth[i:i + n] = tr.buf["acc"][:n], tr.buf["depth"][:n]
    assert float(rgb.std()) > 0 and bool(torch.isfinite(rgb).all())
    for fused in (True, False):
        assert torch.equal(frames[fused]["rgb"], rgb.view(H, W, 3)), fused
        assert torch.equal(frames[fused]["accumulation"], acc.view(H, W, 1)), fused
        assert torch.equal(frames[fused]["depth"], depth.view(H, W, 1)), fused
        assert not torch.equal(frames[fused]["rgb"], pinhole[fused]["rgb"]), fused


# 11. the synthetic dataset
def test_synthetic_dataset_through_a_lens():
    from soccernerfs_amd import ops, synthetic

    cams = synthetic.make_cameras(3, W, H)
    times = torch.tensor([0.0, 0.5])
    base = synthetic.render_dataset(cams, times, [0, 2], DEV, chunk_rows=20)
    assert "distortion" not in base
    # without the entry: today's call, ops.generate_rays without the new argument plus shade, on the same chunks of the same table
    xs = torch.arange(W, device=DEV)
    for m in range(4):
        for r0 in range(0, H, 20):
            rows = torch.arange(r0, min(r0 + 20, H), device=DEV)
            yy, xx = torch.meshgrid(rows, xs, indexing="ij")
            idx = torch.stack([torch.full_like(yy, m), yy, xx], -1).reshape(-1, 3)
            rays = ops.generate_rays(idx, base["fx"], base["fy"], base["cx"], base["cy"], base["c2w"], base["times"])
            col = synthetic.shade(rays["origins"], rays["directions"], rays["times"][:, 0])
            assert torch.equal(base["images"][m, r0:r0 + rows.numel()], (col.view(rows.numel(), W, 3) * 255.0 + 0.5).to(torch.uint8)), (m, r0)
    row = torch.tensor([-0.25, 0.08, -0.01, 0.0, 0.001, 0.0005])
    lens = synthetic.render_dataset({**cams, "distortion": row}, times, [0, 2], DEV, chunk_rows=20)
    assert lens["distortion"].shape == (4, 6) and torch.equal(lens["distortion"].cpu(), row.expand(4, 6))
    assert not torch.equal(lens["images"], base["images"])
    per_cam = torch.stack([row, torch.zeros(6), row])
    lens2 = synthetic.render_dataset({**cams, "distortion": per_cam}, times, [0, 2], DEV, chunk_rows=20)
    assert torch.equal(lens2["images"], lens["images"])
    zero = synthetic.render_dataset({**cams, "distortion": torch.zeros(6)}, times, [0, 2], DEV, chunk_rows=20)
    assert torch.equal(zero["images"], base["images"])

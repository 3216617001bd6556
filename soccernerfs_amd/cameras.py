"""Camera table (perspective, fisheye, equirectangular) + RayGenerator with the interface of NS/cameras/cameras.py and NS/model_components/ray_generators.py.

distortion_params [M,6] (or [6]) are the OpenCV coefficients k1 k2 k3 k4 p1 p2 the dataparsers read.  A table with a non-zero coefficient
generates its rays through the lens, as the reference does (cameras.py:635-653: every pixel coordinate and its two one-pixel offsets are
undistorted with ten Newton steps; ops.generate_rays(distortion_params=...) -> snerf_raygen_lens); a table without coefficients, or with
all-zero rows (for which the undistortion is the identity), takes the pinhole kernel.

camera_type (CameraType, cameras.py:42-58) says how a camera maps its undistorted image coordinates to a direction (cameras.py:663-696):
PERSPECTIVE (x, y, -1); FISHEYE, the equidistant model, theta = |(x, y)| clipped to pi; EQUIRECTANGULAR, longitude -pi x and colatitude
pi (0.5 - y), for which the lens row is ignored (:645-647).  An all-perspective table keeps the two entries above, launch for launch; any
other table -- a mixed one is legal -- takes snerf_raygen_cam, which branches per ray.  RayGenerator(cameras, pose_optimizer) composes a
camera_optimizers.CameraOptimizer's SO3xR3 adjustments into the table first; the camera optimiser's distortion_params_delta is not built.  Image masks belong to the pixel samplers, not to the rays: dataparsers.load_mask_cache, ops.MaskIndex, PixelSampler(mask=...)."""
import copy
from enum import Enum
from typing import Optional, Union

import torch
from torch import nn

from . import ops
from .rays import RayBundle


class CameraType(Enum):
    """Supported camera types: the names and values of NS/cameras/cameras.py:42-47 (auto() counts from 1)."""

    PERSPECTIVE = 1
    FISHEYE = 2
    EQUIRECTANGULAR = 3


# the transforms.json "camera_model" strings the dataparsers accept (NS/cameras/cameras.py:50-58)
CAMERA_MODEL_TO_TYPE = {
    "SIMPLE_PINHOLE": CameraType.PERSPECTIVE,
    "PINHOLE": CameraType.PERSPECTIVE,
    "SIMPLE_RADIAL": CameraType.PERSPECTIVE,
    "RADIAL": CameraType.PERSPECTIVE,
    "OPENCV": CameraType.PERSPECTIVE,
    "OPENCV_FISHEYE": CameraType.FISHEYE,
    "EQUIRECTANGULAR": CameraType.EQUIRECTANGULAR,
}
_TYPE_VALUES = tuple(t.value for t in CameraType)


def camera_type_table(camera_type: Union[None, int, CameraType, torch.Tensor], M: int) -> torch.Tensor:
    """An int, a CameraType or a tensor [M] / [M,1] / [1] -> int32 [M] on the host (cameras.py:228-261); None is perspective.  A value outside
    the enum raises, as cameras.py:698-700 does when rays are asked for."""
    if camera_type is None:
        camera_type = CameraType.PERSPECTIVE
    if isinstance(camera_type, CameraType):
        camera_type = camera_type.value
    if isinstance(camera_type, torch.Tensor):
        if camera_type.is_floating_point() or camera_type.numel() not in (1, M) or camera_type.dim() > 2:
            raise ValueError(f"camera_type {tuple(camera_type.shape)} {camera_type.dtype}: expected an integer tensor [{M}] or [{M}, 1]")
        tab = camera_type.detach().reshape(-1).to("cpu", torch.int32).expand(M).contiguous()
    elif isinstance(camera_type, int) and not isinstance(camera_type, bool):
        tab = torch.full((M,), camera_type, dtype=torch.int32)
    else:
        raise ValueError(f"camera_type {camera_type!r}: expected an int, a CameraType or an integer tensor")
    bad = sorted(set(tab.tolist()) - set(_TYPE_VALUES))
    if bad:
        raise ValueError(f"Camera type {bad[0]} not supported.")
    return tab


class Cameras:
    """camera_to_worlds [M,3,4]; fx, fy, cx, cy [M] (or scalars); width/height ints; times [M]; camera_type an int, a CameraType or an integer
    tensor [M] / [M,1] (default: perspective)."""

    def __init__(self, camera_to_worlds, fx, fy, cx, cy, width: int, height: int, times: Optional[torch.Tensor] = None, **kwargs):
        M = camera_to_worlds.shape[0]
        dev = camera_to_worlds.device
        ex = lambda v: (v.reshape(-1).float() if isinstance(v, torch.Tensor) else torch.tensor([float(v)])).to(dev).expand(M).contiguous()
        self.camera_to_worlds = camera_to_worlds.float().contiguous()
        self.fx, self.fy, self.cx, self.cy = ex(fx), ex(fy), ex(cx), ex(cy)
        self.width, self.height = int(width), int(height)
        self.times = None if times is None else times.reshape(-1).float().to(dev).contiguous()
        self.ids = kwargs.get("ids")  # camera uid per image (Broadcast-style parser), carried for the samplers / metrics
        dp = kwargs.get("distortion_params")
        if dp is not None:
            dp = torch.as_tensor(dp).float()
            if dp.dim() == 0 or dp.shape[-1] != 6 or dp.numel() not in (6, 6 * M):
                raise ValueError(f"distortion_params {tuple(dp.shape)}: expected [6] or [{M}, 6] (k1 k2 k3 k4 p1 p2)")
        # decided once, here, on the host: generate_rays must not read the device back to choose its kernel (.to() copies the flag)
        self.has_distortion = bool(dp is not None and bool((dp != 0).any()))
        self.distortion_params = None if dp is None else dp.reshape(-1, 6).to(dev).expand(M, 6).contiguous()
        # the same for the types: an all-perspective table keeps the pinhole / lens entries; the values are checked here, on the host
        ct = camera_type_table(kwargs.get("camera_type"), M)
        self.all_perspective = bool((ct == CameraType.PERSPECTIVE.value).all())
        self.camera_type = ct.to(dev)  # int32 [M]

    def rescale_output_resolution(self, scaling_factor: float) -> None:
        """NS/cameras/cameras.py:792-816."""
        s = float(scaling_factor)
        self.fx, self.fy, self.cx, self.cy = self.fx * s, self.fy * s, self.cx * s, self.cy * s
        self.height = int(torch.tensor(float(self.height)).mul(torch.tensor(s)).to(torch.int64))
        self.width = int(torch.tensor(float(self.width)).mul(torch.tensor(s)).to(torch.int64))

    def __len__(self):
        return self.camera_to_worlds.shape[0]

    def to(self, device):
        """The same table on `device`.  A copy of this object with its tensors moved: the host flag goes along, nothing is read back."""
        moved = copy.copy(self)
        for name in ("camera_to_worlds", "fx", "fy", "cx", "cy", "times", "distortion_params", "camera_type"):
            t = getattr(self, name)
            setattr(moved, name, None if t is None else t.to(device))
        return moved

    def generate_rays(self, camera_indices: torch.Tensor, coords: Optional[torch.Tensor] = None, aabb=None, near_plane=0.0,
                      training=True, disable_distortion: bool = False, **kwargs) -> RayBundle:
        """camera_indices [R,1] (or an int for a full image); coords [R,2] = (y+0.5, x+0.5) pixel centres.
        disable_distortion (cameras.py:300-311): the lens rows are dropped even for a table that carries non-zero coefficients; the cameras'
        types stay."""
        if isinstance(camera_indices, int):
            ys, xs = torch.meshgrid(torch.arange(self.height), torch.arange(self.width), indexing="ij")
            idx = torch.stack([torch.full_like(ys, camera_indices), ys, xs], -1).reshape(-1, 3).to(self.camera_to_worlds.device)
            shape = (self.height, self.width)
        else:
            yx = torch.floor(coords).long()
            idx = torch.cat([camera_indices.reshape(-1, 1).long(), yx], dim=-1)
            shape = None
        out = ops.generate_rays(idx.contiguous(), self.fx, self.fy, self.cx, self.cy, self.camera_to_worlds, self.times, aabb, near_plane, training,
                                distortion_params=self.distortion_params if self.has_distortion and not disable_distortion else None,
                                camera_type=None if self.all_perspective else self.camera_type, validate_camera_type=False)
        rb = RayBundle(origins=out["origins"], directions=out["directions"], pixel_area=out["pixel_area"], camera_indices=out["camera_indices"],
                       nears=out.get("nears"), fars=out.get("fars"), metadata={"directions_norm": out["directions_norm"]},
                       times=out["times"] if self.times is not None else None)
        if shape is not None:
            rb = rb._map(lambda t: t.view(*shape, t.shape[-1]))
        return rb


class RayGenerator(nn.Module):
    """ray_generators.py:27-59.  pose_optimizer: a camera_optimizers.CameraOptimizer whose adjustments are composed into the whole table
    before the rays are formed (one snerf_pose_apply launch per call; cameras.py:707-708); None, or one with mode "off", issues the
    launches this class always issued."""

    def __init__(self, cameras: Cameras, pose_optimizer=None) -> None:
        super().__init__()
        self.cameras = cameras
        self.pose_optimizer = pose_optimizer

    def forward(self, ray_indices: torch.Tensor) -> RayBundle:
        idx = ray_indices.long()
        coords = idx[:, 1:3].float() + 0.5
        cameras = self.cameras
        if self.pose_optimizer is not None and self.pose_optimizer.config.mode != "off":
            cameras = self.pose_optimizer.adjusted(cameras)
        return cameras.generate_rays(camera_indices=idx[:, 0:1], coords=coords)

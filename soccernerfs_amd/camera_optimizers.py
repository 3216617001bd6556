"""Pose optimisation of the training cameras: CameraOptimizer of NS/cameras/camera_optimizers.py:30-133, mode SO3xR3.

A learned 6-vector per training image (translation, then an so(3) vector) is composed into camera_to_worlds BEFORE ray generation
(NS/cameras/cameras.py:707-708: c2w' = multiply(c2w, exp_map_SO3xR3(adj)), NS/cameras/lie_groups.py:23-58); it trains with Adam at lr 6e-4,
eps 1e-15 under an exponential schedule whose lr_final is None, i.e. a constant lr (NS/engine/schedulers.py:84-106).  Where the reference
leaves the gradient to autograd, the chain here is explicit:

    rays = raygen(opt.adjusted_camera_to_worlds(cameras))        snerf_pose_apply, then the raygen kernels as they are
    trainer.train_step(rays, ...)                                KPlanesTrainConfig(ray_gradients=True) leaves trainer.ray_grads
    opt.backward(indices, trainer.ray_grads)                     snerf_raygen_pose_bwd -> grad [G,6]
    opt.step()                                                   snerf_adam_step over the whole [G,6] buffer

`groups` is this package's addition: a LongTensor [M] mapping each training image to a physical camera, so that the frames of one static
camera share ONE adjustment (dataparsers.camera_pose_groups); None is the reference's one row per image.

Not built: mode "SE3", the reference's debugging pose noise inside the class (tools/train_psnr.py --pose-noise perturbs the table on the
host instead), the distortion-parameter delta.  Bin edges (nears / fars) carry no gradient: a deliberate deviation, see include/snerf.h."""
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import nn

from . import ops

PIPELINE_KEY = "datamanager.train_camera_optimizer.pose_adjustment"  # NS/data/datamanagers/base_datamanager.py:444-449


@dataclass
class CameraOptimizerConfig:
    """NS/cameras/camera_optimizers.py:30-56; optimizer = AdamOptimizerConfig(lr=6e-4, eps=1e-15) and
    scheduler = ExponentialDecaySchedulerConfig(max_steps=10000) flattened into lr / eps / max_steps / lr_final."""

    mode: str = "off"  # "off" | "SO3xR3" | "SE3" (not built)
    position_noise_std: float = 0.0
    orientation_noise_std: float = 0.0
    lr: float = 6e-4
    eps: float = 1e-15
    max_steps: int = 10000
    lr_final: Optional[float] = None  # None = lr: a constant schedule, as the reference's preset has it
    param_group: str = "camera_opt"


def exponential_decay_lr(step: int, lr_init: float, lr_final: Optional[float], max_steps: int) -> float:
    """ExponentialDecayScheduler with warmup_steps = 0 (NS/engine/schedulers.py:84-106): exp(log(lr_init) (1 - t) + log(lr_final) t),
    t = clip(step / max_steps, 0, 1)."""
    lr_final = lr_init if lr_final is None else lr_final
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


class CameraOptimizer(nn.Module):
    """Layer that modifies camera poses to be optimised as well as the field during training (the reference's name and signature;
    `groups` added)."""

    def __init__(self, config: CameraOptimizerConfig, num_cameras: int, device, groups: Optional[torch.Tensor] = None, **kwargs) -> None:
        super().__init__()
        self.config, self.num_cameras, self.device = config, int(num_cameras), torch.device(device)
        if config.mode not in ("off", "SO3xR3", "SE3"):
            raise ValueError(f"CameraOptimizerConfig.mode {config.mode!r}: expected 'off', 'SO3xR3' or 'SE3'")
        if config.mode == "SE3":
            raise NotImplementedError("CameraOptimizer mode 'SE3' is not built (the reference recommends SO3xR3)")
        if config.position_noise_std != 0.0 or config.orientation_noise_std != 0.0:
            raise NotImplementedError("CameraOptimizer pose noise (position_noise_std / orientation_noise_std) is not built: perturb the camera "
                                      "table on the host (tools/train_psnr.py --pose-noise)")
        self.groups, self._groups_i32, self._cameras = None, None, None
        self.num_groups = self.num_cameras
        if groups is not None:
            g = torch.as_tensor(groups)
            if g.is_floating_point() or g.dim() != 1 or g.numel() != self.num_cameras:
                raise ValueError(f"groups {tuple(g.shape)} {g.dtype}: expected an integer tensor [{self.num_cameras}]")
            g = g.detach().to("cpu", torch.int64)
            if self.num_cameras and (int(g.min()) < 0):
                raise ValueError("groups: negative camera index")
            n = int(g.max()) + 1 if self.num_cameras else 0
            if self.num_cameras and len(torch.unique(g)) != n:
                raise ValueError(f"groups: the indices must cover 0..{n - 1} without gaps (a row without images would never be trained)")
            self.num_groups = n
            self.groups = g.to(self.device)  # a plain attribute: not part of the state_dict, which holds the reference's one key
            self._groups_i32 = self.groups.to(torch.int32).contiguous()
        if config.mode == "off":
            return
        G = self.num_groups
        self.pose_adjustment = nn.Parameter(torch.zeros(G, 6, dtype=torch.float32, device=self.device), requires_grad=False)
        self.grad = torch.zeros(G, 6, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.step_count = 0  # scheduler steps = calls of step(); Adam's own counter lives in _dyn (it does not advance on a skipped step)
        if self.device.type == "cuda":
            self._grad_fx = torch.zeros(G, 6, dtype=torch.int64, device=self.device)
            self._dyn = ops.new_adam_dyn(self.device)

    # ---- forward ----
    def _rows(self, indices: torch.Tensor) -> torch.Tensor:
        indices = indices.reshape(-1).long()
        return indices if self.groups is None else self.groups[indices]

    def forward(self, indices: torch.Tensor) -> torch.Tensor:
        """indices [n] of training images -> [n,3,4]: the transforms from optimised camera coordinates to the given ones
        (camera_optimizers.py:98-133).  Mode "off": identities."""
        n = indices.reshape(-1).shape[0]
        eye = torch.eye(4, device=self.device)[None, :3, :4].tile(n, 1, 1).contiguous()
        if self.config.mode == "off":
            return eye
        return ops.pose_apply(eye, self.pose_adjustment.data[self._rows(indices).to(self.device)].contiguous())

    def adjusted_camera_to_worlds(self, cameras) -> torch.Tensor:
        """[M,3,4]: the camera table's camera_to_worlds composed with every image's adjustment (one snerf_pose_apply launch); the table
        itself for mode "off"."""
        if len(cameras) != self.num_cameras:
            raise ValueError(f"the optimiser holds {self.num_cameras} cameras, the table {len(cameras)}")
        self._cameras = cameras  # the unadjusted table backward() differentiates
        if self.config.mode == "off":
            return cameras.camera_to_worlds
        return ops.pose_apply(cameras.camera_to_worlds, self.pose_adjustment.data, self._groups_i32)

    def adjusted(self, cameras):
        """The same Cameras with the adjusted camera_to_worlds: for training rays, for the renderer and for evaluating training views."""
        import copy

        out = copy.copy(cameras)
        out.camera_to_worlds = self.adjusted_camera_to_worlds(cameras)
        return out

    # ---- backward + optimiser ----
    def backward(self, indices: torch.Tensor, ray_grads: Dict[str, torch.Tensor], cameras=None) -> torch.Tensor:
        """grad [G,6] += d(loss) / d(pose_adjustment) of the batch: indices int64 [R,3] (image, row, col) as the rays were generated from,
        ray_grads = {"origins", "directions"} [R,3] (KPlanesTrainer.ray_grads).  cameras: the UNADJUSTED table; default: the one
        adjusted_camera_to_worlds() / adjusted() last composed.  Returns self.grad."""
        if self.config.mode == "off":
            raise RuntimeError("CameraOptimizer.backward: mode is 'off'")
        cameras = self._cameras if cameras is None else cameras
        if cameras is None:
            raise RuntimeError("CameraOptimizer.backward: no camera table (call adjusted_camera_to_worlds(cameras) first, or pass cameras=)")
        ops.raygen_pose_bwd(indices, cameras.fx, cameras.fy, cameras.cx, cameras.cy, cameras.camera_to_worlds, self.pose_adjustment.data,
                            ray_grads["origins"], ray_grads["directions"], self._grad_fx,
                            group=self._groups_i32,
                            distortion_params=cameras.distortion_params if cameras.has_distortion else None,
                            camera_type=None if cameras.all_perspective else cameras.camera_type, dyn=self._dyn)
        ops.fx_to_float(self._grad_fx.view(-1), self.grad.view(-1), accumulate=True)
        return self.grad

    def lr(self, step: Optional[int] = None) -> float:
        c = self.config
        return exponential_decay_lr(self.step_count if step is None else step, c.lr, c.lr_final, c.max_steps)

    def step(self) -> None:
        """Dense Adam over the whole [G,6] buffer (rows without rays see a zero gradient and still move with their moments, as
        torch.optim.Adam moves them); clears the gradient.  A non-finite pose gradient skips the step (skipped_steps())."""
        if self.config.mode == "off":
            return
        lr = self.lr()
        ops.adam_prepare(self._dyn, lr, policy="skip_step")
        ops.adam_step(self.pose_adjustment.data.view(-1), self.grad.view(-1), self.exp_avg.view(-1), self.exp_avg_sq.view(-1), 0, lr,
                      eps=self.config.eps, zero_grad=True, dyn=self._dyn)
        self.step_count += 1

    def skipped_steps(self) -> Dict[str, int]:
        """{"camera_opt": steps skipped for a non-finite gradient}, in the shape of KPlanesTrainer.skipped_steps().  Synchronises."""
        if self.config.mode == "off":
            return {self.config.param_group: 0}
        return {self.config.param_group: int(self._dyn.cpu()[2])}

    # ---- state ----
    def state_dict(self, *args, **kwargs):
        """{"pose_adjustment": [G,6]} (nn.Module's own, so a reference-style pipeline state_dict carries PIPELINE_KEY)."""
        return super().state_dict(*args, **kwargs)

    def optimizer_state_dict(self) -> Dict:
        """torch.optim.Adam-style state of the one parameter: the reference checkpoint's optimizers["camera_opt"]."""
        c = self.config
        adam_t = int(self._dyn.cpu()[1]) if self.device.type == "cuda" else self.step_count
        state = {}
        if adam_t > 0:
            state[0] = {"step": torch.tensor(float(adam_t)), "exp_avg": self.exp_avg.detach().cpu().clone(),
                        "exp_avg_sq": self.exp_avg_sq.detach().cpu().clone()}
        return {"state": state, "param_groups": [{"lr": self.lr(), "betas": (0.9, 0.999), "eps": c.eps, "weight_decay": 0, "amsgrad": False,
                                                  "params": [0]}]}

    @torch.no_grad()
    def load_optimizer_state_dict(self, sd: Dict) -> None:
        st = sd.get("state", {}).get(0)
        if st is None:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            t = 0
        else:
            self.exp_avg.copy_(st["exp_avg"].float().to(self.device))
            self.exp_avg_sq.copy_(st["exp_avg_sq"].float().to(self.device))
            t = int(st["step"])
        self.step_count = t
        if self.device.type == "cuda":
            self._dyn.zero_()
            self._dyn[1] = t

    def checkpoint_entries(self):
        """(pipeline entries, optimiser entries) this optimiser adds to a nerfstudio checkpoint; both empty for mode "off", so that a
        checkpoint written with the feature off has exactly the keys it always had."""
        if self.config.mode == "off":
            return {}, {}
        return ({PIPELINE_KEY: self.pose_adjustment.detach().cpu().clone()}, {self.config.param_group: self.optimizer_state_dict()})

    @torch.no_grad()
    def load_checkpoint_entries(self, pipeline: Dict, optimizers: Optional[Dict] = None) -> None:
        """From a loaded checkpoint's "pipeline" / "optimizers" dicts.  A checkpoint without the key (written with the feature off) starts
        the adjustments from zeros."""
        if self.config.mode == "off":
            return
        t = pipeline.get(PIPELINE_KEY)
        if t is None:
            self.pose_adjustment.zero_()
            self.load_optimizer_state_dict({})
            return
        if tuple(t.shape) != tuple(self.pose_adjustment.shape):
            raise RuntimeError(f"{PIPELINE_KEY}: the checkpoint holds {tuple(t.shape)}, the optimiser {tuple(self.pose_adjustment.shape)}")
        self.pose_adjustment.copy_(t.float().to(self.device))
        self.load_optimizer_state_dict((optimizers or {}).get(self.config.param_group, {}))

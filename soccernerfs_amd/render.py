"""Rendering whole frames and camera paths from a trained model: the `ns-render` / `ns-eval` counterpart on the fused trainers.

What the reference does (scripts/render.py:60-131, scripts/eval.py): per camera Cameras.generate_rays(camera_indices=k), then
Model.get_outputs_for_camera_ray_bundle (NS/models/base_model.py:159-186) pushes the frame through the model in chunks of
--eval-num-rays-per-chunk rays and reshapes rgb / accumulation / depth to [H, W, .].  Here a chunk is one fixed sequence of libsnerf launches
on the caller's stream, built for inference.  For K-Planes (KPlanesRenderer):

  1. snerf_raygen_frame            rays of the chunk's pixels (no index table) + the AABB collider; snerf_raygen_frame_lens for a camera
                                   whose distortion row has a non-zero coefficient, snerf_raygen_frame_cam for a fisheye or
                                   equirectangular camera
  2. snerf_spaced_bins             the first level's bins, no jitter
  3. 2 x (snerf_kplanes_density_fwd + snerf_pdf_resample, u_mode 2)   the proposal levels, eval-mode sampler
  4. snerf_kplanes_field_fwd + snerf_weights_fwd + snerf_render_fwd, or (fused_tail=True / a transmittance cutoff) snerf_kplanes_field_render:
     plane gather -> sigma_net -> colour net -> weights -> rgb / accumulation / median depth in ONE kernel

against ~10 launches per 4096-ray slice through KPlanesTrainer.forward(training=False).  The results are the same bits.

FrameRenderer holds what does not depend on the model -- the host camera table, the choice of the frame ray kernel, the chunk loop with its
ragged last chunk, to_uint8, render_camera_path, evaluate, launch counting and kernel timing.  KPlanesRenderer and NerfplayerRenderer (the
NeRFPlayer-nerfacto trainer's chunk, listed at the class) derive from it.
"""
import ctypes as C
import os
from typing import Dict, Optional, Sequence, Union

import torch

from . import _lib, metrics, ops
from .camera_paths import ALL_CAMERA_TYPES, get_path_from_json, load_camera_path
from .cameras import Cameras, CameraType
from .fused_step import FusedStep, anneal_value


class FrameRenderer:
    """What a frame renderer on a fused trainer does whatever the model: camera -> frame ray kernel -> chunks of `R` pixels -> [H,W,.] outputs,
    camera paths, image metrics, launch counting and kernel timing.  A subclass owns trainer, R (rays per chunk), S, aabb, cfg, dev, its work
    buffers `buf` and the chunk's ray buffers `_rays`, and provides _chunk(), _begin_frame(), default_anneal(), _near_plane() and MODEL."""

    MODEL = "the model"  # named in the refusal of a camera table without times
    _timing, _timing_all = None, False
    _box_interval = None  # where the frame ray kernels write their box interval when that is not _rays' own nears / fars (an unbounded scene)

    # the launches whose argument lists the fused trainers share (fused_step.py), on this object's buffers
    _call = FusedStep._call  # through this object's _ck, which counts the launches
    _p = FusedStep._p
    _span = FusedStep._span
    _spaced_bins = FusedStep._spaced_bins
    _resample = FusedStep._resample
    _render_fwd = FusedStep._render_fwd
    _mlp_fwd = FusedStep._mlp_fwd
    enable_kernel_timing, disable_kernel_timing, kernel_times_ms = FusedStep.enable_kernel_timing, FusedStep.disable_kernel_timing, FusedStep.kernel_times_ms

    def _init_frames(self, rays_per_chunk: int):
        """The chunk's ray buffers, the launch counter and the host camera table cache."""
        R = int(rays_per_chunk)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        self._rays = {"origins": f(R, 3), "directions": f(R, 3), "pixel_area": f(R), "directions_norm": f(R), "times": f(R), "nears": f(R), "fars": f(R)}
        self.launches = 0          # libsnerf launches issued so far (tools/bench_render.py: launches per frame)
        self._host_tables = {}

    def _ck(self, rc: int, what: str = ""):
        self.launches += 1
        _lib.check(rc, what)

    # ---- cameras ----
    def _host_table(self, cameras: Cameras):
        """fx, fy, cx, cy, c2w, times, distortion rows and camera types of a camera table as host lists (snerf_raygen_frame(_lens, _cam) takes
        one camera by value): read back once per table."""
        key = id(cameras)
        hit = self._host_tables.get(key)
        if hit is None or hit[0] is not cameras:
            t = lambda x: x.detach().cpu().tolist()
            hit = (cameras, {"fx": t(cameras.fx), "fy": t(cameras.fy), "cx": t(cameras.cx), "cy": t(cameras.cy),
                             "c2w": t(cameras.camera_to_worlds.reshape(len(cameras), 12)), "times": None if cameras.times is None else t(cameras.times),
                             "distortion": t(cameras.distortion_params) if cameras.has_distortion else None,
                             "camera_type": None if cameras.all_perspective else t(cameras.camera_type)})
            self._host_tables = {key: hit}
        return hit[1]

    def _time_free(self) -> bool:
        """True when no kernel of the model reads the time: a camera table without times then needs no default_time."""
        return False

    def _raygen(self, ra, p0: int, p1: int):
        """The rays of pixels [p0, p1) into _rays, through the entry that matches the camera (render_frame chose the argument struct)."""
        ra.p0, ra.p1 = p0, p1
        with self._span("raygen_frame"):
            if isinstance(ra, _lib.RaygenFrameCamArgs):
                self._call("raygen_frame_cam", C.byref(ra), self._st)
            elif isinstance(ra, _lib.RaygenFrameLensArgs):
                self._call("raygen_frame_lens", C.byref(ra), self._st)
            else:
                self._call("raygen_frame", C.byref(ra), self._st)

    # ---- public ----
    @torch.no_grad()
    def render_frame(self, cameras: Cameras, index: int, anneal: Optional[float] = None, default_time: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """Camera `index` of `cameras` -> {"rgb": [H,W,3], "accumulation": [H,W,1], "depth": [H,W,1]} (device tensors, fresh per call): the keys and
        shapes of Model.get_outputs_for_camera_ray_bundle; depth is the depth the model renders (K-Planes: median; NeRFPlayer-nerfacto: expected).
        anneal: the proposal sampler's annealing exponent (default: default_anneal()); default_time: the time of a camera table without times
        (not needed, and ignored, when the trainer is a static scene or has frozen time planes: its descriptors hold no time plane)."""
        tab = self._host_table(cameras)
        if not 0 <= index < len(tab["fx"]):
            raise IndexError(f"camera index {index} outside the table of {len(tab['fx'])}")
        if tab["times"] is None and default_time is None and not self._time_free():
            raise ValueError(f"the cameras carry no times (a camera path has them only if every entry has render_time) and {self.MODEL} is a dynamic "
                             "model: pass default_time")
        H, W = cameras.height, cameras.width
        row = tab["distortion"][index] if tab["distortion"] is not None else None
        lens = row is not None and any(v != 0.0 for v in row)  # the camera's own row: an all-zero row of a lens table is a pinhole camera
        kind = tab["camera_type"][index] if tab["camera_type"] is not None else CameraType.PERSPECTIVE.value
        if kind != CameraType.PERSPECTIVE.value:  # a perspective camera of a mixed table takes the entries it always took
            ra = _lib.RaygenFrameCamArgs()
            ra.camera_type, ra.has_distortion = kind, int(lens)
            for k in range(6):
                ra.distortion[k] = row[k] if lens else 0.0
        elif lens:
            ra = _lib.RaygenFrameLensArgs()
            for k in range(6):
                ra.distortion[k] = row[k]
        else:
            ra = _lib.RaygenFrameArgs()
        ra.fx, ra.fy, ra.cx, ra.cy = tab["fx"][index], tab["fy"][index], tab["cx"][index], tab["cy"][index]
        ra.time = tab["times"][index] if tab["times"] is not None else float(default_time if default_time is not None else 0.0)
        for k in range(12):
            ra.c2w[k] = tab["c2w"][index][k]
        ra.W, ra.H, ra.near_plane = W, H, self._near_plane()
        for k in range(3):
            ra.aabb_min[k], ra.aabb_max[k] = self.aabb[0][k], self.aabb[1][k]
        rays = self._rays
        ra.origins, ra.dirs, ra.pixel_area, ra.dir_norm = (rays[k].data_ptr() for k in ("origins", "directions", "pixel_area", "directions_norm"))
        box_near, box_far = self._box_interval if self._box_interval is not None else (rays["nears"], rays["fars"])
        ra.times, ra.nears, ra.fars = rays["times"].data_ptr(), box_near.data_ptr(), box_far.data_ptr()
        f = lambda c: torch.empty(H * W, c, dtype=torch.float32, device=self.dev)
        out = {"rgb": f(3), "accumulation": f(1), "depth": f(1)}
        self._st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._begin_frame(H, W)
        anneal = self.default_anneal() if anneal is None else float(anneal)
        for p0 in range(0, H * W, self.R):
            self._chunk(ra, p0, min(p0 + self.R, H * W), anneal, out)
        return {k: v.view(H, W, -1) for k, v in out.items()}

    @staticmethod
    def to_uint8(x: torch.Tensor) -> torch.Tensor:
        """floor(255 clamp(x, 0, 1) + 0.5) as uint8.  The reference hands the float frame to a third-party image library (mediapy, not in its
        tree) for this conversion: this one line is RESTATED, not pinned to the reference."""
        return torch.floor(255.0 * x.clamp(0.0, 1.0) + 0.5).to(torch.uint8)

    @torch.no_grad()
    def render_camera_path(self, path: Union[str, dict], output_dir: str, outputs: Sequence[str] = ("rgb",), format: str = "png",
                           default_time: Optional[float] = None, anneal: Optional[float] = None):
        """Renders every camera of a camera-path dict (or the JSON file holding one) and writes one file per camera, `%05d.png` (or `.npy`: the
        float frame) in output_dir, named as the reference's `--output-format images` (scripts/render.py:83-85, :131-132).  Several outputs
        are concatenated along the width, single-channel ones repeated to three channels (:117-130).  Returns the list of files written."""
        if format not in ("png", "npy"):
            raise ValueError(f"format={format!r}: 'png' or 'npy' (video encoding is out of scope)")
        cameras = get_path_from_json(load_camera_path(path), camera_types=ALL_CAMERA_TYPES)
        if cameras.times is None and default_time is None and not self._time_free():
            raise ValueError(f"the camera path has no render_time on every entry and no default_time was given: {self.MODEL} needs a time per frame")
        os.makedirs(output_dir, exist_ok=True)
        files = []
        for k in range(len(cameras)):
            frame = self.render_frame(cameras, k, anneal=anneal, default_time=default_time)
            parts = []
            for name in outputs:
                if name not in frame:
                    raise KeyError(f"could not find {name!r} in the model outputs {sorted(frame)}")
                img = frame[name]
                parts.append(img.expand(-1, -1, 3) if img.shape[-1] == 1 else img)
            image = torch.cat(parts, dim=1)
            fn = os.path.join(output_dir, f"{k:05d}.{format}")
            if format == "png":
                from PIL import Image

                Image.fromarray(self.to_uint8(image).cpu().numpy()).save(fn)
            else:
                import numpy as np

                np.save(fn, image.cpu().numpy())
            files.append(fn)
        return files

    @torch.no_grad()
    def evaluate(self, cameras: Cameras, images: torch.Tensor, indices: Sequence[int], anneal: Optional[float] = None) -> Dict[str, object]:
        """PSNR and SSIM of full-frame renders against images[indices] (uint8 [M,H,W,3], or float in [0,1]), per image and averaged, as
        get_image_metrics_and_images reports them (NS/models/kplanes.py:454-498; soccernerfs_amd/metrics.py)."""
        psnrs, ssims = [], []
        for m in indices:
            rgb = self.render_frame(cameras, int(m), anneal=anneal)["rgb"]
            gt = images[m].to(self.dev)
            gt = gt.float() / 255.0 if gt.dtype == torch.uint8 else gt.float()
            chw = lambda x: x.permute(2, 0, 1)[None]
            psnrs.append(float(metrics.psnr(rgb, gt)))
            ssims.append(float(metrics.structural_similarity_index_measure(chw(gt), chw(rgb))))
        mean = lambda xs: sum(xs) / max(len(xs), 1)
        return {"psnr": mean(psnrs), "ssim": mean(ssims), "psnr_per_image": psnrs, "ssim_per_image": ssims}


class KPlanesRenderer(FrameRenderer):
    """Eval-mode renderer on a KPlanesTrainer's parameters.

    It shares the trainer's parameter views, plane descriptors and net objects (nothing is copied: it renders whatever the trainer holds when a
    frame is asked for) and owns its own work buffers, sized for `rays_per_chunk`; the trainer's buffers are not touched, so rendering between
    two training steps leaves training bit-for-bit undisturbed.  Launches go to the CURRENT stream, which must be the stream the trainer's
    train_step is called on (or be synchronised with it): before its first read of the parameters a frame joins the trainer's pending optimiser
    sweep with stream waits (KPlanesTrainer._join_prop / _wait_params, the stream-level parts of synchronize()); there is no host synchronise.

    fused_tail=True runs the render tail as one kernel (snerf_kplanes_field_render, the same bits).  It is OFF by default: measured on the trained
    preset the one kernel takes 25.7 ms of a 960 x 540 frame against 20.6 ms for snerf_kplanes_field_fwd + snerf_weights_fwd + snerf_render_fwd
    (DESIGN 4.9).  transmittance_cutoff > 0 opts into early ray termination (an approximation bounded by the cutoff) and turns the fused tail
    on, which it needs.  A shape the render kernel is not built for (S not a multiple of 32, fp32 operands, ...) always runs the unfused tail,
    with gather + snerf_mlp_fwd where the trainer's own forward uses them."""

    MODEL = "K-Planes"
    SPACING = FusedStep.SPACING
    _FIELD_SLICE = 4096  # rays per launch group of the unfused (fp32-operand) field: bounds the [N, 32 n_scales] feature buffer

    def __init__(self, trainer, rays_per_chunk: int = 65536, transmittance_cutoff: float = 0.0, fused_tail: bool = False):
        if rays_per_chunk < 1:
            raise ValueError(f"rays_per_chunk={rays_per_chunk}")
        if not 0.0 <= transmittance_cutoff < 1.0:
            raise ValueError(f"transmittance_cutoff={transmittance_cutoff}: expected 0 <= cutoff < 1")
        self.trainer, self.R, self.dev = trainer, int(rays_per_chunk), trainer.dev
        self.cfg, self.S, self.aabb, self.lib = trainer.cfg, trainer.S, trainer.aabb, trainer.lib
        # an unbounded trainer (cfg.bounded = False): contracted coordinates, the piecewise spacing and NearFarCollider in eval mode (near 0)
        self.contract, self.SPACING = bool(getattr(trainer, "contract", False)), trainer.SPACING
        self.transmittance_cutoff = float(transmittance_cutoff)
        S2 = self.S[2]
        # a cutoff asks for the fused tail: only that kernel knows a ray's transmittance before its last sample is decoded
        self.fused_tail = bool((fused_tail or self.transmittance_cutoff > 0.0) and trainer.fused_field and self.lib.snerf_kplanes_field_render_supported(
            C.byref(trainer._desc_field), C.byref(trainer.sigma_net.desc), C.byref(trainer.color_net.desc), S2))
        if self.transmittance_cutoff > 0.0 and not self.fused_tail:
            raise ValueError("transmittance_cutoff > 0 needs the fused render tail (snerf_kplanes_field_render), which is not built for this shape")
        R = self.R
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        self.buf = {"sb": [f(R, s + 1) for s in self.S], "eb": [f(R, s + 1) for s in self.S],
                    "dens": [f(R, self.S[0]), f(R, self.S[1]), None], "w": [f(R, self.S[0]), f(R, self.S[1]), None]}
        self._init_frames(R)
        if self.contract:
            # the frame ray kernels always write their box interval: it goes to a side buffer nobody reads, and the samplers see the constants
            self._box_interval = (self._rays["nears"], self._rays["fars"])
            self._rays["nears"] = torch.zeros(R, dtype=torch.float32, device=self.dev)
            self._rays["fars"] = torch.full((R,), float(self.cfg.far_plane), dtype=torch.float32, device=self.dev)
        if not self.fused_tail:
            self.buf["dens"][2], self.buf["w"][2], self.buf["rgb"] = f(R, S2), f(R, S2), f(R * S2, 3)
            if not trainer.fused_field:
                n = min(R, self._FIELD_SLICE) * S2
                self.buf["feat"], self.buf["h"] = f(n, trainer.field_planes.out_dim), f(n, 16)
                if trainer.view_dependent:
                    self.buf["cx"] = f(n, 32)
        if not trainer.fused_proposal:
            pf = self.cfg.proposal_feature_dim
            self.buf["pfeat"] = [f(R * self.S[0], pf), f(R * self.S[1], pf)]
            self.buf["pout"] = [f(R * self.S[0], 1), f(R * self.S[1], 1)]
        self.samples_done = None   # int32 [H * W] of the last frame when record_samples_done is set (fused tail only)
        self.record_samples_done = False

    def _time_free(self) -> bool:
        return bool(getattr(self.trainer, "_static", False))  # three planes per scale (a static scene / frozen time planes): no kernel reads the time

    def _near_plane(self) -> float:
        return self.cfg.near_plane

    def default_anneal(self) -> float:
        """The proposal-weight annealing exponent tools/train_psnr.py evaluates with: that of the last completed training step."""
        cfg = self.cfg
        return anneal_value(max(self.trainer.step - 1, 0), cfg.proposal_weights_anneal_max_num_iters, cfg.proposal_weights_anneal_slope)

    def _begin_frame(self, H: int, W: int):
        self.samples_done = torch.empty(H * W, dtype=torch.int32, device=self.dev) if self.record_samples_done and self.fused_tail else None
        # step N's parameters: the proposal chain and the field planes' optimiser sweep (side stream, ping-pong buffers) are joined by stream waits
        self.trainer._join_prop()
        self.trainer._wait_params()

    # ---- one chunk ----
    def _chunk(self, ra, p0: int, p1: int, anneal: float, out: Dict[str, torch.Tensor]):
        tr, b, rays = self.trainer, self.buf, self._rays
        n = p1 - p0
        self._raygen(ra, p0, p1)
        self.rays, self._fwd_rays = rays, n
        self._spaced_bins(None)
        o, d, t = rays["origins"], rays["directions"], rays["times"]
        for lvl in range(2):
            co = ops.coords_from_rays(o, d, t, b["eb"][lvl], self.aabb, False, self.contract)
            N, net = n * self.S[lvl], tr.prop_nets[lvl]
            if tr.fused_proposal:
                with self._span("kplanes_density_fwd"):
                    self._call("kplanes_density_fwd", C.byref(tr._desc_prop[lvl]), self._p(tr.prop_planes[lvl].planes), C.byref(co), N,
                               C.byref(net.desc), self._p(net.params), self._p(b["dens"][lvl]), None, self._st)
            else:
                with self._span("kplanes_gather_fwd.prop"):
                    self._call("kplanes_gather_fwd", C.byref(tr._desc_prop[lvl]), self._p(tr.prop_planes[lvl].planes), C.byref(co), N,
                               self._p(b["pfeat"][lvl]), self._st)
                self._mlp_fwd(net, b["pfeat"][lvl], self.cfg.proposal_feature_dim, N, b["pout"][lvl], 1, 0, b["dens"][lvl])
            self._resample(lvl, None, anneal)
        S2 = self.S[2]
        co = ops.coords_from_rays(o, d, t, b["eb"][2], self.aabb, True, self.contract)
        rgb, acc, depth = out["rgb"][p0:p1], out["accumulation"][p0:p1], out["depth"][p0:p1]
        if self.fused_tail:
            sd = self.samples_done[p0:p1] if self.samples_done is not None else None
            with self._span("kplanes_field_render"):
                self._call("kplanes_field_render", C.byref(tr._desc_field), self._p(tr.field_planes.planes), C.byref(co), n, C.byref(tr.sigma_net.desc),
                           self._p(tr.sigma_net.params), C.byref(tr.color_net.desc), self._p(tr.color_net.params),
                           self.transmittance_cutoff, self._p(rgb), self._p(acc), self._p(depth), None, None,
                           self._p(sd) if sd is not None else None, self._st)
            return
        if tr.fused_field:
            with self._span("kplanes_field_fwd"):
                self._call("kplanes_field_fwd", C.byref(tr._desc_field), self._p(tr.field_planes.planes), C.byref(co), n * S2,
                           C.byref(tr.sigma_net.desc), self._p(tr.sigma_net.params), C.byref(tr.color_net.desc),
                           self._p(tr.color_net.params), self._p(b["dens"][2]), self._p(b["rgb"]), None, None, None, self._st)
        else:  # exact-fp32 operands (or fused_field off): gather + the generic MLP kernels, as the trainer's forward, a slice of rays at a time
            F = tr.field_planes.out_dim
            for r0 in range(0, n, self._FIELD_SLICE):
                r1 = min(r0 + self._FIELD_SLICE, n)
                N = (r1 - r0) * S2
                cs = ops.coords_from_rays(o[r0:r1], d[r0:r1], t[r0:r1], b["eb"][2][r0:r1], self.aabb, True, self.contract)
                with self._span("kplanes_gather_fwd.field"):
                    self._call("kplanes_gather_fwd", C.byref(tr._desc_field), self._p(tr.field_planes.planes), C.byref(cs), N, self._p(b["feat"]),
                               self._st)
                self._mlp_fwd(tr.sigma_net, b["feat"], F, N, b["h"], 16, 15, b["dens"][2][r0:r1])
                rgb_s = b["rgb"][r0 * S2:r1 * S2]
                if tr.view_dependent:
                    with self._span("kplanes_color_input_fwd"):
                        self._call("kplanes_color_input_fwd", self._p(d[r0:r1]), S2, self._p(b["h"]), N, self._p(b["cx"]), self._st)
                    self._mlp_fwd(tr.color_net, b["cx"], 32, N, rgb_s, 3)
                else:
                    self._mlp_fwd(tr.color_net, b["h"], 16, N, rgb_s, 3)
        with self._span("weights_render_fwd"):
            self._call("weights_fwd", self._p(b["dens"][2]), self._p(b["eb"][2]), n, S2, self._p(b["w"][2]), self._st)
            b["rgb_out"], b["acc"], b["depth"] = rgb, acc, depth
            self._render_fwd(False, 1, None, "depth_median")


class NerfplayerRenderer(FrameRenderer):
    """Eval-mode renderer on a NerfplayerTrainer's parameters (the nerfplayer-nerfacto preset; NerfplayerNerfactoModel.get_outputs in eval mode,
    NS/models/nerfplayer_nerfacto.py:206-256, chunked as NS/models/base_model.py:159-186).

    It shares the trainer's parameter views, encoders and nets and owns its work buffers: per-sample intermediates (table features, decode
    output, head input) are sliced _FIELD_SLICE rays at a time, so no buffer grows with the frame.  Launches go to the CURRENT stream, which must
    be the stream train_step is called on; a frame calls trainer.wait_params() (a stream wait for the asynchronous table sweep / tile pass) before
    its first table read and never synchronises the host.  One chunk of `rays_per_chunk` pixels (default: the preset's
    eval_num_rays_per_chunk) is

      1. snerf_raygen_frame(_lens, _cam) with the AABB collider (near 0, as AABBBoxCollider evaluates)
      2. snerf_spaced_bins, piecewise spacing, no jitter
      3. 2 x (proposal density + snerf_pdf_resample, u_mode 2); the density is snerf_tgrid_density_fwd (fused_density, one launch per level)
         or snerf_tgrid_encode_fwd + snerf_mlp_fwd, the same bits
      4. per slice: snerf_tgrid_encode_fwd (field table) -> decode net -> snerf_nerfacto_head_input_fwd -> head net
      5. snerf_weights_fwd, snerf_render_fwd (eval mode, expected depth), the per-ray depth clamp

    and gives the bits of the same rays pushed through NerfplayerTrainer.forward(training=False) with that background
    (tests/test_gpu_nerfplayer_render.py).  The appearance input is use_average_appearance_embedding's mean row, formed once per frame, or none.

    depth: the expected depth clamped PER RAY to that ray's own first and last sample midpoint.  This deviates from the reference on purpose:
    DepthRenderer("expected") clamps to the minimum and maximum midpoint over all rays that share a chunk, which makes a pixel depend on the
    chunk size; the two agree wherever the reference's clamp is inactive.
    background_color: "black" (default), "white", "last_sample", or "random" -- the reference's eval behaviour (noise wherever accumulation is
    below 1, renderers.py:102-104; wrong for a video), which needs a torch.Generator on the trainer's device.
    fused_density: snerf_tgrid_density_fwd for the proposal levels whose shape it supports, the two-launch pair for the others.  ON by default:
    measured on a 960 x 540 frame of the preset it takes 50.8 ms against the pair's 52.4 ms, forty times the run-to-run spread."""

    MODEL = "NeRFPlayer-nerfacto"
    SPACING = 1  # UniformLinDispPiecewise, as NerfplayerStep
    _FIELD_SLICE = 4096  # rays per launch group of the per-sample intermediates
    BACKGROUNDS = ("black", "white", "last_sample", "random")

    def __init__(self, trainer, rays_per_chunk: int = 32768, background_color: str = "black", fused_density: bool = True,
                 generator: Optional[torch.Generator] = None):
        from .nerfplayer_trainer import NerfplayerTrainer

        if not isinstance(trainer, NerfplayerTrainer):
            raise TypeError(f"NerfplayerRenderer renders a NerfplayerTrainer (the nerfplayer-nerfacto preset); {type(trainer).__name__} "
                            "(NerfplayerFullTrainer: the full NeRFPlayer model) is not built")
        if rays_per_chunk < 1:
            raise ValueError(f"rays_per_chunk={rays_per_chunk}")
        if background_color not in self.BACKGROUNDS:
            raise ValueError(f"background_color={background_color!r}: one of {self.BACKGROUNDS}")
        if background_color == "random" and generator is None:
            raise ValueError("background_color='random' (the reference's eval behaviour) needs a torch.Generator: pass generator=")
        self.trainer, self.R, self.dev = trainer, int(rays_per_chunk), trainer.dev
        self.cfg, self.S, self.aabb, self.lib = trainer.cfg, trainer.S, trainer.aabb, trainer.lib
        if self.R * max(self.S) >= 1 << 31:
            raise ValueError(f"rays_per_chunk={rays_per_chunk}: a level's samples per chunk must stay below 2^31")
        self.background_color, self.generator = background_color, generator
        # per level: the fused kernel where it is asked for and built for the level's table and net
        self.fused_density = [bool(fused_density and self.lib.snerf_tgrid_density_fwd_supported(C.byref(enc.desc), C.byref(net.desc)))
                              for enc, net in zip(trainer.prop_enc, trainer.prop_mlp)]
        R, (S0, S1, S2) = self.R, self.S
        ns = min(R, self._FIELD_SLICE)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        self.buf = {"sb": [f(R, s + 1) for s in self.S], "eb": [f(R, s + 1) for s in self.S], "dens": [f(R, s) for s in self.S], "w": [f(R, s) for s in self.S],
                    "rgb": f(R * S2, 3), "feat": f(ns * S2, trainer.enc.output_dim), "h": f(ns * S2, 16),
                    "hx": torch.zeros(ns * S2, 64, dtype=torch.float32, device=self.dev)}  # [SH 16 | geo 15 | appearance 32 | pad]: the pad stays zero
        pair = [lvl for lvl in range(2) if not self.fused_density[lvl]]
        if pair:
            self.buf["pfeat"] = f(ns * max(self.S[lvl] * trainer.prop_enc[lvl].output_dim for lvl in pair))
            self.buf["pout"] = f(ns * max(self.S[lvl] for lvl in pair), 1)
        self._bg_const = {"black": torch.zeros(3, dtype=torch.float32, device=self.dev), "white": torch.ones(3, dtype=torch.float32, device=self.dev)}.get(background_color)
        self._app = None
        self._init_frames(R)

    def _near_plane(self) -> float:
        return 0.0  # AABBBoxCollider(scene_box): near_plane 0 (nerfplayer_nerfacto.py:176), and eval mode applies none anyway

    def default_anneal(self) -> float:
        """The proposal-weight annealing exponent of the last completed training step (tools/train_psnr_nerfplayer.py evaluates held-out views with it)."""
        cfg = self.cfg
        if not cfg.use_proposal_weight_anneal:
            return 1.0
        return anneal_value(max(self.trainer.step - 1, 0), cfg.proposal_weights_anneal_max_num_iters, cfg.proposal_weights_anneal_slope)

    def _begin_frame(self, H: int, W: int):
        tr = self.trainer
        tr.wait_params()  # the field table's asynchronous sweep / tile pass of the last step: a stream wait, no host block
        # the appearance input of eval mode (nerfplayer_nerfacto_field.py:362-372): the mean row, once per frame -- or none
        self._app = tr.appearance.weight.mean(0, keepdim=True).contiguous() if self.cfg.use_average_appearance_embedding else None

    def _density(self, lvl: int, o, d, t, n: int):
        """Proposal level lvl: density of the chunk's n * S[lvl] samples into buf["dens"][lvl]."""
        tr, b, S = self.trainer, self.buf, self.S[lvl]
        enc, net = tr.prop_enc[lvl], tr.prop_mlp[lvl]
        if self.fused_density[lvl]:
            co = ops.coords_from_rays(o, d, t, b["eb"][lvl], self.aabb, False)
            with self._span("tgrid_density_fwd"):
                self._call("tgrid_density_fwd", C.byref(enc.desc), self._p(enc.embeddings), C.byref(co), self._p(t), S, n * S, C.byref(net.desc),
                           self._p(net.params), self._p(b["dens"][lvl]), self._st)
            return
        for r0 in range(0, n, self._FIELD_SLICE):
            r1 = min(r0 + self._FIELD_SLICE, n)
            N = (r1 - r0) * S
            co = ops.coords_from_rays(o[r0:r1], d[r0:r1], t[r0:r1], b["eb"][lvl][r0:r1], self.aabb, False)
            with self._span("tgrid_fwd.prop"):
                self._call("tgrid_encode_fwd", C.byref(enc.desc), self._p(enc.embeddings), C.byref(co), None, self._p(t[r0:r1]), S, N, self._p(b["pfeat"]),
                           self._st)
            self._mlp_fwd(net, b["pfeat"], enc.output_dim, N, b["pout"], 1, 0, b["dens"][lvl][r0:r1])

    # ---- one chunk ----
    def _chunk(self, ra, p0: int, p1: int, anneal: float, out: Dict[str, torch.Tensor]):
        tr, b, rays = self.trainer, self.buf, self._rays
        n = p1 - p0
        self._raygen(ra, p0, p1)
        self.rays, self._fwd_rays = rays, n
        self._spaced_bins(None)
        o, d, t = rays["origins"], rays["directions"], rays["times"]
        for lvl in range(2):
            self._density(lvl, o, d, t, n)
            self._resample(lvl, None, anneal)
        S2, enc, app = self.S[2], tr.enc, self._app
        for r0 in range(0, n, self._FIELD_SLICE):
            r1 = min(r0 + self._FIELD_SLICE, n)
            N = (r1 - r0) * S2
            co = ops.coords_from_rays(o[r0:r1], d[r0:r1], t[r0:r1], b["eb"][2][r0:r1], self.aabb, False)
            with self._span("tgrid_fwd.field"):
                self._call("tgrid_encode_fwd", C.byref(enc.desc), self._p(enc.embeddings), C.byref(co), None, self._p(t[r0:r1]), S2, N, self._p(b["feat"]),
                           self._st)
            self._mlp_fwd(tr.decode, b["feat"], enc.output_dim, N, b["h"], 16, 0, b["dens"][2][r0:r1])
            with self._span("nerfacto_head_input_fwd"):
                self._call("nerfacto_head_input_fwd", self._p(d[r0:r1]), self._p(b["h"]), self._p(app) if app is not None else None, None, S2, r1 - r0,
                           self._p(b["hx"]), self._st)
            self._mlp_fwd(tr.head, b["hx"], 64, N, b["rgb"][r0 * S2:r1 * S2], 3)
        rgb, acc, depth = out["rgb"][p0:p1], out["accumulation"][p0:p1], out["depth"][p0:p1]
        with self._span("weights_render_fwd"):
            self._call("weights_fwd", self._p(b["dens"][2]), self._p(b["eb"][2]), n, S2, self._p(b["w"][2]), self._st)
            b["rgb_out"], b["acc"], b["depth"] = rgb, acc, depth
            if self.background_color == "last_sample":
                self._render_fwd(False, 1, None, "depth_expected")
            elif self.background_color == "random":
                self._render_fwd(False, 0, torch.rand(n, 3, dtype=torch.float32, device=self.dev, generator=self.generator), "depth_expected")
            else:
                self._render_fwd(False, 2, self._bg_const, "depth_expected")
        # the expected depth, clamped per ray to the ray's own first and last sample midpoint (see the class docstring)
        eb = b["eb"][2][:n]
        dv = depth.view(-1)
        torch.clamp(dv, min=(eb[:, 0] + eb[:, 1]) / 2, max=(eb[:, -2] + eb[:, -1]) / 2, out=dv)

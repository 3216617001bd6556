"""What the three fused trainers (KPlanesTrainer, NerfplayerTrainer, NerfplayerFullTrainer) have in common: the flat parameter / gradient / Adam
buffer with its segment table, the schedules of the reference's callbacks, kernel timing, the stream scope, and one copy of each libsnerf launch
whose argument list is the same in all of them (MLP forward / backward, PDF resampling, spaced bins, compositing, the ray losses, the interlevel
loss).  Model-specific launch sequences stay in the trainers' own files; nerfplayer_step.py holds what only the two NeRFPlayer trainers share."""
import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib


def anneal_value(step: int, max_iters: int, slope: float) -> float:
    """set_anneal callback (NS/models/kplanes.py:326-331)."""
    frac = min(max(step / max_iters, 0.0), 1.0)
    return (slope * frac) / ((slope - 1) * frac + 1)


def update_schedule(step: int, warmup: int, every: int) -> float:
    """NS/models/kplanes.py:254-259 (= np.clip(np.interp(step, [0, warmup], [0, every]), 1, every) of NS/models/nerfacto.py:249-263)."""
    return min(max(every * min(max(step / warmup, 0.0), 1.0), 1.0), float(every))


def cosine_lr_factor(step: int, warm_up_end: int, max_steps: int, alpha: float) -> float:
    """CosineDecayScheduler (NS/engine/schedulers.py:126-141)."""
    if step < warm_up_end:
        return step / warm_up_end
    progress = (step - warm_up_end) / (max_steps - warm_up_end)
    return (math.cos(math.pi * progress) + 1.0) * 0.5 * (1 - alpha) + alpha


def _align4(n: int) -> int:
    return (n + 3) // 4 * 4


class FlatParams:
    """One flat fp32 buffer for every parameter, with gradient and Adam moments (and 64-bit fixed-point gradient cells in deterministic mode)
    in the same layout.  Every segment starts 16-B aligned; the module parameters alias their segments."""

    def __init__(self, order: Sequence[Tuple[str, object, str]], device, deterministic: bool = False, shaped: bool = True,
                 pad_to: Optional[Dict[str, int]] = None):
        """order: (name, module, attr) in buffer order.  shaped: views (and the modules' parameters) keep the parameter's shape; False: flat
        views (K-Planes, whose plane sets and nets hold 1-D parameters and whose live buffer changes every step: _repoint).
        pad_to: name -> the segment's length is rounded up to a multiple of that many floats instead of 4; the pad stays zero."""
        self.segments = []  # (name, module, attr, offset, numel)
        self.off = {}       # name -> (offset, numel)
        off = 0
        for name, mod, attr in order:
            n = getattr(mod, attr).numel()
            self.segments.append((name, mod, attr, off, n))
            self.off[name] = (off, n)
            q = (pad_to or {}).get(name, 4)
            off += (n + q - 1) // q * q
        self.n_params = off
        self._shaped = shaped
        self.params = torch.zeros(off, dtype=torch.float32, device=device)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        # deterministic mode: gradients accumulate as 64-bit fixed point (same layout as self.grads) and are converted once per step
        self.grads_fx = torch.zeros(off, dtype=torch.int64, device=device) if deterministic else None
        self.views, self.gviews, self.mviews, self.vviews, self.fxviews = {}, {}, {}, {}, {}
        for name, mod, attr, o, n in self.segments:
            p = getattr(mod, attr)
            self.params[o:o + n].copy_(p.detach().reshape(-1))
            shape = p.shape if shaped else (n,)
            self.gviews[name], self.mviews[name], self.vviews[name] = (t[o:o + n].view(shape) for t in (self.grads, self.exp_avg, self.exp_avg_sq))
            if deterministic:
                self.fxviews[name] = self.grads_fx[o:o + n].view(shape)
        self._repoint(self.params)

    def _repoint(self, flat: torch.Tensor):
        """Make `flat` the live parameter buffer: module parameters and self.views alias its segments."""
        self.params = flat
        for name, mod, attr, o, n in self.segments:
            p = getattr(mod, attr)
            p.data = flat[o:o + n].view(p.shape) if self._shaped else flat[o:o + n]
            self.views[name] = p.data

    def fx(self, gview: torch.Tensor) -> torch.Tensor:
        """The fixed-point cells behind a view of self.grads (deterministic mode)."""
        o = gview.storage_offset() - self.grads.storage_offset()
        return self.grads_fx[o:o + gview.numel()]


class _Span:
    """HIP events (on the launch stream) around a kernel group, when kernel timing asks for that group."""

    def __init__(self, tr, name):
        self.tr, self.name = tr, name

    def __enter__(self):
        t = self.tr._timing
        self.on = t is not None and (self.tr._timing_all or self.name in t)
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.on:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.tr._timing.setdefault(self.name, []).append((self.a, b))


class _On:
    """Run the enclosed launches on `stream` (torch's current stream AND the stream handed to libsnerf)."""

    def __init__(self, tr, stream):
        self.tr, self.stream = tr, stream

    def __enter__(self):
        self.prev = self.tr._st
        self.ctx = torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        self.tr._st = C.c_void_p(self.stream.cuda_stream)

    def __exit__(self, *exc):
        self.tr._st = self.prev
        self.ctx.__exit__(*exc)


class FusedStep(FlatParams):
    """Base of the fused trainers.  A subclass owns cfg, R (rays per batch), S (samples per ray of the three levels), the work buffers `buf`
    (sb / eb / dens / w / gw / gdens per level, rgb, grgb, rgb_out, acc, depth, sqerr, dist_rays, inter_rays), self.rays of the last forward,
    self._fwd_rays (its ray count) and self._st, the HIP stream handle of the launches (set at the top of forward(); switched by _On)."""

    SPACING = 0  # snerf_spaced_bins / snerf_pdf_resample `kind`: 0 = uniform, 1 = UniformLinDispPiecewise (ray_samplers.py:242-243)
    #              the default; a trainer sets it per instance (KPlanesTrainer: 1 with bounded = False, and its renderer follows)
    _timing, _timing_all = None, False
    _ck = staticmethod(_lib.check)  # every launch's return code goes through here (NerfplayerStep counts them)

    def _call(self, name: str, *args):
        """Launches snerf_<name>(*args); the code goes through _ck under the entry's own name."""
        self._ck(_lib.entries[name](*args), name)  # filled when the subclass loaded self.lib

    def _p(self, t, off_floats: int = 0):
        return C.c_void_p(t.data_ptr() + 4 * off_floats)

    # ---- HIP events around kernel groups ----
    def enable_kernel_timing(self, names=None):
        """Record HIP events (on the launch stream) around kernel groups; `names` = None times every group.
        Read back with `kernel_times_ms()` (synchronises)."""
        self._timing = {} if names is None else {n: [] for n in names}
        self._timing_all = names is None

    def disable_kernel_timing(self):
        self._timing = None

    def kernel_times_ms(self) -> Dict[str, Tuple[float, int]]:
        """name -> (mean milliseconds per launch, launches).  Synchronises."""
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in evs) / len(evs), len(evs)) for k, evs in (self._timing or {}).items() if evs}

    def _span(self, name):
        return _Span(self, name)

    # ---- launches ----
    def _mlp_fwd(self, net, X, ldx, N, Y, ldy, aux_col=-1, aux=None):
        with self._span(f"mlp_fwd.{net.desc.d_in}x{net.desc.hidden}x{net.desc.n_hidden}"):
            self._call("mlp_fwd", C.byref(net.desc), self._p(net.params), self._p(X), ldx, N, self._p(Y), ldy, aux_col,
                       self._p(aux) if aux is not None else None, self._st)

    def _mlp_bwd(self, net, gW, X, ldx, N, gY, ldgy, aux_col, gaux, gX, ldgx):
        """gW: the net's view of self.grads; in deterministic mode the weight gradient goes to the fixed-point cells behind it."""
        with self._span(f"mlp_bwd.{net.desc.d_in}x{net.desc.hidden}x{net.desc.n_hidden}"):
            fx = self.grads_fx is not None
            self._call("mlp_bwd_fx" if fx else "mlp_bwd",
                       C.byref(net.desc), self._p(net.params), self._p(X), ldx, N, self._p(gY) if gY is not None else None, ldgy, aux_col,
                       self._p(gaux) if gaux is not None else None, self._p(gX) if gX is not None else None, ldgx, self._p(self.fx(gW) if fx else gW),
                       self._st)

    def _spaced_bins(self, t_rand):
        """The first level's bins from nears / fars; t_rand = None: no jitter."""
        b, rays = self.buf, self.rays
        self._call("spaced_bins", self._p(rays["nears"]), self._p(rays["fars"]), self._p(t_rand) if t_rand is not None else None,
                   t_rand.shape[-1] if t_rand is not None else 0, self._fwd_rays, self.S[0], self.SPACING, self._p(b["sb"][0]),
                   self._p(b["eb"][0]), self._st)

    def _resample(self, lvl, rand, anneal):
        """density[lvl] -> weights[lvl] (stored) -> PDF sample level lvl+1 bins."""
        b, a = self.buf, _lib.ResampleArgs()
        a.density, a.ebins_prev, a.weights_out = b["dens"][lvl].data_ptr(), b["eb"][lvl].data_ptr(), b["w"][lvl].data_ptr()
        a.sbins_prev, a.nears, a.fars = b["sb"][lvl].data_ptr(), self.rays["nears"].data_ptr(), self.rays["fars"].data_ptr()
        if rand is None:
            a.u_mode = 2
        else:
            a.u_mode, a.u_or_rand, a.rand_cols = 1, rand.data_ptr(), rand.shape[-1]
        a.sbins_out, a.ebins_out = b["sb"][lvl + 1].data_ptr(), b["eb"][lvl + 1].data_ptr()
        a.R, a.S_prev, a.S, a.kind = self._fwd_rays, self.S[lvl], self.S[lvl + 1], self.SPACING
        a.anneal, a.histogram_padding, a.eps = anneal, 0.01, 1e-5
        with self._span("pdf_resample"):
            self._call("pdf_resample", C.byref(a), self._st)

    def _render_fwd(self, training: bool, bg_mode: int, bg: Optional[torch.Tensor], depth: str):
        """Compositing of the nerf level: rgb_out / acc / depth (`depth` = the RenderArgs field the model renders: "depth_median" or
        "depth_expected").  bg_mode 0: per-ray colours `bg`, 1: no background, 2: one colour `bg`."""
        b, a = self.buf, _lib.RenderArgs()
        a.weights, a.rgb, a.ebins = b["w"][2].data_ptr(), b["rgb"].data_ptr(), b["eb"][2].data_ptr()
        a.bg_mode = bg_mode
        if bg is not None:
            a.bg = bg.data_ptr()
        a.R, a.S, a.training = self._fwd_rays, self.S[2], int(training)
        a.rgb_out, a.acc_out = b["rgb_out"].data_ptr(), b["acc"].data_ptr()
        setattr(a, depth, b["depth"].data_ptr())
        self._call("render_fwd", C.byref(a), self._st)

    def _ray_train(self, target, bg, go_scale: float, dist_scale: float, median_depth: bool, dyn: Optional[torch.Tensor]):
        """The nerf level's weights -> compositing -> MSE / distortion backward -> weights backward as ONE launch (snerf_ray_train_fwd_bwd,
        bit-identical to the five kernels).  dyn: the parameter group's device-side state, whose non-finite flag the kernel raises."""
        b, R, ra = self.buf, self.R, _lib.RayTrainArgs()
        ra.density, ra.ebins, ra.sbins, ra.rgb = b["dens"][2].data_ptr(), b["eb"][2].data_ptr(), b["sb"][2].data_ptr(), b["rgb"].data_ptr()
        ra.bg, ra.target, ra.R, ra.S, ra.bg_mode = bg.data_ptr(), target.data_ptr(), R, self.S[2], 0
        ra.go_scale, ra.dist_scale = go_scale, dist_scale
        ra.weights, ra.rgb_out, ra.acc_out = b["w"][2].data_ptr(), b["rgb_out"].data_ptr(), b["acc"].data_ptr()
        ra.depth_median = b["depth"].data_ptr() if median_depth else None
        ra.sqerr_rays, ra.dist_rays, ra.g_rgb, ra.g_density = b["sqerr"].data_ptr(), b["dist_rays"].data_ptr(), b["grgb"].data_ptr(), b["gdens"][2].data_ptr()
        ra.g_weights, ra.nonfinite_flag = None, dyn.data_ptr() if dyn is not None else None
        with self._span("ray_train_fwd_bwd"):
            self._call("ray_train_fwd_bwd", C.byref(ra), self._st)

    def _mse_distortion_bwd(self, target, bg, go_scale: float, dist_scale: float):
        """The unfused form, first two of three: MSELoss folded into the render backward (g_rgb_out = go_scale * (rgb_out - target); value lazily
        from sqerr) writes gw[2] and grgb, the distortion loss adds to gw[2].  The caller adds its own terms to gw[2], then _weights_bwd(2)."""
        b, R, S2 = self.buf, self.R, self.S[2]
        self._call("render_mse_bwd", self._p(b["w"][2]), self._p(b["rgb"]), self._p(bg), 0, self._p(b["rgb_out"]), self._p(target), go_scale, R, S2,
                   self._p(b["gw"][2]), self._p(b["grgb"]), self._p(b["sqerr"]), self._st)
        self._call("distortion", self._p(b["w"][2]), self._p(b["sb"][2]), R, S2, dist_scale, self._p(b["dist_rays"]), self._p(b["gw"][2]), 1,
                   self._st)

    def _weights_bwd(self, lvl: int, dyn: Optional[torch.Tensor] = None):
        """gw[lvl] -> gdens[lvl]; dyn as in _ray_train."""
        b = self.buf
        self._call("weights_bwd", self._p(b["dens"][lvl]), self._p(b["eb"][lvl]), self._p(b["gw"][lvl]), self.R, self.S[lvl], self._p(b["gdens"][lvl]),
                   0, self._p(dyn) if dyn is not None else None, self._st)

    def _interlevel(self, lvl: int, mult: float, with_grad: bool):
        """Proposal supervision of level lvl (interlevel loss, losses.py:106-121): per-ray values, and gw[lvl] when with_grad."""
        b, R, S2 = self.buf, self.R, self.S[2]
        self._call("interlevel", self._p(b["sb"][2]), self._p(b["w"][2]), S2, self._p(b["sb"][lvl]), self._p(b["w"][lvl]), self.S[lvl], R,
                   mult / (R * S2), self._p(b["inter_rays"][lvl]), self._p(b["gw"][lvl]) if with_grad else None, self._st)

"""Fused training step of the reference's NeRFPlayer-nerfacto model (config 4) on libsnerf: one flat parameter / gradient / Adam
buffer, preallocated per-sample work buffers, no autograd graph and no host synchronisation inside a step (the only tensors created
per step are three per-RAY temporaries -- SH of the directions, the gathered appearance rows and their summed gradient -- from
torch's caching allocator).

What the reference does per step: Trainer.train_iteration -> NerfplayerNerfactoModel.get_outputs / get_metrics_dict / get_loss_dict
(NS/models/nerfplayer_nerfacto.py:206-318) -> autograd backward -> 2x Adam (NS/configs/method_configs.py:648-657: lr 1e-2,
eps 1e-12, cosine schedule with 512 warm-up steps) -> callbacks (proposal-weight annealing, proposal update schedule:
NS/models/nerfacto.py:235-264).  Same mathematics here, in this order:

  collider (AABB) -> piecewise sampler (single jitter) -> [temporal hash grid -> 10->16->1 MLP -> trunc_exp -> weights -> PDF] x2
  -> main grid (16 levels) -> 32->64->16 MLP (density = trunc_exp(col 0)) -> [SH4(dir) | 15 geo features | appearance(cam)] ->
  63->64->64->3 sigmoid MLP -> weights -> rgb / accumulation / expected depth -> MSE + interlevel + 1e-3 distortion + temporal TV x3
  -> gradients of all of it -> one Adam sweep (gradient cleared in the sweep) with the TV gradient added just before it.

The nerfstudio-shaped autograd model (nerfplayer_nerfacto.py, pinned against the reference by golden G12) is the checker of this file:
tests/test_gpu_nerfplayer_trainer.py compares losses and every gradient tensor on identical draws."""
import ctypes as C
from typing import Dict, Optional

import torch

from . import ops
from .nerfplayer_nerfacto import NerfplayerNerfactoModelConfig
from .nerfplayer_step import NerfplayerStep
from .streams import side_stream
from .temporal_grid import TemporalGridEncoder


class NerfplayerTrainer(NerfplayerStep):
    def __init__(self, cfg: NerfplayerNerfactoModelConfig, num_rays: int, num_images: int, aabb_scale: float = 1.0, device="cuda:0",
                 lr: float = 1e-2, adam_eps: float = 1e-12, warm_up_end: int = 512, max_steps: int = 30000, seed: int = 0, deterministic: bool = False,
                 async_field_sweep: bool = False, mlp_operands: str = "fp32", tiled_field_backward: bool = False, tiled_first_level: int = 0):
        """mlp_operands: "fp32" (exact: the parity path, what G12 pins) or "bf16" (bf16 MFMA operands, fp32 accumulation, for every net whose shape the
        16-bit fused kernels are built for -- the decode net and the colour head of the preset; the reference runs all of them in tcnn's fp16).
        async_field_sweep (round 5): inside train_step the optimiser sweep of the FIELD's table (most of the parameters) is launched on a side stream
        as soon as that table's gradient is complete (right behind the field's temporal-grid backward) and is joined only in front of the NEXT forward's
        field level: it runs beside the proposal networks' backward (atomic-bound) and the next step's ray generation and proposal levels, which read
        the two small tables only.  Same arithmetic, same bits in deterministic mode.  Readers of the field table outside forward() call wait_params() /
        synchronize() first; off by default for that reason (bench.py's config-4 leg and tools/bench_nerfplayer.py turn it on).
        tiled_field_backward (round 6): inside train_step the FIELD table's gradient scatter and its Adam sweep are one owner-computes pass
        (temporal_grid.TiledTableBackward, csrc/tgrid_tiles.hip): the batch's (sample, level, corner) touches are binned by tile of 256 table rows, one
        workgroup per tile sums its rows in LDS and steps them with Adam straight from there -- no float atomics (the run-length kernel ran AT the chip's
        atomic rate: 1.26 ms per step on camera rays) and no dense gradient for this table (24 instead of 32 B per parameter in the sweep).  Same
        mathematics; float sums in another association order.  The fused pass goes where the asynchronous sweep goes (side stream with
        async_field_sweep, else the caller's stream).  backward() called outside train_step, and deterministic mode, keep the atomic scatter into
        self.grads.  tiled_first_level: levels below it stay with the atomic kernel (0: every level tiled).
        deterministic: every gradient scatter (temporal-grid tables, MLP weight gradients, appearance embedding) accumulates 2^50-scaled 64-bit
        integers instead of float atomics (csrc/common.hpp: integer addition is associative), converted once per step: two runs from the same seed give
        the same bits.  Costs 8 B per parameter and 64-bit atomics; off by default."""
        if not cfg.disable_scene_contraction or cfg.use_same_proposal_network or cfg.num_proposal_iterations != 2:
            raise NotImplementedError("NerfplayerTrainer covers the nerfplayer-nerfacto preset (AABB collider, two proposal networks)")
        self._init_common(cfg, num_rays, aabb_scale, device, lr, adam_eps, warm_up_end, max_steps, seed, mlp_operands)
        # ---- modules exactly as the fields build them (nerfplayer_nerfacto_field.py:83-104, 238-311) ----
        self.enc = TemporalGridEncoder(input_dim=3, temporal_dim=cfg.temporal_dim, num_levels=cfg.num_levels, level_dim=cfg.features_per_level,
                                       log2_hashmap_size=cfg.log2_hashmap_size, desired_resolution=1024 * 2.0 * aabb_scale)
        self.decode = self._net(cfg.num_levels * cfg.features_per_level, 16, 64, 1, "None")
        self.head = self._net(16 + 15 + 32, 3, 64, 2, "Sigmoid")
        self.appearance = torch.nn.Embedding(num_images, 32)
        # ---- one flat buffer; the tables in the order of the reference's TV row draws: field, proposal 0, proposal 1 ----
        self._init_flat((("field.table", self.enc, "embeddings"), ("field.decode", self.decode, "params"), ("field.head", self.head, "params"),
                         ("field.appearance", self.appearance, "weight")), ("field.table", "prop0.table", "prop1.table"), deterministic)
        # ---- work buffers ----
        R, S2 = num_rays, self.S[2]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)
        self.buf = {
            **self._level_buffers(f, z),
            "feat": f(R * S2, self.enc.output_dim), "gfeat": f(R * S2, self.enc.output_dim),
            "h": f(R * S2, 16), "gh": z(R * S2, 16),
            "hx": z(R * S2, 64), "ghx": f(R * S2, 64),           # head input [SH 16 | geo 15 | appearance 32 | pad], and its gradient
            "rgb": f(R * S2, 3), "grgb": f(R * S2, 3),
        }
        self.async_field_sweep = bool(async_field_sweep)
        self.tiled_field_backward = bool(tiled_field_backward) and not deterministic
        self._tiled, self._bin_done, self.early_bin = None, None, True
        if self.tiled_field_backward:
            from .temporal_grid import TiledTableBackward

            self._tiled = TiledTableBackward(self.enc, R * S2, first_tiled_level=tiled_first_level)
        self._tv0_done, self._tv12_done = None, None
        self.fused_ray_loss, self._ray_deferred = True, False  # train_step: the nerf level's per-ray work as one launch (snerf_ray_train_fwd_bwd)

    def _field_tv_early(self):
        """async_field_sweep: the field table's TV pass reads parameters only, so it goes to the side stream at the START of the backward instead of between the
        table's gradient scatter and its sweep (~0.1 ms off the chain scatter -> sweep -> next forward)."""
        self._tv0_done = self._tv_early(self._sweep_stream(), (0,))
        # (r06) the two proposal tables' TV passes read parameters only as well: on the "sort" stream now, beside the field's backward, instead of behind the
        # proposal backward on the caller's stream -- where they shared the memory system with the tile pass / sweep of the main table (0.5 ms of column reads
        # over the tables inside the window of the step's critical kernel).  Same order of the reference's row draws: field, proposal 0, proposal 1.
        self._tv12_done = self._tv_early(side_stream(self.dev, "sort"), (1, 2))

    def _field_table_fused_adam(self, on_side: bool):
        """tiled_field_backward: the field table's scatter + temporal TV + Adam as one owner-computes pass over the tiles filed by `bin`; on the side stream
        (async_field_sweep) it reads only the tiler's own buffers and gfeat, which the next step rewrites after wait_params() at the earliest."""
        lr = self._lr()
        o, n = self.off["field.table"]
        sl = slice(o, o + n)
        tv = self._tv_cols[0] if self.cfg.temporal_tv_weight > 0 else None
        gt = self.gviews["field.table"] if self._tiled.plan.first_tiled_level > 0 else None

        def run(st):
            with self._span("tgrid_tiles_adam.field"):
                self._tiled.scatter_adam(self.buf["gfeat"], gt, self.params[sl], self.exp_avg[sl], self.exp_avg_sq[sl], lr, self.step + 1, self.adam_eps, tv_cols=tv,
                                         srow=self._srow[0] if tv is not None else None, stream=st)

        if on_side:
            side = self._sweep_stream()
            side.wait_stream(torch.cuda.current_stream())  # (the table's TV pass has been on this stream since the start of the backward)
            with torch.cuda.stream(side):
                run(C.c_void_p(side.cuda_stream))
                self._sweeps_done = side.record_event()
        else:
            run(self._st)
        self._swept = (0,)

    # ---- forward ----
    def forward(self, rays: Dict[str, torch.Tensor], cams: Optional[torch.Tensor], rng: Dict[str, torch.Tensor], anneal: float, training: bool = True):
        """rays: origins [R,3], directions [R,3] (unit), times [R,1]; cams int64 [R]; rng: t_rand [R,1], u [2 x [R,1]], bg [R,3].
        training=False (exactly R rays): no jitter, deterministic PDF samples, average / zero appearance embedding
        (nerfplayer_nerfacto_field.py:362-372), eval-mode compositing; rng needs only bg (the "random" background is drawn in eval too,
        renderers.py:102-104)."""
        cfg, b, R = self.cfg, self.buf, self.R
        self._st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        o, d, t = rays["origins"], rays["directions"], rays["times"].reshape(-1)
        rays = dict(rays)
        rays["nears"], rays["fars"] = ops.aabb_collide(o, d, self.aabb, 0.0, training)  # AABBBoxCollider(scene_box): near_plane 0
        if cams is not None and (cams.dtype != torch.int64 or not cams.is_contiguous()):
            cams = cams.to(torch.int64).contiguous()
        self.rays, self.cams = rays, cams
        self._proposal_levels(o, d, t, rng, anneal, training)
        co = ops.coords_from_rays(o, d, t, b["eb"][2], self.aabb, False)
        self._coords.append(co)
        S, N = self.S[2], R * self.S[2]
        self.wait_params()  # the field table's sweep of the last step (async_field_sweep) must be complete before the table is read
        if self._tiled is not None and self._in_train_step and training and self.early_bin:
            # the binning pass of the tiled backward needs the sample positions only: on a side stream NOW, beside the field forward and the MLP
            # backward, instead of between the decode net's backward and the tile pass on the critical chain (~0.19 ms).  Behind wait_params(): the
            # previous step's tile pass has read the tiler's buffers by then.
            main = torch.cuda.current_stream()
            sb = side_stream(self.dev, "sort")
            sb.wait_stream(main)
            with torch.cuda.stream(sb), self._span("tgrid_bin.field"):
                self._tiled.bin(co, t, S, None, C.c_void_p(sb.cuda_stream))
                self._bin_done = sb.record_event()
        self._tgrid_fwd(self.enc, self.enc.embeddings, co, t, S, N, b["feat"])
        self._mlp_fwd(self.decode, b["feat"], self.enc.output_dim, N, b["h"], 16, 0, b["dens"][2])
        # colour head input [SH 16 | geo 15 | appearance 32 | 0] in one launch (csrc/nerfplayer.hip; ~35 ATen kernels before round 5)
        if training:
            app, cm = self.appearance.weight, cams
        elif cfg.use_average_appearance_embedding:
            app, cm = self.appearance.weight.mean(0, keepdim=True).contiguous(), None
        else:
            app, cm = None, None
        dd = d if d.is_contiguous() else d.contiguous()
        self._call("nerfacto_head_input_fwd", self._p(dd), self._p(b["h"]), self._p(app) if app is not None else None,
                   self._p(cm) if cm is not None else None, S, R, self._p(b["hx"]), self._st)
        self._mlp_fwd(self.head, b["hx"], 64, N, b["rgb"], 3)
        self._ray_deferred = bool(training and self._in_train_step and self.fused_ray_loss)
        if self._ray_deferred:
            # train_step: weights, compositing, MSE backward, distortion and the weights' backward are ONE launch at the start of backward()
            # (snerf_ray_train_fwd_bwd, bit-identical to the five kernels); the expected depth (an output no loss of this model reads) is not rendered
            return b["rgb_out"]
        self._call("weights_fwd", self._p(b["dens"][2]), self._p(b["eb"][2]), R, S, self._p(b["w"][2]), self._st)
        self._render_fwd(training, 0, rng["bg"], "depth_expected")
        return b["rgb_out"]

    # ---- backward ----
    def backward(self, target: torch.Tensor, rng: Dict[str, torch.Tensor], proposal_grads: bool):
        cfg, b, R = self.cfg, self.buf, self.R
        S2, N2 = self.S[2], R * self.S[2]
        t = self.rays["times"].reshape(-1)
        target = target if target.is_contiguous() else target.contiguous()
        # a backward that raised after its asynchronous sweep was issued never reached optimizer_step(): start from clean flags, or this step's TV pass and
        # sweep of the field table would be skipped
        self._swept, self._tv0_done = (), None
        early = bool(self.async_field_sweep and self._in_train_step)
        if cfg.temporal_tv_weight > 0:
            b["tv"].zero_()
            if early:
                self._field_tv_early()
        if self._ray_deferred:
            self._ray_train(target, rng["bg"], 2.0 / (3 * R), cfg.distortion_loss_mult / R, False, None)
            self._ray_deferred = False
        else:
            self._mse_distortion_bwd(target, rng["bg"], 2.0 / (3 * R), cfg.distortion_loss_mult / R)
            self._weights_bwd(2)
        # colour head: gX = [dSH (unused) | d geo | d appearance | pad]
        self._mlp_bwd(self.head, self.gviews["field.head"], b["hx"], 64, N2, b["grgb"], 3, -1, None, b["ghx"], 64)
        # gh[:, 1:16] = ghx[:, 16:31] (column 0, the density, enters through gaux below); appearance gradient = per-ray sums of ghx[:, 31:63] added to the
        # cameras' rows -- fixed-point cells in deterministic mode
        fx = self.grads_fx is not None
        self._call("nerfacto_head_input_bwd", self._p(b["ghx"]), self._p(self.cams), S2, R, self._p(b["gh"]),
                   None if fx else self._p(self.gviews["field.appearance"]),
                   self._p(self.fxviews["field.appearance"]) if fx else None, self._st)
        self._mlp_bwd(self.decode, self.gviews["field.decode"], b["feat"], self.enc.output_dim, N2, b["gh"], 16, 0, b["gdens"][2], b["gfeat"],
                      self.enc.output_dim)
        if self._tiled is not None and self._in_train_step:
            # owner-computes form: bin on this stream (it reads the ray buffers), then scatter + Adam of the table as ONE pass where the sweep would go
            if self._bin_done is not None:  # binned beside the forward (early_bin): the tile pass's stream waits for it below
                torch.cuda.current_stream().wait_event(self._bin_done)
                self._bin_done = None
            else:
                with self._span("tgrid_bin.field"):
                    self._tiled.bin(self._coords[2], t, S2, b["gfeat"], self._st)
            self._tiled.coarse_levels(self._coords[2], t, S2, b["gfeat"], self.gviews["field.table"], self._st)
            if cfg.temporal_tv_weight > 0 and not early:
                self._tv_sign(0)  # the fused pass adds the TV step itself: its per-row signs must exist first (row draw order unchanged: field first)
            self._field_table_fused_adam(early)
        else:
            self._tgrid_bwd(self.enc, self._coords[2], t, S2, N2, b["gfeat"], self.gviews["field.table"])
            if early:
                self._early_table_sweeps((0,))
        self._proposal_backward(t, proposal_grads)
        # temporal TV of the three tables (temporal_grid.py:352-376; nerfplayer_nerfacto.py:311-316): one pass over two columns per table
        # gives the value and the per-row signed step; the gradient itself is added inside the Adam sweep (optimizer_step)
        if cfg.temporal_tv_weight > 0:
            if early:  # all three passes were issued at the start of the backward (_field_tv_early)
                # loss_dict reads the TV values and optimizer_step the proposal tables' per-row signs on the caller's stream
                torch.cuda.current_stream().wait_event(self._tv0_done)
                torch.cuda.current_stream().wait_event(self._tv12_done)
            else:
                self._tv_rest()

    def loss_dict(self) -> Dict[str, torch.Tensor]:
        return self._ray_losses()

    def train_step(self, rays: Dict[str, torch.Tensor], cams: torch.Tensor, target: torch.Tensor, rng: Optional[Dict[str, torch.Tensor]] = None):
        """One optimiser step; returns the rendered colours of the batch (a work buffer, valid until the next call).  With fused_ray_loss (default) the nerf
        level's weights, compositing, MSE backward, distortion term and weights' backward are one launch and the expected DEPTH of the batch is not rendered
        (no loss of this model reads it: buf["depth"] keeps the last forward(training=False)'s values); forward() + backward() called separately render it."""
        return self._train_step(target, rng, rays, cams)

    # ---- nerfstudio checkpoint files (trainer.py:331-380 of the reference; formats in soccernerfs_amd/checkpoint.py) ----
    _CK_NAMES = {"field.mlp_base.embeddings": "field.table", "field.mlp_base_decode.params": "field.decode", "field.mlp_head.params": "field.head",
                 "field.embedding_appearance.weight": "field.appearance",
                 "proposal_networks.0.encoding.embeddings": "prop0.table", "proposal_networks.0.linear.params": "prop0.mlp",
                 "proposal_networks.1.encoding.embeddings": "prop1.table", "proposal_networks.1.linear.params": "prop1.mlp"}

    def _named_module(self) -> torch.nn.Module:
        """The trainer's parameters under NerfplayerNerfactoModel's module names, registered in its order (nerfplayer_nerfacto.py,
        nerfplayer_nerfacto_field.py), so a checkpoint's keys -- the temporal grids' index buffers and `embedding.weight` included -- are that model's."""
        nn = torch.nn
        root = nn.Module()
        root.device_indicator_param = nn.Parameter(torch.empty(0))
        aabb = lambda: nn.Parameter(torch.tensor(self.aabb, dtype=torch.float32), requires_grad=False)
        root.field = nn.Module()
        root.field.aabb = aabb()
        root.field.embedding_appearance, root.field.mlp_base = self.appearance, self.enc
        root.field.mlp_base_decode, root.field.mlp_head = self.decode, self.head
        root.proposal_networks = nn.ModuleList()
        for enc, net in zip(self.prop_enc, self.prop_mlp):
            m = nn.Module()
            m.aabb = aabb()
            m.encoding, m.linear = enc, net
            root.proposal_networks.append(m)
        return root

    def save_checkpoint(self, checkpoint_dir: str, save_only_latest_checkpoint: bool = True) -> str:
        """Writes `step-%09d.ckpt` with the keys of NerfplayerNerfactoModel and the Adam moments of both parameter groups.  The saved step is the
        index of the last completed iteration, as the reference saves it; load_checkpoint resumes at step + 1."""
        from . import checkpoint as CK

        self.synchronize()  # the asynchronous sweep and the tiled pass may still be writing the field table and its moments
        moments = {ck: (self.mviews[seg], self.vviews[seg], self.step) for ck, seg in self._CK_NAMES.items()} if self.step > 0 else {}
        root = self._named_module()
        hyper = {"lr": self.lr, "betas": (0.9, 0.999), "eps": self.adam_eps, "weight_decay": 0, "amsgrad": False}
        opt = CK.export_optimizer_states(root, moments, {"fields": hyper, "proposal_networks": hyper})
        return CK.save_checkpoint(checkpoint_dir, max(self.step - 1, 0), root, opt, save_only_latest_checkpoint)

    def load_checkpoint(self, load_dir: str, load_step: Optional[int] = None, params_only: bool = False) -> int:
        """Parameters (+ Adam moments when the file holds them) from a nerfstudio checkpoint of this model; returns the step training resumes at.
        params_only: the parameters are loaded, the moments are cleared and the optimiser restarts at step 0; returns 0."""
        from . import checkpoint as CK

        self.synchronize()
        start, moments = CK.load_checkpoint(load_dir, self._named_module(), load_step)
        self.grads.zero_()
        if self.grads_fx is not None:
            self.grads_fx.zero_()
        self._steps_since_update, self._swept, self._sweeps_done = 0, (), None
        if params_only or not moments:  # Adam's bias correction counts optimiser updates: without moments the optimiser restarts
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.step = 0
        else:
            for ck, (m, v, _) in moments.items():
                seg = self._CK_NAMES[ck]
                self.mviews[seg].copy_(m.reshape(self.mviews[seg].shape).to(self.dev))
                self.vviews[seg].copy_(v.reshape(self.vviews[seg].shape).to(self.dev))
            self.step = start
        torch.cuda.synchronize(self.dev)
        return 0 if params_only else start

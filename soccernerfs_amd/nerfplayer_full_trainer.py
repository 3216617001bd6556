"""Fused training step of the reference's full NeRFPlayer model (`nerfplayer` preset, NS/configs/method_configs.py:562-614) on libsnerf:
one flat parameter / gradient / Adam buffer, preallocated work buffers, hand-derived backward, no autograd graph, no host
synchronisation inside a step.  ~80 kernel launches per step instead of the ~285 the nerfstudio-shaped autograd model issues
(soccernerfs_amd.nerfplayer.NerfplayerModel, which is pinned against the reference's own model by golden G13 and is the checker of this
file: tests/test_gpu_nerfplayer_full_trainer.py compares outputs, losses and every gradient tensor on identical draws).

Per step (NS/models/nerfplayer.py:218-343, NS/fields/nerfplayer_field.py:330-414, NS/models/nerfacto.py:235-264):

  collider (AABB) -> piecewise sampler (single jitter) -> [temporal hash grid -> 10->16->1 MLP -> trunc_exp -> weights -> PDF] x 2
  -> positions p -> deformation MLP 3->128x3->3 -> static hash grid at p AND at p + delta (one launch over 2N points)
  -> [grid features | t] -> 33->64->32 MLP (both halves) -> newness temporal grid, decomposition temporal grid -> 32->64->3 MLP
  -> softmax mixing (csrc/nerfplayer.hip) -> 32->64->64->16 MLP (density = trunc_exp(col 0)) -> 15->64x3->3 sigmoid MLP -> weights
  -> rgb / accumulation / expected depth / rendered probabilities
  -> MSE + interlevel + 1e-3 distortion + temporal TV / 4 of four tables + 0.1 (0.01 mean p_deform + mean p_new)
  -> gradients of all of it (incl. the hash grid's coordinate gradient into the deformation MLP)
  -> Adam (lr 1e-2 x cosine, eps 1e-6) with the TV gradient folded into the tables' sweeps, gradients cleared in the sweep."""
import ctypes as C
from typing import Dict, Optional

import torch

from . import ops
from .nerfplayer import NerfplayerModelConfig
from .nerfplayer_step import NerfplayerStep
from .streams import side_stream
from .tcnn_compat import Encoding
from .temporal_grid import TemporalGridEncoder

_ACT = {"none": 0, "relu": 1, "sigmoid": 2}


class NerfplayerFullTrainer(NerfplayerStep):
    TV_SCALE = 0.25  # temporal TV / 4 of four tables (nerfplayer.py:329-333)

    def __init__(self, cfg: NerfplayerModelConfig, num_rays: int, aabb_scale: float = 1.0, device="cuda:0", lr: float = 1e-2,
                 adam_eps: float = 1e-6, warm_up_end: int = 512, max_steps: int = 30000, seed: int = 0, deterministic: bool = False,
                 async_table_sweeps: bool = False, mlp_operands: str = "fp32", tiled_table_backward: bool = False, tiled_hash_backward: bool = False):
        """mlp_operands: "fp32" (exact: every net on the fp32 matrix instructions -- the parity path, what G13 / G13b pin) or "bf16" (round 5: bf16 MFMA
        operands with fp32 accumulation in every net -- the fused kernels for the shapes in their table, csrc/dense_lp.hip's single layers for the
        deformation net, the 33 -> 64 -> 32 MLP and the colour head; the reference itself runs all of them in tcnn's fp16).
        async_table_sweeps (round 5): inside train_step the optimiser sweeps of the newness and decomposition tables (most of the parameters) go to a side
        stream as soon as their gradients are complete (right behind their temporal-grid backward, early in the backward pass) and are joined in front of
        the next forward's first read of those tables: they run beside the rest of the backward (hash-grid scatter, deformation net, proposal networks)
        and the next step's proposal levels.  Same arithmetic (same bits in deterministic mode).  Readers of those tables outside forward() call
        wait_params() / synchronize() first; off by default for that reason.
        tiled_table_backward (round 6): inside train_step the newness and decomposition tables' gradient scatter, temporal-TV step and Adam sweep are ONE
        owner-computes pass each (temporal_grid.TiledTableBackward, csrc/tgrid_tiles.hip): no float atomics on the deformed positions (tgrid_runs_kernel
        <true, false> ran at the atomic rate, 2.0 ms per step) and no dense gradient for the two tables (24 instead of 32 B per parameter).  Same mathematics, float
        sums in another order.  Needs temporal_tv_weight > 0 (the preset); not with `deterministic`; backward() outside train_step keeps the atomic scatter.
        deterministic: every gradient accumulated across samples -- the temporal-grid and hash-grid table scatters, the hash grid's coordinate
        gradient (one add per level and sample), the weight gradients of all seven nets -- goes into 2^50-scaled 64-bit cells
        (snerf_*_bwd_fx; integer adds are associative) and is converted once per step: two runs from the same state and draws give the same bits.
        Costs 8 bytes per parameter (3.7 GB at the preset) and 64-bit atomics."""
        if not cfg.disable_scene_contraction or cfg.use_same_proposal_network or cfg.num_proposal_iterations != 2 or not cfg.disable_viewing_dependent:
            raise NotImplementedError("NerfplayerFullTrainer covers the `nerfplayer` preset (AABB collider, two proposal networks, no view dependence)")
        self._init_common(cfg, num_rays, aabb_scale, device, lr, adam_eps, warm_up_end, max_steps, seed, mlp_operands)  # (layer-chained nets pick their kernels in _dense_chain_*)
        a, net = aabb_scale, self._net
        F = cfg.num_levels * cfg.features_per_level
        self.F = F
        # ---- modules exactly as the fields build them (nerfplayer_field.py:223-316) ----
        self.deform = net(3, 3, 128, 3, "None")                                                       # :231
        self.hash = Encoding(3, {"otype": "HashGrid", "n_levels": cfg.num_levels, "n_features_per_level": cfg.features_per_level,
                                 "log2_hashmap_size": cfg.log2_hashmap_size, "base_resolution": 16, "per_level_scale": 1.4472692012786865})  # :243
        self.stat_mlp = net(F + 1, F, 64, 1, "None")                                                  # :254
        grid = dict(input_dim=3, temporal_dim=cfg.temporal_dim, num_levels=cfg.num_levels, level_dim=cfg.features_per_level, base_resolution=16,
                    log2_hashmap_size=cfg.log2_hashmap_size, desired_resolution=1024 * 2.0 * a)
        self.newness = TemporalGridEncoder(**grid)                                                    # :270
        self.decomp = TemporalGridEncoder(**grid)                                                     # :280
        self.decomp_mlp = net(F, 3, 64, 1, "None")                                                    # :290
        self.decode = net(F, 16, 64, 2, "None")                                                       # :301
        self.head = net(15, 3, 64, 3, "Sigmoid")                                                      # :309
        for m in (self.decomp_mlp, self.decode, self.prop_mlp[0], self.prop_mlp[1]):
            assert m.fused, "these nets run through the fused MLP kernels"
        # ---- one flat buffer: [proposal_networks | fields]; the tables in the temporal-TV order of nerfplayer.py:329-333 ----
        self._init_flat((("field.deform", self.deform, "params"), ("field.hash", self.hash, "params"), ("field.stat_mlp", self.stat_mlp, "params"),
                         ("field.newness", self.newness, "embeddings"), ("field.decomp", self.decomp, "embeddings"), ("field.decomp_mlp", self.decomp_mlp, "params"),
                         ("field.decode", self.decode, "params"), ("field.head", self.head, "params")),
                        ("field.newness", "field.decomp", "prop0.table", "prop1.table"), deterministic)
        # ---- work buffers ----
        R, S2 = num_rays, self.S[2]
        N = R * S2
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)
        self.buf = {
            **self._level_buffers(f, z),
            "mid": f(R, S2), "tN": f(N), "t2N": f(2 * N),
            "x2": f(2 * N, 3),                               # rows [0,N) = p, rows [N,2N) = p + deformation(p)
            "dh": [f(N, 128) for _ in range(3)], "delta": f(N, 3), "gdh": [f(N, 128), f(N, 128)],
            "enc2": f(2 * N, F), "genc2": f(2 * N, F), "gx2": z(2 * N, 3),
            "sx": z(2 * N, 36), "gsx": f(2 * N, 36),         # [grid features | t | pad], row stride 36 (16-B aligned rows)
            "sh": f(2 * N, 64), "gsh": f(2 * N, 64), "sv": f(2 * N, F), "gsv": f(2 * N, F),
            "vnew": f(N, F), "gvnew": f(N, F), "dfeat": f(N, F), "gdfeat": f(N, F),
            "logits": f(N, 3), "glogits": f(N, 3), "probs": f(N, 3), "gprobs": f(N, 3), "v": f(N, F), "gv": f(N, F),
            "h": f(N, 16), "gh": z(N, 16), "hh": [f(N, 64) for _ in range(3)], "ghh": [f(N, 64), f(N, 64)],
            "rgb": f(N, 3), "grgb": f(N, 3), "tmpN": f(N),
        }
        self._gx_fx = torch.zeros(N * 3, dtype=torch.int64, device=self.dev) if deterministic else None  # the deformed half's coordinate gradient
        amin = torch.tensor(self.aabb[0], dtype=torch.float32, device=self.dev)
        self._amin, self._arange = amin, torch.tensor(self.aabb[1], dtype=torch.float32, device=self.dev) - amin
        self._cvec = torch.tensor([0.0, 0.01, 1.0], dtype=torch.float32, device=self.dev)  # prob loss weights (nerfplayer.py:339-341)
        self.async_table_sweeps = bool(async_table_sweeps)
        self._tiled, self._tiled_hash, self._hash_swept, self._bin_done, self._hash_bin_done, self.early_bin = None, None, False, None, None, True
        if tiled_table_backward and not deterministic and cfg.temporal_tv_weight > 0:
            from .temporal_grid import TiledTableBackward

            self._tiled = [TiledTableBackward(self.newness, N, first_tiled_level=0), TiledTableBackward(self.decomp, N, first_tiled_level=0)]
            self._tiled[1].share_bins_of(self._tiled[0])  # both grids are evaluated at the same (undeformed) positions and times: one binning pass (early_bin)
            if tiled_hash_backward:
                # the static hash grid's table the same way (csrc/hashgrid_tiles.hip); opt-in: see DESIGN section 7 for where it pays
                from .tcnn_compat import TiledHashTableBackward

                self._tiled_hash = TiledHashTableBackward(self.hash, 2 * N)  # both halves of x2 (undeformed and deformed positions) in one pass
        self._tv01_done = None

    def _tiled_fused_adam(self, gouts, on_side: bool):
        """tiled_table_backward: scatter + temporal TV + Adam of the newness (k = 0) and decomposition (k = 1) tables, one owner-computes pass each, over the
        tiles filed by `bin`; on the side stream (async_table_sweeps) it reads only the tilers' own buffers and the two feature-gradient buffers, which the
        next step rewrites after wait_params() at the earliest."""
        lr = self._lr()

        def run(st):
            for k in (0, 1):
                o, n = self.off[self._enc_names[k]]
                sl = slice(o, o + n)
                self._tiled[k].scatter_adam(gouts[k], None, self.params[sl], self.exp_avg[sl], self.exp_avg_sq[sl], lr, self.step + 1, self.adam_eps,
                                            tv_cols=self._tv_cols[k], srow=self._srow[k], stream=st)
                self.launches += 1

        if on_side:
            side = self._sweep_stream()
            side.wait_stream(torch.cuda.current_stream())  # (the two tables' TV passes have been on this stream since the start of the backward)
            with torch.cuda.stream(side):
                run(C.c_void_p(side.cuda_stream))
                self._sweeps_done = side.record_event()
        else:
            run(self._st)
        self._swept = (0, 1)

    def _dense_chain_fwd(self, net, acts, X, ldx, x_off, N, outs):
        """Bias-free dense layers of `net` chained from snerf_dense_fwd; outs[l] = layer l's (activated) output, contiguous [N, dims[l+1]]."""
        woff, cur, ld, xo = 0, X, ldx, x_off
        for l, y in enumerate(outs):
            K, M = net.dims[l], net.dims[l + 1]
            if self._dense_operands:
                self._call("dense_fwd_lp", self._p(net.params, woff), K, M, _ACT[acts[l]], self._p(cur, xo), ld, N, self._p(y), y.stride(0),
                           self._dense_operands, self._st)
            else:
                self._call("dense_fwd", self._p(net.params, woff), K, M, _ACT[acts[l]], self._p(cur, xo), ld, N, self._p(y), y.stride(0),
                           self._st)
            woff += K * M
            cur, ld, xo = y, y.stride(0), 0

    def _dense_chain_bwd(self, net, gname, acts, X, ldx, x_off, N, outs, gY, ldgy, scratch, gX, ldgx, gx_off=0):
        """Backward of _dense_chain_fwd: gY = gradient of the last output; scratch = two [N, width] buffers for the hidden gradients;
        gX (may be None) receives the gradient of the chain's input."""
        woffs = [0]
        for l in range(len(outs)):
            woffs.append(woffs[-1] + net.dims[l] * net.dims[l + 1])
        g, ldg = gY, ldgy
        gW = self.gviews[gname]
        for l in reversed(range(len(outs))):
            K, M = net.dims[l], net.dims[l + 1]
            xin, ldi, xo = (X, ldx, x_off) if l == 0 else (outs[l - 1], outs[l - 1].stride(0), 0)
            if l == 0:
                gx, ldgx_, go = gX, ldgx, gx_off
            else:
                gx, ldgx_, go = scratch[l % 2], scratch[l % 2].stride(0), 0
            fx = self.grads_fx is not None
            if self._dense_operands:
                self._call(
                    "dense_bwd_lp",
                    self._p(net.params, woffs[l]), K, M, _ACT[acts[l]], self._p(xin, xo), ldi, N, self._p(outs[l]), outs[l].stride(0), self._p(g), ldg,
                    self._p(gx, go) if gx is not None else None, ldgx_, None if fx else self._p(gW, woffs[l]), self._p(self.fx(gW)[woffs[l]:]) if fx else None,
                    self._dense_operands, self._st)
                g, ldg = gx, ldgx_
                continue
            self._call(
                "dense_bwd_fx" if fx else "dense_bwd",
                self._p(net.params, woffs[l]), K, M, _ACT[acts[l]], self._p(xin, xo), ldi, N, self._p(outs[l]), outs[l].stride(0), self._p(g), ldg,
                self._p(gx, go) if gx is not None else None, ldgx_, self._p(self.fx(gW)[woffs[l]:]) if fx else self._p(gW, woffs[l]), self._st)
            g, ldg = gx, ldgx_

    # ---- forward ----
    def forward(self, rays: Dict[str, torch.Tensor], rng: Dict[str, torch.Tensor], anneal: float, training: bool = True):
        """rays: origins [R,3], directions [R,3] (unit), times [R,1]; rng: t_rand [R,1], u [2 x [R,1]], bg [R,3] (training) -- eval renders on
        the white background without jitter (nerfplayer.py:228-231).  Returns rgb [R,3] (a work buffer)."""
        cfg, b, R, F = self.cfg, self.buf, self.R, self.F
        self._st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        o, d = ops._f32c(rays["origins"], "origins"), ops._f32c(rays["directions"], "directions")
        t = ops._f32c(rays["times"], "times").reshape(-1)
        rays = dict(rays)
        rays["nears"], rays["fars"] = ops.aabb_collide(o, d, self.aabb, 0.0, training)  # AABBBoxCollider(scene_box): near_plane 0
        self.rays = rays
        self._proposal_levels(o, d, t, rng, anneal, training)
        # ---- main field on the N = R * S2 final samples ----
        S, N = self.S[2], R * self.S[2]
        eb = b["eb"][2]
        torch.add(eb[:, :-1], eb[:, 1:], out=b["mid"])
        b["mid"].div_(2)                                                    # (starts + ends) / 2 (rays.py:54)
        p = b["x2"][:N].view(R, S, 3)
        torch.mul(d[:, None, :], b["mid"][:, :, None], out=p)
        p.add_(o[:, None, :]).sub_(self._amin).div_(self._arange)           # SceneBox.get_normalized_positions (scene_box.py:55-65)
        b["tN"].view(R, S).copy_(t[:, None].expand(R, S))
        self._dense_chain_fwd(self.deform, ("relu", "relu", "relu", "none"), b["x2"], 3, 0, N, b["dh"] + [b["delta"]])
        torch.add(b["x2"][:N], b["delta"], out=b["x2"][N:])                 # deformed = x + deformation_field(x) (:346)
        self._call("hashgrid_encode_fwd", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"]), 2 * N, self._p(b["enc2"]),
                   self._st)
        b["sx"][:, :F].copy_(b["enc2"])
        b["sx"][:N, F].copy_(b["tN"])
        b["sx"][N:, F].copy_(b["tN"])                                       # cat([stationary_field(.), t]) (:349-351)
        self._dense_chain_fwd(self.stat_mlp, ("relu", "none"), b["sx"], 36, 0, 2 * N, [b["sh"], b["sv"]])
        self._pts = ops.coords_from_points(b["x2"])                         # explicit points for the temporal grids (pts [N,3], mode 0)
        self.wait_params()  # the newness / decomposition tables' sweeps of the last step (async_table_sweeps)
        if self._tiled is not None and self._in_train_step and training and self.early_bin:
            # the binning passes of the tiled backward need positions only: on a side stream NOW, beside the rest of the forward and the backward's MLP chain,
            # instead of on the critical chain in front of the tile passes.  ONE pass for the newness and decomposition grids (same positions, same times).
            main = torch.cuda.current_stream()
            sb = side_stream(self.dev, "sort")
            sb.wait_stream(main)
            with torch.cuda.stream(sb):
                stb = C.c_void_p(sb.cuda_stream)
                self._tiled[0].bin(self._pts, b["tN"], 1, None, stb)
                self._bin_done = sb.record_event()
                if self._tiled_hash is not None:
                    self._tiled_hash.bin(b["x2"], None, stb)
                    self._hash_bin_done = sb.record_event()
            self.launches += 5 + (5 if self._tiled_hash is not None else 0)
        self._tgrid_fwd(self.newness, self.newness.embeddings, self._pts, b["tN"], 1, N, b["vnew"])
        self._tgrid_fwd(self.decomp, self.decomp.embeddings, self._pts, b["tN"], 1, N, b["dfeat"])
        self._mlp_fwd(self.decomp_mlp, b["dfeat"], F, N, b["logits"], 3)
        self._call("nerfplayer_mix_fwd", self._p(b["logits"]), self._p(b["sv"]), self._p(b["sv"], N * F), self._p(b["vnew"]), N, F,
                   self._p(b["probs"]), self._p(b["v"]), self._st)
        self._mlp_fwd(self.decode, b["v"], F, N, b["h"], 16, 0, b["dens"][2])   # density = trunc_exp(column 0) (:374-377)
        self._dense_chain_fwd(self.head, ("relu", "relu", "relu", "sigmoid"), b["h"], 16, 1, N, b["hh"] + [b["rgb"]])  # geo features = columns 1..15
        self._call("weights_fwd", self._p(b["dens"][2]), self._p(eb), R, S, self._p(b["w"][2]), self._st)
        if training:
            self._render_fwd(True, 0, rng["bg"], "depth_expected")
        else:
            self._white = torch.ones(3, dtype=torch.float32, device=self.dev)
            self._render_fwd(False, 2, self._white, "depth_expected")
        return b["rgb_out"]

    def rendered_probs(self) -> torch.Tensor:
        """DecompositionRenderer (renderers.py:422-444): sum_s weights * probs -> [R,3]."""
        R, S = self.R, self.S[2]
        return (self.buf["w"][2][:, :, None] * self.buf["probs"].view(R, S, 3)).sum(1)

    # ---- backward ----
    def backward(self, target: torch.Tensor, rng: Dict[str, torch.Tensor], proposal_grads: bool):
        cfg, b, R, F = self.cfg, self.buf, self.R, self.F
        S2, N = self.S[2], R * self.S[2]
        t = self.rays["times"].reshape(-1)
        target = ops._f32c(target, "target")
        # a backward that raised after its asynchronous sweeps were issued never reached optimizer_step(): start from clean flags, or this step's TV pass
        # and sweep of those tables would be skipped
        self._swept, self._tv01_done, self._hash_swept = (), None, False
        early = bool(self.async_table_sweeps and self._in_train_step and cfg.temporal_tv_weight > 0)
        if cfg.temporal_tv_weight > 0:
            b["tv"].zero_()
        if early:
            self._tv01_done = self._tv_early(self._sweep_stream(), (0, 1))  # (the critical path of this model is the caller's stream)
        self._mse_distortion_bwd(target, rng["bg"], 2.0 / (3 * R), cfg.distortion_loss_mult / R)
        # probability regulariser: mult * (0.01 mean_r P_deform + mean_r P_new), P = sum_s w * probs (nerfplayer.py:336-341)
        k = cfg.prob_reg_loss_mult / R
        torch.mul(b["w"][2].view(N, 1), self._cvec, out=b["gprobs"])
        b["gprobs"].mul_(k)                                                  # d loss / d probs
        torch.mul(b["probs"][:, 1], 0.01, out=b["tmpN"])                     # probs . (0, 0.01, 1) without a BLAS call (a [N,3] x [3] gemv took 0.14 ms)
        b["tmpN"].add_(b["probs"][:, 2])
        b["gw"][2].view(-1).add_(b["tmpN"], alpha=k)                          # d loss / d weights
        self._weights_bwd(2)
        # colour head -> geometry features (columns 1..15 of gh; column 0 = density enters the decode net through gaux)
        self._dense_chain_bwd(self.head, "field.head", ("relu", "relu", "relu", "sigmoid"), b["h"], 16, 1, N, b["hh"] + [b["rgb"]], b["grgb"], 3, b["ghh"],
                              b["gh"], 16, 1)
        self._mlp_bwd(self.decode, self.gviews["field.decode"], b["v"], F, N, b["gh"], 16, 0, b["gdens"][2], b["gv"], F)
        self._call("nerfplayer_mix_bwd", self._p(b["probs"]), self._p(b["sv"]), self._p(b["sv"], N * F), self._p(b["vnew"]), self._p(b["gv"]),
                   self._p(b["gprobs"]), N, F, self._p(b["gsv"]), self._p(b["gsv"], N * F), self._p(b["gvnew"]),
                   self._p(b["glogits"]), self._st)
        self._mlp_bwd(self.decomp_mlp, self.gviews["field.decomp_mlp"], b["dfeat"], F, N, b["glogits"], 3, -1, None, b["gdfeat"], F)
        if self._tiled is not None and self._in_train_step:
            # owner-computes form: bin both tables' touches here (the pass reads the deformed positions), then scatter + TV + Adam per table as one pass
            gouts = (b["gvnew"], b["gdfeat"])
            if self._bin_done is not None:  # binned beside the forward (early_bin, one pass for both tables)
                torch.cuda.current_stream().wait_event(self._bin_done)
                self._bin_done = None
            else:
                # late binning without the zero-gradient filter as well: the two tables share ONE set of records (share_bins_of)
                self._tiled[0].bin(self._pts, b["tN"], 1, None, self._st)
                self.launches += 5
            if not early:
                for k in (0, 1):
                    self._tv_sign(k)  # the fused pass adds the TV step itself (row draw order unchanged: newness, decomposition first)
            self._tiled_fused_adam(gouts, early)
        else:
            self._tgrid_bwd(self.decomp, self._pts, b["tN"], 1, N, b["gdfeat"], self.gviews["field.decomp"])
            self._tgrid_bwd(self.newness, self._pts, b["tN"], 1, N, b["gvnew"], self.gviews["field.newness"])
            if early:
                self._early_table_sweeps((0, 1))
        self._dense_chain_bwd(self.stat_mlp, "field.stat_mlp", ("relu", "none"), b["sx"], 36, 0, 2 * N, [b["sh"], b["sv"]], b["gsv"], F, [b["gsh"], b["gsh"]],
                              b["gsx"], 36)
        b["genc2"].copy_(b["gsx"][:, :F])
        # static hash grid: table gradient from both halves, coordinate gradient only for the deformed half (x itself carries no gradient)
        if self._tiled_hash is not None and self._in_train_step:
            # owner-computes form (round 6): one binning pass over all 2N points, then scatter + Adam of the table as one pass; the coordinate gradient of
            # the deformed half is a gather (the atomic kernel without a table gradient)
            th = self._tiled_hash
            lc = th.plan.first_tiled_level
            gth = self.gviews["field.hash"]
            if self._hash_bin_done is not None:
                torch.cuda.current_stream().wait_event(self._hash_bin_done)
                self._hash_bin_done = None
            else:
                th.bin(b["x2"], b["genc2"], self._st)
            b["gx2"][N:].zero_()
            # the coarse levels (every point of the batch in a handful of tiles) through the atomic kernel: table gradient from both halves ...
            th.coarse_levels(b["x2"], b["genc2"], gth, self._st)
            # ... and the coordinate gradient of the deformed half: levels [0, lc) were handled just above for the table, so one gather-only launch per range
            self._call("hashgrid_encode_bwd", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"], 3 * N), N,
                       self._p(b["genc2"], N * F), None, self._p(b["gx2"], 3 * N), self._st)
            oh, nh = self.off["field.hash"]
            th.scatter_adam(b["x2"], b["genc2"], gth if lc > 0 else None, self.params[oh:oh + nh], self.exp_avg[oh:oh + nh], self.exp_avg_sq[oh:oh + nh], self._lr(),
                            self.step + 1, self.adam_eps, stream=self._st)
            self.launches += 6
            self._hash_swept = True
        elif self.grads_fx is not None:
            gt = self._p(self.fx(self.gviews["field.hash"]))
            self._call("hashgrid_encode_bwd_fx", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"]), N, self._p(b["genc2"]),
                       gt, None, self._st)
            self._call("hashgrid_encode_bwd_fx", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"], 3 * N), N,
                       self._p(b["genc2"], N * F), gt, self._p(self._gx_fx), self._st)
            ops.fx_to_float(self._gx_fx, b["gx2"][N:].view(-1))  # written, cells cleared
        else:
            self._call("hashgrid_encode_bwd", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"]), N, self._p(b["genc2"]),
                       self._p(self.gviews["field.hash"]), None, self._st)
            b["gx2"][N:].zero_()
            self._call("hashgrid_encode_bwd", C.byref(self.hash.desc), self._p(self.hash.params), self._p(b["x2"], 3 * N), N,
                       self._p(b["genc2"], N * F), self._p(self.gviews["field.hash"]), self._p(b["gx2"], 3 * N), self._st)
        self._dense_chain_bwd(self.deform, "field.deform", ("relu", "relu", "relu", "none"), b["x2"], 3, 0, N, b["dh"] + [b["delta"]], b["gx2"][N:], 3,
                              b["gdh"], None, 0)
        self._proposal_backward(t, proposal_grads)
        # temporal TV of the four tables, weight / 4 (nerfplayer.py:329-333): values + per-row signed steps; the gradient is added in the Adam sweep
        if cfg.temporal_tv_weight > 0:
            self._tv_rest()
            if early:
                torch.cuda.current_stream().wait_event(self._tv01_done)  # loss_dict reads those tables' TV values on the caller's stream

    def loss_dict(self) -> Dict[str, torch.Tensor]:
        d = self._ray_losses()
        pm = self.rendered_probs().mean(0)
        d["prob_loss"] = (0.01 * pm[1] + pm[2]) * self.cfg.prob_reg_loss_mult
        return d

    def optimizer_step(self):
        """NerfplayerStep.optimizer_step, around the hash table when its owner-computes pass (tiled_hash_backward) has stepped it already."""
        ho, hn = self.off["field.hash"]
        super().optimizer_step(stepped=(ho, ho + hn) if self._hash_swept else None)
        self._hash_swept = False

    def train_step(self, rays: Dict[str, torch.Tensor], target: torch.Tensor, rng: Optional[Dict[str, torch.Tensor]] = None):
        return self._train_step(target, rng, rays)

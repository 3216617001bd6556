"""What the two fused NeRFPlayer trainers (NerfplayerTrainer: the nerfacto variant, NerfplayerFullTrainer: the full model) share on top of
fused_step.FusedStep: the two proposal networks (temporal hash grid -> 10->16->1 MLP) and their levels of the forward and backward pass, the
temporal-TV bookkeeping of the tables (indexed by k: the order of the reference's row draws), the tables' Adam sweeps (with the TV gradient
added on the fly; optionally issued early on a side stream), the optimiser's walk over the flat buffer and train_step's schedule."""
import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, ops
from .fused_step import FusedStep, _On, _align4, anneal_value, cosine_lr_factor, update_schedule
from .streams import side_stream
from .tcnn_compat import Network
from .temporal_grid import TemporalGridEncoder


class NerfplayerStep(FusedStep):
    SPACING = 1     # UniformLinDispPiecewise (ray_samplers.py:242-243)
    TV_SCALE = 1.0  # factor on cfg.temporal_tv_weight (the full model averages over its four tables: nerfplayer.py:329-333)

    def _init_common(self, cfg, num_rays, aabb_scale, device, lr, adam_eps, warm_up_end, max_steps, seed, mlp_operands):
        self.cfg, self.R, self.dev = cfg, num_rays, torch.device(device)
        self.lr, self.adam_eps, self.warm_up_end, self.max_steps = lr, adam_eps, warm_up_end, max_steps
        a = aabb_scale
        self.aabb = [[-a, -a, -a], [a, a, a]]
        torch.manual_seed(seed)
        if mlp_operands not in ("fp32", "bf16"):
            raise ValueError(f"mlp_operands must be 'fp32' or 'bf16', got {mlp_operands!r}")
        self.mlp_operands = mlp_operands
        self._dense_operands = {"fp32": 0, "bf16": 1}[mlp_operands]
        S0, S1 = cfg.num_proposal_samples_per_ray
        self.S = (S0, S1, cfg.num_nerf_samples_per_ray)
        self._fwd_rays = num_rays  # every forward of these trainers takes exactly R rays
        self.lib = _lib.lib()
        self.step = 0
        self._steps_since_update = 0
        self.launches = 0  # libsnerf launches of the last step (diagnostics)
        # _swept: the tables (k) whose sweep of this step has been issued already (on the side stream, or by an owner-computes pass)
        self._side, self._sweeps_done, self._swept, self._in_train_step = None, None, (), False
        # ---- the proposal networks exactly as the fields build them (nerfplayer_nerfacto_field.py:83-104) ----
        self.prop_enc: List[TemporalGridEncoder] = []
        self.prop_mlp: List[Network] = []
        for args in cfg.proposal_net_args_list[:2]:
            L, H = args.get("num_levels", 8), args.get("hidden_dim", 64)
            growth = float(np.exp((np.log(args.get("max_res", 1024)) - np.log(16)) / (L - 1)))
            self.prop_enc.append(TemporalGridEncoder(input_dim=3, temporal_dim=args.get("temporal_dim", 64), num_levels=L, level_dim=2,
                                                     per_level_scale=growth, base_resolution=16, log2_hashmap_size=args.get("log2_hashmap_size", 18)))
            self.prop_mlp.append(self._net(2 * L, 1, H, 1, "None"))

    def _net(self, din, dout, h, nh, act):
        """A tcnn-shaped net; 16-bit operands (mlp_operands = "bf16") where the fused 16-bit kernels are built for its shape."""
        d = _lib.MlpDesc()
        d.d_in, d.d_out, d.hidden, d.n_hidden, d.hidden_act, d.out_act, d.operands = din, dout, h, nh, 1, int(act == "Sigmoid"), self._dense_operands
        fused16 = self._dense_operands != 0 and bool(_lib.lib().snerf_mlp_supported(C.byref(d)))
        return Network(din, dout, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h, "n_hidden_layers": nh},
                       operands=self.mlp_operands if fused16 else "fp32")

    def _init_flat(self, field_order, tables, deterministic: bool):
        """One flat buffer [proposal_networks | fields]; tables: names of the temporal tables in the order of the reference's TV row draws."""
        order = [(f"prop{i}.{k}", mod, attr) for i in range(2) for k, mod, attr in (("table", self.prop_enc[i], "embeddings"), ("mlp", self.prop_mlp[i], "params"))]
        super().__init__(order + list(field_order), self.dev, deterministic=deterministic)
        mods = {name: mod for name, mod, _, _, _ in self.segments}
        self._enc_names = list(tables)
        self._encs = [mods[name] for name in tables]
        self._srow = [torch.zeros(e.embeddings.shape[0], dtype=torch.float32, device=self.dev) for e in self._encs]  # per-row TV step of each table
        self.tv_rows: Optional[List[int]] = None  # parity hook: fixed table rows (one per table) instead of the random draw
        self._tv_cols = [(0, 1)] * len(tables)

    def _level_buffers(self, f, z):
        """The work buffers of the sampling levels, the compositing and the ray losses (f: uninitialised, z: zeroed fp32 tensor)."""
        R, (S0, S1, _) = self.R, self.S
        return {
            "sb": [f(R, s + 1) for s in self.S], "eb": [f(R, s + 1) for s in self.S],
            "dens": [f(R, s) for s in self.S], "w": [f(R, s) for s in self.S], "gw": [f(R, s) for s in self.S], "gdens": [f(R, s) for s in self.S],
            "pfeat": [f(R * S0, self.prop_enc[0].output_dim), f(R * S1, self.prop_enc[1].output_dim)],
            "pout": [f(R * S0, 1), f(R * S1, 1)],
            "gpfeat": [f(R * S0, self.prop_enc[0].output_dim), f(R * S1, self.prop_enc[1].output_dim)],
            "rgb_out": f(R, 3), "acc": f(R), "depth": f(R), "sqerr": z(R), "dist_rays": f(R), "inter_rays": [f(R), f(R)],
            "tv": z(len(self._encs), 64, 16),
        }

    def _ck(self, rc, what):
        self.launches += 1
        _lib.check(rc, what)

    def _lr(self) -> float:
        return self.lr * cosine_lr_factor(self.step, self.warm_up_end, self.max_steps, 0.0)

    def _sweep_stream(self):
        if self._side is None:
            self._side = side_stream(self.dev, "adam")  # the process-wide sweep stream (streams.py)
        return self._side

    def wait_params(self):
        """The current stream waits for the asynchronous table sweeps (no host block)."""
        # the event is KEPT until the next sweep replaces it: waiting for a completed event is free, and a later reader on ANOTHER stream (a checkpoint
        # save, a side-stream evaluation) that calls wait_params() is then ordered behind the sweep too
        if self._sweeps_done is not None:
            torch.cuda.current_stream().wait_event(self._sweeps_done)

    def synchronize(self):
        self.wait_params()
        torch.cuda.synchronize()

    # ---- temporal grids ----
    def _tgrid_fwd(self, enc, table, co, times, S, N, out):
        with self._span("tgrid_fwd.prop" if enc is self.prop_enc[0] or enc is self.prop_enc[1] else "tgrid_fwd.field"):
            self._call("tgrid_encode_fwd", C.byref(enc.desc), self._p(table), C.byref(co), None, self._p(times), S, N, self._p(out),
                       self._st)

    def _tgrid_bwd(self, enc, co, times, S, N, gout, gtable):
        with self._span("tgrid_bwd.prop" if enc is self.prop_enc[0] or enc is self.prop_enc[1] else "tgrid_bwd.field"):
            if self.grads_fx is not None:
                self._call("tgrid_encode_bwd_fx", C.byref(enc.desc), C.byref(co), None, self._p(times), S, N, self._p(gout),
                           self._p(self.fx(gtable)), self._st)
                return
            self._call("tgrid_encode_bwd", C.byref(enc.desc), C.byref(co), None, self._p(times), S, N, self._p(gout), self._p(gtable),
                       self._st)

    def _tv_sign(self, k: int):
        """Value + per-row signed step of table k's temporal TV; the row draw is the reference's randint."""
        enc = self._encs[k]
        row = self.tv_rows[k] if self.tv_rows is not None else int(torch.randint(0, len(enc._index_list_host), [1]).item())
        ca, cb = enc._index_list_host[row]
        self._tv_cols[k] = (ca, cb)
        rows_, gc = enc.embeddings.shape
        self._call("tgrid_tv_sign", self._p(enc.embeddings), rows_, gc, ca, cb, float(self.cfg.temporal_tv_weight) * self.TV_SCALE,
                   self._p(self.buf["tv"][k]), 64, self._p(self._srow[k]), self._st)

    def _tv_early(self, stream, ks):
        """The TV passes of tables `ks` read parameters only: on a side stream at the START of the backward, beside it, instead of on the caller's
        stream between the tables' gradient scatters and their sweeps.  Returns the event behind them."""
        stream.wait_stream(torch.cuda.current_stream())  # b["tv"] zeroed; the forward's reads of everything else are irrelevant to them
        with _On(self, stream):
            for k in ks:
                self._tv_sign(k)
        return stream.record_event()

    def _tv_rest(self):
        """The TV passes of the tables not swept yet (a swept table's pass came before its sweep): the same order of row draws either way."""
        for k in range(len(self._encs)):
            if k not in self._swept:
                self._tv_sign(k)

    def materialize_tv_gradient(self):
        """Adds the temporal-TV gradient into self.grads explicitly (what the Adam sweep otherwise does on the fly); for parity tests."""
        if self.cfg.temporal_tv_weight <= 0:
            return
        for k, name in enumerate(self._enc_names):
            ca, cb = self._tv_cols[k]
            self.gviews[name][:, ca] += self._srow[k]
            self.gviews[name][:, cb] -= self._srow[k]

    # ---- the tables' Adam sweeps ----
    def _sweep_table(self, k: int, lr: float, st):
        """Adam over temporal table k on the current stream (st = its handle), with the temporal-TV gradient of its two columns added on the fly."""
        o, n = self.off[self._enc_names[k]]
        sl = slice(o, o + n)
        if self.cfg.temporal_tv_weight <= 0:
            ops.adam_step(self.params[sl], self.grads[sl], self.exp_avg[sl], self.exp_avg_sq[sl], self.step + 1, lr, eps=self.adam_eps, zero_grad=True)
            return
        ca, cb = self._tv_cols[k]
        rows_, gc = self._encs[k].embeddings.shape
        with self._span("adam_tv." + self._enc_names[k]):
            self._call("adam_step_tv", self._p(self.params[sl]), self._p(self.grads[sl]), self._p(self.exp_avg[sl]), self._p(self.exp_avg_sq[sl]),
                       rows_, gc, ca, cb, self._p(self._srow[k]), lr, 0.9, 0.999, self.adam_eps, self.step + 1, 1.0, 1,
                       None, st)

    def _early_table_sweeps(self, ks):
        """The Adam sweeps of tables `ks` on the side stream, behind everything the caller's stream holds (their gradient scatters) and behind their
        TV passes (on that stream since the start of the backward: _tv_early)."""
        side = self._sweep_stream()
        side.wait_stream(torch.cuda.current_stream())
        lr = self._lr()
        with torch.cuda.stream(side):
            st = C.c_void_p(side.cuda_stream)
            for k in ks:
                if self.grads_fx is not None:
                    gv = self.gviews[self._enc_names[k]]
                    ops.fx_to_float(self.fx(gv), gv.view(-1), accumulate=True)
                self._sweep_table(k, lr, st)
            self._sweeps_done = side.record_event()
        self._swept = tuple(ks)

    def gradients_to_float(self):
        """Deterministic mode: fold the fixed-point cells into self.grads (cells cleared).  optimizer_step does this itself; callers that read
        self.gviews after backward() call it first."""
        if self.grads_fx is None:
            return
        lo = 0
        for o, n in sorted(self.off[self._enc_names[k]] for k in self._swept):
            if o > lo:  # the tables swept on the side stream have been converted there (and are being written by it)
                ops.fx_to_float(self.grads_fx[lo:o], self.grads[lo:o], accumulate=True)
            lo = o + n
        if lo < self.n_params:
            ops.fx_to_float(self.grads_fx[lo:], self.grads[lo:], accumulate=True)

    def optimizer_step(self, stepped=None):
        """Adam (lr x cosine schedule) over the flat buffer, gradient cleared in the sweep; the temporal tables go through snerf_adam_step_tv,
        which adds the temporal-TV gradient of their two columns on the fly.  Every float is swept exactly once: one plain sweep per run of
        segments between (and after) the tables, around `stepped` = (lo, hi), the floats an owner-computes pass has stepped already."""
        lr = self._lr()
        self.gradients_to_float()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def plain(lo, hi):
            parts = [(lo, hi)]
            if stepped is not None and lo < stepped[1] and hi > stepped[0]:
                parts = [(lo, stepped[0]), (_align4(stepped[1]), hi)]
            for a_, b_ in parts:
                if b_ > a_:
                    ops.adam_step(self.params[a_:b_], self.grads[a_:b_], self.exp_avg[a_:b_], self.exp_avg_sq[a_:b_], self.step + 1, lr, eps=self.adam_eps, zero_grad=True)
                    self.launches += 1

        done = 0  # first float not yet swept
        tables = range(len(self._encs)) if self.cfg.temporal_tv_weight > 0 else self._swept
        for k in sorted(tables, key=lambda i: self.off[self._enc_names[i]][0]):
            o, n = self.off[self._enc_names[k]]
            if o > done:  # the small segments in front of this table
                plain(done, o)
            if k not in self._swept:
                self._sweep_table(k, lr, st)
            done = o + n
        if done < self.n_params:
            plain(done, self.n_params)
        self._swept = ()
        self.step += 1

    # ---- proposal levels ----
    def _proposal_levels(self, o, d, t, rng, anneal: float, training: bool):
        """Piecewise sampler -> [temporal hash grid -> MLP -> trunc_exp -> weights -> PDF] x 2: leaves the nerf level's bins in buf["sb"/"eb"][2]."""
        b, R = self.buf, self.R
        self.launches = 0
        self._spaced_bins(rng["t_rand"] if training else None)
        self._coords = []
        for lvl in range(2):
            co = ops.coords_from_rays(o, d, t, b["eb"][lvl], self.aabb, False)
            self._coords.append(co)
            S, N = self.S[lvl], R * self.S[lvl]
            enc, net = self.prop_enc[lvl], self.prop_mlp[lvl]
            self._tgrid_fwd(enc, enc.embeddings, co, t, S, N, b["pfeat"][lvl])
            self._mlp_fwd(net, b["pfeat"][lvl], enc.output_dim, N, b["pout"][lvl], 1, 0, b["dens"][lvl])
            self._resample(lvl, rng["u"][lvl] if training else None, anneal)

    def _proposal_backward(self, t, proposal_grads: bool):
        """Proposal supervision (interlevel loss, losses.py:106-121); gradients only on steps that update the proposal networks."""
        b, R = self.buf, self.R
        for lvl in range(2):
            Sp, Np = self.S[lvl], R * self.S[lvl]
            self._interlevel(lvl, self.cfg.interlevel_loss_mult, proposal_grads)
            if proposal_grads:
                enc, net = self.prop_enc[lvl], self.prop_mlp[lvl]
                self._weights_bwd(lvl)
                self._mlp_bwd(net, self.gviews[f"prop{lvl}.mlp"], b["pfeat"][lvl], enc.output_dim, Np, None, 1, 0, b["gdens"][lvl], b["gpfeat"][lvl],
                              enc.output_dim)
                self._tgrid_bwd(enc, self._coords[lvl], t, Sp, Np, b["gpfeat"][lvl], self.gviews[f"prop{lvl}.table"])

    def _ray_losses(self) -> Dict[str, torch.Tensor]:
        b, cfg, R = self.buf, self.cfg, self.R
        d = {"rgb_loss": b["sqerr"].sum() / (3 * R),
             "interlevel_loss": (b["inter_rays"][0].sum() + b["inter_rays"][1].sum()) / (R * self.S[2]) * cfg.interlevel_loss_mult,
             "distortion_loss": b["dist_rays"].mean() * cfg.distortion_loss_mult}
        if cfg.temporal_tv_weight > 0:
            d["temporal_tv_loss"] = sum(b["tv"][k, :, 0].sum() / e.embeddings.shape[0] for k, e in enumerate(self._encs)) * cfg.temporal_tv_weight * self.TV_SCALE
        return d

    def random_draws(self) -> Dict[str, torch.Tensor]:
        R = self.R
        flat = torch.rand(R * 6, device=self.dev)  # single jitter: one draw per ray and level (nerfplayer_nerfacto.py:99) + background
        return {"t_rand": flat[:R].view(R, 1), "u": [flat[R:2 * R].view(R, 1), flat[2 * R:3 * R].view(R, 1)], "bg": flat[3 * R:].view(R, 3)}

    def _train_step(self, target, rng, *fwd_args):
        """One optimiser step with the reference's callbacks: self.forward(*fwd_args, rng, anneal) -> backward -> optimizer_step."""
        cfg = self.cfg
        anneal = anneal_value(self.step, cfg.proposal_weights_anneal_max_num_iters, cfg.proposal_weights_anneal_slope) \
            if cfg.use_proposal_weight_anneal else 1.0
        sstep = max(self.step - 1, 0)  # the sampler's counter is set by the AFTER_TRAIN_ITERATION callback (nerfacto.py:249-263)
        updated = self._steps_since_update > update_schedule(sstep, cfg.proposal_warmup, cfg.proposal_update_every) or sstep < 10
        rng = rng if rng is not None else self.random_draws()
        self._in_train_step = True
        try:
            out = self.forward(*fwd_args, rng, anneal)
            self.backward(target, rng, proposal_grads=updated)
        finally:
            self._in_train_step = False
        self.optimizer_step()
        if updated:
            self._steps_since_update = 0
        self._steps_since_update += 1
        return out

"""GPU: every per-ray kernel of csrc/render_loss.hip against the float64 references of tests/per_ray_reference.py, over a lattice of sample
counts (1 ... 320, both sides of every multiple of 64), ragged ray counts (1, 2, 3, 4, 5, 133), the five production interlevel pairs and nine
edge pairs, and four input families: (a) pipeline-shaped, (b) nerf edges tied to proposal edges, (c) wide / single-bin envelopes, (d) exact
values (dyadic weights whose running sum hits 0.5 exactly, midpoints that equal D - sigma and D + sigma).

Every call goes through the C ABI with buffers of its own: each output carries GUARD extra rows behind row R filled with one sentinel and
live rows filled with another; afterwards the extra rows must be untouched (a dead wave that writes) and no live element may still hold its
sentinel (a tail lane that does not).  The ops.* wrappers allocate their own outputs, so they get one ragged case of their own at the end.

Bounds.  E32 below is the deviation of the float32 ORACLE from the same references (max |got - want| over the largest |want| of a case,
maximised over this lattice), measured on the CPU by tests/test_per_ray_reference_cpu.py, which also holds this table to its measurement
(profiles/r10_per_ray_reference_e32.json).  A kernel may deviate by MARGIN = 5 times that (README: "bounds = ~5x the measured deviations"):
it sums in a wave tree where the oracle sums sequentially, and expf / logf differ from the host libm by an ulp or two.  Integer results and
pure copies (median_index, median_rgb, depth_median given the index) are compared exactly.  Measured kernel deviations are recorded through
tests/_measure.record; the copy of this file's run is profiles/r10_per_ray_deviations.json.
"""
import ctypes as C
import re

import pytest
import torch

from tests import _measure
from tests import per_ray_reference as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MARGIN = 5.0
# One E32 per QUANTITY -- its maximum over the lattice -- bounds every case of that quantity, not the case's own E32.  A case's own figure is
# a sample of a handful of roundings: at R = 1 a value output is ONE number, whose float32 error against float64 can be 1e-10 by luck and is
# not zero, so 5 x that would fail a kernel that merely sums in another order.  The per-quantity maximum (which the issue's fallback for
# E32 = 0 cases already is) is stable under such luck; it is looser than a per-case figure at small S, where sums are short.  What the bounds
# are there to catch -- a wrong tie rule, window edge, gate, tail lane or carry -- moves a result by 1e-3 .. 1 of its largest element, five
# orders above them (profiles/r10_per_ray_INDEX.md lists eight such mutations and the tests each one fails).
# quantity: E32 (measured, rounded up to two digits)                 -> bound = MARGIN * E32
E32 = {
    "render.rgb": 3.1e-07,                                            # 1.55e-06
    "render.accumulation": 1.8e-07,                                   # 9.0e-07
    "render.depth_expected": 2.6e-07,                                 # 1.3e-06
    "render_bwd.g_weights": 2.2e-07,                                  # 1.1e-06
    "render_bwd.g_rgb": 4.7e-08,                                      # 2.35e-07
    "render_mse_bwd.g_weights": 2.5e-07,                              # 1.25e-06
    "render_mse_bwd.g_rgb": 8.7e-08,                                  # 4.35e-07
    "render_mse_bwd.sqerr": 7.3e-08,                                  # 3.65e-07
    "distortion.value": 1.6e-07,                                      # 8.0e-07
    "distortion.g_weights": 2.2e-07,                                  # 1.1e-06
    "interlevel.value": 2.0e-07,                                      # 1.0e-06
    "interlevel.g_wprop": 2.7e-07,                                    # 1.35e-06
    "ds_nerf.value": 1.8e-06,                                         # 9.0e-06
    "ds_nerf.g_weights": 1.8e-06,                                     # 9.0e-06
    "urf.value": 5.7e-07,                                             # 2.85e-06
    "urf.g_weights": 3.2e-07,                                         # 1.6e-06
    "urf.g_pred": 5.5e-07,                                            # 2.75e-06
    "ray_train.weights": 9.4e-08,                                     # 4.7e-07
    "ray_train.rgb_out": 2.5e-07,                                     # 1.25e-06
    "ray_train.acc": 3.6e-07,                                         # 1.8e-06
    "ray_train.dist_rays": 3.2e-07,                                   # 1.6e-06
    "ray_train.g_density": 9.2e-07,                                   # 4.6e-06
    "ray_train.g_weights": 4.3e-07,                                   # 2.15e-06
    "ray_train.g_rgb": 3.3e-07,                                       # 1.65e-06
    "ray_train.sqerr": 4.1e-07,                                       # 2.05e-06
}
BOUND = {k: MARGIN * v for k, v in E32.items()}

GUARD = 4
DEAD, LIVE = -7777.0, 12345.678  # sentinels of the guard rows / of the live rows before the call


# ---------------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from soccernerfs_amd import _lib as L

    return L, L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dv(t):
    return None if t is None else t.to(DEV).contiguous()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Out:
    """An output buffer [R + GUARD, *tail]: guard rows hold DEAD, live rows LIVE (or the prefill of an accumulating call)."""

    def __init__(self, R, *tail, dtype=torch.float32, prefill=None):
        self.R, self.prefilled = R, prefill is not None
        self.buf = torch.full((R + GUARD,) + tail, DEAD if dtype.is_floating_point else int(DEAD), dtype=dtype, device=DEV)
        if prefill is not None:
            self.buf[:R] = prefill.to(DEV)
        else:
            self.buf[:R] = LIVE if dtype.is_floating_point else int(LIVE)
        self.before = self.buf.clone()

    @property
    def p(self):
        return C.c_void_p(self.buf.data_ptr())

    def addr(self):
        return self.buf.data_ptr()

    def untouched(self):
        return torch.equal(self.buf, self.before)

    def get(self, name=""):
        """The live rows, after checking the guard rows and that every live element was written."""
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.R:], self.before[self.R:]), f"{name}: rows behind R were written"
        if not self.prefilled:
            assert not bool((self.buf[: self.R] == self.before[: self.R]).any()), f"{name}: live elements were left unwritten"
        return self.buf[: self.R].cpu()


class Report:
    """Collects every deviation of one test, records it, and fails at the end with all that exceed their bound."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def close(self, quantity, got, want):
        d = PR.deviation(got, want)
        # recorded in units of the case's largest |want|: _measure keeps the entry with the largest max_abs, which is then the worst case
        scale = float(torch.as_tensor(want).abs().max()) or 1.0
        _measure.record(f"per_ray.{quantity}", torch.as_tensor(got).detach().double().cpu() / scale, torch.as_tensor(want).detach().double().cpu() / scale)
        print(f"{self.label} {quantity}: deviation {d:.3e} (bound {BOUND[quantity]:.3e})")
        if not d <= BOUND[quantity]:
            self.bad.append((quantity, d, BOUND[quantity]))

    def exact(self, name, got, want):
        got, want = torch.as_tensor(got).cpu(), torch.as_tensor(want).cpu()
        same = torch.equal(got, want.to(got.dtype))
        if not same:
            self.bad.append((name, "not bit-exact", int((got != want.to(got.dtype)).sum())))

    def done(self):
        assert not self.bad, f"{self.label}: {self.bad}"


def _bg_for(case, mode):
    return {0: case["bg"], 1: None, 2: case["bg"][0].contiguous()}[mode]


def render_fwd(case, mode, training, skip=None):
    """snerf_render_fwd on guarded buffers; `skip` names one optional output passed as NULL.  Returns the live rows of every output."""
    L, lib = _lib()
    R, S = case["R"], case["S"]
    keep = [dv(case["weights"]), dv(case["rgb"]), dv(case["ebins"]), dv(_bg_for(case, mode))]
    outs = {"rgb": Out(R, 3), "accumulation": Out(R), "depth_median": Out(R), "depth_expected": Out(R), "median_rgb": Out(R, 3),
            "median_index": Out(R, dtype=torch.int64)}
    a = L.RenderArgs()
    a.weights, a.rgb, a.ebins = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    a.bg = keep[3].data_ptr() if keep[3] is not None else None
    a.R, a.S, a.bg_mode, a.training = R, S, mode, int(training)
    a.rgb_out, a.acc_out = outs["rgb"].addr(), outs["accumulation"].addr()
    for name, field in (("depth_median", "depth_median"), ("depth_expected", "depth_expected"), ("median_rgb", "median_rgb"),
                        ("median_index", "median_index")):
        setattr(a, field, None if name == skip else outs[name].addr())
    L.check(lib.snerf_render_fwd(C.byref(a), _stream()), "render_fwd")
    torch.cuda.synchronize()
    if skip:
        assert outs[skip].untouched(), f"{skip} was passed as NULL"
    return {k: o.get(k) for k, o in outs.items() if k != skip}


def check_render(rep, case, mode, training, skip=None):
    got = render_fwd(case, mode, training, skip)
    ref = PR.render_ref(case["weights"], case["rgb"], case["ebins"], _bg_for(case, mode), mode, training)
    rep.close("render.rgb", got["rgb"], ref["rgb"])
    rep.close("render.accumulation", got["accumulation"], ref["accumulation"])
    if "depth_expected" in got:
        rep.close("render.depth_expected", got["depth_expected"], ref["depth_expected"])
    for name in ("median_index", "depth_median", "median_rgb"):
        if name in got:
            rep.exact(f"{name} (mode {mode}, training {training})", got[name], ref[name])


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_render_fwd
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", PR.LATTICE)
def test_render_fwd_lattice(S, R):
    """All three background modes, train and eval, on family (a); each optional output passed as NULL in turn."""
    case = PR.pipeline_case(R, S, S, "a")
    rep = Report(f"render_fwd S={S} R={R}")
    for mode in (0, 1, 2):
        for training in (True, False):
            check_render(rep, case, mode, training)
    for skip in ("depth_median", "depth_expected", "median_rgb", "median_index"):
        check_render(rep, case, 0, True, skip)
    rep.done()


@pytest.mark.parametrize("S,R,Sp,fam", PR.RENDER_FAMILY_CASES)
def test_render_fwd_tied_and_wide_bins(S, R, Sp, fam):
    """Families (b) and (c): zero-width and independently drawn bins under the renderers (depth_median and depth_expected read them)."""
    case = PR.pipeline_case(R, S, Sp, fam)
    rep = Report(f"render_fwd S={S} R={R} ({fam})")
    for mode, training in ((0, True), (1, True), (2, False)):
        check_render(rep, case, mode, training)
    rep.done()


@pytest.mark.parametrize("S", PR.SAMPLE_COUNTS)
def test_render_fwd_exact_values(S):
    """Family (d): running sums that hit 0.5 exactly, all-zero rays, totals below 0.5, accumulation above 1 -- the median index is exact."""
    case = PR.exact_render_case(S)
    rep = Report(f"render_fwd exact S={S}")
    for mode, training in ((0, True), (1, False), (2, False)):
        check_render(rep, case, mode, training)
    rep.done()


@pytest.mark.parametrize("S,R", PR.LATTICE)
def test_render_fwd_eval_nonfinite_colours(S, R):
    """Eval mode with NaN and +-inf in rgb and in the last sample: nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX) before compositing, the clamp to
    [0, 1] after it, on rgb, on the last-sample background and on median_rgb."""
    case = PR.with_nonfinite_rgb(PR.pipeline_case(R, S, S, "a"))
    assert not bool(torch.isfinite(case["rgb"]).all())
    rep = Report(f"render_fwd eval non-finite S={S} R={R}")
    for mode in (0, 1, 2):
        got = render_fwd(case, mode, False)
        assert bool(torch.isfinite(got["rgb"]).all()) and bool(torch.isfinite(got["median_rgb"]).all()), mode
        ref = PR.render_ref(case["weights"], case["rgb"], case["ebins"], _bg_for(case, mode), mode, False)
        rep.close("render.rgb", got["rgb"], ref["rgb"])
        rep.close("render.accumulation", got["accumulation"], ref["accumulation"])
        for name in ("median_index", "depth_median", "median_rgb"):
            rep.exact(f"{name} (mode {mode})", got[name], ref[name])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_render_bwd, snerf_render_mse_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(PR.LATTICE)), ids=[f"S{s}-R{r}" for s, r in PR.LATTICE])
def test_render_bwd_lattice(k):
    L, lib = _lib()
    S, R = PR.LATTICE[k]
    case = PR.pipeline_case(R, S, S, "a")
    go, ga, out = PR.upstream(case, k)
    w, rgb, tgt = dv(case["weights"]), dv(case["rgb"]), dv(case["target"])
    go_d, ga_d, out_d = dv(go), dv(ga), dv(out)
    rep = Report(f"render_bwd S={S} R={R}")
    for mode in (0, 2):
        bg = _bg_for(case, mode)
        bg_d = dv(bg)
        for use_acc in (False, True):
            for accumulate in (0, 1):
                want_w, want_rgb = PR.render_bwd_ref(case["weights"], case["rgb"], bg, mode, go, ga if use_acc else None)
                pre = PR.prefill_like(want_w, "render_bwd", k, mode, use_acc) if accumulate else None
                if accumulate:
                    want_w = PR.render_bwd_ref(case["weights"], case["rgb"], bg, mode, go, ga if use_acc else None, pre)[0]
                gw, grgb = Out(R, S, prefill=pre), Out(R, S, 3)
                L.check(lib.snerf_render_bwd(ptr(w), ptr(rgb), ptr(bg_d), mode, ptr(go_d), ptr(ga_d) if use_acc else None, R, S, gw.p, grgb.p,
                                             accumulate, _stream()), "render_bwd")
                rep.close("render_bwd.g_weights", gw.get("g_weights"), want_w)
                rep.close("render_bwd.g_rgb", grgb.get("g_rgb"), want_rgb)
        gw = Out(R, S)  # g_rgb is optional
        L.check(lib.snerf_render_bwd(ptr(w), ptr(rgb), ptr(bg_d), mode, ptr(go_d), None, R, S, gw.p, None, 0, _stream()), "render_bwd")
        rep.close("render_bwd.g_weights", gw.get("g_weights"), PR.render_bwd_ref(case["weights"], case["rgb"], bg, mode, go)[0])
        # the MSE-folded backward
        scale = 2 * 0.7 / (3 * R)
        want_w, want_rgb, want_sq = PR.render_mse_bwd_ref(case["weights"], case["rgb"], bg, mode, out, case["target"], scale)
        gw, grgb, sq = Out(R, S), Out(R, S, 3), Out(R)
        L.check(lib.snerf_render_mse_bwd(ptr(w), ptr(rgb), ptr(bg_d), mode, ptr(out_d), ptr(tgt), scale, R, S, gw.p, grgb.p, sq.p, _stream()),
                "render_mse_bwd")
        rep.close("render_mse_bwd.g_weights", gw.get("g_weights"), want_w)
        rep.close("render_mse_bwd.g_rgb", grgb.get("g_rgb"), want_rgb)
        rep.close("render_mse_bwd.sqerr", sq.get("sqerr"), want_sq)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_distortion
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(PR.LATTICE)), ids=[f"S{s}-R{r}" for s, r in PR.LATTICE])
def test_distortion_lattice(k):
    """Per-ray value and gradient with grad_scale, accumulate 0 and 1, on family (a) and on family (b) (zero-width bins)."""
    L, lib = _lib()
    S, R = PR.LATTICE[k]
    rep = Report(f"distortion S={S} R={R}")
    scale = 1e-3 / R
    for fam in ("a", "b"):
        case = PR.pipeline_case(R, S, S, fam)
        w, sb = dv(case["weights"]), dv(case["c_bins"])
        want_v, want_g = PR.distortion_ref(case["weights"], case["c_bins"], scale)
        for accumulate in (0, 1):
            pre = PR.prefill_like(want_g, "distortion", k) if accumulate else None
            want = PR.distortion_ref(case["weights"], case["c_bins"], scale, pre)[1] if accumulate else want_g
            val, g = Out(R), Out(R, S, prefill=pre)
            L.check(lib.snerf_distortion(ptr(w), ptr(sb), R, S, scale, val.p, g.p, accumulate, _stream()), "distortion")
            rep.close("distortion.value", val.get("loss_rays"), want_v)
            rep.close("distortion.g_weights", g.get("g_weights"), want)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_interlevel
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Sp,R,fam,mode", PR.interlevel_cases())
def test_interlevel_lattice(S, Sp, R, fam, mode):
    """Per-ray value and d/d w_prop against the float64 emulation (float32 cumsum and one float32 rounding of w_outer, float64 after that)."""
    L, lib = _lib()
    case = PR.pipeline_case(R, S, Sp, fam)
    w_nerf = case["weights"] if mode == "natural" else PR.scaled_nerf_weights(case)
    scale = 1.0 / (R * S)
    want_v, want_g = PR.interlevel_ref(case["c_bins"], w_nerf, case["p_bins"], case["w_prop"], scale)
    keep = [dv(case["c_bins"]), dv(w_nerf), dv(case["p_bins"]), dv(case["w_prop"])]
    val, g = Out(R), Out(R, Sp)
    L.check(lib.snerf_interlevel(ptr(keep[0]), ptr(keep[1]), S, ptr(keep[2]), ptr(keep[3]), Sp, R, scale, val.p, g.p, _stream()), "interlevel")
    rep = Report(f"interlevel S={S} Sp={Sp} R={R} ({fam}, {mode})")
    rep.close("interlevel.value", val.get("loss_rays"), want_v)
    rep.close("interlevel.g_wprop", g.get("g_wprop"), want_g)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_depth_loss, snerf_urf_depth_loss
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_depth_losses(rep, case, key):
    L, lib = _lib()
    R, S = case["R"], case["S"]
    scale = 0.5 / R
    w, eb, term, dn, pred = (dv(case[n]) for n in ("weights", "ebins", "termination_depth", "directions_norm", "predicted_depth"))
    for use_norm in (False, True):
        for accumulate in (0, 1):
            want_v, want_g = PR.ds_nerf_depth_ref(case, use_norm, scale)
            pre = PR.prefill_like(want_g, "ds_nerf", key, use_norm) if accumulate else None
            if accumulate:
                want_g = PR.ds_nerf_depth_ref(case, use_norm, scale, pre)[1]
            val, g = Out(R), Out(R, S, prefill=pre)
            L.check(lib.snerf_depth_loss(ptr(w), ptr(eb), ptr(term), ptr(dn) if use_norm else None, case["sigma"], R, S, scale, val.p, g.p, accumulate,
                                         _stream()), "depth_loss")
            rep.close("ds_nerf.value", val.get("loss_rays"), want_v)
            rep.close("ds_nerf.g_weights", g.get("g_weights"), want_g)
            want_v, want_g, want_p = PR.urf_depth_ref(case, use_norm, scale)
            pre = PR.prefill_like(want_g, "urf", key, use_norm) if accumulate else None
            if accumulate:
                want_g = PR.urf_depth_ref(case, use_norm, scale, pre)[1]
            val, g, gp = Out(R), Out(R, S, prefill=pre), Out(R)
            L.check(lib.snerf_urf_depth_loss(ptr(w), ptr(eb), ptr(term), ptr(dn) if use_norm else None, ptr(pred), case["sigma"], R, S, scale, val.p,
                                             g.p, gp.p, accumulate, _stream()), "urf_depth_loss")
            rep.close("urf.value", val.get("loss_rays"), want_v)
            rep.close("urf.g_weights", g.get("g_weights"), want_g)
            rep.close("urf.g_pred", gp.get("g_pred"), want_p)


@pytest.mark.parametrize("k", range(len(PR.LATTICE)), ids=[f"S{s}-R{r}" for s, r in PR.LATTICE])
def test_depth_losses_lattice(k):
    """DS-NeRF and URF: value, g_weights, g_pred; D <= 0 rays, directions_norm given or not, accumulate 0 and 1."""
    case = PR.lattice_depth_case(k)
    assert PR.depth_margin(case) > PR.MARGIN  # a property of the inputs: float32 and float64 put every midpoint on the same side
    rep = Report(f"depth losses S={case['S']} R={case['R']} sigma={case['sigma']}")
    check_depth_losses(rep, case, k)
    rep.done()


@pytest.mark.parametrize("S", PR.SAMPLE_COUNTS)
def test_depth_losses_exact_window_edges(S):
    """Family (d): midpoints that equal D - sigma and D + sigma exactly belong to the window (<= and >=); D = 0 and D < 0 rays are gated off."""
    case = PR.exact_depth_case(S)
    assert min(PR.edge_hits(case)) >= 1
    rep = Report(f"depth losses exact S={S}")
    check_depth_losses(rep, case, 1000 + S)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_ray_train_fwd_bwd against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", [(48, 133), (48, 3), (64, 133), (64, 2), (320, 133), (320, 5)])
def test_ray_train_kernel_against_float64(S, R):
    """The one-launch kernel has a reference of its own, not only the five-kernel chain's: weights, rgb_out, acc, sqerr, dist_rays, g_rgb, g_weights and g_density
    in float64 on finite inputs (tests/test_gpu_render_loss.py proves it equal to the chain bit for bit, non-finite inputs included)."""
    L, lib = _lib()
    case = PR.pipeline_case(R, S, S, "a")
    go_scale, dist_scale = 2.0 / (3 * R), 1e-3 / R
    ref = PR.ray_train_ref(case, go_scale, dist_scale)
    keep = {n: dv(case[n]) for n in ("density", "ebins", "c_bins", "rgb", "bg", "target")}
    o = {"weights": Out(R, S), "rgb_out": Out(R, 3), "acc": Out(R), "depth_median": Out(R), "sqerr": Out(R), "dist_rays": Out(R),
         "g_rgb": Out(R, S, 3), "g_density": Out(R, S), "g_weights": Out(R, S)}
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    ra = L.RayTrainArgs()
    ra.density, ra.ebins, ra.sbins = keep["density"].data_ptr(), keep["ebins"].data_ptr(), keep["c_bins"].data_ptr()
    ra.rgb, ra.bg, ra.target = keep["rgb"].data_ptr(), keep["bg"].data_ptr(), keep["target"].data_ptr()
    ra.R, ra.S, ra.bg_mode, ra.go_scale, ra.dist_scale = R, S, 0, go_scale, dist_scale
    ra.weights, ra.rgb_out, ra.acc_out, ra.depth_median = o["weights"].addr(), o["rgb_out"].addr(), o["acc"].addr(), o["depth_median"].addr()
    ra.sqerr_rays, ra.dist_rays, ra.g_rgb, ra.g_density = o["sqerr"].addr(), o["dist_rays"].addr(), o["g_rgb"].addr(), o["g_density"].addr()
    ra.g_weights, ra.nonfinite_flag = o["g_weights"].addr(), flag.data_ptr()
    L.check(lib.snerf_ray_train_fwd_bwd(C.byref(ra), _stream()), "ray_train_fwd_bwd")
    got = {k: v.get(k) for k, v in o.items()}
    assert int(flag[0]) == 0
    rep = Report(f"ray_train S={S} R={R}")
    for name in ("weights", "rgb_out", "acc", "dist_rays", "g_density", "g_weights", "g_rgb", "sqerr"):
        rep.close(f"ray_train.{name}", got[name], ref[name])
    # the median depth: exact given the index of the kernel's own (float32) weights
    idx = PR.median_index_ref(got["weights"])
    steps = (case["ebins"][:, :-1] + case["ebins"][:, 1:]) / 2.0
    rep.exact("depth_median", got["depth_median"], torch.gather(steps, 1, idx[:, None])[:, 0])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------------------------
def _entry_points(R, S, Sp):
    """(name, call, outputs) of every per-ray entry point on a family (a) case of S x Sp samples declared as R rays."""
    L, lib = _lib()
    rows = max(R, 1)
    case = PR.pipeline_case(rows, min(S, 320), min(Sp, 320), "a")
    pad = lambda t, n: dv(torch.cat([t, t[:, -1:].expand(-1, n - t.shape[1])], 1)) if n > t.shape[1] else dv(t)  # inputs as wide as declared
    w, eb, sb = pad(case["weights"], S), pad(case["ebins"], S + 1), pad(case["c_bins"], S + 1)
    wp, tp = pad(case["w_prop"], Sp), pad(case["p_bins"], Sp + 1)
    rgb = dv(case["rgb"][:, :1].expand(-1, S, -1))
    dens = pad(case["density"], S)
    bg, tgt = dv(case["bg"]), dv(case["target"])
    term = dv(torch.ones(rows))
    st = _stream()
    out = []
    o = [Out(rows, 3), Out(rows), Out(rows), Out(rows), Out(rows, 3), Out(rows, dtype=torch.int64)]
    a = L.RenderArgs()
    a.weights, a.rgb, a.ebins, a.bg, a.R, a.S, a.bg_mode, a.training = w.data_ptr(), rgb.data_ptr(), eb.data_ptr(), bg.data_ptr(), R, S, 0, 1
    a.rgb_out, a.acc_out, a.depth_median, a.depth_expected, a.median_rgb, a.median_index = (x.addr() for x in o)
    out.append(("render_fwd", lambda a=a: lib.snerf_render_fwd(C.byref(a), st), o))
    o = [Out(rows), Out(rows, S)]
    out.append(("distortion", lambda o=o: lib.snerf_distortion(ptr(w), ptr(sb), R, S, 1.0, o[0].p, o[1].p, 0, st), o))
    o = [Out(rows), Out(rows, Sp)]
    out.append(("interlevel", lambda o=o: lib.snerf_interlevel(ptr(sb), ptr(w), S, ptr(tp), ptr(wp), Sp, R, 1.0, o[0].p, o[1].p, st), o))
    o = [Out(rows), Out(rows, S)]
    out.append(("depth_loss", lambda o=o: lib.snerf_depth_loss(ptr(w), ptr(eb), ptr(term), None, 0.05, R, S, 1.0, o[0].p, o[1].p, 0, st), o))
    o = [Out(rows), Out(rows, S), Out(rows)]
    out.append(("urf_depth_loss", lambda o=o: lib.snerf_urf_depth_loss(ptr(w), ptr(eb), ptr(term), None, ptr(term), 0.05, R, S, 1.0, o[0].p, o[1].p,
                                                                       o[2].p, 0, st), o))
    o = [Out(rows, S), Out(rows, 3), Out(rows), Out(rows), Out(rows), Out(rows), Out(rows, S, 3), Out(rows, S), Out(rows, S)]
    ra = L.RayTrainArgs()
    ra.density, ra.ebins, ra.sbins, ra.rgb, ra.bg, ra.target = dens.data_ptr(), eb.data_ptr(), sb.data_ptr(), rgb.data_ptr(), bg.data_ptr(), tgt.data_ptr()
    ra.R, ra.S, ra.bg_mode, ra.go_scale, ra.dist_scale = R, S, 0, 1.0, 1.0
    (ra.weights, ra.rgb_out, ra.acc_out, ra.depth_median, ra.sqerr_rays, ra.dist_rays, ra.g_rgb, ra.g_density, ra.g_weights) = (x.addr() for x in o)
    out.append(("ray_train_fwd_bwd", lambda ra=ra: lib.snerf_ray_train_fwd_bwd(C.byref(ra), st), o))
    if S <= 320:  # elementwise kernels without LDS rows: no limit on S, so only the R = 0 case applies to them
        o = [Out(rows, S), Out(rows, S, 3)]
        out.append(("render_bwd", lambda o=o: lib.snerf_render_bwd(ptr(w), ptr(rgb), ptr(bg), 0, ptr(tgt), None, R, S, o[0].p, o[1].p, 0, st), o))
        o = [Out(rows, S), Out(rows, S, 3), Out(rows)]
        out.append(("render_mse_bwd", lambda o=o: lib.snerf_render_mse_bwd(ptr(w), ptr(rgb), ptr(bg), 0, ptr(tgt), ptr(tgt), 1.0, R, S, o[0].p, o[1].p,
                                                                           o[2].p, st), o))
    keep = (w, eb, sb, wp, tp, rgb, dens, bg, tgt, term)
    return out, keep


def test_sample_counts_beyond_the_lds_rows_are_refused():
    """S = 321 (and Sp = 321) exceed the kernels' LDS rows: the entry points return an error, name the argument, and write nothing."""
    L, lib = _lib()
    for S, Sp in ((321, 64), (64, 321)):
        calls, keep = _entry_points(5, S, Sp)
        for name, call, outs in calls:
            if Sp == 321 and name != "interlevel":
                continue
            rc = call()
            torch.cuda.synchronize()
            assert rc != 0, f"{name} accepted S={S} Sp={Sp}"
            what = rf"{name}: .*\b{'Sp' if Sp == 321 else 'S'}=321\b"  # the entry point's own message with the offending value
            assert re.search(what, lib.snerf_last_error().decode()), (name, lib.snerf_last_error().decode())
            with pytest.raises(RuntimeError, match=what):
                L.check(rc, name)
            assert all(o.untouched() for o in outs), f"{name} wrote to its outputs although it refused the call"


def test_zero_rays_succeed_and_launch_nothing():
    calls, keep = _entry_points(0, 64, 128)
    assert {"render_bwd", "render_mse_bwd"} <= {name for name, *_ in calls}
    for name, call, outs in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, name
        assert all(o.untouched() for o in outs), f"{name} wrote to its outputs with R = 0"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the ops.* wrappers (they allocate their own outputs: one ragged case each, same references and bounds)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ops_wrappers_on_a_ragged_case():
    from soccernerfs_amd import ops

    R, S, Sp = 5, 65, 129
    case = PR.pipeline_case(R, S, Sp, "b")
    rep = Report(f"ops wrappers S={S} Sp={Sp} R={R}")
    go, ga, _ = PR.upstream(case, "ops")
    w, rgb = dv(case["weights"]).requires_grad_(True), dv(case["rgb"]).requires_grad_(True)
    o = ops.render(w, rgb, dv(case["ebins"]), dv(case["bg"]), True)
    ref = PR.render_ref(case["weights"], case["rgb"], case["ebins"], case["bg"], 0, True)
    rep.close("render.rgb", o["rgb"], ref["rgb"])
    rep.close("render.accumulation", o["accumulation"], ref["accumulation"])
    rep.close("render.depth_expected", o["depth_expected"], ref["depth_expected"])
    for name in ("median_index", "depth_median", "median_rgb"):
        rep.exact(name, o[name], ref[name])
    ((o["rgb"] * dv(go)).sum() + (o["accumulation"] * dv(ga)).sum()).backward()
    want_w, want_rgb = PR.render_bwd_ref(case["weights"], case["rgb"], case["bg"], 0, go, ga)
    rep.close("render_bwd.g_weights", w.grad, want_w)
    rep.close("render_bwd.g_rgb", rgb.grad, want_rgb)
    w = dv(case["weights"]).requires_grad_(True)
    val = ops.distortion_loss(w, dv(case["c_bins"]))
    val.backward()
    want_v, want_g = PR.distortion_ref(case["weights"], case["c_bins"], 1.0 / R)
    rep.close("distortion.value", val, want_v.mean())
    rep.close("distortion.g_weights", w.grad, want_g)
    wp = dv(case["w_prop"]).requires_grad_(True)
    val = ops.interlevel_loss([wp, dv(case["weights"])], [dv(case["p_bins"]), dv(case["c_bins"])])
    val.backward()
    want_v, want_g = PR.interlevel_ref(case["c_bins"], case["weights"], case["p_bins"], case["w_prop"], 1.0 / (R * S))
    rep.close("interlevel.value", val, want_v.sum() / (R * S))
    rep.close("interlevel.g_wprop", wp.grad, want_g)
    dcase = PR.depth_case(R, S, seed=77)
    w = dv(dcase["weights"]).requires_grad_(True)
    val = ops.ds_nerf_depth_loss(w, dv(dcase["ebins"]), dv(dcase["termination_depth"]), dcase["sigma"], dv(dcase["directions_norm"]))
    val.backward()
    want_v, want_g = PR.ds_nerf_depth_ref(dcase, True, 1.0 / R)
    rep.close("ds_nerf.value", val, want_v.mean())
    rep.close("ds_nerf.g_weights", w.grad, want_g)
    w, pd = dv(dcase["weights"]).requires_grad_(True), dv(dcase["predicted_depth"]).requires_grad_(True)
    val = ops.urf_depth_loss(w, dv(dcase["ebins"]), dv(dcase["termination_depth"]), pd, dcase["sigma"])
    val.backward()
    want_v, want_g, want_p = PR.urf_depth_ref(dcase, False, 1.0 / R)
    rep.close("urf.value", val, want_v.mean())
    rep.close("urf.g_weights", w.grad, want_g)
    rep.close("urf.g_pred", pd.grad, want_p)
    rep.done()

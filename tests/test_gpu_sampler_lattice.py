"""GPU: the ray samplers of csrc/ray_ops.hip (spaced_bins_kernel; resample_kernel behind snerf_pdf_resample and snerf_weights_fwd;
weights_bwd_kernel) against tests/sampler_reference.py over a lattice: Sp and S on both sides of every multiple of 64 and at the limit (1, 2, 3,
63 ... 320; S = 320 gives 321 new edges), the production and the fixtures' pairs, R = 1, 2, 3, 4, 5, 133 (sampler_reference.resample_pairs holds
the pruning rule), and four input families: X exact (dyadic weights, bins and u: u on cdf knots, on repeated knots of zero-width pdf bins, 0, 1
and above the cdf's last entry), P pipeline-shaped, Z degenerate (the eps padding as the whole pdf, one non-zero weight, 1e-30 beside 1e30, all
edges equal), A the inexact routes (annealing, get_weights in the kernel).

Every call goes through the C ABI with buffers of its own: each output carries GUARD rows behind row R that hold one sentinel and live rows that
hold another; afterwards the guard rows must be bit-unchanged (a dead wave that writes) and no live element may still hold its sentinel (a tail
lane that does not).  inds_out and weights_out are passed as NULL and non-NULL: the other outputs must not change.

Assertions.  With the weights given and anneal == 1 every operation between the inputs and inds / sbins / ebins is a correctly rounded float32
operation or the double-accumulated cumsum, whose float32 result does not depend on the order of summation on these inputs
(sampler_reference.sums_order_independent, asserted per case by the generators): spaced_bins and families X, P, Z are compared by EQUALITY on
every element, all three u modes, both rand_cols, both kinds; family X also against the float64 reference.  Family A and the weights entry
points go through expf / powf: bounded by MARGIN = 5 x E32, the float32 restatement's own deviation from float64 measured on the CPU
(sampler_reference.E32), with tau = 5 x E32 of the cdf for the index criterion and for u_back, on every element.  Measured kernel deviations are
recorded through tests/_measure.record; the copy of this file's run is profiles/r30_sampler_deviations.json.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _measure
from tests import sampler_reference as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GUARD = 4
DEAD, LIVE = -7777.0, 12345.678  # sentinels of the guard rows / of the live rows before the call
KIND = {"uniform": 0, "piecewise": 1}
KINDS = ("uniform", "piecewise")


# ---------------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from soccernerfs_amd import _lib as L

    return L, L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Out:
    """An output buffer [R + GUARD, *tail]: guard rows hold DEAD, live rows LIVE (or the prefill of an accumulating call)."""

    def __init__(self, R, *tail, dtype=torch.float32, prefill=None):
        self.R, self.prefilled = R, prefill is not None
        self.buf = torch.full((R + GUARD,) + tail, DEAD if dtype.is_floating_point else int(DEAD), dtype=dtype, device=DEV)
        if prefill is not None:
            self.buf[:R] = torch.from_numpy(prefill).to(DEV)
        else:
            self.buf[:R] = LIVE if dtype.is_floating_point else int(LIVE)
        self.before = self.buf.clone()

    @property
    def p(self):
        return C.c_void_p(self.buf.data_ptr())

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.buf, self.before)

    def get(self, name=""):
        """The live rows, after checking the guard rows and that every live element was written."""
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.R:], self.before[self.R:]), f"{name}: rows behind R were written"
        if not self.prefilled:
            assert not bool((self.buf[: self.R] == self.before[: self.R]).any()), f"{name}: live elements were left unwritten"
        return self.buf[: self.R].cpu().numpy()


def same(name, got, want):
    """Equality on every element (-0.0 == 0.0; there are no NaNs on either side)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"got {got[bad][0]!r}, want {want[bad][0]!r}"


def spaced(nears, fars, S, t_rand, kind):
    L, lib = _lib()
    R = len(nears)
    keep = [dv(nears), dv(fars), dv(t_rand)]
    sb, eb = Out(R, S + 1), Out(R, S + 1)
    L.check(lib.snerf_spaced_bins(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), 0 if t_rand is None else t_rand.shape[1], R, S, KIND[kind], sb.p, eb.p,
                                  _stream()), "spaced_bins")
    return sb.get("sbins"), eb.get("ebins")


def resample(case, kind="uniform", inds=True, weights_out=False):
    """snerf_pdf_resample on guarded buffers.  Returns {"sbins", "ebins", "inds" (if asked), "weights_out" (if asked, density route)}."""
    L, lib = _lib()
    R, Sp, S = case["R"], case["Sp"], case["S"]
    fused = case.get("density") is not None
    keep = {k: dv(case.get(k)) for k in ("density", "ebins_prev", "weights", "sbins_prev", "nears", "fars")}
    mode = case["u_mode"]
    keep["ur"] = dv(case["u"] if mode == 0 else case["rand"] if mode == 1 else None)
    o = {"sbins": Out(R, S + 1), "ebins": Out(R, S + 1), "inds": Out(R, S + 1, dtype=torch.int64), "weights_out": Out(R, Sp)}
    a = L.ResampleArgs()
    if fused:
        a.density, a.ebins_prev = keep["density"].data_ptr(), keep["ebins_prev"].data_ptr()
    else:
        a.weights_in = keep["weights"].data_ptr()
    a.weights_out = o["weights_out"].buf.data_ptr() if weights_out else None
    a.sbins_prev, a.nears, a.fars = keep["sbins_prev"].data_ptr(), keep["nears"].data_ptr(), keep["fars"].data_ptr()
    a.u_or_rand = keep["ur"].data_ptr() if keep["ur"] is not None else None
    a.sbins_out, a.ebins_out = o["sbins"].buf.data_ptr(), o["ebins"].buf.data_ptr()
    a.inds_out = o["inds"].buf.data_ptr() if inds else None
    a.R, a.S_prev, a.S, a.u_mode, a.kind = R, Sp, S, mode, KIND[kind]
    a.rand_cols = case["rand"].shape[1] if mode == 1 else 0
    a.anneal, a.histogram_padding, a.eps = case["anneal"], case["histogram_padding"], case["eps"]
    L.check(lib.snerf_pdf_resample(C.byref(a), _stream()), "pdf_resample")
    out = {"sbins": o["sbins"].get("sbins"), "ebins": o["ebins"].get("ebins")}
    if inds:
        out["inds"] = o["inds"].get("inds")
    else:
        assert o["inds"].untouched(), "inds_out was passed as NULL"
    if weights_out and fused:
        out["weights_out"] = o["weights_out"].get("weights_out")
    else:
        assert o["weights_out"].untouched(), "weights_out was NULL, or the weights were given (then nothing is to be written)"
    return out


def check_equal(label, case, kind, f64_too=False, optional=False):
    """inds, sbins, ebins of one call equal the float32 restatement on every element (family X: the float64 reference as well); with
    `optional`, the call is repeated with inds_out NULL and with weights_out given, and sbins / ebins must come out bit-identical."""
    want = SR.reference(case, kind, SR.f32)
    got = resample(case, kind)
    same(f"{label} {kind} inds", got["inds"], want["inds"])
    same(f"{label} {kind} sbins", got["sbins"], want["sbins"])
    same(f"{label} {kind} ebins", got["ebins"], want["ebins"])
    if f64_too:
        w64 = SR.reference(case, kind, SR.f64)
        same(f"{label} {kind} inds (float64)", got["inds"], w64["inds"])
        same(f"{label} {kind} sbins (float64)", got["sbins"].astype(np.float64), w64["sbins"])
        if kind == "uniform" and case["u_mode"] == 0:
            same(f"{label} ebins (float64)", got["ebins"].astype(np.float64), w64["ebins"])
    if optional:
        for kw in ({"inds": False}, {"weights_out": True}, {"inds": False, "weights_out": True}):
            again = resample(case, kind, **kw)
            for name in again:
                assert np.array_equal(again[name].view(np.int32) if again[name].dtype == np.float32 else again[name],
                                      got[name].view(np.int32) if got[name].dtype == np.float32 else got[name]), (label, kind, kw, name)


PAIRS = SR.resample_pairs()
PAIR_IDS = [f"Sp{sp}-S{s}-R{r}" for sp, s, r in PAIRS]


# ---------------------------------------------------------------------------------------------------------------------------------------
# spaced_bins
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", SR.spaced_cases())
def test_spaced_bins_lattice(S, R):
    """Eval bins, single jitter [R, 1] and per-edge jitter [R, S + 1] (draws include 0 and the largest float32 below 1), both kinds: sbins and
    ebins equal restatement (a) on every element.  near < 1 < far, so the piecewise spacing takes both of its branches and its inverse both of
    its own."""
    rng = SR._rng("spaced", S, R)
    near = (rng.random(R) * 0.5 + 0.05).astype(np.float32)
    far = (near + 2.0 + rng.random(R) * 4.0).astype(np.float32)
    full = rng.random((R, S + 1)).astype(np.float32)
    full[0, 0], full[-1, -1] = 0.0, np.float32(1.0 - 2.0 ** -24)
    for t_rand in (None, full[:, :1].copy(), full):
        want_sb = SR.spaced_bins(R, S, t_rand)
        for kind in KINDS:
            sb, eb = spaced(near, far, S, t_rand, kind)
            label = f"spaced_bins S={S} R={R} {kind} t_rand={None if t_rand is None else t_rand.shape}"
            same(label + " sbins", sb, want_sb)
            same(label + " ebins", eb, SR.to_euclidean(want_sb, near, far, kind))
    if S + 1 > 2:  # t_rand of any other width is refused, and nothing is written
        L, lib = _lib()
        keep = [dv(near), dv(far), dv(full[:, :2])]
        sb, eb = Out(R, S + 1), Out(R, S + 1)
        assert lib.snerf_spaced_bins(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), 2, R, S, 0, sb.p, eb.p, _stream()) != 0
        assert sb.untouched() and eb.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------
# pdf_resample, weights given, anneal == 1: equality
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(PAIRS)), ids=PAIR_IDS)
def test_resample_exact_family(k):
    """Family X, explicit u: histogram_padding 0 (zero-width pdf bins) and one dyadic padding of 2^-10, 2^-9, 2^-8 in turn; both kinds."""
    Sp, S, R = PAIRS[k]
    for p in (0, (1, 2, 4)[k % 3]):
        case = SR.exact_case(R, Sp, S, p, 0)
        SR.assert_exact(case)
        for kind in KINDS:
            check_equal(f"X Sp={Sp} S={S} R={R} p={p}", case, kind, f64_too=True, optional=(kind == KINDS[k % 2] and p == 0))


X_KERNEL_U = [(Sp, S, SR.RAY_COUNTS[(i + j) % 6]) for i, S in enumerate(SR.POW2_S) for j, Sp in enumerate((1, 3, 64, 65, 257, 320))]


@pytest.mark.parametrize("Sp,S,R", X_KERNEL_U)
def test_resample_exact_family_u_formed_in_the_kernel(Sp, S, R):
    """Family X with S + 1 a power of two: 1 / nb, the linspace step, rand / nb and hence u are exact, with u on the strata edges where rand is 0.
    Training draws as [R, 1] and [R, S + 1], and eval mode."""
    for mode, cols in ((1, 1), (1, S + 1), (2, None)):
        for p in (0, 2):
            case = SR.exact_case(R, Sp, S, p, mode, cols)
            SR.assert_exact(case)
            for kind in KINDS:
                check_equal(f"X Sp={Sp} S={S} R={R} p={p} u_mode={mode} cols={cols}", case, kind, f64_too=True)


@pytest.mark.parametrize("k", range(len(PAIRS)), ids=PAIR_IDS)
def test_resample_pipeline_family(k):
    """Family P: explicit u, training draws as [R, 1] and as [R, S + 1], eval mode; the kind alternates with the mode and the case."""
    Sp, S, R = PAIRS[k]
    for m, (mode, cols) in enumerate(((0, None), (1, 1), (1, S + 1), (2, None))):
        case = SR.pipeline_case(R, Sp, S, mode, cols)
        assert SR.prefix_sums_off_midpoints(case)
        check_equal(f"P Sp={Sp} S={S} R={R} u_mode={mode} cols={cols}", case, KINDS[(k + m) % 2], optional=(m == k % 4))


Z_SHAPES = ((1, 1, 1), (1, 320, 3), (2, 3, 5), (3, 2, 2), (63, 65, 4), (64, 64, 133), (65, 63, 5), (129, 192, 3), (256, 128, 133), (257, 1, 2),
            (320, 320, 5), (319, 257, 1))  # (Sp, S, R)


@pytest.mark.parametrize("Sp,S,R", Z_SHAPES)
@pytest.mark.parametrize("which", SR.DEGENERATE)
def test_resample_degenerate_family(which, Sp, S, R):
    """Family Z: per-edge draws, then single draws, eval mode and explicit u (0, 1 and 1.25 among them) on the same weights."""
    case = SR.degenerate_case(which, R, Sp, S)
    assert SR.prefix_sums_off_midpoints(case)
    label = f"Z {which} Sp={Sp} S={S} R={R}"
    check_equal(label, case, "uniform", optional=True)
    check_equal(label, case, "piecewise")
    single = dict(case, rand=np.ascontiguousarray(case["rand"][:, :1]))
    check_equal(label + " cols=1", single, "uniform")
    check_equal(label + " eval", dict(case, rand=None, u_mode=2), "piecewise")
    u = case["rand"].copy()
    u.flat[0::9], u.flat[3::9], u.flat[6::9] = 0.0, 1.0, 1.25
    check_equal(label + " explicit u", dict(case, rand=None, u=u, u_mode=0), "uniform")


# ---------------------------------------------------------------------------------------------------------------------------------------
# pdf_resample through powf / expf: bounded on every element
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sp,S,R", SR.INEXACT_SHAPES)
@pytest.mark.parametrize("route", SR.INEXACT_ROUTES)
def test_resample_inexact_routes(route, Sp, S, R):
    """Family A against float64.  weights_out within 5 x E32; every index accepted iff cdf64[ind - 1] - tau <= u < cdf64[ind] + tau; every new
    edge inside the bin of the kernel's own index; edges non-decreasing along a ray (u is sorted); the float64 cdf at the kernel's edges gives u
    back within tau; ebins equal restatement (a) of the kernel's own sbins."""
    case = SR.inexact_case(route, R, Sp, S)
    fused = route.startswith("fused")
    label = f"A {route} Sp={Sp} S={S} R={R}"
    ref = SR.reference(case, "uniform", SR.f64)
    u = SR.case_u(case, SR.f64)
    assert np.all(np.diff(u, axis=-1) >= 0)
    got = resample(case, "uniform", weights_out=True)
    plain = resample(case, "uniform", inds=False)
    assert np.array_equal(plain["sbins"].view(np.int32), got["sbins"].view(np.int32)) and np.array_equal(plain["ebins"].view(np.int32),
                                                                                                          got["ebins"].view(np.int32)), label
    bad = []
    if fused:
        w64 = SR.case_weights(case, SR.f64)
        d = SR.deviation(got["weights_out"], w64)
        scale = float(np.abs(w64).max())
        _measure.record("sampler.resample.weights_out", torch.from_numpy(got["weights_out"].astype(np.float64) / scale), torch.from_numpy(w64 / scale))
        print(f"{label} weights_out: deviation {d:.3e} (bound {SR.MARGIN * SR.E32['resample.weights_out']:.3e})")
        if not d <= SR.MARGIN * SR.E32["resample.weights_out"]:
            bad.append(("weights_out", d))
    ok = SR.index_within(got["inds"], ref["cdf"], u, SR.TAU)
    if not ok.all():
        bad.append(("indices outside cdf64 +- tau", int((~ok).sum())))
    inside = SR.bins_inside(got["inds"], got["sbins"], case["sbins_prev"])
    if not inside.all():
        bad.append(("edges outside the bin of their index", int((~inside).sum())))
    if not np.all(np.diff(got["sbins"], axis=-1) >= 0):
        bad.append(("edges decrease along a ray", int((np.diff(got["sbins"], axis=-1) < 0).sum())))
    back = SR.u_back(got["sbins"], case["sbins_prev"], ref["cdf"])
    d = float(np.abs(back - u).max())
    _measure.record("sampler.resample.u_back", torch.from_numpy(back), torch.from_numpy(u))
    print(f"{label} u_back: max |u_back - u| {d:.3e} (tau {SR.TAU:.3e})")
    if not d <= SR.TAU:
        bad.append(("u_back", d))
    same(label + " ebins of the kernel's sbins", got["ebins"], SR.to_euclidean(got["sbins"], case["nears"], case["fars"], "uniform"))
    assert not bad, f"{label}: {bad}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# snerf_weights_fwd, snerf_weights_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bounded(label, name, got, want, bad):
    d = SR.deviation(got, want)
    scale = float(np.abs(want).max()) or 1.0
    _measure.record(f"sampler.{name}", torch.from_numpy(np.asarray(got, dtype=np.float64) / scale), torch.from_numpy(want / scale))
    print(f"{label} {name}: deviation {d:.3e} (bound {SR.MARGIN * SR.E32[name]:.3e})")
    if not d <= SR.MARGIN * SR.E32[name]:
        bad.append((name, d, SR.MARGIN * SR.E32[name]))


@pytest.mark.parametrize("S,R", SR.WEIGHT_CASES)
def test_weights_entry_points_lattice(S, R):
    """weights and d/d density against float64 within 5 x E32; accumulate = 1 onto a prefill is the prefill plus the accumulate = 0 result bit for
    bit (one float32 add per element); the non-finite flag stays clear on finite inputs."""
    L, lib = _lib()
    c = SR.weights_case(R, S)
    d, e, g = dv(c["density"]), dv(c["ebins"]), dv(c["grad_weights"])
    label = f"weights S={S} R={R}"
    bad = []
    w = Out(R, S)
    L.check(lib.snerf_weights_fwd(ptr(d), ptr(e), R, S, w.p, _stream()), "weights_fwd")
    _bounded(label, "weights_fwd.weights", w.get("weights"), SR.get_weights(c["density"], c["ebins"], SR.f64), bad)
    want = SR.get_weights_grad(c["density"], c["ebins"], c["grad_weights"], SR.f64)
    prefill = SR.prefill_like(want, "weights_bwd", S, R)

    def call(accumulate):
        buf = Out(R, S, prefill=prefill) if accumulate else Out(R, S)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        L.check(lib.snerf_weights_bwd(ptr(d), ptr(e), ptr(g), R, S, buf.p, accumulate, ptr(flag), _stream()), "weights_bwd")
        out = buf.get("g_density")
        assert int(flag) == 0, f"{label}: the non-finite flag was set on finite inputs"
        return out

    plain, added = call(0), call(1)
    _bounded(label, "weights_bwd.g_density", plain, want, bad)
    same(label + " accumulate = 1", added, prefill + plain)
    buf = Out(R, S)  # the flag is optional
    L.check(lib.snerf_weights_bwd(ptr(d), ptr(e), ptr(g), R, S, buf.p, 0, None, _stream()), "weights_bwd")
    assert np.array_equal(buf.get("g_density").view(np.int32), plain.view(np.int32))
    assert not bad, f"{label}: {bad}"


@pytest.mark.parametrize("S,R", [(2, 5), (65, 3), (320, 133)])
def test_weights_bwd_flags_a_planted_overflow(S, R):
    """An infinite density on a zero-width bin (0 * inf) in the LAST ray: the flag is set, every gradient stays finite, the other rays' gradients
    are those of the clean call bit for bit, and rows behind R stay untouched."""
    L, lib = _lib()
    c = SR.weights_case(R, S)
    dens, eb = c["density"].copy(), c["ebins"].copy()
    k = S // 2
    dens[R - 1, k], eb[R - 1, k + 1] = np.inf, eb[R - 1, k]
    g = dv(c["grad_weights"])

    def call(density, ebins):
        d, e = dv(density), dv(ebins)
        buf, flag = Out(R, S), torch.zeros(1, dtype=torch.int32, device=DEV)
        L.check(lib.snerf_weights_bwd(ptr(d), ptr(e), ptr(g), R, S, buf.p, 0, ptr(flag), _stream()), "weights_bwd")
        return buf.get("g_density"), int(flag)

    clean, flag0 = call(c["density"], c["ebins"])
    planted, flag1 = call(dens, eb)
    assert flag0 == 0 and flag1 == 1
    assert np.isfinite(planted).all()
    assert np.array_equal(planted[: R - 1].view(np.int32), clean[: R - 1].view(np.int32))

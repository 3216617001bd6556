"""The MLP kernel family (csrc/mlp.hip, mlp_lp.hip, mlp_rows.hip, mlp_rows128.hip, dense_lp.hip) against EXACT answers.

The exactness argument
  1. Inputs are small integers, weights and upstream-gradient targets small dyadic numbers: every operand rounding the kernels perform (X, W,
     hidden activations, gradient tiles; to bf16, or to fp16 after the 8192 scale and the +-65504 clamp) is then the identity.
  2. Every accumulation (a layer product, a weight-gradient element over all N samples, a dense K block) sums terms that are multiples of one
     power of two u with sum |terms| / u < 2^24: every partial sum in any order is a multiple of u below 2^24 u, i.e. a float.  MFMA slot order,
     waves, float atomics, the 16 workspace replicas and the 2^50 fixed-point cells (|sum| < 2^13, u >= 2^-50) all give the same bits.
  3. A zero pre-activation is exactly zero in every implementation, so the ReLU mask is the same everywhere.
  4. A Sigmoid or trunc_exp head has a derivative that is not dyadic.  The incoming gradient is therefore built as float32(t / act'(z)) with t
     from the dyadic target set and z the exact raw output, so that the kernel's float32 product gY * act' is t (1 + e).  For the exp head e is a
     few float32 roundings plus the kernel's exp (the fast __expf at |z| <= 15 included): below 3e-6.  For Sigmoid the kernels form s (1 - s), and
     1 - s cancels: an error of k ulps in s (2^-24 k) is a relative error of 2^-24 k e^|z| in 1 - s.  Sigmoid columns therefore keep |z| <= 4
     (e^4 = 55): 3.3e-6 per ulp, 3.3e-5 for a fast exp and reciprocal that are 10 ulps off together.  The nearest rounding midpoint of the gradient
     tile is 2^-10 = 9.8e-4 relative away for bf16 (a power-of-two t, downward) and 2^-12 = 2.4e-4 for fp16 after the scale: a margin of 7 x for the
     Sigmoid under that pessimistic error and of 80 x for exp.  (At |z| <= 8 one ulp alone is 1.8e-4, too close to 2.4e-4: measured on the CPU with
     torch's float32 sigmoid before any kernel ran.)  The rounded tile is exactly t and everything downstream is exact again.  Where gY and gaux
     both reach the aux column, gY of that column is a dyadic value of the same sign as the gaux target (no cancellation that would leave the
     e-sized residue standing alone).
  5. So every kernel must return the bits of the float64 restatement below: one oracle, equality, no tolerance.
The generator ASSERTS 1, 2 and 4 in float64 for every case (`make_mlp`, `make_dense` raise otherwise).  The exact-fp32 kernels (operands = 0) round
nothing, so a head's product is not snapped back to t there.  Their heads are pinned in two ways.  EXACTLY, on rows whose raw head outputs are
exactly 0 (plant 'o'): sigmoid(0) = 1/2, s (1 - s) = 1/4 and exp(0) = 1 are exact in float32, so the whole backward is exact again (a derivative
formed as s, or a head that is skipped, changes the bits).  And BOUNDED, for the values no exact case reaches (the trunc_exp clamp at +-15 with
raw outputs +-16 planted, a Sigmoid at |z| <= 4): gX and gW against float64 within 5 x the float32 restatement's deviation, max |a - b| / max |b|
over the output (`is_bounded_backward`); a clamp moved to 16 changes the planted rows' gradient by a factor e.

Only the forward outputs behind a Sigmoid or exp are inexact; they are bounded by 5 x the float32 restatement's deviation from the float64 one
(profiles/r17_mlp_deviations.json, written by tools/measure_mlp_deviations.py).

Importable on the CPU; reads nothing outside the repository."""
import functools
import math
from collections import namedtuple

import torch

GS = 8192.0          # Ops<fp16>::GS: the power-of-two scale of the fp16 gradient tiles
FP16_MAX = 65504.0   # Ops<fp16>::cvt / cvtg clamp
F64 = torch.float64
_DT = {1: torch.bfloat16, 2: torch.float16}
TARGETS = (0.0, 1.0 / 16, -1.0 / 16)
ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1000)
GUARD_ROWS = 3


# ------------------------------------------------------------------------------------------------ roundings
def rd(t, operands):
    """Operand rounding (Ops<T>::cvt): identity, to bf16, or to fp16 with the +-65504 clamp."""
    if operands == 0:
        return t
    f = t.float()
    if operands == 2:
        f = f.clamp(-FP16_MAX, FP16_MAX)
    return f.to(_DT[operands]).to(t.dtype)


def rg(t, operands):
    """Gradient-tile rounding (Ops<T>::cvtg): fp16 tiles hold 8192 x the gradient, clamped to +-65504."""
    if operands == 0:
        return t
    if operands == 1:
        return t.float().to(torch.bfloat16).to(t.dtype)
    return (t * GS).float().clamp(-FP16_MAX, FP16_MAX).to(torch.float16).to(t.dtype) / GS


def unit(t):
    """The largest power of two that divides every entry of t (1.0 for an all-zero tensor)."""
    nz = t[t != 0].double()
    if nz.numel() == 0:
        return 1.0
    m, e = torch.frexp(nz)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    tz = torch.log2((mi & -mi).double())
    return 2.0 ** float((e.double() - 53 + tz).min())


def _round(fn, t, operands, name, trace):
    out = fn(t, operands)
    if trace is not None:
        pre = t.clamp(-FP16_MAX / GS, FP16_MAX / GS) if (operands == 2 and fn is rg) else t  # the clamp is part of the statement, not a rounding
        trace.append(("round", name, int((out != pre).sum())))
    return out


def _mm(A, B, name, trace):
    if trace is not None:
        u = unit(A) * unit(B)
        trace.append(("acc", name, float((A.abs() @ B.abs()).max()) / u))
        trace.append(("cell", name, float((A.abs() @ B.abs()).max()), u))
    return A @ B


def _sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def f32_bits(t):
    return t.detach().float().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ restatement
def restate(X, Ws, hidden_act, out_act, operands, gY=None, aux_col=-1, gaux=None, ldg=None, dtype=F64, trace=None):
    """Forward and backward of the bias-free MLP in `dtype`, rounding what the kernels round.  Ws: list of [in, out] matrices (the ABI's
    input-major layers).  Returns z (raw outputs), Y, aux, and with an incoming gradient g_out (the rounded output tile), gX, gW (flat), G = gX .* X
    and the quotient epilogue's fix set {(n * ldg + col, float32 bits of gX)} (X vanished, gX did not; G = 0 there)."""
    nh = len(Ws) - 1
    x = _round(rd, X.to(dtype), operands, "X", trace)
    W = [_round(rd, w.to(dtype), operands, f"W{l}", trace) for l, w in enumerate(Ws)]
    acts = [x]
    for l in range(nh):
        pre = _mm(acts[-1], W[l], f"layer{l}", trace)
        acts.append(_round(rd, torch.relu(pre) if hidden_act == 1 else pre, operands, f"act{l + 1}", trace))
    z = _mm(acts[-1], W[nh], "out", trace)
    out = {"z": z, "Y": _sigmoid(z) if out_act == 1 else z, "aux": torch.exp(z[:, aux_col]) if aux_col >= 0 else None, "acts": acts}
    if gY is None and gaux is None:
        return out
    g = torch.zeros_like(z)
    if gY is not None:
        g = gY.to(dtype) * (out["Y"] * (1.0 - out["Y"])) if out_act == 1 else gY.to(dtype).clone()
    if gaux is not None:
        g[:, aux_col] += gaux.to(dtype) * torch.exp(z[:, aux_col].clamp(-15.0, 15.0))  # trunc_exp's clamped backward
    g = rg(g, operands)  # a head's product is NOT a fixed point (it is t (1 + e)): make_mlp asserts that it rounds to t
    out["g_out"] = g
    if trace is not None and out_act == 0 and gaux is None:
        _round(rg, g, operands, "g_out", trace)
    gWs = [None] * (nh + 1)
    gWs[nh] = _mm(acts[nh].t(), g, f"gW{nh}", trace)
    for l in range(nh, 0, -1):
        g = _mm(g, W[l].t(), f"g_act{l}", trace)
        if hidden_act == 1:
            g = g * (acts[l] > 0)  # derivative 0 at 0
        out["g_hidden_pre_max"] = max(out.get("g_hidden_pre_max", 0.0), float(g.abs().max()))  # before cvtg's clamp
        g = _round(rg, g, operands, f"g{l}", trace)
        gWs[l - 1] = _mm(acts[l - 1].t(), g, f"gW{l - 1}", trace)
    gX = _mm(g, W[0].t(), "gX", trace)
    out["gX"] = gX
    out["gW"] = torch.cat([w.reshape(-1) for w in gWs])
    vanished = x == 0
    out["G"] = torch.where(vanished, torch.zeros_like(gX), gX * x)
    ld = X.shape[1] if ldg is None else ldg
    idx = (vanished & (gX != 0)).nonzero()
    bits = f32_bits(gX)[idx[:, 0], idx[:, 1]]
    out["fix"] = set(zip((idx[:, 0] * ld + idx[:, 1]).tolist(), bits.tolist()))
    return out


def restate_dense(X, W, act, operands, Y=None, gY=None, dtype=F64, trace=None):
    """One dense layer Y = act(X W) (act 0 none, 1 ReLU, 2 Sigmoid) and its backward FROM THE STORED OUTPUT Y: dZ = gY .* (Y > 0) or
    gY .* Y (1 - Y); gX = dZ W^T, gW = X^T dZ."""
    x = _round(rd, X.to(dtype), operands, "X", trace)
    w = _round(rd, W.to(dtype), operands, "W", trace)
    z = _mm(x, w, "XW", trace)
    out = {"z": z, "Y": torch.relu(z) if act == 1 else (_sigmoid(z) if act == 2 else z)}
    if gY is None:
        return out
    y = (out["Y"] if Y is None else Y).to(dtype)
    dz = gY.to(dtype)
    if act == 1:
        dz = dz * (y > 0)
    elif act == 2:
        dz = dz * y * (1.0 - y)
    dz = _round(rg, dz, operands, "dZ", trace)
    out["gX"] = _mm(dz, w.t(), "gX", trace)
    out["gW"] = _mm(x.t(), dz, "gW", trace).reshape(-1)
    return out


def check_trace(trace, what, cells=False):
    """Preconditions (a) and (b) of the module docstring; cells: also the range and grain of the 2^50 fixed-point cells of the weight gradients."""
    for rec in trace:
        if rec[0] == "round" and rec[2] != 0:
            raise AssertionError(f"{what}: {rec[2]} elements of {rec[1]} are not fixed points of the kernel's rounding")
        if rec[0] == "acc" and not rec[2] < 2.0 ** 24:
            raise AssertionError(f"{what}: accumulation {rec[1]} has sum |terms| / unit = {rec[2]:.3g} >= 2^24")
        if cells and rec[0] == "cell" and rec[1].startswith("gW") and not (rec[2] < 2.0 ** 13 and rec[3] >= 2.0 ** -50):
            raise AssertionError(f"{what}: {rec[1]} does not fit the fixed-point cells (sum {rec[2]:.3g}, unit {rec[3]:.3g})")


# ------------------------------------------------------------------------------------------------ exact cases
# An MLP case.  call: which entry point; aux: 0 none, 1 gaux only (gY = NULL), 2 gY and gaux; plant: '' or letters z (an all-zero input row, which is
# also a row whose hidden pre-activations are all exactly 0, with a non-zero upstream gradient), a (raw aux outputs exactly -16, -15, 15, 16),
# c (an upstream gradient of 16: the fp16 clamp acts on the output tile and, with two hidden layers, on the hidden gradient),
# o (every row's raw head outputs -- all columns under a Sigmoid, the aux column under the exp head -- are exactly 0: heads exact in float32);
# pattern: 'exact' (sparse circulant / dense dyadic weights, random integer inputs) or 'addr' (one-hot rows, weights whose magnitudes encode
# (row, column)); gw0: what the weight-gradient buffer starts at; null: '' or 'gX' / 'gW' passed as NULL; rows: SNERF_MLP_SIGMA_ROWS ('' unset, '0').
MlpCase = namedtuple("MlpCase", "call d_in hidden n_hidden d_out hidden_act out_act operands N ldx ldgy ldgx aux plant pattern gw0 null rows")
DenseCase = namedtuple("DenseCase", "call K M act operands N ldx ldy ldgy ldgx gw0")


def case_id(c):
    if isinstance(c, DenseCase):
        return f"{c.call}-{c.K}x{c.M}-act{c.act}-op{c.operands}-N{c.N}-ld{c.ldx}.{c.ldy}.{c.ldgy}.{c.ldgx}-gw{c.gw0:g}"
    return (f"{c.call}-{c.d_in}x{'x'.join([str(c.hidden)] * c.n_hidden)}x{c.d_out}-h{c.hidden_act}o{c.out_act}-op{c.operands}-N{c.N}-ld{c.ldx}.{c.ldgy}.{c.ldgx}"
            f"-aux{c.aux}-{c.plant or 'plain'}-{c.pattern}-gw{c.gw0:g}" + (f"-no{c.null}" if c.null else "") + (f"-rows{c.rows}" if c.rows else ""))


def _signs(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).to(F64) * 2 - 1


def _circulant(K, M, nnz, gen, mul=3):
    """[K, M] with +-1 in `nnz` rows of every column, rows (mul u + k K / nnz) mod K: for K = M = 64 that is also `nnz` per row."""
    nnz = min(nnz, K)
    step = K // nnz
    W = torch.zeros(K, M, dtype=F64)
    u = torch.arange(M)
    for k in range(nnz):
        W[(mul * u + k * step) % K, u] = _signs((M,), gen)
    return W


def _weights(c, gen):
    dims = [c.d_in] + [c.hidden] * c.n_hidden
    Ws = []
    for l in range(c.n_hidden):
        K, M = dims[l], dims[l + 1]
        i, j = torch.arange(K)[:, None], torch.arange(M)[None, :]
        if c.pattern == "addr" and l == 0:
            Ws.append(_signs((K, M), gen) * ((7 * i + 3 * j) % 61 + 1).to(F64))  # moduli incommensurate with the 16- and 32-wide fragments
        elif c.pattern == "addr":
            # second hidden layer: one entry per row and column at (7 + 3 j) mod K, magnitude 2^((5 i + 3 j) mod 3) -- a power of two, because the
            # activations behind it must stay 8-bit integers times a power of two (bf16); the first layer's magnitudes make every unit's value its own
            W1 = torch.zeros(K, M, dtype=F64)
            jj = torch.arange(M)
            ii = (7 + 3 * jj) % K
            W1[ii, jj] = _signs((M,), gen) * 2.0 ** ((5 * ii + 3 * jj) % 3).to(F64)
            Ws.append(W1)
        elif l == 0 and K <= 16:
            Ws.append(_signs((K, M), gen) * torch.where(torch.rand(K, M, generator=gen) < 0.5, 1.0, 0.5).to(F64))  # the densest exact pattern
        else:
            Ws.append(_circulant(K, M, 4, gen))
    H, D = c.hidden, c.d_out
    u, col = torch.arange(H)[:, None], torch.arange(D)[None, :]
    if c.pattern == "addr":
        Wo = _signs((H, D), gen) * ((5 * u + 3 * col) % (3 if c.n_hidden == 2 else 13) + 1).to(F64)
    else:
        nnz = 2 if ("o" in c.plant and c.out_act == 1) else max(4, min(16, H // D))  # 'o' under a Sigmoid: z = 0 on EVERY column must be frequent
        step = max(H // nnz, 1)
        Wo = torch.zeros(H, D, dtype=F64)
        for k in range(nnz):
            Wo[(torch.arange(D) + k * step) % H, torch.arange(D)] = _signs((D,), gen)
        if c.aux:  # the aux column takes 16 units: its raw output then ranges beyond +-16 at unit grain, so that +-15 and +-16 can be planted
            Wo[(D - 1 + torch.arange(16) * (H // 16)) % H, D - 1] = torch.tensor([1.0, -1.0] * 8, dtype=F64)[torch.randperm(16, generator=gen)]  # balanced
    Ws.append(Wo)
    return Ws


def _content_key(c):
    """What the tensors of a case depend on: not the call, the strides, the initial gW, the NULL arguments or the kernel switch."""
    return c._replace(call="fwd" if c.call == "fwd" else "", ldx=0, ldgy=0, ldgx=0, gw0=0.0, null="", rows="")


@functools.lru_cache(maxsize=None)
def _make_mlp(c):
    gen = torch.Generator().manual_seed(1000 * c.d_in + 10 * c.hidden + c.N % 997 + c.d_out)
    N, D = c.N, c.d_out
    aux_col = (D - 1) if c.aux else -1
    Ws = _weights(c, gen)
    # an aux head draws twice the rows and keeps those whose raw aux output lies in [-32, 32] (exp stays far from float32's overflow)
    pool = (2 * N + (32768 if "a" in c.plant else 64)) if c.aux else N
    if "o" in c.plant:  # rows are kept only where the raw head outputs are exactly 0
        assert (c.out_act == 1 or c.aux) and c.pattern == "exact" and not set(c.plant) & set("ac")
        pool = 64 * N + 8192
    if c.pattern == "addr":
        X = torch.zeros(pool, c.d_in, dtype=F64)
        X[torch.arange(pool), torch.arange(pool) % c.d_in] = 1.0  # one-hot, cycling through every input column, the last one included
    else:
        X = torch.randint(-2, 3, (pool, c.d_in), generator=gen).to(F64)
        X[torch.rand(pool, c.d_in, generator=gen) < 0.15] = 0.0  # vanished features for the quotient epilogue's fix list
    z = restate(X, Ws, c.hidden_act, 0, c.operands)["z"]
    # power-of-two scale of the output layer: |z| <= 4 on Sigmoid columns (module docstring, 4.); with an aux head the 90 % quantile of the
    # raw aux output near 16, so that the planted values +-15 and +-16 are values the pool reaches often
    if c.out_act == 1 or c.aux:
        zmax = float(z.abs().max()) if c.out_act == 1 else float(z[:, aux_col].abs().quantile(0.9))
        if zmax > 0:
            e = math.ceil(math.log2(zmax / 4.0)) if c.out_act == 1 else max(0, math.floor(math.log2(zmax / 16.0)))
            Ws[-1] = Ws[-1] * 2.0 ** -e
            z = z * 2.0 ** -e
    if c.aux or "o" in c.plant:
        ok = torch.ones(pool, dtype=torch.bool)
        if c.aux:
            ok &= z[:, aux_col].abs() <= 32.0
        if "o" in c.plant:
            ok &= (z == 0).all(1) if c.out_act == 1 else (z[:, aux_col] == 0)
        keep = ok.nonzero()[:, 0]
        if keep.numel() < N:
            raise AssertionError(f"{case_id(c)}: only {keep.numel()} of {pool} candidate rows keep the raw head outputs where the case wants them")
        cand = X
        X = X[keep[:N]].clone()
        if "a" in c.plant:
            assert N >= 16, "aux plants need 16 rows"
            for tgt, row in zip((-16.0, -15.0, 15.0, 16.0), (0, N // 3, N - 2, N - 1)):  # the tail row included
                hit = (z[:, aux_col] == tgt).nonzero()
                if hit.numel() == 0:
                    raise AssertionError(f"{case_id(c)}: no candidate row reaches a raw aux output of {tgt}")
                X[row] = cand[int(hit[0])]
    X = X[:N].clone()
    zero_row = N // 2
    if "z" in c.plant:
        X[zero_row] = 0.0
    z = restate(X, Ws, c.hidden_act, 0, c.operands)["z"]
    tset = torch.tensor(TARGETS, dtype=F64)
    T = tset[torch.randint(0, 3, (N, D), generator=gen)]
    Ta = tset[torch.randint(0, 3, (N,), generator=gen)]
    if "z" in c.plant:
        T[zero_row], Ta[zero_row] = 1.0 / 16, 1.0 / 16
    if "c" in c.plant:
        assert c.aux == 0 and c.out_act == 0 and N >= 2
        T[1] = 16.0
    if c.call == "fwd":  # forward only: the exact-fp32 kernels take heads here (their outputs are bounded, not exact), no gradient is built
        trace = []
        ref = restate(X, Ws, c.hidden_act, c.out_act, c.operands, aux_col=aux_col, trace=trace)
        check_trace(trace, case_id(c))
        return {"X": X, "Ws": Ws, "W": torch.cat([w.reshape(-1) for w in Ws]), "aux_col": aux_col, "ref": ref, "trace": trace}
    gY, gaux, target = None, None, torch.zeros(N, D, dtype=F64)
    if c.aux != 1:
        target += T
        gY = (T / (_sigmoid(z) * (1 - _sigmoid(z)))).float() if c.out_act == 1 else T.float()
    if c.aux:
        assert c.out_act == 0, "the aux head sits on a linear output"
        if c.aux == 2:
            Ta = torch.where(T[:, aux_col] * Ta < 0, -Ta, Ta)  # no cancellation between the two contributions
        target[:, aux_col] += Ta
        gaux = (Ta / torch.exp(z[:, aux_col].clamp(-15.0, 15.0))).float()
    trace = []
    if is_bounded_backward(c):  # not exact: the head's product is t (1 + e) and nothing rounds it back; only the forward's preconditions hold
        restate(X, Ws, c.hidden_act, c.out_act, c.operands, aux_col=aux_col, trace=trace)
        ref = restate(X, Ws, c.hidden_act, c.out_act, c.operands, gY, aux_col, gaux)
    else:
        ref = restate(X, Ws, c.hidden_act, c.out_act, c.operands, gY, aux_col, gaux, trace=trace)
    check_trace(trace, case_id(c))
    want = target.clamp(-FP16_MAX / GS, FP16_MAX / GS) if c.operands == 2 else target
    if "o" in c.plant:
        assert not bool(ref["z"].any() if c.out_act == 1 else ref["z"][:, aux_col].any()), case_id(c)
    if (c.operands != 0 or "o" in c.plant) and not torch.equal(ref["g_out"], want):
        raise AssertionError(f"{case_id(c)}: the rounded output-gradient tile is not the dyadic target in {int((ref['g_out'] != want).sum())} elements")
    if "a" in c.plant:
        assert sorted(set(ref["z"][:, aux_col].tolist()) & {-16.0, -15.0, 15.0, 16.0}) == [-16.0, -15.0, 15.0, 16.0]
    return {"X": X, "Ws": Ws, "W": torch.cat([w.reshape(-1) for w in Ws]), "gY": gY, "gaux": gaux, "aux_col": aux_col, "target": target, "ref": ref, "trace": trace}


def make_mlp(c):
    """Tensors (float64 X and weights, float32 gY / gaux as the kernel receives them) and the float64 restatement of an MlpCase.  Raises if a
    precondition of the exactness argument fails.  Cached: cases that differ only in call, strides or buffers share one reference."""
    m = _make_mlp(_content_key(c))
    if c.call.endswith("fx"):
        check_trace(m["trace"], case_id(c), cells=True)
    return m


def with_ldg(m, c, ldg):
    """Fix set and G for the row stride the quotient call uses."""
    return restate(m["X"], m["Ws"], c.hidden_act, c.out_act, c.operands, m["gY"], m["aux_col"], m["gaux"], ldg=ldg)


@functools.lru_cache(maxsize=None)
def _make_dense(c):
    gen = torch.Generator().manual_seed(77 * c.K + c.M + c.N % 997)
    X = torch.randint(-2, 3, (c.N, c.K), generator=gen).to(F64)
    W = _signs((c.K, c.M), gen) * torch.where(torch.rand(c.K, c.M, generator=gen) < 0.5, 1.0, 0.5).to(F64)
    if c.act == 2:
        # |z| <= 8.  The module docstring's |z| <= 4 guards a BACKWARD that forms s (1 - s) from its own forward; no dense case does: the Sigmoid
        # forward here is bounded, not exact, and the dense backward works from the stored dyadic Y below, whatever z is
        W = W / 2.0 ** math.ceil(math.log2(max(c.K, 2) * 2.0 / 8.0))
    tset = torch.tensor(TARGETS, dtype=F64)
    gY = tset[torch.randint(0, 3, (c.N, c.M), generator=gen)]
    fwd = restate_dense(X, W, c.act, c.operands)
    # the backward works from the STORED output, which the caller hands in: for Sigmoid a dyadic Y (y (1 - y) = 3/16 or 1/4 exactly), so that the
    # exact-fp32 kernels, which round nothing, are exact as well; for none / ReLU the forward's own exact output
    Y = torch.tensor([0.25, 0.5, 0.75], dtype=F64)[torch.randint(0, 3, (c.N, c.M), generator=gen)] if c.act == 2 else fwd["Y"]
    trace = []
    ref = restate_dense(X, W, c.act, c.operands, Y, gY, trace=trace)
    check_trace(trace, case_id(c))
    return {"X": X, "W": W, "Y": Y, "gY": gY, "ref": ref, "trace": trace}


def make_dense(c):
    m = _make_dense(c._replace(call="", ldx=0, ldy=0, ldgy=0, ldgx=0, gw0=0.0))
    if c.call.endswith("fx"):
        check_trace(m["trace"], case_id(c), cells=True)
    return m


# ------------------------------------------------------------------------------------------------ the lattice
# (padded d_in, hidden, n_hidden) of csrc/mlp.hip's SNERF_MLP_SHAPES (padding to 16) and csrc/mlp_lp.hip's SNERF_MLP_BF16_SHAPES (padding to 32);
# tests/test_mlp_reference_cpu.py checks the lattice against snerf_mlp_supported, so a shape added there without a case here fails the CPU suite.
FP32_SHAPES = ((16, 64, 1), (16, 64, 2), (32, 128, 1), (64, 128, 1), (96, 128, 1), (128, 128, 1), (160, 128, 1), (192, 128, 1), (32, 64, 1), (64, 64, 1),
               (128, 64, 1), (160, 64, 1), (16, 16, 1), (32, 64, 2), (48, 64, 2), (64, 64, 2))
LP_SHAPES = ((32, 64, 1), (32, 128, 1), (64, 128, 1), (96, 128, 1), (128, 128, 1), (160, 128, 1), (192, 128, 1), (32, 64, 2), (64, 64, 2))
# a ragged width per padding class where one exists below the padded width, else the padded width itself
RAGGED = {16: (8, 10, 15), 32: (20, 31), 48: (40,), 64: (50, 63), 96: (90,), 128: (120,), 160: (160,), 192: (192,)}
D_OUTS = (1, 3, 5, 16)


def padding_class(d_in, hidden, n_hidden, operands):
    pad = 16 if operands == 0 else 32
    return ((d_in + pad - 1) // pad * pad, hidden, n_hidden, operands)


# Smallest N at which a workgroup of a persistent grid walks a second tile, plus 1.  launch_persistent (csrc/mlp_args.hpp) starts
# min(256 * per_cu, n_tiles) workgroups, per_cu = min(cap, LDS_LIMIT / lds_bytes) >= 1, so with n_tiles = 256 * cap + 1 (N = 256 * cap * TS + 1)
# workgroup 0 walks tiles 0 and 256 * per_cu whatever the LDS plan allows, and where per_cu = cap that is the smallest such N.
#   fp32 backward / forward (mlp.hip)      cap 4, TS 64 (32 for the two-hidden-layer 64-wide nets: pick_ts)  -> 65 537
#   fp32 forward, weights in registers     cap 4, TS 64 (hidden 64, 16); cap 2, TS 16 (hidden 128)           -> 65 537 / 8 193
#   fp32 forward, two hidden layers        mlp_fwd_kernel<D0P, 64, 2>, a kernel of its own: cap 4, TS <= 64   -> 65 537 (fwd 15x64x64x3)
#   16-bit forward (mlp_lp.hip)            cap 4, TS 64 (hidden 64, one layer) / 32                          -> 65 537 / 32 769
#   16-bit tile backward, 64 wide          cap 2, TS 64 (launch_b_tr)                                        -> 32 769
#   16-bit tile backward, 128 wide         cap 4, TS 32 (fp32 X); cap 1, TS 64 or 32 (16-bit X)              -> 32 769 / 16 385
#   rows backward (mlp_rows.hip)           256 workgroups x 8 waves x one 32-row pair                        -> 65 537
#   rows128 backward (mlp_rows128.hip)     256 workgroups x one 128-row tile                                 -> 32 769
#   dense fp32 (mlp.hip)                   cap 2, TS 64                                                      -> 32 769
#   dense 16-bit (dense_lp.hip)            cap 2, TS 64                                                      -> 32 769
# Every entry below is >= its kernel's figure (a larger N only walks more second tiles); one case per kernel, not the whole product.
TWO_TILES = {"fp32": 65537, "lp_fwd": 65537, "tile64": 32769, "tile128": 32769, "x16_tile": 16385, "rows": 65537, "rows128": 32769, "dense": 32769, "dense_lp": 32769}


def _pad4(n):
    return (n + 3) // 4 * 4


def _odd_ld(n):
    """The smallest row stride >= n that is no multiple of 4."""
    return n if n % 4 else n + 1


def _mlp(call, d_in, hidden, nh, d_out, operands, N, *, ha=1, oa=0, ldx=None, ldgy=None, ldgx=None, aux=0, plant="", pattern="exact", gw0=0.0, null="", rows=""):
    return MlpCase(call, d_in, hidden, nh, d_out, ha, oa, operands, N, d_in if ldx is None else ldx, d_out if ldgy is None else ldgy,
                   d_in if ldgx is None else ldgx, aux, plant, pattern, gw0, null, rows)


def _deal(combos, per, start=0):
    """Pruning rule of the lattice: the full product of the axes is several hundred thousand cases, so inside a kernel family the row counts are DEALT
    over the family's (shape, operands) combinations -- combination i takes ROWS[start + per i], ..., ROWS[start + per i + per - 1] (cyclically), `per`
    chosen so that the family as a whole holds every row count and `start` differing between the families, so that every operand type meets every row count -- and the remaining axes (d_out, activations, strides, head, initial gW) rotate with the running
    index at strides coprime to their lengths, so that every value of every axis meets every kernel family, though not every other value."""
    k = 0
    for i, combo in enumerate(combos):
        for j in range(per):
            yield k, combo, ROWS[(start + per * i + j) % len(ROWS)]
            k += 1


def _per(n):
    return max(1, -(-len(ROWS) // n))


def _head(k, operands, allow_aux=True):
    """Rotates (out_act, aux): linear, Sigmoid, gaux only, gY + gaux (16-bit operands; the exact-fp32 kernels: `_head32`)."""
    assert operands != 0
    return ((0, 0), (1, 0), (0, 1), (0, 2))[k % (4 if allow_aux else 2)]


def _head32(k, d_out):
    """(out_act, aux, plant) of the exact-fp32 kernels' dealt backward cases: the same rotation, the heads on rows whose raw head outputs are exactly
    0 (plant 'o', module docstring).  A Sigmoid sits on EVERY column, and all of them vanish together often enough only for d_out <= 3."""
    oa, aux = ((0, 0), (1, 0), (0, 1), (0, 2))[k % 4]
    if oa and d_out > 3:
        oa = 0
    return oa, aux, "o" if (oa or aux) else ""


def is_bounded_backward(c):
    """Backward cases of the exact-fp32 kernels with a head away from z = 0: gX and gW are bounded (profiles/r17_mlp_deviations.json), not exact."""
    return isinstance(c, MlpCase) and c.call not in ("fwd", "cross") and c.operands == 0 and (c.out_act == 1 or c.aux != 0) and "o" not in c.plant


def _ragged(d0p, k):
    r = RAGGED[d0p]
    return r[k % len(r)]


def mlp_backward_cases():
    out = []
    # ---- exact-fp32 kernels (mlp.hip): every instantiated shape
    for k, (d0p, H, nh), N in _deal(FP32_SHAPES, _per(len(FP32_SHAPES))):
        d_in = _ragged(d0p, k)
        call = ("bwd", "bwd", "bwd_ws", "bwd_fx", "bwd_tile")[k % 5]
        oa, aux, plant = _head32(k + k // 4, D_OUTS[k % 4])  # k + k // 4: every head meets every d_out
        out.append(_mlp(call, d_in, H, nh, D_OUTS[k % 4], 0, N, oa=oa, aux=aux, plant=plant, ha=0 if k % 7 == 3 else 1, ldx=d_in + (k % 3 == 1),
                        ldgy=D_OUTS[k % 4] + 2 * (k % 2), ldgx=d_in + 3 * (k % 3 == 2), gw0=0.25 * (k % 4 == 1),
                        null=("", "", "", "gX", "gW")[k % 5] if call == "bwd" else ""))
    # the exact-fp32 heads away from z = 0 (bounded, `is_bounded_backward`): the trunc_exp clamp with raw aux outputs -16, -15, 15, 16 planted, gaux alone
    # and beside gY, and a Sigmoid at |z| <= 4; N = 257 and 1000, so that the float32 yardstick is taken over some thousand elements
    out.append(_mlp("bwd", 8, 64, 1, 1, 0, 257, aux=1, plant="a"))
    out.append(_mlp("bwd", 160, 128, 1, 16, 0, 257, aux=2, plant="a", ldgy=16))
    out.append(_mlp("bwd_ws", 15, 64, 2, 3, 0, 1000, aux=2, plant="a", ldx=16, ldgx=16))
    out.append(_mlp("bwd", 15, 64, 2, 3, 0, 1000, oa=1, ldx=16, ldgx=16))
    out.append(_mlp("bwd_tile", 90, 128, 1, 5, 0, 257, oa=1))
    # ---- rows backward (mlp_rows.hip): 64 hidden units, float4-granular fp32 rows
    rows_shapes = [(8, 1), (15, 2), (10, 1), (15, 1), (20, 1), (31, 1), (10, 2), (25, 1)]  # 16-bit operands: one hidden layer of 64 takes d_in <= 32
    combos = [(s, op) for op in (1, 2) for s in rows_shapes]
    for k, ((d_in, nh), op), N in _deal(combos, 2):
        oa, aux = _head(k, op)
        d_out = D_OUTS[(k + 1) % 4]
        call = ("bwd", "bwd_ws", "bwd", "bwd_fx")[k % 4]
        out.append(_mlp(call, d_in, 64, nh, d_out, op, N, oa=oa, aux=aux, ha=0 if k % 9 == 4 else 1, ldx=_pad4(d_in) + 4 * (k % 3 == 0), ldgy=d_out + (k % 2),
                        ldgx=d_in + (k % 3), gw0=0.25 * (k % 4 == 2), null=("", "gX", "gW")[k % 3] if call == "bwd" and k % 2 == 0 else ""))
    # the trainers' own layouts: color_net on h[:, :15] (stride 16), gX into gh[:, :15]; the proposal net with the density gradient through gaux only
    for op in (1, 2):
        out.append(_mlp("bwd", 15, 64, 2, 3, op, 1000, oa=1, ldx=16, ldgx=16, plant="z"))
        out.append(_mlp("bwd", 8, 64, 1, 1, op, 257, aux=1, plant="za"))
        out.append(_mlp("bwd_ws", 32, 64, 1, 16, op, 129, aux=2, plant="za"))
        out.append(_mlp("bwd", 15, 64, 2, 3, op, TWO_TILES["rows"], oa=1, ldx=16, ldgx=16))
    out.append(_mlp("bwd", 15, 64, 2, 3, 2, 65, plant="zc"))
    out.append(_mlp("bwd", 8, 64, 1, 5, 2, 33, plant="c"))
    # ---- 64-wide workgroup-tile backward (mlp_lp.hip, transposed reads): snerf_mlp_bwd_tile, the two-hidden-layer nets wider than 16 inputs, and
    # an ldx that is no multiple of 4 (which must take this kernel and give the same bits)
    tile_shapes = [(15, 2), (8, 1), (31, 2), (63, 2), (20, 1), (50, 2)]
    combos = [(s, op) for op in (1, 2) for s in tile_shapes]
    for k, ((d_in, nh), op), N in _deal(combos, 2, 5):
        oa, aux = _head(k + 1, op)
        d_out = D_OUTS[(k + 2) % 4]
        call = ("bwd_tile", "bwd_tile", "bwd") [k % 3] if (nh == 1 or d_in <= 16) else ("bwd", "bwd_ws", "bwd_fx", "bwd_tile")[k % 4]
        ldx = _odd_ld(d_in) if call == "bwd" and (nh == 1 or d_in <= 16) else d_in + (k % 2)
        out.append(_mlp(call, d_in, 64, nh, d_out, op, N, oa=oa, aux=aux, ldx=ldx, ldgy=d_out + 3 * (k % 2), ldgx=d_in + (k % 4 == 1), gw0=0.25 * (k % 4 == 3)))
    for op in (1, 2):
        out.append(_mlp("bwd_tile", 15, 64, 2, 3, op, TWO_TILES["tile64"], oa=1, ldx=16, ldgx=16))
        out.append(_mlp("bwd", 15, 64, 2, 3, op, 500, oa=1, ldx=15, ldgx=15, plant="z"))  # ldx = 15: not float4-granular
    out.append(_mlp("bwd_tile", 63, 64, 2, 3, 2, 64, plant="zc"))
    # ---- 128-wide workgroup-tile backward from fp32 X (mlp_lp.hip)
    wide = [32, 64, 96, 128, 160, 192]
    combos = [(d0p, op) for op in (1, 2) for d0p in wide]
    for k, (d0p, op), N in _deal(combos, 2, 11):
        d_in = _ragged(d0p, k)
        oa, aux = _head(k + 2, op)
        d_out = D_OUTS[(k + 3) % 4]
        call = ("bwd", "bwd_ws", "bwd_fx", "bwd", "bwd_tile")[k % 5]
        out.append(_mlp(call, d_in, 128, 1, d_out, op, N, oa=oa, aux=aux, ha=0 if k % 8 == 5 else 1, ldx=d_in + (k % 3), ldgy=d_out + (k % 2), ldgx=d_in + 2 * (k % 2),
                        gw0=0.25 * (k % 4 == 0), null=("", "gW", "gX")[k % 3] if call == "bwd" and k % 2 == 1 else ""))
    out.append(_mlp("bwd", 160, 128, 1, 16, 1, TWO_TILES["tile128"], aux=2))
    out.append(_mlp("bwd", 120, 128, 1, 16, 2, 129, plant="zc"))
    # ---- sigma_net from the 16-bit feature tile: rows128 (default; ldgy = 16) and the workgroup-tile kernel (SNERF_MLP_SIGMA_ROWS=0), plain and quotient
    for fam, (calls, rows_env) in enumerate(((("bwd_x16", "quot", "quot_ws", "quot"), ""), (("bwd_x16", "quot", "quot", "quot_ws"), "0"))):
        for k, (d_in, op), N in _deal(combos, 2, 3 + 5 * fam):
            oa, aux = _head(k + fam, op)
            d_out = (16, 16, 5, 16, 3, 1)[k % 6]
            call = calls[k % 4]
            ldg = d_in + 4 * (k % 3 == 1) if call != "bwd_x16" else d_in + (k % 3)
            out.append(_mlp(call, d_in, 128, 1, d_out, op, N, oa=oa, aux=aux, ldx=d_in + 8 * (k % 2), ldgy=16 if rows_env == "" or k % 2 else d_out, ldgx=ldg,
                            gw0=0.25 * (k % 4 == 1), rows=rows_env))
    for op in (1, 2):  # the trainer's layout: column 15 = log density through gaux, ldx = d_in + 8
        out.append(_mlp("quot", 160, 128, 1, 16, op, 1000, aux=2, ldx=168, ldgy=16, plant="za"))
        out.append(_mlp("quot_ws", 192, 128, 1, 16, op, 257, aux=2, ldx=200, ldgy=16, plant="za", rows="0"))
        out.append(_mlp("bwd_x16", 32, 128, 1, 16, op, 129, aux=1, ldgy=16, plant="za"))
    out.append(_mlp("quot", 160, 128, 1, 16, 1, TWO_TILES["rows128"], aux=2, ldx=168, ldgy=16))
    out.append(_mlp("bwd_x16", 64, 128, 1, 16, 2, TWO_TILES["rows128"], ldgy=16))
    out.append(_mlp("quot", 96, 128, 1, 16, 1, TWO_TILES["x16_tile"], aux=2, ldgy=16, rows="0"))
    out.append(_mlp("bwd_x16", 64, 128, 1, 16, 2, 255, ldgy=16, plant="zc"))
    out.append(_mlp("bwd_x16", 64, 128, 1, 16, 2, 255, ldgy=16, plant="zc", rows="0"))
    # ---- address cases: a transposed, shifted or wrongly permuted fragment shows as a wrong number at a known place
    for op in (1, 2):
        out.append(_mlp("bwd", 15, 64, 2, 3, op, 130, ldx=16, ldgx=16, pattern="addr"))
        out.append(_mlp("bwd_tile", 15, 64, 2, 3, op, 130, ldx=16, ldgx=16, pattern="addr"))
        out.append(_mlp("bwd", 8, 64, 1, 1, op, 67, pattern="addr"))
        out.append(_mlp("bwd", 31, 64, 1, 16, op, 200, ldx=32, pattern="addr"))
        out.append(_mlp("bwd", 63, 64, 2, 3, op, 131, pattern="addr"))
        out.append(_mlp("bwd", 160, 128, 1, 16, op, 330, pattern="addr"))
        out.append(_mlp("bwd_x16", 160, 128, 1, 16, op, 330, ldgy=16, pattern="addr"))
        out.append(_mlp("quot", 192, 128, 1, 16, op, 400, ldgy=16, pattern="addr"))
        out.append(_mlp("bwd_x16", 96, 128, 1, 16, op, 200, ldgy=16, pattern="addr", rows="0"))
    out.append(_mlp("bwd", 15, 64, 2, 3, 0, 130, pattern="addr"))
    out.append(_mlp("bwd", 160, 128, 1, 16, 0, 330, pattern="addr"))
    out.append(_mlp("bwd", 63, 64, 2, 3, 0, 131, pattern="addr"))
    out.append(_mlp("bwd", 160, 128, 1, 16, 0, TWO_TILES["fp32"]))
    out.append(_mlp("bwd", 15, 64, 2, 3, 0, TWO_TILES["fp32"], plant="z"))
    return out


def mlp_forward_cases():
    """snerf_mlp_fwd: every instantiated shape and operand type; linear outputs are exact, Sigmoid outputs and aux_out are bounded."""
    out = []
    combos = [(s, 0) for s in FP32_SHAPES] + [(s, op) for s in LP_SHAPES for op in (1, 2)]
    # A bounded output's yardstick is the float32 restatement's WORST deviation over the case's own elements.  Over a handful of elements that worst
    # figure is whatever those few draws give (1e-10 on one N = 1 case: every float32 activation happened to round as float64 did), which says nothing
    # about float32; over >= 1000 elements it is the 0.5 - 1.5 ulp of the float32 formula.  So the dealt row counts run with LINEAR heads (exact, every
    # N), and every combination adds one head case (Sigmoid, aux_out in turn) at N in {255, 257, 1000} with at least 1000 bounded elements.
    for k, ((d0p, H, nh), op), N in _deal(combos, 2):
        d_in = (8, 15, 20, 31)[k % 4] if (op and d0p == 32) else _ragged(d0p, k)
        d_out = D_OUTS[k % 4]
        out.append(_mlp("fwd", d_in, H, nh, d_out, op, N, ha=0 if k % 10 == 7 else 1, ldx=d_in + (k % 3), ldgy=d_out + 2 * (k % 2)))
    for k, ((d0p, H, nh), op) in enumerate(combos):
        d_in = (15, 8, 31, 20)[k % 4] if (op and d0p == 32) else _ragged(d0p, k + 1)
        oa, aux = ((1, 0), (0, 1))[k % 2]
        d_out = (16, 5, 3, 16)[k % 4] if oa else (16, 1, 5, 3)[k % 4]
        N = 1000 if (d_out < 5 or aux) else (255, 257, 1000)[k % 3]
        out.append(_mlp("fwd", d_in, H, nh, d_out, op, N, oa=oa, aux=aux, ldx=d_in + (k % 2), ldgy=d_out + (k % 3)))
    out.append(_mlp("fwd", 160, 128, 1, 16, 0, TWO_TILES["fp32"], aux=1))
    out.append(_mlp("fwd", 8, 64, 1, 1, 0, TWO_TILES["fp32"], aux=1))
    out.append(_mlp("fwd", 8, 64, 1, 1, 1, TWO_TILES["lp_fwd"], aux=1))
    out.append(_mlp("fwd", 160, 128, 1, 16, 2, TWO_TILES["lp_fwd"], aux=1, plant="a"))
    out.append(_mlp("fwd", 15, 64, 2, 3, 1, TWO_TILES["lp_fwd"], oa=1, ldx=16))
    out.append(_mlp("fwd", 15, 64, 2, 3, 0, TWO_TILES["fp32"], ldx=16))  # mlp_fwd_kernel<D0P, 64, 2>: not the weights-in-registers forward
    out.append(_mlp("fwd", 15, 64, 2, 3, 0, 130, ldx=16, pattern="addr"))
    out.append(_mlp("fwd", 160, 128, 1, 16, 1, 330, pattern="addr"))
    return out


DENSE_FP32 = ((160, 1), (3, 128), (128, 480), (300, 200), (256, 256))  # K and M blocks of 128: (300, 200) is 3 x 2 blocks with ragged last ones
DENSE_LP = ((33, 64), (64, 32), (128, 128), (1, 1))


def dense_cases():
    out = []
    combos = [(s, act, 0) for s in DENSE_FP32 for act in (0, 1, 2)] + [(s, act, 1) for s in DENSE_LP for act in (0, 1, 2)]
    for k, ((K, M), act, op), N in _deal(combos, 2):
        ld = dict(ldx=K + (k % 3), ldy=M + (k % 2), ldgy=M + 2 * (k % 2), ldgx=K + (k % 4 == 1))
        # a Sigmoid forward is bounded, not exact: at least 1000 elements behind its yardstick (see mlp_forward_cases)
        Nf = N if (act != 2 or N * M >= 1000) else (1000 if M < 4 else (255, 257, 1000)[k % 3])
        out.append(DenseCase("fwd", K, M, act, op, Nf, gw0=0.0, **ld))
        out.append(DenseCase(("bwd", "bwd_fx", "bwd_nogx", "bwd_nogw")[k % 4], K, M, act, op, N, gw0=0.25 * (k % 3 == 1), **ld))
    out.append(DenseCase("bwd", 300, 200, 1, 0, TWO_TILES["dense"], 300, 200, 200, 300, 0.0))
    out.append(DenseCase("fwd", 300, 200, 2, 0, TWO_TILES["dense"], 300, 200, 200, 300, 0.0))
    out.append(DenseCase("bwd", 128, 128, 1, 1, TWO_TILES["dense_lp"], 128, 128, 128, 128, 0.0))
    out.append(DenseCase("fwd", 33, 64, 2, 1, TWO_TILES["dense_lp"], 33, 64, 64, 33, 0.0))
    return out


def cross_kernel_cases():
    """Nets whose backward is run through snerf_mlp_bwd, _bwd_tile, (_bwd_x16) and with fp32 operands: identical gX and gW bits."""
    return [_mlp("cross", 15, 64, 2, 3, 1, 257, ldx=16, ldgx=16), _mlp("cross", 8, 64, 1, 1, 2, 129), _mlp("cross", 32, 64, 1, 16, 1, 65),
            _mlp("cross", 160, 128, 1, 16, 1, 257, ldgy=16), _mlp("cross", 64, 128, 1, 16, 2, 33, ldgy=16), _mlp("cross", 63, 64, 2, 3, 2, 127, ldx=64),
            # heads on rows with raw head outputs exactly 0: exact for the fp32-operand leg as well
            _mlp("cross", 15, 64, 2, 1, 1, 129, oa=1, plant="o", ldx=16, ldgx=16), _mlp("cross", 32, 128, 1, 16, 2, 65, aux=2, plant="o", ldgy=16)]


def needs_bound(c):
    """Cases with an inexact output, which therefore need a yardstick: forward cases behind a Sigmoid or an exp head (Y, aux: elementwise),
    and the bounded backward cases of the exact-fp32 kernels (gX, gW: max-norm, `is_bounded_backward`)."""
    if isinstance(c, DenseCase):
        return c.call == "fwd" and c.act == 2
    return is_bounded_backward(c) or (c.call == "fwd" and (c.out_act == 1 or c.aux != 0))


def deviation(a32, b64):
    """Worst elementwise relative deviation of a float32 evaluation from the float64 one."""
    b = b64.double()
    return float(((a32.double() - b).abs() / b.abs()).max())


def norm_deviation(a32, b64):
    """max |a - b| / max |b| over an output: the measure of the bounded backward cases, whose elements are sums that may cancel."""
    b = b64.double()
    return float((a32.double() - b).abs().max() / b.abs().max())


def backward_deviations(c):
    """{gX, gW: deviation of the float32 restatement from the float64 one} for a bounded backward case (`is_bounded_backward`)."""
    m = make_mlp(c)
    r32 = restate(m["X"], m["Ws"], c.hidden_act, c.out_act, c.operands, m["gY"], m["aux_col"], m["gaux"], dtype=torch.float32)
    return {"gX": norm_deviation(r32["gX"], m["ref"]["gX"]), "gW": norm_deviation(r32["gW"], m["ref"]["gW"])}


def case_deviations(c):
    """{output name: deviation of the float32 restatement from the float64 one} for a case that needs a bound (`needs_bound`): the worst
    elementwise relative deviation for forward outputs, `norm_deviation` for gX and gW of a bounded backward case."""
    if is_bounded_backward(c):
        return backward_deviations(c)
    if isinstance(c, DenseCase):
        m = make_dense(c)
        return {"Y": deviation(restate_dense(m["X"], m["W"], c.act, c.operands, dtype=torch.float32)["Y"], m["ref"]["Y"])}
    m = make_mlp(c)
    r32 = restate(m["X"], m["Ws"], c.hidden_act, c.out_act, c.operands, aux_col=m["aux_col"], dtype=torch.float32)
    out = {}
    if c.out_act == 1:
        out["Y"] = deviation(r32["Y"], m["ref"]["Y"])
    if c.aux:
        out["aux"] = deviation(r32["aux"], m["ref"]["aux"])
    return out

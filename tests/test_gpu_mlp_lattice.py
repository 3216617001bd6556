"""The MLP kernel family against exact answers (tests/mlp_reference.py): snerf_mlp_fwd, snerf_mlp_bwd and its _tile, _ws (+ snerf_mlp_gw_reduce),
_fx, _x16 and quotient forms, and the dense layers, through the C ABI.

Every case is built so that every rounding the kernels perform is the identity and every accumulation is exact in any order (the generator asserts
both in float64), so every comparison below is an EQUALITY with the float64 restatement: gX, G, gW (plain atomics, workspace + reduce, fixed-point
cells x 2^-50), the fix list as a set of (index, gradient bits) pairs, Y of linear outputs.  The only bounds are those of the forward outputs behind
a Sigmoid or an exp, and gX / gW of the five backward cases of the exact-fp32 kernels whose head sits away from a raw output of 0
(mlp_reference.is_bounded_backward; those kernels round nothing, so nothing snaps the head's product back to its dyadic target): 5 x the float32
restatement's deviation from float64, per case, from profiles/r17_mlp_deviations.json.

Buffers: every output has guard rows behind row N and pad columns beyond its width holding 7.0, which must be intact afterwards; the pad columns of
inputs hold 1.0e4 and their guard rows NaN; weight-gradient buffers start at zero or at 0.25 (ACCUMULATED) and end in sentinel cells; a workspace
starts at zero, or, where gW starts at 0.25, with 0.125 in every replica (an earlier launch's share, which the reduce must fold in as well)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import mlp_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, PAD, GR, TAIL = 7.0, 1.0e4, R.GUARD_ROWS, 64
_X16 = {1: torch.bfloat16, 2: torch.float16}

with open(os.path.join(ROOT, "profiles", "r17_mlp_deviations.json")) as _f:
    BOUNDS = json.load(_f)["cases"]


def _in(t, ld, dtype=torch.float32):
    """[N, w] -> device [N + GR, ld]: pad columns 1.0e4, guard rows NaN."""
    N, w = t.shape
    b = torch.full((N + GR, ld), PAD, dtype=dtype)
    b[:N, :w] = t.to(dtype)
    b[N:] = float("nan")
    return b.to(DEV)


def _in_vec(t):
    b = torch.full((t.numel() + GR,), float("nan"))
    b[:t.numel()] = t.float()
    return b.to(DEV)


def _out(N, ld):
    return torch.full((N + GR, ld), SENT, device=DEV)


def _flat(n, start, dtype=torch.float32):
    b = torch.full((n + TAIL,), 7 if dtype == torch.int64 else SENT, dtype=dtype, device=DEV)
    b[:n] = start
    return b


WS0 = 0.125  # what every replica of a workspace holds on entry in the cases whose gW starts at 0.25


def _workspace(L, d, P, start):
    """The 16-replica workspace of snerf_mlp_bwd_ws.  The ABI wants it zero before the FIRST use and lets launches ACCUMULATE into it until one
    snerf_mlp_gw_reduce folds it: a workspace that holds an earlier launch's share is a valid input, so the cases that start gW at 0.25 also start
    the flat-gradient part of every replica at 0.125 (the reduce must add 16 x 0.125 = 2.0 on top, exactly).  The padding between the replicas
    (stride - P floats) stays zero: the reduce neither reads nor clears it."""
    n = int(L.snerf_mlp_gw_workspace_floats(C.byref(d)))
    ws = _flat(n, 0.0)
    if start:
        assert n % 16 == 0 and n // 16 >= P
        ws[:n].view(16, n // 16)[:, :P] = start
    return ws


def _same(got, want, cid, what):
    """Equality of a device result with the float64 restatement (which must itself be a float32 value)."""
    w32 = want.float()
    assert torch.equal(w32.double(), want.double()), f"{cid}: the restatement's {what} is not a float32 value"
    got = got.detach().cpu().double()
    w32 = w32.double()
    if torch.equal(got, w32):
        return
    diff = got != w32
    first = diff.reshape(got.shape).nonzero()[0].tolist()
    i = tuple(first)
    raise AssertionError(f"{cid}: {what} differs in {int(diff.sum())} of {got.numel()} elements; first at {first}: kernel {float(got[i])!r}, restatement {float(w32[i])!r}")


def _guards(buf, N, w, cid, what):
    """Guard rows behind row N and pad columns beyond the width still hold the sentinel."""
    assert bool((buf[N:] == SENT).all()), f"{cid}: {what}: guard rows behind row {N} were written"
    if buf.dim() == 2 and buf.shape[1] > w:
        assert bool((buf[:N, w:] == SENT).all()), f"{cid}: {what}: pad columns beyond {w} were written"


def _desc(c, operands=None):
    from soccernerfs_amd import _lib

    d = _lib.MlpDesc()
    d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act = c.d_in, c.hidden, c.n_hidden, c.d_out, c.hidden_act, c.out_act
    d.operands = c.operands if operands is None else operands
    return d


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Env:
    """SNERF_MLP_SIGMA_ROWS as the case wants it ('' = unset) for the length of the call; the value it had on entry is put back."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.old = os.environ.get("SNERF_MLP_SIGMA_ROWS")
        if self.rows:
            os.environ["SNERF_MLP_SIGMA_ROWS"] = self.rows
        else:
            os.environ.pop("SNERF_MLP_SIGMA_ROWS", None)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("SNERF_MLP_SIGMA_ROWS", None)
        else:
            os.environ["SNERF_MLP_SIGMA_ROWS"] = self.old


def _run_backward(c, m, call=None, operands=None, sync=True):
    """One backward call of case c on the tensors m; returns what it left behind (one synchronisation, or the caller's)."""
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    call = call or c.call
    d = _desc(c, operands)
    assert L.snerf_mlp_supported(C.byref(d)), R.case_id(c)
    N, P = c.N, m["W"].numel()
    x16 = call in ("bwd_x16", "quot", "quot_ws")
    W = m["W"].float().to(DEV)
    X = _in(m["X"], c.ldx, _X16[d.operands] if x16 else torch.float32)
    gY = _in(m["gY"], c.ldgy) if m["gY"] is not None else None
    gaux = _in_vec(m["gaux"]) if m["gaux"] is not None else None
    gX = None if c.null == "gX" else _out(N, c.ldgx)
    res = {"gX": gX}
    st = ops._stream()
    head = (C.byref(d), _p(W), _p(X), c.ldx, C.c_int64(N), _p(gY), c.ldgy, m["aux_col"], _p(gaux))
    with _Env(c.rows):
        if call in ("bwd", "bwd_tile", "bwd_x16"):
            gW = None if c.null == "gW" else _flat(P, c.gw0)
            fn = {"bwd": L.snerf_mlp_bwd, "bwd_tile": L.snerf_mlp_bwd_tile, "bwd_x16": L.snerf_mlp_bwd_x16}[call]
            _lib.check(fn(*head, _p(gX), c.ldgx, _p(gW), st), call)
            res["gW"] = gW
        elif call == "bwd_ws":
            ws = _workspace(L, d, P, WS0 if c.gw0 else 0.0)
            gW = _flat(P, c.gw0)
            _lib.check(L.snerf_mlp_bwd_ws(*head, _p(gX), c.ldgx, _p(ws), st), call)
            _lib.check(L.snerf_mlp_gw_reduce(C.byref(d), _p(ws), _p(gW), st), "gw_reduce")
            res["gW"], res["ws"] = gW, ws
        elif call == "bwd_fx":
            fx = _flat(P, int(c.gw0 * 2 ** 50), torch.int64)
            _lib.check(L.snerf_mlp_bwd_fx(*head, _p(gX), c.ldgx, _p(fx), st), call)
            res["fx"] = fx
        else:  # the quotient epilogue: G and the fix list instead of gX
            want = R.with_ldg(m, c, c.ldgx)
            cap = len(want["fix"]) + 8
            fl = torch.full((2 * cap + TAIL,), -1, dtype=torch.int32, device=DEV)
            # with the other counter given the kernel resets THAT one and fix_count is 0 on entry; without it fix_count is reset here
            two = c.N % 2 == 1
            cnt = torch.tensor([0, 5] if two else [9, 5], dtype=torch.int32, device=DEV)
            tail = (_p(gX), c.ldgx, _p(fl), cap, _p(cnt[0:1]), _p(cnt[1:2]) if two else None)
            if call == "quot":
                gW = _flat(P, c.gw0)
                _lib.check(L.snerf_mlp_bwd_x16_quotient(*head, *tail, _p(gW), st), call)
            else:
                ws = _workspace(L, d, P, WS0 if c.gw0 else 0.0)
                gW = _flat(P, c.gw0)
                _lib.check(L.snerf_mlp_bwd_x16_quotient_ws(*head, *tail, _p(ws), st), call)
                _lib.check(L.snerf_mlp_gw_reduce(C.byref(d), _p(ws), _p(gW), st), "gw_reduce")
                res["ws"] = ws
            res.update(gW=gW, fl=fl, cnt=cnt, cap=cap, two=two, want=want)
    if sync:
        torch.cuda.synchronize()
    return res


def _norm_bounded(got, want64, cid, what):
    """max |kernel - float64| / max |float64| <= 5 x the float32 restatement's same figure (the exact-fp32 kernels' heads away from z = 0)."""
    bound = 5.0 * BOUNDS[cid][what]
    dev = float((got.detach().cpu().double() - want64).abs().max() / want64.abs().max())
    print(f"{cid} {what} deviation {dev:.3e} / bound {bound:.3e}")
    assert dev <= bound, f"{cid}: {what} deviates {dev:.3e} from float64, bound {bound:.3e}"


def _check_backward(c, m, res, cid):
    N, P = c.N, m["W"].numel()
    ref = res.get("want", m["ref"])
    same = _norm_bounded if R.is_bounded_backward(c) else _same  # the only inexact backward cases; their ids are in the yardstick file
    if res["gX"] is not None:
        same(res["gX"][:N, :c.d_in], ref["G"] if "fl" in res else ref["gX"], cid, "G" if "fl" in res else "gX")
        _guards(res["gX"], N, c.d_in, cid, "gX")
    if res.get("gW") is not None:
        same(res["gW"][:P], ref["gW"] + c.gw0 + (16 * WS0 if "ws" in res and c.gw0 else 0.0), cid, "gW")
        assert bool((res["gW"][P:] == SENT).all()), f"{cid}: cells behind gW were written"
    if "ws" in res:
        n = res["ws"].numel() - TAIL
        assert not bool(res["ws"][:n].any()), f"{cid}: the workspace is not zero after the reduce"
        assert bool((res["ws"][n:] == SENT).all()), f"{cid}: cells behind the workspace were written"
    if "fx" in res:
        _same(res["fx"][:P].double() * 2.0 ** -50, ref["gW"] + c.gw0, cid, "gW (fixed-point cells x 2^-50)")
        assert bool((res["fx"][P:] == 7).all()), f"{cid}: cells behind the fixed-point cells were written"
    if "fl" in res:
        cnt, n = res["cnt"].cpu().tolist(), len(ref["fix"])
        assert cnt[0] == n, f"{cid}: fix_count {cnt[0]}, restatement {n}"
        assert cnt[1] == (0 if res["two"] else 5), f"{cid}: the other counter is {cnt[1]}"
        ent = res["fl"][:2 * n].view(n, 2).cpu()
        got = set(zip(ent[:, 0].tolist(), ent[:, 1].tolist()))
        assert got == ref["fix"], f"{cid}: fix list differs in {len(got ^ ref['fix'])} entries, e.g. {sorted(got ^ ref['fix'])[:3]}"
        assert bool((res["fl"][2 * n:] == -1).all()), f"{cid}: entries behind the fix list were written"


BACKWARD = R.mlp_backward_cases()
FORWARD = R.mlp_forward_cases()
DENSE = R.dense_cases()
CROSS = R.cross_kernel_cases()


@pytest.mark.parametrize("c", BACKWARD, ids=R.case_id)
def test_mlp_backward_is_exact(c):
    cid = R.case_id(c)
    m = R.make_mlp(c)
    _check_backward(c, m, _run_backward(c, m), cid)


def _bounded(got, want64, cid, what):
    """Elementwise |kernel - float64| <= 5 x the float32 restatement's worst relative deviation on the same case."""
    bound = 5.0 * BOUNDS[cid][what]
    rel = ((got.detach().cpu().double() - want64).abs() / want64.abs()).max()
    print(f"{cid} {what} deviation {float(rel):.3e} / bound {bound:.3e}")
    assert float(rel) <= bound, f"{cid}: {what} deviates {float(rel):.3e} from float64, bound {bound:.3e}"


@pytest.mark.parametrize("c", FORWARD, ids=R.case_id)
def test_mlp_forward(c):
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    cid = R.case_id(c)
    m = R.make_mlp(c)
    d = _desc(c)
    assert L.snerf_mlp_supported(C.byref(d)), cid
    N, ldy = c.N, c.ldgy
    W, X = m["W"].float().to(DEV), _in(m["X"], c.ldx)
    Y = _out(N, ldy)
    aux = torch.full((N + GR,), SENT, device=DEV) if c.aux else None
    _lib.check(L.snerf_mlp_fwd(C.byref(d), _p(W), _p(X), c.ldx, C.c_int64(N), _p(Y), ldy, m["aux_col"], _p(aux), ops._stream()), "mlp_fwd")
    torch.cuda.synchronize()
    ref = m["ref"]
    if c.out_act == 1:
        _bounded(Y[:N, :c.d_out], ref["Y"], cid, "Y")
    else:
        _same(Y[:N, :c.d_out], ref["Y"], cid, "Y")
    _guards(Y, N, c.d_out, cid, "Y")
    if c.aux:
        _bounded(aux[:N], ref["aux"], cid, "aux")
        _guards(aux, N, 1, cid, "aux_out")


@pytest.mark.parametrize("c", DENSE, ids=R.case_id)
def test_dense_layer(c):
    from soccernerfs_amd import _lib, ops

    L = _lib.lib()
    cid = R.case_id(c)
    m = R.make_dense(c)
    ref = m["ref"]
    N, K, M = c.N, c.K, c.M
    if c.operands:
        assert L.snerf_dense_lp_supported(K, M, c.operands), cid
    W, X, st = m["W"].float().to(DEV), _in(m["X"], c.ldx), ops._stream()
    if c.call == "fwd":
        Y = _out(N, c.ldy)
        if c.operands:
            _lib.check(L.snerf_dense_fwd_lp(_p(W), K, M, c.act, _p(X), c.ldx, C.c_int64(N), _p(Y), c.ldy, c.operands, st), "dense_fwd_lp")
        else:
            _lib.check(L.snerf_dense_fwd(_p(W), K, M, c.act, _p(X), c.ldx, C.c_int64(N), _p(Y), c.ldy, st), "dense_fwd")
        torch.cuda.synchronize()
        (_bounded if c.act == 2 else _same)(Y[:N, :M], ref["Y"], cid, "Y")
        _guards(Y, N, M, cid, "Y")
        return
    Ys, gY = _in(m["Y"], c.ldy), _in(m["gY"], c.ldgy)
    gX = None if c.call == "bwd_nogx" else _out(N, c.ldgx)
    gW = _flat(K * M, c.gw0) if c.call in ("bwd", "bwd_nogx") else None
    fx = _flat(K * M, int(c.gw0 * 2 ** 50), torch.int64) if c.call == "bwd_fx" else None
    head = (_p(W), K, M, c.act, _p(X), c.ldx, C.c_int64(N), _p(Ys), c.ldy, _p(gY), c.ldgy, _p(gX), c.ldgx)
    if c.operands:
        _lib.check(L.snerf_dense_bwd_lp(*head, _p(gW), _p(fx), c.operands, st), "dense_bwd_lp")
    elif fx is not None:
        _lib.check(L.snerf_dense_bwd_fx(*head, _p(fx), st), "dense_bwd_fx")
    else:
        _lib.check(L.snerf_dense_bwd(*head, _p(gW), st), "dense_bwd")
    torch.cuda.synchronize()
    if gX is not None:
        _same(gX[:N, :K], ref["gX"], cid, "gX")
        _guards(gX, N, K, cid, "gX")
    if gW is not None:
        _same(gW[:K * M], ref["gW"] + c.gw0, cid, "gW")
        assert bool((gW[K * M:] == SENT).all()), f"{cid}: cells behind gW were written"
    if fx is not None:
        _same(fx[:K * M].double() * 2.0 ** -50, ref["gW"] + c.gw0, cid, "gW (fixed-point cells x 2^-50)")
        assert bool((fx[K * M:] == 7).all()), f"{cid}: cells behind the fixed-point cells were written"


@pytest.mark.parametrize("c", CROSS, ids=R.case_id)
def test_every_backward_of_a_net_gives_the_same_bits(c):
    """snerf_mlp_bwd, _bwd_tile, _bwd_x16 (sigma_net shapes: the rows128 and the tile kernel) and the exact-fp32 backward of the same net: on an exact
    case their gX and gW are the same bits, and the message names the one that is not."""
    cid = R.case_id(c)
    m = R.make_mlp(c)
    run = lambda *a, **k: _run_backward(*a, sync=False, **k)
    runs = {"bwd": run(c, m, "bwd"), "bwd_tile": run(c, m, "bwd_tile"), "fp32 operands": run(c, m, "bwd", operands=0)}
    if c.hidden == 128 and c.d_in % 32 == 0:
        runs["bwd_x16"] = run(c, m, "bwd_x16")
        runs["bwd_x16, SNERF_MLP_SIGMA_ROWS=0"] = run(c._replace(rows="0"), m, "bwd_x16")
    torch.cuda.synchronize()
    for name, res in runs.items():
        _check_backward(c, m, res, f"{cid} [{name}]")
    first = runs["bwd"]
    for name, res in runs.items():
        assert torch.equal(res["gX"], first["gX"]) and torch.equal(res["gW"], first["gW"]), f"{cid}: {name} differs from snerf_mlp_bwd"

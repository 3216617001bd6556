"""Same results before and after a change to the MLP kernel family (csrc/mlp.hip, mlp_lp.hip, mlp_rows*.hip, dense_lp.hip, color_vd.hip and their shared
headers): on seeded inputs it saves what every MLP entry point of libsnerf writes, at the smallest shapes that reach each kernel and at two batch sizes
(333: ragged against every tile size; 70 001: more tiles than the largest grid, so the persistent loop's second trip and its prefetch run).  Dev tool.

    python tools/mlp_state.py run TREE OUTDIR       # imports soccernerfs_amd from TREE (a checkout with a built libsnerf.so); one process per tree
    python tools/mlp_state.py cmp A B [A2]          # Y / aux / gX / G / the sorted fix list / fixed-point weight gradients array_equal; weight gradients
                                                    # summed by float atomics ("gWa:..."): max |B - A| may not exceed max |A2 - A| of a second run of A's
                                                    # tree; exit 1 otherwise
"""
import ctypes as C
import os
import sys

import torch


def compare(a, b, a2):
    bad = n_exact = n_sum = 0
    for f in sorted(os.listdir(a)):
        x, y = torch.load(os.path.join(a, f)), torch.load(os.path.join(b, f))
        x2 = torch.load(os.path.join(a2, f)) if a2 else x
        assert x.keys() == y.keys(), (f, sorted(set(x) ^ set(y)))
        for k in x:
            if k.startswith("gWa:"):
                d, d0 = float((y[k] - x[k]).abs().max()), float((x2[k] - x[k]).abs().max())
                ok = d <= d0
                n_sum += 1
                print(f"{f:22s} {k:34s} n = {x[k].numel():9d}  max|B - A| = {d:.3e}  max|A2 - A| = {d0:.3e}  {'ok' if ok else 'EXCEEDS'}")
            else:
                ok = bool(torch.equal(x[k], y[k]))
                n_exact += 1
                if not ok:
                    print(f"{f:22s} {k:34s} n = {x[k].numel():9d}  DIFFERENT")
            bad += not ok
    print(f"{n_exact} exact tensors, {n_sum} atomically summed weight gradients")
    print("VERDICT", "exact tensors equal, atomic sums within the first tree's own run-to-run difference" if bad == 0 else f"{bad} differ")
    return bad


if sys.argv[1] == "cmp":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None) else 0)
tree, out = os.path.abspath(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import soccernerfs_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(soccernerfs_amd.__file__))) == tree, soccernerfs_amd.__file__
from soccernerfs_amd import _lib
from soccernerfs_amd.ops import _ptr, _stream

os.makedirs(out, exist_ok=True)
DEV = "cuda:0"
L = _lib.lib()
i32, i64 = C.c_int32, C.c_int64
NULL = C.c_void_p(0)


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV).contiguous()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device=DEV, dtype=dtype)


def net(gen, d_in, hidden, n_hidden, d_out):
    dims = [d_in] + [hidden] * n_hidden + [d_out]
    return torch.cat([(torch.randn(a, b, generator=gen) * a ** -0.5).flatten() for a, b in zip(dims[:-1], dims[1:])]).to(DEV).contiguous()


def mlp_case(res, gen, N, tag, d_in, hidden, n_hidden, d_out, out_act, aux, operands):
    desc = _lib.MlpDesc(d_in, hidden, n_hidden, d_out, 1, out_act, operands)
    assert L.snerf_mlp_supported(C.byref(desc)), tag
    P = int(L.snerf_mlp_param_count(C.byref(desc)))
    ldx = (d_in + 3) // 4 * 4  # float4-granular rows, as the trainers hand them over: the wave-owns-rows kernels need them
    W, X = net(gen, d_in, hidden, n_hidden, d_out), rnd(gen, N, ldx, scale=0.5)
    gY, gaux = rnd(gen, N, d_out, scale=1e-3), rnd(gen, N, scale=1e-3)
    aux_col, pga = (d_out - 1, _ptr(gaux)) if aux else (-1, NULL)
    Y, aux_out = zeros(N, d_out), zeros(N)
    _lib.check(L.snerf_mlp_fwd(C.byref(desc), _ptr(W), _ptr(X), i32(ldx), i64(N), _ptr(Y), i32(d_out), i32(aux_col), _ptr(aux_out) if aux else NULL, _stream()))
    res[f"{tag}/Y"], res[f"{tag}/aux"] = Y.cpu(), aux_out.cpu()
    back = (C.byref(desc), _ptr(W), _ptr(X), i32(ldx), i64(N), _ptr(gY), i32(d_out), i32(aux_col), pga)
    for name, fn in (("bwd", L.snerf_mlp_bwd), ("tile", L.snerf_mlp_bwd_tile)):
        if name == "tile" and operands == 0:
            continue
        gX, gW = zeros(N, d_in), zeros(P)
        _lib.check(fn(*back, _ptr(gX), i32(d_in), _ptr(gW), _stream()))
        res[f"{tag}/{name}/gX"], res[f"gWa:{tag}/{name}"] = gX.cpu(), gW.cpu()
    gX, gfx = zeros(N, d_in), zeros(P, dtype=torch.int64)
    _lib.check(L.snerf_mlp_bwd_fx(*back, _ptr(gX), i32(d_in), _ptr(gfx), _stream()))
    res[f"{tag}/fx/gX"], res[f"{tag}/fx/gW"] = gX.cpu(), gfx.cpu()
    gX, gW, ws = zeros(N, d_in), zeros(P), zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(desc))))
    _lib.check(L.snerf_mlp_bwd_ws(*back, _ptr(gX), i32(d_in), _ptr(ws), _stream()))
    _lib.check(L.snerf_mlp_gw_reduce(C.byref(desc), _ptr(ws), _ptr(gW), _stream()))
    res[f"{tag}/ws/gX"], res[f"gWa:{tag}/ws"] = gX.cpu(), gW.cpu()
    assert float(ws.abs().max()) == 0.0  # the reduce clears the replicas
    if operands == 0 or not (hidden == 128 and n_hidden == 1 and d_in % 32 == 0):
        return
    # ---- 16-bit input (what the fused field forward hands over) and the quotient epilogue, through the wave-owns-rows kernel (default) and,
    #      with SNERF_MLP_SIGMA_ROWS=0, through the workgroup-tile kernel ----
    X16 = X[:, :d_in].to(torch.bfloat16 if operands == 1 else torch.float16)
    X16[::7, 3] = 0  # vanished features: the fix list
    X16[5::11, d_in - 1] = 0
    X16 = X16.contiguous()
    back16 = (C.byref(desc), _ptr(W), _ptr(X16), i32(d_in), i64(N), _ptr(gY), i32(d_out), i32(aux_col), pga)
    cap = N
    for rows in ("1", "0"):
        os.environ["SNERF_MLP_SIGMA_ROWS"] = rows
        t = f"{tag}/rows{rows}"
        gX, gW = zeros(N, d_in), zeros(P)
        _lib.check(L.snerf_mlp_bwd_x16(*back16, _ptr(gX), i32(d_in), _ptr(gW), _stream()))
        res[f"{t}/x16/gX"], res[f"gWa:{t}/x16"] = gX.cpu(), gW.cpu()
        for with_ws in (False, True):
            G, gW, fix, cnt = zeros(N, d_in), zeros(P), zeros(2 * cap, dtype=torch.int32), torch.tensor([0, 7], device=DEV, dtype=torch.int32)  # [this step's counter, the next step's: the kernel clears it]
            args = (*back16, _ptr(G), i32(d_in), _ptr(fix), i32(cap), C.c_void_p(cnt.data_ptr()), C.c_void_p(cnt.data_ptr() + 4))
            if with_ws:
                ws = zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(desc))))
                _lib.check(L.snerf_mlp_bwd_x16_quotient_ws(*args, _ptr(ws), _stream()))
                _lib.check(L.snerf_mlp_gw_reduce(C.byref(desc), _ptr(ws), _ptr(gW), _stream()))
            else:
                _lib.check(L.snerf_mlp_bwd_x16_quotient(*args, _ptr(gW), _stream()))
            n = int(cnt[0])
            assert 0 < n <= cap and int(cnt[1]) == 0, (t, cnt.tolist())
            pairs = fix[: 2 * n].view(n, 2).cpu()
            q = f"{t}/quotient{'_ws' if with_ws else ''}"
            res[f"{q}/G"], res[f"{q}/fix"], res[f"gWa:{q}"] = G.cpu(), pairs[torch.argsort(pairs[:, 0])], gW.cpu()
    del os.environ["SNERF_MLP_SIGMA_ROWS"]


def dense_case(res, gen, N, K, M, act, operands):
    tag = f"dense{'_lp' if operands else ''}_{K}x{M}"
    W, X, gY = rnd(gen, K, M, scale=K ** -0.5), rnd(gen, N, K, scale=0.5), rnd(gen, N, M, scale=1e-3)
    Y = zeros(N, M)
    head = (_ptr(W), i32(K), i32(M), i32(act), _ptr(X), i32(K), i64(N))
    if operands:
        assert L.snerf_dense_lp_supported(i32(K), i32(M), i32(operands))
        _lib.check(L.snerf_dense_fwd_lp(*head, _ptr(Y), i32(M), i32(operands), _stream()))
    else:
        _lib.check(L.snerf_dense_fwd(*head, _ptr(Y), i32(M), _stream()))
    res[f"{tag}/Y"] = Y.cpu()
    back = (*head, _ptr(Y), i32(M), _ptr(gY), i32(M))
    gX, gW, gX2, gfx = zeros(N, K), zeros(K, M), zeros(N, K), zeros(K, M, dtype=torch.int64)
    if operands:
        _lib.check(L.snerf_dense_bwd_lp(*back, _ptr(gX), i32(K), _ptr(gW), NULL, i32(operands), _stream()))
        _lib.check(L.snerf_dense_bwd_lp(*back, _ptr(gX2), i32(K), NULL, _ptr(gfx), i32(operands), _stream()))
    else:
        _lib.check(L.snerf_dense_bwd(*back, _ptr(gX), i32(K), _ptr(gW), _stream()))
        _lib.check(L.snerf_dense_bwd_fx(*back, _ptr(gX2), i32(K), _ptr(gfx), _stream()))
    res[f"{tag}/bwd/gX"], res[f"gWa:{tag}/bwd"], res[f"{tag}/fx/gX"], res[f"{tag}/fx/gW"] = gX.cpu(), gW.cpu(), gX2.cpu(), gfx.cpu()


def color_vd_case(res, gen, N, S, operands):
    desc = _lib.MlpDesc(31, 64, 2, 3, 1, 1, operands)
    assert L.snerf_kplanes_color_bwd_vd_supported(C.byref(desc))
    tag = f"color_vd_op{operands}"
    P = int(L.snerf_mlp_param_count(C.byref(desc)))
    W, h, gY = net(gen, 31, 64, 2, 3), rnd(gen, N, 16, scale=0.5), rnd(gen, N, 3, scale=1e-3)
    dirs = torch.nn.functional.normalize(torch.randn(N // S, 3, generator=gen), dim=-1).to(DEV).contiguous()
    head = (C.byref(desc), _ptr(W), _ptr(dirs), i32(S), _ptr(h), i64(N), _ptr(gY), i32(3))
    gh, gW = zeros(N, 16), zeros(P)
    _lib.check(L.snerf_kplanes_color_bwd_vd(*head, _ptr(gh), _ptr(gW), _stream()))
    res[f"{tag}/gh"], res[f"gWa:{tag}"] = gh.cpu(), gW.cpu()
    gh, gW, ws = zeros(N, 16), zeros(P), zeros(int(L.snerf_mlp_gw_workspace_floats(C.byref(desc))))
    _lib.check(L.snerf_kplanes_color_bwd_vd_ws(*head, _ptr(gh), _ptr(ws), _stream()))
    _lib.check(L.snerf_mlp_gw_reduce(C.byref(desc), _ptr(ws), _ptr(gW), _stream()))
    res[f"{tag}/ws/gh"], res[f"gWa:{tag}/ws"] = gh.cpu(), gW.cpu()


# (d_in, hidden, hidden layers, d_out, out_act (1 = Sigmoid), trunc_exp side output on the last column)
FP32 = [(8, 64, 1, 1, 0, False), (15, 64, 2, 3, 1, False), (160, 128, 1, 16, 0, True)]
LP = [(8, 64, 1, 1, 0, False), (15, 64, 2, 3, 1, False), (63, 64, 2, 3, 1, False), (32, 128, 1, 16, 0, True), (160, 128, 1, 16, 0, True)]
for N, S in ((333, 9), (70001, 1)):
    res, gen = {}, torch.Generator().manual_seed(13)
    for operands, shapes in ((0, FP32), (1, LP), (2, LP)):
        for d_in, hidden, nh, d_out, out_act, aux in shapes:
            mlp_case(res, gen, N, f"mlp_op{operands}_{d_in}x{hidden}x{nh}x{d_out}", d_in, hidden, nh, d_out, out_act, aux, operands)
    dense_case(res, gen, N, 200, 300, 1, 0)  # more than one 128 block both ways: ldw_g, acc_y and acc_gx are live
    dense_case(res, gen, N, 64, 128, 1, 1)
    for operands in (1, 2):
        color_vd_case(res, gen, N, S, operands)
    torch.cuda.synchronize()
    torch.save(res, os.path.join(out, f"n{N}.pt"))
    print(f"N = {N}: {len(res)} tensors", flush=True)

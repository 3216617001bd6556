"""CPU: tests/table_reference.py -- the float64 restatement of both table encoders that tests/test_gpu_table_lattice.py holds the kernels to --
against everything else the repository knows about them: the two float32 oracles (oracle/tgrid_oracle.py, oracle/hashgrid_oracle.py: values by
their own code, gradients by autograd), the reference's known-answer test and the hand-computed dense-level answers (tests/tgrid_dense_kat.py),
the encoder classes' geometry and the library's host-side layout.  It also asserts, per lattice case, the CONDITION under which the GPU test may
ask for bit equality: the restatement evaluated in float32 equals the one in float64, and for every sum (A + what an accumulating buffer held
before) / granule < 2^24, A being the sum of |terms| and the granule the largest power of two that divides every term -- every partial sum in any
order is then a multiple of the granule below 2^24 granules, hence a float32.  That is a condition on the inputs, not a tolerance on a kernel.

Why the factors multiply exactly in any association on the lattice: every factor is a multiple of 2^-5 below 2 (fractions, 1 - fraction), of 2^-2
up to 1 (table values, time weights) or an integer below 2^6 (scales, upstream gradients); a product of at most six of them (three fractions,
scale, value, time weight, gradient never all at once) needs fewer than 24 bits."""
import numpy as np
import pytest
import torch

from tests import table_reference as TR

T_IDS = [c["case_id"] for c in TR.TGRID_LATTICE]
H_IDS = [c["case_id"] for c in TR.HASH_LATTICE]
TB_IDS = [c["case_id"] for c in TR.TGRID_BOUNDARY]
HB_IDS = [c["case_id"] for c in TR.HASH_BOUNDARY]


def _tgrid_oracle(d, dtype=torch.float32):
    """(out, gtable, gx) by oracle.tgrid_oracle.encode + autograd, in dtype"""
    from oracle import tgrid_oracle as TO

    geo, kw = d["geo"], d["case"]["kw"]
    x = torch.from_numpy(d["x"]).to(dtype).requires_grad_(True)
    emb = torch.from_numpy(d["emb"]).to(dtype).requires_grad_(True)
    trow = TO.temporal_index(torch.from_numpy(d["t_sample"]), TO.channel_table(geo["T"], geo["C"])).to(dtype)
    out = TO.encode(x, trow, emb, geo["offsets"], float(np.log2(geo["per_level_scale"])), kw["base_resolution"], 0 if kw.get("gridtype", "hash") == "hash" else 1,
                    geo["C"], geo["align_corners"])
    out.backward(torch.from_numpy(d["gout"]).to(dtype))
    return out.detach().numpy(), emb.grad.numpy(), x.grad.numpy()


def _hash_oracle(d, dtype=torch.float32):
    from oracle import hashgrid_oracle as HG

    c = d["case"]["cfg"]
    x = torch.from_numpy(d["x"]).to(dtype).requires_grad_(True)
    table = torch.from_numpy(d["table"]).to(dtype).requires_grad_(True)
    out = HG.encode(x, table, c["n_levels"], c["n_features_per_level"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"])
    out.backward(torch.from_numpy(d["gout"]).to(dtype))
    return out.detach().numpy(), table.grad.numpy(), x.grad.numpy()


def _bits(a):
    return np.asarray(a, np.float64).astype(np.float32)


# ---- lattice: bit equality with the oracles, and the exactness condition ----
@pytest.mark.parametrize("cid", T_IDS)
def test_tgrid_reference_equals_the_oracle_bit_for_bit_on_the_lattice(cid):
    d, ref = TR.case_and_reference(cid)
    out, gtab, gx = _tgrid_oracle(d)
    B = d["B"]
    assert np.array_equal(_bits(ref["out"]).reshape(B, -1), out)
    assert np.array_equal(_bits(ref["gtable"]), gtab)
    assert np.array_equal(_bits(ref["gx"]), gx)
    # what the case must contain: out-of-range samples (10 .. 20 %) that read and receive nothing, exact corners, every knot, dense and hashed levels
    share = 1.0 - float(ref["inside"].mean())
    assert 0.10 <= share <= 0.20, share
    outside = ~ref["inside"]
    assert not ref["out"][outside].any() and not ref["dy_dx"][outside].any() and not ref["gx"][outside].any()
    assert (d["x"] == 1).all(axis=1).any() and (d["x"] == 0).all(axis=1).any()
    n = d["geo"]["T"] - 2
    assert set(np.arange(n + 1, dtype=np.float32) / np.float32(n)) <= set(d["t_sample"].tolist()) and float(d["t_sample"].min()) >= 0 and float(d["t_sample"].max()) <= 1
    one = (d["x"] == 1).all(axis=1) & (d["t_sample"] == 1)
    assert one.any()                                                  # t == 1 together with x == (1, .., 1)
    kinds = {lv["hashed"] for lv in d["geo"]["levels"]}
    assert kinds == ({False} if cid in ("t_all_dense", "t_c1_tiled") else {False, True}), kinds
    assert (ref["A_gtable"] == 0).any() and (ref["gtable"] != 0).any()
    if d["case"]["mode"] == "rays":
        assert d["S"] % 32 and np.array_equal(d["x"], TR.ray_x(d["origins"], d["dirs"], d["ebins"], *d["aabb"]))
        cells = ref["cells"][-1].reshape(d["R"], d["S"], 3)
        same = (cells[:, 1:] == cells[:, :-1]).all(axis=-1)
        moving3 = (~same[:, 1:] & ~same[:, :-1])                     # a sample whose cell differs from both neighbours': a stretch that moves at every sample
        assert same.any() and moving3.any()


@pytest.mark.parametrize("cid", H_IDS)
def test_hashgrid_reference_equals_the_oracle_bit_for_bit_on_the_lattice(cid):
    d, ref = TR.case_and_reference(cid)
    out, gtab, gx = _hash_oracle(d)
    assert np.array_equal(_bits(ref["out"]).reshape(d["B"], -1), out)
    assert np.array_equal(_bits(ref["gtable"]), gtab)
    assert np.array_equal(_bits(ref["gx"]), gx)
    assert float(d["x"].min()) == -0.25 and float(d["x"].max()) == 1.25 and (d["x"] == 1).all(axis=1).any() and (d["x"] == 0).all(axis=1).any()
    # the wrap-around is exercised: some cell is "negative" (>= 2^31 after the cast) on a dense level and on a hashed one
    for hashed in {lv["hashed"] for lv in d["geo"]["levels"]}:
        assert any((cell >= 2 ** 31).any() for cell, lv in zip(ref["cells"], d["geo"]["levels"]) if lv["hashed"] == hashed)
    kinds = {lv["hashed"] for lv in d["geo"]["levels"]}
    assert kinds == {"h_f4_all_dense": {False}, "h_f2_all_hashed": {True}}.get(cid, {False, True}), kinds


@pytest.mark.parametrize("cid", T_IDS + H_IDS)
def test_lattice_cases_are_exact_in_float32_in_any_order(cid):
    d, ref = TR.case_and_reference(cid)
    tg = d["geo"]["kind"] == "tgrid"
    names = ("out", "dy_dx", "gtable", "gx") if tg else ("out", "gtable", "gx")
    r32 = (TR.tgrid_encode(d["geo"], d["x"], d["t_sample"], d["emb"], d["gout"], np.float32) if tg
           else TR.hash_encode(d["geo"], d["x"], d["table"], d["gout"], np.float32))
    for k, (gr, ratio) in TR.exactness(ref, names).items():
        assert np.array_equal(r32[k].astype(np.float64), ref[k]), k
        print(f"{cid} {k}: granule 2^{int(np.log2(gr))}, max (A + {TR.START:g}) / granule = 2^{np.log2(ratio):.2f}")
        assert ratio < 2 ** 24, (k, ratio)
        assert np.array_equal(np.round(ref[k] / gr) * gr, ref[k])    # every sum is a multiple of the granule


def test_cases_cover_the_sizes():
    assert {c["kw"]["level_dim"] for c in TR.TGRID_LATTICE} == {1, 2, 4, 8} and {c["cfg"]["n_features_per_level"] for c in TR.HASH_LATTICE} == {1, 2, 4, 8}
    assert any(c["kw"].get("input_dim") == 2 for c in TR.TGRID_LATTICE) and any(c["cfg"].get("D") == 2 for c in TR.HASH_LATTICE)
    assert any(c["kw"].get("gridtype") == "tiled" for c in TR.TGRID_LATTICE) and any(c["kw"].get("align_corners") for c in TR.TGRID_LATTICE)
    for B in (TR.LATTICE_B, TR.RAYS * TR.SAMPLES):
        assert B % 256 and B % 32
    for c in TR.TGRID_LATTICE:
        n = c["kw"]["temporal_dim"] - 2
        assert n & (n - 1) == 0


# ---- continuous cases: the oracles within float32 rounding ----
@pytest.mark.parametrize("cid", TB_IDS)
def test_tgrid_reference_agrees_with_the_oracle_within_float32_rounding(cid):
    d, ref = TR.case_and_reference(cid)
    out, gtab, gx = _tgrid_oracle(d)
    geo = d["geo"]
    # the oracle evaluates exp2 with numpy's float32 routine: where that is an ulp off the correctly rounded scale the boundary points change cell
    theirs = [float(np.float32(np.exp2(np.float32(l * float(np.log2(geo["per_level_scale"]))))) * np.float32(d["case"]["kw"]["base_resolution"]) - np.float32(1.0))
              for l in range(geo["L"])]
    same = np.array([float(lv["scale"]) == s for lv, s in zip(geo["levels"], theirs)])
    assert same.sum() >= 2, (theirs, [float(lv["scale"]) for lv in geo["levels"]])
    err = np.abs(out.reshape(ref["out"].shape).astype(np.float64) - ref["out"])
    assert (err <= TR.K_TG_OUT * TR.U * ref["A_out"])[:, same].all(), float((err / (TR.U * ref["A_out"].clip(1e-30)))[:, same].max())
    if same.all():
        assert (np.abs(gtab - ref["gtable"]) <= TR.table_bound(ref["A_gtable"], ref["n_gtable"], TR.K_TG_TERM)).all()
        assert (np.abs(gx - ref["gx"]) <= TR.k_tg_gx(geo["L"], geo["C"]) * TR.U * ref["A_gx"]).all()


@pytest.mark.parametrize("cid", HB_IDS)
def test_hashgrid_reference_agrees_with_the_oracle_within_float32_rounding(cid):
    from oracle import hashgrid_oracle as HG

    d, ref = TR.case_and_reference(cid)
    c, geo = d["case"]["cfg"], d["geo"]
    scales, ress, offsets = HG.level_geometry(c["n_levels"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"], geo["D"])
    assert [float(lv["scale"]) for lv in geo["levels"]] == [float(s) for s in scales] and offsets == geo["offsets"]
    out, gtab, gx = _hash_oracle(d)
    assert (np.abs(out.reshape(ref["out"].shape) - ref["out"]) <= TR.K_HT_OUT * TR.U * ref["A_out"]).all()
    assert (np.abs(gtab - ref["gtable"]) <= TR.table_bound(ref["A_gtable"], ref["n_gtable"], TR.K_HT_TERM)).all()
    assert (np.abs(gx - ref["gx"]) <= TR.k_ht_gx(geo["L"], geo["F"]) * TR.U * ref["A_gx"]).all()


@pytest.mark.parametrize("cid", TB_IDS + HB_IDS)
def test_boundary_cases_sit_on_the_boundaries_and_a_wrong_cell_would_show(cid):
    """Part B's purpose, checked in the reference: the cases hold points whose cell is decided by the float32 rounding of pos (and, taken together,
    points where the two encoders' rounding rules part); nothing has to be excluded, because the reference takes the float32 pos (share 0, cap
    2 %); and across a triple (x-, x, x+) whose members fall into different cells the coordinate derivative moves by far more than its bound."""
    d, ref = TR.case_and_reference(cid)
    geo = d["geo"]
    tg = geo["kind"] == "tgrid"
    decided = TR.rounding_decided(geo, d["x"])
    if not geo.get("align_corners"):      # x * scale + 0 is one rounding of a product: floor agrees with the exact one except at an exact integer
        assert decided.any()
    excluded = 0
    print(f"{cid}: {int(decided.sum())} (point, level, axis) decided by rounding, excluded share {excluded / decided.size:.4f}")
    assert excluded / decided.size <= 0.02
    # what jumps: the temporal grid's dy_dx of that level and axis (summed over channels), and either grid's coordinate gradient on that axis
    k_gx = TR.k_tg_gx(geo["L"], geo["C"]) if tg else TR.k_ht_gx(geo["L"], geo["F"])
    jumps = {"dy_dx": [], "gx": []}
    changed = 0
    for i, l, axis in d["triples"]:
        cells = ref["cells"][l][i:i + 3, axis]
        if len(set(cells.tolist())) < 2:
            continue
        changed += 1
        if tg and not ref["inside"][i:i + 3].all():
            continue
        a, b = (i, i + 2) if cells[0] != cells[2] else (i, i + 1)
        jumps["gx"].append(abs(ref["gx"][a, axis] - ref["gx"][b, axis]) / (k_gx * TR.U * max(ref["A_gx"][a, axis], ref["A_gx"][b, axis])))
        if tg:
            dy, A = ref["dy_dx"][:, l, axis].sum(axis=-1), ref["A_dy_dx"][:, l, axis].sum(axis=-1)
            jumps["dy_dx"].append(abs(dy[a] - dy[b]) / (TR.K_TG_DYDX * TR.U * max(A[a], A[b])))
    assert changed >= 10
    for name, r in jumps.items():
        if r:
            print(f"{cid}: {len(r)} triples change cell; {name} jump / bound: median {np.median(r):.3g}, min {min(r):.3g}")
            assert np.median(r) > 1e3, name
    assert jumps["gx"]


def test_the_two_rounding_rules_part_somewhere():
    """hashgrid.hip contracts and the temporal grid's files do not: the boundary cases hold points at which applying the other encoder's rule to pos
    lands in the neighbouring cell, for each encoder."""
    t = sum(int(TR.rules_differ(TR.case_and_reference(c)[0]["geo"], TR.case_and_reference(c)[0]["x"]).sum()) for c in TB_IDS)
    h = sum(int(TR.rules_differ(TR.case_and_reference(c)[0]["geo"], TR.case_and_reference(c)[0]["x"]).sum()) for c in HB_IDS)
    assert t >= 3 and h >= 3, (t, h)


# ---- known answers ----
def test_reference_known_answer():
    """NSR/tests/field_components/test_temporal_grid.py:15-40: out == 0.5, the gradient lands in rows 0 and 1 of column 0 only."""
    geo = TR.tgrid_geometry(temporal_dim=2, input_dim=1, num_levels=1, level_dim=1, per_level_scale=1, base_resolution=1, log2_hashmap_size=2, gridtype="tiled")
    assert geo["offsets"] == [0, 8]
    emb = np.random.default_rng(0).random((8, 3)).astype(np.float32)
    emb[:, 0] = np.arange(8)
    g = np.random.default_rng(1).standard_normal((1024, 1)).astype(np.float32)
    r = TR.tgrid_encode(geo, np.zeros((1024, 1), np.float32), np.zeros(1024, np.float32), emb, g)
    assert (r["out"] == 0.5).all()
    assert abs(r["gtable"].sum() - g.astype(np.float64).sum()) < 1e-9 and not r["gtable"][2:].any() and not r["gtable"][:, 1:].any()


@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
def test_dense_levels_hand_computed_answers(gridtype):
    from tests import tgrid_dense_kat as K

    geo = TR.tgrid_geometry(gridtype=gridtype, **K.KW)
    assert geo["offsets"] == K.OFFSETS and not any(lv["hashed"] for lv in geo["levels"])
    x, t, want = K.inputs(torch)
    emb = K.embedding(torch).numpy()
    r = TR.tgrid_encode(geo, x.numpy(), t[:, 0].numpy(), emb, np.ones((4, 2), np.float32))
    assert np.array_equal(r["out"][:, :, 0], want.numpy().astype(np.float64))
    one = TR.tgrid_encode(geo, x[1:2].numpy(), t[1:2, 0].numpy(), emb, np.ones((1, 2), np.float32))
    assert np.array_equal(one["gtable"], K.expected_grad(torch).numpy().astype(np.float64))


# ---- geometry ----
@pytest.mark.parametrize("cid", T_IDS + TB_IDS)
def test_tgrid_geometry_equals_the_encoder_class(cid):
    from soccernerfs_amd.temporal_grid import TemporalGridEncoder

    d, _ = TR.case_and_reference(cid)
    geo = d["geo"]
    enc = TemporalGridEncoder(**d["case"]["kw"])
    assert enc.offsets.tolist() == geo["offsets"] == list(enc.desc.offsets)[: geo["L"] + 1]
    assert np.float32(enc.desc.S) == geo["S"] and enc.desc.grid_C == geo["grid_C"] and enc.desc.H == d["case"]["kw"]["base_resolution"]
    # the explicit rows the reference builds are the class's get_temporal_index, bit for bit
    assert np.array_equal(enc.get_temporal_index(torch.from_numpy(d["t_sample"])).numpy(), d["trow"])


@pytest.mark.parametrize("cid", H_IDS + HB_IDS)
def test_hashgrid_geometry_equals_the_library_layout_and_the_oracle(cid):
    from oracle import hashgrid_oracle as HG
    from soccernerfs_amd import ops

    d, _ = TR.case_and_reference(cid)
    c, geo = d["case"]["cfg"], d["geo"]
    desc, rows = ops.hashgrid_desc(geo["D"], c["n_levels"], c["n_features_per_level"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"])
    assert rows == geo["offsets"][-1] and list(desc.offsets)[: geo["L"] + 1] == geo["offsets"]
    assert [np.float32(desc.scale[l]) for l in range(geo["L"])] == [lv["scale"] for lv in geo["levels"]]
    assert [desc.resolution[l] for l in range(geo["L"])] == [lv["resolution"] for lv in geo["levels"]]
    scales, ress, offsets = HG.level_geometry(c["n_levels"], c["base_resolution"], c["per_level_scale"], c["log2_hashmap_size"], geo["D"])
    assert offsets == geo["offsets"] and ress == [lv["resolution"] for lv in geo["levels"]] and [np.float32(s) for s in scales] == [lv["scale"] for lv in geo["levels"]]
    for lv, res in zip(geo["levels"], ress):
        assert lv["hashed"] == (res ** geo["D"] > lv["rows"])

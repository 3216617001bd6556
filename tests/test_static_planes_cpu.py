"""Static scenes on the fused path, the parts decided on the host (no GPU): the shape probes of the three-plane kernels, the refusals of
KPlanesTrainConfig(freeze_time_planes=True) / a 3-coordinate model, the host-side refusal of NULL times with a 4-coordinate descriptor, the
exchange plan's sizes of a 3-coordinate layout, the restated frozen reference against the oracle it composes, and the empty synthetic scene."""
import ctypes as C

import pytest
import torch


def _mlp_desc(d_in, hidden, n_hidden, d_out, out_act, operands):
    from soccernerfs_amd import _lib

    m = _lib.MlpDesc()
    m.d_in, m.hidden, m.n_hidden, m.d_out, m.hidden_act, m.out_act, m.operands = d_in, hidden, n_hidden, d_out, 1, out_act, operands
    return m


def _plane_sets():
    from soccernerfs_amd.plane_set import PlaneSet

    gen = torch.Generator().manual_seed(0)
    field3 = PlaneSet(32, [[12, 10, 9], [24, 20, 18]], concat=True, generator=gen)
    field4 = PlaneSet(32, [[12, 10, 9, 6], [24, 20, 18, 6]], concat=True, generator=gen)
    prop3 = PlaneSet(8, [[24, 20, 18]], concat=False, generator=gen)
    prop4 = PlaneSet(8, [[24, 20, 18, 6]], concat=False, generator=gen)
    return field3, field4, prop3, prop4


def test_probes_answer_for_three_planes():
    from soccernerfs_amd import _lib

    l = _lib.lib()
    field3, field4, prop3, prop4 = _plane_sets()
    assert field3.space_desc().n_coords == 3 and list(field3.space_desc().off[1])[:3] == field3.offsets[1]  # a 3-coordinate set: the plain descriptor
    sd = field4.space_desc()
    assert sd.n_coords == 3 and [sd.off[1][k] for k in range(3)] == [field4.offsets[1][p] for p in (0, 1, 3)]
    for ops_ in (1, 2):
        sig, col, net = _mlp_desc(64, 128, 1, 16, 0, ops_), _mlp_desc(15, 64, 2, 3, 1, ops_), _mlp_desc(8, 64, 1, 1, 0, ops_)
        for fd, pd in ((field3.desc(), prop3.desc()), (field4.space_desc(), prop4.space_desc())):
            assert fd.n_coords == 3 and pd.n_coords == 3
            assert l.snerf_kplanes_field_fwd_supported(C.byref(fd), C.byref(sig), C.byref(col)) == 1
            assert l.snerf_kplanes_field_render_supported(C.byref(fd), C.byref(sig), C.byref(col), 32) == 1
            assert l.snerf_kplanes_field_render_supported(C.byref(fd), C.byref(sig), C.byref(col), 33) == 0  # the same S rule as six planes
            assert l.snerf_kplanes_density_fwd_supported(C.byref(pd), C.byref(net)) == 1
            # deliberately not built: the fused proposal backward walks 12 (plane, row) streams
            assert l.snerf_kplanes_density_bwd_supported(C.byref(pd), C.byref(net)) == 0
        assert l.snerf_kplanes_density_bwd_supported(C.byref(prop4.desc()), C.byref(net)) == 1  # six planes: as before
    sig, col, net = _mlp_desc(64, 128, 1, 16, 0, 0), _mlp_desc(15, 64, 2, 3, 1, 0), _mlp_desc(8, 64, 1, 1, 0, 0)
    for fd, pd in ((field3.desc(), prop3.desc()), (field4.space_desc(), prop4.space_desc())):  # fp32 operands run unfused, three planes or six
        assert l.snerf_kplanes_field_fwd_supported(C.byref(fd), C.byref(sig), C.byref(col)) == 0
        assert l.snerf_kplanes_field_render_supported(C.byref(fd), C.byref(sig), C.byref(col), 32) == 0
        assert l.snerf_kplanes_density_fwd_supported(C.byref(pd), C.byref(net)) == 0
    bad = field3.desc()
    bad.n_coords = 2
    assert l.snerf_kplanes_field_fwd_supported(C.byref(bad), C.byref(_mlp_desc(64, 128, 1, 16, 0, 1)), C.byref(_mlp_desc(15, 64, 2, 3, 1, 1))) == 0


def test_null_times_with_four_coordinates_is_refused_on_the_host():
    """Mode-1 coordinates without a times buffer are legal exactly for a 3-coordinate descriptor.  Every buffer a kernel would touch is NULL here
    and the ray pointers are host words, so a call that got past its checks could still launch nothing: the plane / weight buffers are
    checked behind the coordinates."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    _, field4, _, prop4 = _plane_sets()
    word = (C.c_float * 8)()
    ptr = C.cast(word, C.c_void_p).value
    co = _lib.Coords()
    co.mode, co.S, co.origins, co.dirs, co.ebins, co.times = 1, 4, ptr, ptr, ptr, None
    sig, col, net = _mlp_desc(64, 128, 1, 16, 0, 1), _mlp_desc(15, 64, 2, 3, 1, 1), _mlp_desc(8, 64, 1, 1, 0, 1)
    d4 = field4.desc()
    rc = l.snerf_kplanes_field_fwd(C.byref(d4), None, C.byref(co), C.c_int64(8), C.byref(sig), None, C.byref(col), None, None, None, None, None, None, None)
    assert rc != 0 and b"times" in l.snerf_last_error()
    rc = l.snerf_kplanes_field_render(C.byref(d4), None, C.byref(co), 2, C.byref(sig), None, C.byref(col), None, 0.0, None, None, None, None, None, None, None)
    assert rc != 0  # (S = 4 is no render shape either: refused one way or the other, on the host)
    p4 = prop4.desc()
    rc = l.snerf_kplanes_density_fwd(C.byref(p4), None, C.byref(co), C.c_int64(8), C.byref(net), None, None, None, None)
    assert rc != 0 and b"times" in l.snerf_last_error()
    rc = l.snerf_kplanes_gather_fwd(C.byref(p4), None, C.byref(co), C.c_int64(8), None, None)
    assert rc != 0 and b"times" in l.snerf_last_error()
    # the same calls on the three-plane view get past the coordinates and stop at the NULL plane buffer
    s4, sp4 = field4.space_desc(), prop4.space_desc()
    rc = l.snerf_kplanes_field_fwd(C.byref(s4), None, C.byref(co), C.c_int64(8), C.byref(sig), None, C.byref(col), None, None, None, None, None, None, None)
    assert rc != 0 and b"null buffer" in l.snerf_last_error()
    rc = l.snerf_kplanes_density_fwd(C.byref(sp4), None, C.byref(co), C.c_int64(8), C.byref(net), None, None, None, None)
    assert rc != 0 and b"null buffer" in l.snerf_last_error()
    # a ray order is for the time planes' rows: refused with three coordinates
    order = C.cast((C.c_int32 * 4)(), C.c_void_p)
    co.S = 32
    rc = l.snerf_kplanes_field_fwd_ordered(C.byref(s4), None, C.byref(co), C.c_int64(64), C.byref(sig), None, C.byref(col), None, None, None, None, None, None,
                                           order, None)
    assert rc != 0 and b"4-coordinate" in l.snerf_last_error()


def test_trainer_refusals_come_before_any_allocation(monkeypatch):
    from soccernerfs_amd import plane_set
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    def no_alloc(*a, **k):
        raise AssertionError("the trainer allocated a plane set before refusing the configuration")

    monkeypatch.setattr(plane_set.PlaneSet, "__init__", no_alloc)
    monkeypatch.setattr(torch, "zeros_like", no_alloc)
    S3 = dict(spacetime_resolution=(16, 16, 16), proposal_resolutions=((24, 24, 24), (32, 32, 32)))
    assert KPlanesTrainConfig().freeze_time_planes is False and KPlanesTrainConfig().freeze_space_planes is False
    with pytest.raises(ValueError, match="proposal_resolutions"):
        KPlanesTrainer(KPlanesTrainConfig(spacetime_resolution=(16, 16, 16)), 64, "cpu")  # the preset's 4-value proposal levels
    with pytest.raises(ValueError, match="proposal_resolutions"):
        KPlanesTrainer(KPlanesTrainConfig(proposal_resolutions=((24, 24, 24, 4), (32, 32, 32))), 64, "cpu")
    with pytest.raises(ValueError, match="freeze_time_planes on a 3-coordinate model"):
        KPlanesTrainer(KPlanesTrainConfig(freeze_time_planes=True, **S3), 64, "cpu")
    with pytest.raises(NotImplementedError, match="freeze_space_planes"):
        KPlanesTrainer(KPlanesTrainConfig(freeze_space_planes=True), 64, "cpu")
    for kw, what in ((dict(freeze_time_planes=True), "freeze_time_planes"), (S3, "3-coordinate")):
        with pytest.raises(NotImplementedError, match=f"{what}.* with ray_gradients"):
            KPlanesTrainer(KPlanesTrainConfig(ray_gradients=True, **kw), 64, "cpu")
        with pytest.raises(NotImplementedError, match=f"{what}.* with pipeline_sweep"):
            KPlanesTrainer(KPlanesTrainConfig(pipeline_sweep="fine_first", **kw), 64, "cpu")
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda group=None: 0)
    for kw, what in ((dict(freeze_time_planes=True), "freeze_time_planes"), (S3, "3-coordinate")):
        with pytest.raises(NotImplementedError, match=f"{what}.* with world > 1"):
            KPlanesTrainer(KPlanesTrainConfig(**kw), 64, "cpu", process_group=object())


def test_exchange_plan_describes_a_three_coordinate_layout():
    from soccernerfs_amd.exchange_plan import align4, kplanes_segment_sizes, plane_layout
    from soccernerfs_amd.plane_set import PlaneSet

    base, ms, prop = (12, 10, 9), (1, 2, 4), ((24, 20, 18), (32, 30, 28))
    counts = {"prop": 8 * 64 + 64, "sigma": 96 * 128 + 128 * 16, "color": 15 * 64 + 64 * 64 + 64 * 3}
    sz = kplanes_segment_sizes(base, ms, 32, prop, 8, counts, 1)
    field = PlaneSet(32, [[r * m for r in base] for m in ms], concat=True)
    props = [PlaneSet(8, [list(r)], concat=False) for r in prop]
    assert len(field.combs) == 3 and field.n_coords == 3
    want_field = 32 * sum((12 * 10 + 12 * 9 + 10 * 9) * m * m for m in ms)
    assert field.numel == want_field == sz["field_floats"] == sz["field_padded"]
    assert plane_layout(32, field.resolutions) == (field.offsets, field.numel)
    n_prop = sum(align4(p.numel) + align4(counts["prop"]) for p in props)
    assert sz["n_proposal_params"] == sz["field_offset"] == n_prop
    assert sz["n_params"] == n_prop + field.numel + align4(counts["sigma"]) + align4(counts["color"])
    assert sz["finest_offset"] == field.offsets[-1][0] and sz["n_scales"] == 3
    # against the same model with a time axis: exactly the three time planes per scale are gone
    sz4 = kplanes_segment_sizes(base + (6,), ms, 32, tuple(r + (6,) for r in prop), 8, counts, 1)
    assert sz4["field_floats"] - sz["field_floats"] == 32 * 6 * sum((12 + 10 + 9) * m for m in ms)


def test_restated_reference_reproduces_the_oracle_without_the_flag():
    """tests/static_reference.py composes the oracle's pieces; with the flag off it must be the oracle's own forward and loss dict, bit for bit,
    gradients included.  With the flag the time planes receive no gradient and the loss dict has no time terms."""
    from oracle import kplanes_oracle as KO
    from tests import static_reference as SR

    (S01, S2), R = SR.THREE_STEPS_SAMPLES, SR.THREE_STEPS_RAYS
    b = SR.draw_batch(torch.Generator().manual_seed(SR.THREE_STEPS_SEED), R)
    grads = []
    for restated in (False, True):
        P = KO.make_kplanes_params(**SR.THREE_STEPS)
        leaves = KO.all_param_tensors(P)
        for x in leaves:
            x.requires_grad_(True)
        if restated:
            out = SR.forward(P, b["rays"], b["rng"], S01, S2, 0.37)
            ld = SR.loss_dict(P, out, b["target"])
        else:
            out = KO.kplanes_forward(P, b["rays"], b["rng"], S01, S2, anneal=0.37)
            ld = KO.kplanes_loss_dict(P, out, b["target"])
        sum(ld.values()).backward()
        grads.append((out["rgb"].detach(), {k: v.detach() for k, v in ld.items()}, [x.grad for x in leaves]))
    (rgb0, ld0, g0), (rgb1, ld1, g1) = grads
    assert torch.equal(rgb0, rgb1) and list(ld0) == list(ld1) and all(torch.equal(ld0[k], ld1[k]) for k in ld0)
    assert all((a is None) == (c is None) and (a is None or torch.equal(a, c)) for a, c in zip(g0, g1))
    # with the flag
    P = KO.make_kplanes_params(**SR.THREE_STEPS)
    leaves = KO.all_param_tensors(P)
    for x in leaves:
        x.requires_grad_(True)
    out = SR.forward(P, b["rays"], b["rng"], S01, S2, 0.37, freeze_time_planes=True)
    ld = SR.loss_dict(P, out, b["target"], freeze_time_planes=True)
    assert not set(ld) & set(SR.TIME_TERMS) and set(ld) == set(ld0) - set(SR.TIME_TERMS)
    sum(ld.values()).backward()
    frozen = SR.time_plane_leaves(P)
    assert len(frozen) == 3 * (2 + 2) and all(t.grad is None for t in frozen)
    ms, vs = [torch.zeros_like(x) for x in leaves], [torch.zeros_like(x) for x in leaves]
    assert SR.adam_on_touched(leaves, ms, vs, 1, 1e-2) == len(leaves) - len(frozen)
    assert all(bool((t == 1).all()) for t in frozen)
    # the time planes are ones, so their 1-D total variation -- which the reference's space_tv_loss still takes under the flag -- is exactly zero
    assert float(SR.space_tv_space_planes(P["field_grids"]).detach() - KO.space_tv_loss(P["field_grids"]).detach()) == 0.0


def test_empty_scene_is_the_scene_without_players_and_constant_in_time():
    from soccernerfs_amd import synthetic

    gen = torch.Generator().manual_seed(3)
    cams = synthetic.make_cameras(4, 96, 54)
    N = 4000
    ci = torch.randint(0, 4, (N,), generator=gen)
    px = torch.stack([torch.rand(N, generator=gen) * 96, torch.rand(N, generator=gen) * 54], -1)
    dcam = torch.stack([(px[:, 0] - 48) / cams["fx"][ci], -(px[:, 1] - 27) / cams["fy"][ci], -torch.ones(N)], -1)
    d = torch.nn.functional.normalize(torch.einsum("nij,nj->ni", cams["c2w"][ci][:, :, :3], dcam), dim=-1)
    o = cams["c2w"][ci][:, :, 3]
    t = torch.rand(N, generator=gen)
    for variant in ("default", "textured", "stadium"):
        full = synthetic.shade(o, d, t, variant)
        assert torch.equal(full, synthetic.shade(o, d, t, variant, dynamic=True))
        empty = synthetic.shade(o, d, t, variant, dynamic=False)
        assert torch.equal(empty, synthetic.shade(o, d, torch.zeros(N), variant, dynamic=False))  # constant in time
        # a pixel whose colour in the full scene never changes over the clip (and is that colour at t too) is covered by no player or ball:
        # there the empty scene must show the same colour; and wherever the two scenes differ, the full scene's colour did change
        sweep = torch.stack([synthetic.shade(o, d, torch.full((N,), float(tk)), variant) for tk in torch.linspace(0, 1, 41)] + [full])
        never_covered = (sweep == sweep[:1]).all(-1).all(0)
        assert int(never_covered.sum()) > N // 2
        assert torch.equal(empty[never_covered], full[never_covered])
        assert not bool(never_covered[(full != empty).any(-1)].any())

"""snerf_tgrid_density_fwd and the NeRFPlayer-nerfacto renderer, the parts decided on the host (no GPU): the two entries are bound, the shape probe
answers 1 for what csrc/tgrid_density.hip is built for and 0 for everything else, the entry refuses bad arguments under its own name before
anything is launched, the renderer is exported beside KPlanesRenderer on one base class, and the trainer's checkpoint keys are the reference
model's."""
import ctypes as C
import inspect

import pytest
import torch


def _mlp_desc(d_in, hidden=16, n_hidden=1, d_out=1, hidden_act=1, out_act=0, operands=0):
    from soccernerfs_amd import _lib

    m = _lib.MlpDesc()
    m.d_in, m.hidden, m.n_hidden, m.d_out, m.hidden_act, m.out_act, m.operands = d_in, hidden, n_hidden, d_out, hidden_act, out_act, operands
    return m


def _enc(L=5, C_=2, max_res=64, temporal_dim=32, log2=17, input_dim=3):
    import numpy as np

    from soccernerfs_amd.temporal_grid import TemporalGridEncoder

    growth = float(np.exp((np.log(max_res) - np.log(16)) / (L - 1)))
    return TemporalGridEncoder(input_dim=input_dim, temporal_dim=temporal_dim, num_levels=L, level_dim=C_, per_level_scale=growth, base_resolution=16,
                               log2_hashmap_size=log2)


def test_the_two_entries_are_bound_and_declared():
    from soccernerfs_amd import _lib

    l = _lib.lib()
    assert _lib.SIGNATURES["snerf_tgrid_density_fwd_supported"] == "i:PP"
    assert _lib.SIGNATURES["snerf_tgrid_density_fwd"] == "s:PPPPILPPPP"
    for name in ("snerf_tgrid_density_fwd_supported", "snerf_tgrid_density_fwd"):
        assert hasattr(l, name) and name[len("snerf_"):] in _lib.entries
    assert l.snerf_abi_revision() == _lib.ABI_REVISION == 2  # added to revision 2's surface: the number callers pin does not move


def test_supported_answers_for_the_preset_and_for_nothing_else():
    from soccernerfs_amd import _lib

    l = _lib.lib()
    ok = lambda enc, net: l.snerf_tgrid_density_fwd_supported(C.byref(enc.desc), C.byref(net))
    for max_res in (64, 256):  # the preset's two proposal shapes: D = 3, C = 2, L = 5, temporal_dim 32, net 10 -> 16 -> 1
        assert ok(_enc(max_res=max_res), _mlp_desc(10)) == 1
    assert ok(_enc(L=8, temporal_dim=8, log2=12), _mlp_desc(16)) == 1   # L * C = 16: the widest table it is built for
    assert ok(_enc(L=2, temporal_dim=8, log2=12), _mlp_desc(4)) == 1
    assert ok(_enc(L=4, C_=4, log2=12), _mlp_desc(16)) == 0             # C = 4
    assert ok(_enc(L=9, log2=12), _mlp_desc(18)) == 0                   # L * C = 18
    assert ok(_enc(), _mlp_desc(10, operands=1)) == 0                   # 16-bit operands
    assert ok(_enc(), _mlp_desc(10, operands=2)) == 0
    assert ok(_enc(), _mlp_desc(10, out_act=1)) == 0                    # Sigmoid output
    assert ok(_enc(), _mlp_desc(10, n_hidden=2)) == 0                   # two hidden layers
    assert ok(_enc(), _mlp_desc(10, hidden=64)) == 0
    assert ok(_enc(), _mlp_desc(10, hidden_act=0)) == 0                 # no ReLU
    assert ok(_enc(), _mlp_desc(10, d_out=2)) == 0
    assert ok(_enc(), _mlp_desc(12)) == 0                               # the net's input is not the table's output
    assert ok(_enc(input_dim=2, log2=12), _mlp_desc(10)) == 0           # D = 2
    assert l.snerf_tgrid_density_fwd_supported(None, C.byref(_mlp_desc(10))) == 0
    assert l.snerf_tgrid_density_fwd_supported(C.byref(_enc().desc), None) == 0


def test_the_entry_refuses_by_name_before_any_launch():
    """Every buffer is host memory filled with a sentinel: a call that got past its checks could only fail in the launch, and a refused one must
    say `tgrid_density_fwd` and leave the sentinel in place."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    enc, net = _enc(), _mlp_desc(10)
    S, R = 4, 2
    N = R * S
    words = (C.c_float * 64)(*([-7.0] * 64))
    ptr = C.cast(words, C.c_void_p)

    def coords(mode=1, contract=0, S_=S, origins=True):
        co = _lib.Coords()
        co.mode, co.S, co.contract = mode, S_, contract
        co.pts = ptr.value if mode == 0 else None
        co.origins, co.dirs, co.ebins = (ptr.value if origins else None), ptr.value, ptr.value
        for k in range(3):
            co.aabb_min[k], co.aabb_max[k] = -1.0, 1.0
        return co

    def refused(word, desc=enc.desc, co=None, times=ptr, S_=S, N_=N, net_=net, table=ptr, W=ptr, dens=ptr):
        co = coords() if co is None else co
        rc = l.snerf_tgrid_density_fwd(C.byref(desc) if desc is not None else None, table, C.byref(co), times, S_, C.c_int64(N_),
                                       C.byref(net_) if net_ is not None else None, W, dens, None)
        msg = l.snerf_last_error().decode()
        assert rc != 0 and msg.startswith("tgrid_density_fwd:") and word in msg, (rc, msg)
        assert all(v == -7.0 for v in words)

    refused("null descriptor", desc=None)
    refused("null descriptor", net_=None)
    refused("mode=0", co=coords(mode=0))
    refused("contract=1", co=coords(contract=1))
    refused("built for", desc=_enc(L=4, C_=4, log2=12).desc, net_=_mlp_desc(16))
    refused("built for", net_=_mlp_desc(10, operands=1))
    refused("built for", net_=_mlp_desc(10, out_act=1))
    refused("coords.S", S_=S + 1, N_=R * (S + 1))
    refused("N=", N_=N + 1)  # not whole rays
    refused("incomplete ray coordinates", co=coords(origins=False))
    for null in ("table", "times", "W", "dens"):
        refused("null buffer", **{null: None})
    # nothing to do is not an error, and needs no buffer
    assert l.snerf_tgrid_density_fwd(C.byref(enc.desc), None, C.byref(coords()), None, S, C.c_int64(0), C.byref(net), None, None, None) == 0


def test_both_renderers_share_one_base():
    from soccernerfs_amd import render

    assert issubclass(render.KPlanesRenderer, render.FrameRenderer) and issubclass(render.NerfplayerRenderer, render.FrameRenderer)
    for name in ("render_frame", "render_camera_path", "evaluate", "to_uint8", "_host_table", "_ck"):
        assert name not in vars(render.KPlanesRenderer) and name not in vars(render.NerfplayerRenderer), name  # defined once, on the base
    sig = inspect.signature(render.NerfplayerRenderer.__init__).parameters
    assert list(sig)[1:5] == ["trainer", "rays_per_chunk", "background_color", "fused_density"]
    assert sig["rays_per_chunk"].default == 32768 and sig["background_color"].default == "black"
    doc = render.NerfplayerRenderer.__doc__
    assert "PER RAY" in doc and "deviates from the reference on purpose" in doc  # the depth decision is stated where a user reads it


def test_renderer_refusals_come_before_any_launch():
    from soccernerfs_amd.render import NerfplayerRenderer

    class NerfplayerFullTrainer:  # stands for any trainer that is not the nerfacto variant
        pass

    with pytest.raises(TypeError, match="NerfplayerFullTrainer"):
        NerfplayerRenderer(NerfplayerFullTrainer())


def test_trainer_checkpoint_keys_are_the_reference_models():
    """NerfplayerTrainer._named_module against NerfplayerNerfactoModel, on the CPU: same keys in the same order (the temporal grids' index buffers
    and embedding.weight among them), the strict loader accepts them, and the Adam moments go out and come back under the trainer's names."""
    from soccernerfs_amd import checkpoint as CK
    from soccernerfs_amd.nerfplayer_nerfacto import NerfplayerNerfactoModel, NerfplayerNerfactoModelConfig
    from soccernerfs_amd.nerfplayer_trainer import NerfplayerTrainer
    from soccernerfs_amd.scene_colliders import SceneBox

    prop = {"hidden_dim": 16, "temporal_dim": 8, "log2_hashmap_size": 12, "num_levels": 5}
    cfg = NerfplayerNerfactoModelConfig(num_levels=4, log2_hashmap_size=12, temporal_dim=8, num_proposal_samples_per_ray=(32, 16), num_nerf_samples_per_ray=8,
                                        proposal_net_args_list=[{**prop, "max_res": 64}, {**prop, "max_res": 256}])
    tr = NerfplayerTrainer(cfg, 128, 5, aabb_scale=1.0, device="cpu")
    root = tr._named_module()
    model = NerfplayerNerfactoModel(cfg, SceneBox(torch.tensor(tr.aabb)), 5)
    got, want = CK.reference_state_dict(root), CK.reference_state_dict(model)
    assert list(got) == list(want)
    assert "_model.field.embedding_appearance.embedding.weight" in got and "_model.proposal_networks.1.encoding.index_list" in got
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    CK.load_reference_state_dict(model, got, strict=True)
    assert torch.equal(model.field.mlp_base.embeddings.detach(), tr.enc.embeddings.detach())
    assert set(tr._CK_NAMES.values()) == set(tr.off)  # every segment of the flat buffer has a checkpoint name
    with torch.no_grad():
        tr.exp_avg.copy_(torch.arange(tr.n_params, dtype=torch.float32))
    moments = {ck: (tr.mviews[seg], tr.vviews[seg], 3) for ck, seg in tr._CK_NAMES.items()}
    back = CK.import_optimizer_states(root, CK.export_optimizer_states(root, moments, {}))
    assert sorted(back) == sorted(tr._CK_NAMES)
    for ck, (m, _, step) in back.items():
        assert step == 3 and torch.equal(m.reshape(-1), tr.mviews[tr._CK_NAMES[ck]].reshape(-1)), ck

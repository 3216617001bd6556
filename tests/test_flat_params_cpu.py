"""The flat parameter store every fused trainer builds on (soccernerfs_amd/fused_step.py: FlatParams), on the CPU with stand-in modules, and the one
proposal update schedule against the np.clip(np.interp(...)) form the two NeRFPlayer trainers used to spell out."""
import numpy as np
import pytest
import torch

from soccernerfs_amd import exchange_plan as XP
from soccernerfs_amd.fused_step import FlatParams, update_schedule


class _Mod(torch.nn.Module):
    """A module with one parameter `attr` of the given shape (values 1, 2, 3, ... so that every float is distinguishable)."""

    def __init__(self, attr, *shape):
        super().__init__()
        n = int(np.prod(shape))
        setattr(self, attr, torch.nn.Parameter(torch.arange(1, n + 1, dtype=torch.float32).reshape(shape)))


# a small K-Planes shape whose segment sizes are NOT multiples of 4 (nor of 4 * world), so that every alignment rule shows
SMALL = dict(base_res=(5, 6, 7, 3), multiscale=(1, 2), feature_dim=3, proposal_resolutions=((9, 9, 9, 3), (11, 10, 9, 3)), proposal_feature_dim=1)
MLP = {"prop": 577, "sigma": 1001, "color": 333}


def _kplanes_order():
    reso = [[r * m for r in SMALL["base_res"][:3]] + list(SMALL["base_res"][3:]) for m in SMALL["multiscale"]]
    order = []
    for i, r in enumerate(SMALL["proposal_resolutions"]):
        order += [(f"prop{i}.planes", _Mod("planes", XP.plane_layout(SMALL["proposal_feature_dim"], [list(r)])[1]), "planes"),
                  (f"prop{i}.mlp", _Mod("params", MLP["prop"]), "params")]
    order += [("field.planes", _Mod("planes", XP.plane_layout(SMALL["feature_dim"], reso)[1]), "planes"),
              ("field.sigma", _Mod("params", MLP["sigma"]), "params"), ("field.color", _Mod("params", MLP["color"]), "params")]
    return order


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_kplanes_layout_matches_the_exchange_plan(world):
    fp = FlatParams(_kplanes_order(), "cpu", shaped=False, pad_to={"field.planes": 4 * world})
    sz = XP.kplanes_segment_sizes(SMALL["base_res"], SMALL["multiscale"], SMALL["feature_dim"], SMALL["proposal_resolutions"], SMALL["proposal_feature_dim"], MLP, world)
    assert any(n % 4 for _, n in fp.off.values())  # the shape exercises the alignment
    assert all(o % 4 == 0 for o, _ in fp.off.values())
    o, n = fp.off["field.planes"]
    assert fp.n_params == sz["n_params"] and (o, n) == (sz["field_offset"], sz["field_floats"])
    assert fp.off["field.sigma"][0] - o == sz["field_padded"] and sz["field_padded"] % (4 * world) == 0
    assert [s[3] for s in fp.segments] == sorted(s[3] for s in fp.segments) and [(s[3], s[4]) for s in fp.segments] == [fp.off[s[0]] for s in fp.segments]
    assert fp.params.numel() == fp.grads.numel() == fp.exp_avg.numel() == fp.exp_avg_sq.numel() == fp.n_params and fp.grads_fx is None
    # the pads stay zero, the segments hold the modules' values
    used = torch.zeros(fp.n_params, dtype=torch.bool)
    for name, (o, n) in fp.off.items():
        used[o:o + n] = True
        assert torch.equal(fp.params[o:o + n], torch.arange(1, n + 1, dtype=torch.float32))
    assert float(fp.params[~used].abs().sum()) == 0.0


@pytest.mark.parametrize("shaped", [False, True])
def test_views_alias_the_modules_both_ways(shaped):
    table, net = _Mod("embeddings", 37, 6), _Mod("params", 53)
    fp = FlatParams([("t", table, "embeddings"), ("n", net, "params")], "cpu", deterministic=True, shaped=shaped)
    assert fp.off == {"t": (0, 222), "n": (224, 53)} and fp.n_params == 224 + 56
    assert fp.views["t"].shape == ((37, 6) if shaped else (222,)) and fp.gviews["t"].shape == fp.views["t"].shape == fp.mviews["t"].shape == fp.vviews["t"].shape
    assert table.embeddings.shape == ((37, 6) if shaped else (222,))
    # a write through the view is seen by the module's parameter and by the flat buffer, and the other way round
    fp.views["t"].view(-1)[5] = -7.0
    assert float(table.embeddings.detach().view(-1)[5]) == -7.0 and float(fp.params[5]) == -7.0
    with torch.no_grad():
        net.params[3] = 11.5
    assert float(fp.views["n"][3]) == 11.5 and float(fp.params[224 + 3]) == 11.5
    for d, flat in ((fp.gviews, fp.grads), (fp.mviews, fp.exp_avg), (fp.vviews, fp.exp_avg_sq)):
        d["n"][2] = 3.0
        assert float(flat[224 + 2]) == 3.0
    # the fixed-point cells behind a gradient view: same offsets, same length, 8-byte cells
    for name, (o, n) in fp.off.items():
        cells = fp.fx(fp.gviews[name])
        assert cells.dtype == torch.int64 and cells.numel() == n and cells.data_ptr() == fp.grads_fx.data_ptr() + 8 * o
        assert fp.fxviews[name].data_ptr() == cells.data_ptr() and fp.fxviews[name].shape == fp.gviews[name].shape
    part = fp.gviews["n"][8:20]  # a view of a view (a layer's weights inside a net's segment)
    assert fp.fx(part).data_ptr() == fp.grads_fx.data_ptr() + 8 * (224 + 8) and fp.fx(part).numel() == 12
    # another live buffer (K-Planes' ping-pong): modules and views follow
    other = torch.zeros_like(fp.params)
    fp._repoint(other)
    assert fp.params is other and table.embeddings.data_ptr() == other.data_ptr() and fp.views["n"].data_ptr() == other.data_ptr() + 4 * 224


def test_update_schedule_equals_the_interp_form():
    warmup, every = 5000, 5  # the presets' proposal_warmup / proposal_update_every
    steps = np.arange(0, 31001)
    ref = np.clip(np.interp(steps, [0, warmup], [0, every]), 1, every)
    got = np.array([update_schedule(int(s), warmup, every) for s in steps])
    for count in range(0, 7):  # ProposalNetworkSampler: update when steps_since_update > schedule
        assert np.array_equal(count > got, count > ref), count

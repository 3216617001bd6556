"""CPU: the view-dependent K-Planes colour path (KPlanesTrainConfig.disable_viewing_dependent = False; ABI 16) -- its entry points are declared and
exported, its `_supported` probes accept exactly the 31 -> 64 -> 64 -> 3 colour net, and the switch defaults to the `k-planes` preset (no compute)."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

NEW = ("snerf_kplanes_color_input_fwd", "snerf_kplanes_color_input_bwd", "snerf_kplanes_color_bwd_vd", "snerf_kplanes_color_bwd_vd_ws",
       "snerf_kplanes_color_bwd_vd_supported")


def _desc(d_in, hidden=64, n_hidden=2, d_out=3, hidden_act=1, out_act=1, operands=1):
    from soccernerfs_amd import _lib

    d = _lib.MlpDesc()
    d.d_in, d.hidden, d.n_hidden, d.d_out, d.hidden_act, d.out_act, d.operands = d_in, hidden, n_hidden, d_out, hidden_act, out_act, operands
    return d


def test_new_symbols_declared_and_exported():
    from soccernerfs_amd import _lib, build

    build.build(verbose=False)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snerf.h")).read(), flags=re.S)
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", txt), s
        assert s in _lib.EXPORTS and hasattr(l, s), s
    assert _lib.ABI_VERSION == 16 == l.snerf_abi_version()


def test_supported_probes_accept_the_view_dependent_colour_net_only():
    from soccernerfs_amd import _lib
    from soccernerfs_amd.plane_set import PlaneSet

    l = _lib.lib()
    for ops_ in (1, 2):
        assert l.snerf_kplanes_color_bwd_vd_supported(C.byref(_desc(31, operands=ops_))) == 1
    for bad in (_desc(15), _desc(32), _desc(31, operands=0), _desc(31, hidden=128), _desc(31, n_hidden=1), _desc(31, d_out=4), _desc(31, out_act=0)):
        assert l.snerf_kplanes_color_bwd_vd_supported(C.byref(bad)) == 0
    assert l.snerf_kplanes_color_bwd_vd_supported(None) == 0
    # the fused field forward: both colour nets with 16-bit operands, nothing in between, never fp32
    ps = PlaneSet(32, [[8, 8, 8, 4], [16, 16, 16, 4]], concat=True)
    dp = ps.desc()
    sig = _desc(64, hidden=128, n_hidden=1, d_out=16, out_act=0)
    for d_in, want in ((15, 1), (31, 1), (23, 0), (32, 0)):
        assert l.snerf_kplanes_field_fwd_supported(C.byref(dp), C.byref(sig), C.byref(_desc(d_in))) == want, d_in
    assert l.snerf_kplanes_field_fwd_supported(C.byref(dp), C.byref(_desc(64, 128, 1, 16, 1, 0, 0)), C.byref(_desc(31, operands=0))) == 0
    assert l.snerf_mlp_supported(C.byref(_desc(31))) == 1  # the generic 16-bit kernels (unfused / deterministic paths) take the shape too


def test_switch_defaults_to_the_preset():
    from soccernerfs_amd.kplanes import KPlanesModelConfig
    from soccernerfs_amd.trainer import KPlanesTrainConfig

    assert KPlanesTrainConfig().disable_viewing_dependent is True
    assert KPlanesTrainConfig.__dataclass_fields__["disable_viewing_dependent"].default is True
    assert KPlanesModelConfig.k_planes_preset().disable_viewing_dependent is True

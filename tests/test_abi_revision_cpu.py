"""CPU: the additions of the rendering round are counted as a REVISION of ABI 16 -- header, library and binding agree on it, the version
itself stays 16 for the callers pinned to it, and the new entry points are declared, exported and bound."""
import os
import re

from tests.conftest import ROOT

NEW = ["snerf_abi_revision", "snerf_raygen_frame", "snerf_kplanes_field_render", "snerf_kplanes_field_render_supported"]


def test_revision_agrees_between_header_library_and_binding():
    from soccernerfs_amd import _lib, build

    build.build(verbose=False)
    txt = open(os.path.join(ROOT, "include", "snerf.h")).read()
    header_version = int(re.search(r"#define\s+SNERF_ABI_VERSION\s+(\d+)", txt).group(1))
    header_revision = int(re.search(r"#define\s+SNERF_ABI_REVISION\s+(\d+)", txt).group(1))
    l = _lib.lib()
    assert header_version == _lib.ABI_VERSION == l.snerf_abi_version() == 16
    assert header_revision == _lib.ABI_REVISION == l.snerf_abi_revision() >= 1


def test_render_entries_declared_exported_and_bound():
    import ctypes as C

    from soccernerfs_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snerf.h")).read(), flags=re.S)
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", txt), s
        assert s in _lib.EXPORTS and hasattr(l, s), s
    # the float argument of the render kernel must be declared, or ctypes would pass it as an int
    assert l.snerf_kplanes_field_render.argtypes[8] is C.c_float
    # snerf_raygen_frame_args: 4 + 12 + 1 floats, W, H, pad, two int64, 7 floats + pad, 7 pointers
    assert C.sizeof(_lib.RaygenFrameArgs) == 68 + 12 + 16 + 28 + 4 + 7 * 8


def test_render_kernel_refuses_shapes_it_is_not_built_for():
    """The shape probe runs on the host: S must be a multiple of 32 up to 320, operands 16-bit."""
    import ctypes as C

    from soccernerfs_amd import _lib
    from soccernerfs_amd.plane_set import PlaneSet
    from soccernerfs_amd.tcnn_compat import Network

    l = _lib.lib()
    ps = PlaneSet(32, [[8, 8, 8, 4], [16, 16, 16, 4]], concat=True)
    mk = lambda i, o, h, nh, act, ops_: Network(i, o, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": act, "n_neurons": h,
                                                        "n_hidden_layers": nh}, seed=1, operands=ops_)
    probe = lambda sigma, color, S: l.snerf_kplanes_field_render_supported(C.byref(ps.desc()), C.byref(sigma.desc), C.byref(color.desc), S)
    s16, c16, cvd = mk(64, 16, 128, 1, "None", "bf16"), mk(15, 3, 64, 2, "Sigmoid", "bf16"), mk(31, 3, 64, 2, "Sigmoid", "bf16")
    assert [probe(s16, c16, S) for S in (32, 64, 320)] == [1, 1, 1] and probe(s16, cvd, 64) == 1
    assert [probe(s16, c16, S) for S in (0, 16, 48, 352)] == [0, 0, 0, 0]
    assert probe(mk(64, 16, 128, 1, "None", "fp32"), mk(15, 3, 64, 2, "Sigmoid", "fp32"), 64) == 0

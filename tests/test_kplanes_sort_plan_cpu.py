"""Host side of the sample sort (no GPU): snerf_kplanes_sort_workspace sizes the two workspaces from the plan, and refuses planes larger than the
largest tested plan (finest resolution 2048) instead of planning them."""
import ctypes as C

import pytest

from soccernerfs_amd import _lib


def _desc(resolutions, n_coords=4, channels=32):
    d = _lib.KPlanesDesc()
    d.n_scales, d.C, d.concat, d.n_coords = len(resolutions), channels, 1, n_coords
    for s, reso in enumerate(resolutions):
        for k, r in enumerate(reso):
            d.res[s][k] = r
    return d


def _workspace(desc, N):
    hc, ie = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().snerf_kplanes_sort_workspace(C.byref(desc), C.c_int64(N), C.byref(hc), C.byref(ie)), "sort_workspace")
    return hc.value, ie.value


@pytest.mark.parametrize("ms", [(1, 2, 4, 8, 16), (1, 2, 4, 8, 16, 32)])
def test_workspace_follows_the_entries_not_the_cells(ms):
    N = 262144
    hist, index = _workspace(_desc([[64 * m] * 3 + [100] for m in ms]), N)
    assert index == 6 * N  # also sizes sorted_rec
    records = 4 * 6 * N  # the intermediate records, in int32 words
    assert records < hist < records + (1 << 21)  # + count matrix, totals, bases: under 8 MB whatever the finest scale
    assert _workspace(_desc([[64, 64, 64]], n_coords=3), 1000)[1] == 3 * 1000
    assert _workspace(_desc([[8, 8, 8, 4]]), 0)[1] == 0


def test_planes_beyond_the_tested_size_are_refused():
    _workspace(_desc([[2048, 2048, 2048, 100]]), 1000)
    with pytest.raises(RuntimeError, match="finest resolution above 2048"):
        _workspace(_desc([[4096, 4096, 4096, 100]]), 1000)

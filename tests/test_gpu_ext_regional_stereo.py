"""The device entries of the stereographic regional grids (ogg_regional_stereo_tables_dev / ogg_regional_stereo_band_dev) held to their
extents with the harness of tests/test_gpu_extents.py, exactly as tests/test_gpu_ext_regional.py holds the other kinds: every case
runs plain, with every byte of the arena 0xFF and with seeded random bytes; the guard bands must be intact and the three results the
same bytes.  The six fields and the workspace are exact-size views of the arena, flush against their guards: a wavefront's last lane,
which computes a column it does not own, the lanes beyond a row's last point or last cell, the last row's missing dy and area, the
tables' one line beyond the grid, and a band that begins in the middle of the arrays must write nothing else.  The cases are recorded
in that module's COVERED set, which its census (test_every_device_entry_ran_guarded) reads: this module's name sorts before it, so in
a run of the whole GPU suite the entries are covered when the census runs."""
import numpy as np
import pytest

import test_gpu_extents as TE
from test_gpu_extents import arena, record_entries, three_runs   # noqa: F401  (fixtures of the harness)

pytestmark = pytest.mark.gpu
FAR_BELOW = TE.PEAK_USED // 4
ENTRIES = {"ogg_regional_stereo_tables_dev", "ogg_regional_stereo_band_dev"}


@pytest.fixture(scope="module")
def S(hip):
    from ocean_model_grid_generator_amd import regional_stereo
    return regional_stereo


@pytest.mark.parametrize("lat_c", [55.0, 90.0])
@pytest.mark.parametrize("metrics", [True, False])
@pytest.mark.parametrize("nx, ny", [(2, 2), (130, 4), (4, 130)])
def test_the_two_entries(S, arena, three_runs, nx, ny, metrics, lat_c):
    for bands in (1, 3, ny + 1):
        res = three_runs(lambda: S.stereo_grid_dev(-140.5, lat_c, nx, ny, 0.25, tilt=40.0, metrics=metrics, bands=bands),
                         "regional stereo %dx%d lat_c=%g metrics=%s bands=%d" % (nx, ny, lat_c, metrics, bands))
        assert ENTRIES <= TE.COVERED
        assert sorted(res) == (sorted(S.FIELDS) if metrics else ["x", "y"])
        for f, v in res.items():
            a = np.frombuffer(v[3], dtype=np.float64)
            assert v[2] == S.shapes(nx, ny)[f] and np.all(np.isfinite(a)), f
    assert arena.used(guards=True) < FAR_BELOW

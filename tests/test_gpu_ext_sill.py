"""The device entry of the sill depths (ogg_sill_depth_dev) held to its extents with the harness of tests/test_gpu_extents.py: every
case runs plain, with every byte of the arena 0xFF and with seeded random bytes; the guard bands must be intact and the three results
the same bytes.  The weights, the seeds, the workspace and the five outputs are exact-size views of the arena, flush against their
guards: the last column's seam partner, the last row's fold partner, the faces that are never read, the tile cells beyond the grid and
the reach words that every round zeroes must neither write nor depend on anything else.  The cases are recorded in that module's
COVERED set, which its census (test_every_device_entry_ran_guarded) reads: this module's name sorts before it, as
tests/test_gpu_ext_regional.py explains."""
import numpy as np
import pytest

import sill_definition as D
import test_gpu_extents as TE
from test_gpu_extents import arena, record_entries, three_runs   # noqa: F401  (fixtures of the harness)

pytestmark = pytest.mark.gpu
FAR_BELOW = TE.PEAK_USED // 4
ENTRY = "ogg_sill_depth_dev"


@pytest.fixture(scope="module")
def S(hip):
    from ocean_model_grid_generator_amd import sill_depth
    return sill_depth


@pytest.mark.parametrize("topology", [0, 1, 2, 3])
@pytest.mark.parametrize("bits", [1, 30])
@pytest.mark.parametrize("ny, nx", [(2, 2), (130, 4), (4, 130)])
def test_the_entry(S, arena, three_runs, ny, nx, bits, topology):
    rng = np.random.default_rng(100 * ny + 10 * bits + topology)
    top = (1 << bits) - 1
    wu, wv = rng.integers(-1, top + 2, (ny, nx + 1)), rng.integers(-1, top + 2, (ny + 1, nx))
    seeds = np.array([ny * nx - 1, 0, ny * nx, -7], dtype=np.int64)

    def run():
        return S.sill_depth_faces_dev(TE.up(wu), TE.up(wv), TE.up(seeds), bool(topology & 1), bool(topology & 2), bits)
    res = three_runs(run, "sill %dx%d bits=%d topology=%d" % (ny, nx, bits, topology))
    assert ENTRY in TE.COVERED
    want = D.sill(wu, wv, seeds, topology, bits)
    for k in ("b", "region", "gate_u", "gate_v"):
        assert res[k][3] == want[k].tobytes(), k
    assert res["counts"] == want["counts"]
    assert arena.used(guards=True) < FAR_BELOW

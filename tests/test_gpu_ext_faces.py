"""The device entry of face topography (ogg_topog_faces_dev) held to its extents with the harness of tests/test_gpu_extents.py: every
case runs plain, with every byte of the arena 0xFF and with seeded random bytes; the guard bands must be intact and the three results
the same bytes.  The records of the two families and the workspace are exact-size views of the arena, flush against their guards: the
lanes beyond a face's last sample or last line, the faces beyond a row's last, row ranges that start in the middle of the grid, rows
padded to a stride ld, and the periodic and fold partners that lie at the far end of the arrays must write nothing else.  The cases
are recorded in that module's COVERED set, which its census (test_every_device_entry_ran_guarded) reads: this module's name sorts
before it, as tests/test_gpu_ext_regional.py explains."""
import numpy as np
import pytest

import small_grids as G
import test_gpu_extents as TE
from test_gpu_extents import arena, record_entries, three_runs   # noqa: F401  (fixtures of the harness)

pytestmark = pytest.mark.gpu
FAR_BELOW = TE.PEAK_USED // 4
ENTRY = "ogg_topog_faces_dev"


@pytest.fixture(scope="module")
def mods(hip):
    from ocean_model_grid_generator_amd import face_topography, topography
    return face_topography, topography


def source(T, kind):
    r = G.raster(kind)
    return T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])


@pytest.mark.parametrize("topology", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["int16_fill2", "float32_q0.01", "window"])
@pytest.mark.parametrize("ny, nx", [(2, 2), (130, 4), (4, 130)])
def test_the_entry(mods, arena, three_runs, ny, nx, kind, topology):
    FT, T = mods
    x, y = G.grid(ny, nx, lon0=97.0, shear=True)
    src = source(T, kind)
    nym = ny // 2
    ranges = [(None, None), ((nym // 2, nym), (nym // 2 + 1, nym + 1)), ((0, 0), (nym, nym + 1)), ((nym - 1, nym), (1, 1))]
    for pad in (0, 3):
        xp, yp = (np.pad(a, ((0, 0), (0, pad)), constant_values=np.nan) for a in (x, y))     # a row stride of nx + 1 + pad
        for refine in (None, 9, 65):
            for u_rows, v_rows in ranges:
                def run():
                    dev = T.DeviceSource(src, TE.DEV, sea_level=0.5)
                    xd, yd = TE.up(xp)[:, :nx + 1], TE.up(yp)[:, :nx + 1]
                    res = FT.face_topography_dev(xd, yd, dev, refine=refine, topology=topology, u_rows=u_rows, v_rows=v_rows)
                    return {fam: res[fam]["records"] for fam in ("u", "v")}
                res = three_runs(run, "faces %dx%d %s topology=%d pad=%d refine=%s rows=%s %s" % (ny, nx, kind, topology, pad, refine, u_rows, v_rows))
                assert ENTRY in TE.COVERED
                nu = nym if u_rows is None else u_rows[1] - u_rows[0]
                nv = nym + 1 if v_rows is None else v_rows[1] - v_rows[0]
                assert res["u"][2] == (nu, nx // 2 + 1) and res["v"][2] == (nv, nx // 2)
    assert arena.used(guards=True) < FAR_BELOW

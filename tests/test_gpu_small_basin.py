"""GPU tests of the basin codes on the hand-made meshes of tests/small_meshes.py: every small shape under several masks, and the
four (periodic, fold) cuts of the golden tripolar grid, where walls of land leave the seam and the fold as the only ways from one
band of water to the next, so a flood crosses them exactly when the flag says so; a fold of odd width; periodic bands one and two
cells wide.  Everything against tests/basin_definition.py, bit for bit, through the checks of test_gpu_basin_codes.run."""
import numpy as np
import pytest

import small_meshes as sm
from test_gpu_basin_codes import FULL, centre, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def BC(hip):
    from ocean_model_grid_generator_amd import basin_codes as m
    return m


def shape_of(g):
    return (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2


@pytest.mark.parametrize("name", sorted(sm.SHAPES))
def test_every_small_shape(BC, name):
    g = sm.shape_grid(name)
    ny, nx = shape_of(g)
    periodic, fold = sm.SHAPE_TOPOLOGY.get(name, (False, False))
    j, i = np.indices((ny, nx))
    rules = [(1,) + centre(g, 0, 0) + FULL, (2,) + centre(g, ny - 1, nx - 1) + FULL, (3,) + centre(g, ny // 2, nx // 2) + FULL]
    for wet in (np.ones((ny, nx), np.uint8), ((i + j) % 2).astype(np.uint8), np.zeros((ny, nx), np.uint8), sm.wet_mask(ny, nx)):
        for p, f in {(periodic, fold), (False, False)}:
            res = run(BC, g["x"], g["y"], wet, rules, p, f, host=wet.all())
        if wet.all():
            assert np.all(res["code"] == 1) and res["records"]["status"].tolist() == [0, 3, 3]
        if not wet.any():
            assert res["records"]["status"].tolist() == [1, 1, 1] and res["counts"]["wet"] == 0


def banded(ny, nx):
    """walls of land in the columns nx // 4 and nx // 2: the bands A (west of the first), B (between them) and C (east of the second).
    The seam joins A and C; the fold joins column i of the top row to column nx - 1 - i, so A and B both to C."""
    wet = np.ones((ny, nx), np.uint8)
    wet[:, nx // 4] = wet[:, nx // 2] = 0
    band = np.zeros((ny, nx), np.int8)   # 0: wall, 1: A, 2: B, 3: C
    band[:, :nx // 4], band[:, nx // 4 + 1:nx // 2], band[:, nx // 2 + 1:] = 1, 2, 3
    return wet, band


@pytest.mark.parametrize("name", sorted(sm.CUTS))
def test_floods_cross_the_seam_and_the_fold_exactly_when_the_flag_says_so(BC, name):
    g = sm.topology_cuts()[name]
    ny, nx = shape_of(g)
    wet, band = banded(ny, nx)
    rules = [(5,) + centre(g, 2, 1) + FULL]
    for periodic in (False, True):
        for fold in (False, True):
            res = run(BC, g["x"], g["y"], wet, rules, periodic, fold, host=(periodic, fold) == g["topology"])
            reached = sorted(set(band[res["code"] == 5].tolist()))
            assert reached == ([1, 2, 3] if fold else ([1, 3] if periodic else [1])), (periodic, fold)
            assert np.all(res["code"][np.isin(band, reached)] == 5)   # and every cell of a band that is reached
    # the cut's own topology, under rules whose boxes cut the real coordinates
    lon, lat = centre(g, ny // 2, 3 * nx // 4)
    rules = [(1,) + centre(g, 2, 1) + (-180.0, 180.0, -90.0, float(np.nanmedian(g["y"]))),
             (2, lon, lat, lon - 40.0, lon + 40.0, -90.0, 90.0), (3,) + centre(g, ny - 1, nx - 2) + FULL, (1,) + centre(g, ny - 1, 1) + FULL]
    res = run(BC, g["x"], g["y"], wet, rules, *g["topology"])
    assert res["counts"]["coded"] > 0.5 * wet.sum() and len(set(res["records"]["status"].tolist())) >= 1
    from ocean_model_grid_generator_amd import ocean_mask as M
    assert M.detect_topology(g["x"], g["y"], 2) == g["topology"]


def test_fold_of_odd_width(BC):
    g = sm.shape_grid("fold_5x7")
    wet = np.zeros((5, 7), np.uint8)
    wet[4] = 1
    wet[4, 3] = 0   # the top row without its middle cell: the halves meet through the fold alone
    rules = [(1,) + centre(g, 4, 0) + FULL]
    res = run(BC, g["x"], g["y"], wet, rules, False, True, host=True)
    assert res["code"][4].tolist() == [1, 1, 1, 0, 1, 1, 1]
    res = run(BC, g["x"], g["y"], wet, rules, False, False)
    assert res["code"][4].tolist() == [1, 1, 1, 0, 0, 0, 0]
    wet[:] = 1   # the middle cell is its own partner
    res = run(BC, g["x"], g["y"], wet, rules, False, True)
    assert np.all(res["code"] == 1)


@pytest.mark.parametrize("name", ["band_2x1", "band_3x1", "band_2x2", "band_3x2"])
def test_periodic_bands_one_and_two_cells_wide(BC, name):
    g = sm.shape_grid(name)
    ny, nx = shape_of(g)
    wet = np.ones((ny, nx), np.uint8)
    wet[ny - 1, 0] = 0
    rules = [(1,) + centre(g, 0, 0) + FULL, (2,) + centre(g, ny - 1, nx - 1) + FULL]
    for periodic in (True, False):
        for fold in (True, False):
            res = run(BC, g["x"], g["y"], wet, rules, periodic, fold)
            assert np.array_equal(res["code"], wet) and res["records"]["cells"][0] == wet.sum()

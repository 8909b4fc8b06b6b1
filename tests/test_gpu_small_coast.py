"""GPU tests of the distance to the coast on hand-made inputs (tests/small_meshes.py, tests/coast_inputs.py): flag bytes, coastal
lists, nearest and d2 bit for bit against the definition in tests/coast_distance_definition.py run on the device's own unit vectors,
for every small shape and topology cut under six masks, grids around the tile's size, coastal sets around the chunk's size, and
degenerate geometry: NaN and pole cells, scattered centres, a coast across the seam, an antipodal target, exact and near ties.
tests/test_coast_distance_cpu.py checks on the CPU that each named input reaches its branch."""
import numpy as np
import pytest

import coast_distance_definition as D
import coast_inputs as CI
import small_meshes as sm

pytestmark = pytest.mark.gpu
RE = sm.RE


@pytest.fixture(scope="module")
def CD(hip):
    from ocean_model_grid_generator_amd import coast_distance as m
    return m


def run(CD, x, y, wet, periodic, fold, sides="both", host=False):
    """the device result, checked against the definition: flags, lists, unit vectors, nearest and d2, counts"""
    import torch
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    wet = np.ascontiguousarray(wet, dtype=np.uint8)
    res = CD.coast_distance_dev(to(x), to(y), wet, sides=sides, periodic=periodic, fold=fold, Re=RE, keep_lists=True)
    fl = D.flags(x, y, wet, periodic, fold)
    assert np.array_equal(res["flags"], fl)
    L, W = D.sets(fl)
    assert np.array_equal(res["land_cell"], L) and np.array_equal(res["wet_cell"], W)
    assert res["land_u"].tobytes() == res["u"][L].tobytes() and res["wet_u"].tobytes() == res["u"][W].tobytes()
    lon, lat = D.centres(x, y)
    ok = ((fl & D.F_VALID) != 0).reshape(-1)
    u_np = D.unit(lon.reshape(-1)[ok], lat.reshape(-1)[ok])
    assert np.max(np.abs(res["u"][ok] - u_np), initial=0.0) <= 4e-16
    n, d2 = D.coast_distance(res["u"], fl, sides)
    assert np.array_equal(res["nearest"], n) and res["d2"].tobytes() == d2.tobytes()
    qw, ql = D.queries(fl, sides)
    c = res["counts"]
    assert (c["coast_wet"], c["coast_land"], c["queries"], c["answered"]) == (W.size, L.size, qw.size + ql.size, int((n >= 0).sum()))
    assert not np.any(res["nearest"].reshape(-1) == np.arange(fl.size))
    if host:
        h = CD.coast_distance(x, y, wet, sides=sides, periodic=periodic, fold=fold, Re=RE)
        for k in ("nearest", "d2", "flags", "distance", "nearest_j", "nearest_i", "wet", "coast"):
            assert h[k].tobytes() == res[k].tobytes(), k
        assert h["summary"] == res["summary"]
    return res


def masks(ny, nx):
    one_land, one_wet = np.ones((ny, nx), np.uint8), np.zeros((ny, nx), np.uint8)
    one_land[ny // 2, nx // 2] = 0
    one_wet[ny // 2, nx // 2] = 1
    j, i = np.indices((ny, nx))
    return {"one_land": one_land, "one_wet": one_wet, "checkerboard": ((i + j) % 2).astype(np.uint8), "all_wet": np.ones((ny, nx), np.uint8),
            "all_land": np.zeros((ny, nx), np.uint8), "wet_mask": sm.wet_mask(ny, nx)}


@pytest.mark.parametrize("name", sorted(sm.SHAPES) + sorted(sm.CUTS))
def test_every_shape_and_cut_under_six_masks(CD, name):
    if name in sm.CUTS:
        g = sm.topology_cuts()[name]
        periodic, fold = g["topology"]
    else:
        g = sm.shape_grid(name)
        periodic, fold = sm.SHAPE_TOPOLOGY.get(name, (False, False))
    ny, nx = (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2
    for mname, wet in masks(ny, nx).items():
        res = run(CD, g["x"], g["y"], wet, periodic, fold, host=mname == "wet_mask")
        if mname in ("all_wet", "all_land"):
            assert np.all(res["nearest"] == -1) and np.all(np.isposinf(res["d2"])) and np.all(res["distance"] == 1e20)
    # the topology read from the grid's corner points is the one the shapes are listed with
    from ocean_model_grid_generator_amd import ocean_mask as M
    assert M.detect_topology(g["x"], g["y"], 2) == (periodic, fold)


@pytest.mark.parametrize("ny", [15, 16, 17])
@pytest.mark.parametrize("nx", [15, 16, 17])
def test_grids_around_the_tile_size(CD, ny, nx, monkeypatch):
    g = sm.latlon_grid(ny, nx)
    want = run(CD, g["x"], g["y"], sm.wet_mask(ny, nx), False, False)
    assert want["counts"]["tiles"] == ((ny + 15) // 16) * ((nx + 15) // 16)
    monkeypatch.setenv("OGG_COAST_TILE_X", str(nx - 1))   # and a tile one cell narrower and one shorter than the grid
    monkeypatch.setenv("OGG_COAST_TILE_Y", str(min(ny - 1, 256 // (nx - 1))))
    res = run(CD, g["x"], g["y"], sm.wet_mask(ny, nx), False, False)
    assert res["counts"]["tiles"] >= 4 and res["d2"].tobytes() == want["d2"].tobytes()


@pytest.mark.parametrize("n", [31, 32, 33])
def test_coastal_sets_around_the_chunk_size(CD, n, monkeypatch):
    c = CI.coast_of(n)
    monkeypatch.setenv("OGG_COAST_CHUNK", "32")
    monkeypatch.setenv("OGG_COAST_CUBES", "1")   # one cube holds every target: n targets are n - 1, n and n + 1 of a chunk
    res = run(CD, c["x"], c["y"], c["wet"], False, False, sides="wet")
    assert res["counts"]["coast_land"] == n and res["counts"]["cubes"] == 1
    assert res["counts"]["tests"] == res["counts"]["queries"] * n
    monkeypatch.setenv("OGG_COAST_BRUTE", "1")
    brute = run(CD, c["x"], c["y"], c["wet"], False, False, sides="wet")
    assert brute["counts"]["cubes"] == 0 and brute["counts"]["tests"] == res["counts"]["tests"]


def test_zoo_row(CD):
    x, y, where = sm.cell_zoo()
    nx = (x.shape[1] - 1) // 2
    res = run(CD, x, y, sm.zoo_mask(nx), False, False, host=True)
    fl = res["flags"][0]
    for name in ("nan_lat", "nan_lon"):   # the cell's centre is the mean of its corners: not finite
        assert not fl[where[name]] & D.F_VALID and res["nearest"][0, where[name]] == -1
    assert fl[where["four_poles"]] & D.F_VALID and fl[where["point"]] & D.F_VALID
    assert res["counts"]["answered"] == int(((fl & D.F_VALID) != 0).sum())


@pytest.mark.parametrize("name", sorted(CI.CASES))
def test_named_inputs(CD, name, monkeypatch):
    c = CI.CASES[name]()
    res = run(CD, c["x"], c["y"], c["wet"], c["periodic"], c["fold"], host=True)
    if name == "exact_tie":
        assert np.all(res["nearest"][c["wet"] != 0] == 6)
    if name == "antipodal":
        assert res["nearest"][0, 1] == 0 and 4.0 - res["d2"][0, 1] < 1e-15
        assert abs(res["distance"][0, 1] - np.pi * RE) < 1.0
    if name == "seam_band":
        assert np.all(res["nearest"][:, 0] % 36 == 34)
    if name == "invalid_centres":
        assert res["nearest"][1, 2] == -1 and res["nearest"][2, 4] == -1
    for sides in ("wet", "land"):
        run(CD, c["x"], c["y"], c["wet"], c["periodic"], c["fold"], sides=sides)
    for knobs in (dict(OGG_COAST_BRUTE="1"), dict(OGG_COAST_CUBES="128"), dict(OGG_COAST_CUBES="3", OGG_COAST_CHUNK="1"),
                  dict(OGG_COAST_TILE_X="5", OGG_COAST_TILE_Y="3")):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        other = run(CD, c["x"], c["y"], c["wet"], c["periodic"], c["fold"])
        assert other["nearest"].tobytes() == res["nearest"].tobytes() and other["d2"].tobytes() == res["d2"].tobytes(), knobs
        for k in knobs:
            monkeypatch.delenv(k)

"""GPU tests of point location and sampling on hand-made inputs (tests/small_meshes.py): the corner table, cell, s, t, m, values and
flags bit for bit and at every point against the definition in tests/locate_definition.py run on the device's own corner table and
query vectors (tests/locate_inputs.py), for the four topology cuts, the cell zoo, the small shapes and a fold of odd width; query
counts around the workgroup's size, none at all, all in one cube, longitudes two turns away; the same answers under a permutation of
the queries, for every knob and through the host-pointer entry; and properties of the sampling that do not come from the definition."""
import numpy as np
import pytest

import locate_definition as D
import locate_inputs as LI
import small_meshes as sm
from test_locate_cpu import cut_queries

pytestmark = pytest.mark.gpu
KEYS = ("cell", "s", "t", "margin")


@pytest.fixture(scope="module")
def LOC(hip):
    from ocean_model_grid_generator_amd import locate as m
    return m


def grid_of(name):
    if name in sm.CUTS:
        g = sm.topology_cuts()[name]
        return g["x"], g["y"], g["topology"]
    g = sm.shape_grid(name)
    return g["x"], g["y"], sm.SHAPE_TOPOLOGY.get(name, (False, False))


def same(a, b, keys=KEYS):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


@pytest.mark.parametrize("name", sorted(sm.CUTS))
def test_topology_cuts(LOC, name):
    x, y, (periodic, fold) = grid_of(name)
    lon, lat = cut_queries(dict(x=x, y=y, topology=(periodic, fold)), 11)
    ll, la = LI.line_points(x, y, fold)
    res = LI.check(LOC, x, y, np.concatenate([lon, ll]), np.concatenate([lat, la]), periodic, fold)
    assert np.all(res["cell"][:lon.size] >= 0)          # every point of the CPU test's set gets a cell
    assert res["counts"]["cubes"] > 1 and res["counts"]["tests"] < 0.2 * res["cell"].size * res["shape"][0] * res["shape"][1]
    from ocean_model_grid_generator_amd import ocean_mask as M
    assert M.detect_topology(x, y, 2) == (periodic, fold)


@pytest.mark.parametrize("cubes", ["0", "32", "128"])
def test_zoo_row(LOC, cubes, monkeypatch):
    """pole corners in every arrangement, clockwise, collapsed, bow-tie and NaN-cornered cells, and the 172-degree-wide cell, which is
    on the large-cells list once the cubes are smaller than it"""
    if cubes != "0":
        monkeypatch.setenv("OGG_LOCATE_CUBES", cubes)
    x, y, where = sm.cell_zoo()
    ny, nx = LI.shape_of(x)
    lon, lat = D.mesh_queries(x, y)
    rl, ra, rc = LI.interior_points(x, y, np.random.default_rng(3), 2000, 0.0, 1.0)
    res = LI.check(LOC, x, y, np.concatenate([lon, rl]), np.concatenate([lat, ra]), False, False)
    g = D.cells(res["cu"], ny, nx)
    for name in ("nan_lat", "nan_lon", "point", "parallel"):
        assert g["sigma"][where[name]] == 0 and not np.any(res["cell"] == where[name]), name
    for name in ("ordinary", "on_edges", "seam", "north_corner", "south_corner", "two_adjacent", "clockwise", "long"):
        assert g["sigma"][where[name]] != 0 and np.any(res["cell"] == where[name]), name
    assert g["sigma"][where["clockwise"]] == -1 and g["sigma"][where["ordinary"]] == 1
    G = res["counts"]["cubes"]
    large = LI.large_cells(res["cu"], ny, nx, G)
    assert res["counts"]["large_cells"] == int(large.sum())
    if cubes != "0":
        assert G == int(cubes) and large[where["long"]]
    else:
        assert G == 1 and not large.any()


@pytest.mark.parametrize("name", ["1x1", "1x63", "1x64", "1x65", "129x1", "band_2x1", "band_2x2", "band_3x1", "band_3x2", "fold_5x7"])
def test_small_shapes(LOC, name):
    x, y, (periodic, fold) = grid_of(name)
    lon, lat = D.mesh_queries(x, y)
    rl, ra, rc = LI.interior_points(x, y, np.random.default_rng(4), 1000, 0.0, 1.0)
    ll, la = LI.line_points(x, y, fold)
    res = LI.check(LOC, x, y, np.concatenate([lon, rl, ll]), np.concatenate([lat, ra, la]), periodic, fold)
    if name.startswith("band_"):
        # a cell 360 degrees wide has its west and east corners in one point (the periodic copy): S and N are collapsed, E = -W, so
        # O = 0 and it holds no point; a cell 180 degrees wide has great-circle S and N edges over the pole.  Only the definition is held.
        if name.endswith("x1"):
            assert np.all(res["cell"] == -1) and res["counts"]["outside"] == int(np.isfinite(res["qu"]).all(axis=1).sum())
    else:
        assert (res["cell"] >= 0).sum() > 1000


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_query_counts_around_the_workgroup_size(LOC, n):
    g = sm.latlon_grid(9, 11)
    x, y, periodic, fold = g["x"], g["y"], False, False
    lon, lat, c = LI.interior_points(x, y, np.random.default_rng(n), n)
    res = LI.check(LOC, x, y, lon, lat, periodic, fold)
    assert res["cell"].size == n and np.array_equal(res["cell"], c)
    host = LOC.locate(x, y, lon, lat, periodic=periodic, fold=fold)
    assert same(host, res) and host["counts"] == res["counts"]


def test_all_queries_in_one_cube_and_spread_over_many(LOC, monkeypatch):
    x, y, (periodic, fold) = grid_of("full")
    rng = np.random.default_rng(8)
    lon, lat = 20.0 + 0.5 * rng.random(3000), 10.0 + 0.5 * rng.random(3000)          # half a degree square: one cube of 10 per axis
    res = LI.check(LOC, x, y, lon, lat, periodic, fold)
    G = res["counts"]["cubes"]
    assert np.unique(LI.cube_of(res["qu"], G) @ np.array([1, G, G * G])).size == 1 and np.all(res["cell"] >= 0)
    monkeypatch.setenv("OGG_LOCATE_CUBES", "128")                                      # and about one query per cube
    lon, lat = 360.0 * rng.random(3000), 170.0 * rng.random(3000) - 85.0
    res = LI.check(LOC, x, y, lon, lat, periodic, fold)
    assert np.unique(LI.cube_of(res["qu"], 128) @ np.array([1, 128, 128 * 128])).size > 2500


@pytest.mark.parametrize("name", ["full", "periodic_only", "neither"])
def test_longitudes_two_turns_away(LOC, name):
    x, y, (periodic, fold) = grid_of(name)
    lon, lat, c = LI.interior_points(x, y, np.random.default_rng(6), 2000)             # s, t in [0.05, 0.95] by construction
    res = LI.check(LOC, x, y, lon, lat, periodic, fold)
    assert np.array_equal(res["cell"], c)
    for turn in (-720.0, 720.0):
        other = LI.check(LOC, x, y, lon + turn, lat, periodic, fold)
        assert np.array_equal(other["cell"], c)
        assert np.abs(other["s"] - res["s"]).max() <= 1e-9 and np.abs(other["t"] - res["t"]).max() <= 1e-9


@pytest.mark.parametrize("name", ["full", "neither"])
def test_answers_do_not_depend_on_order_index_or_entry(LOC, name, monkeypatch):
    x, y, (periodic, fold) = grid_of(name)
    lon, lat = cut_queries(dict(x=x, y=y, topology=(periodic, fold)), 12)
    rng = np.random.default_rng(1)
    keep = rng.choice(lon.size, 20000, replace=False)
    lon, lat = lon[keep], lat[keep]
    dev = (LI.to_device(x), LI.to_device(y))
    run = lambda a, b: LOC.locate_dev(dev[0], dev[1], a, b, periodic=periodic, fold=fold)   # noqa: E731
    want = LI.check(LOC, x, y, lon, lat, periodic, fold, xy_dev=dev)
    perm = rng.permutation(lon.size)
    got = run(lon[perm], lat[perm])
    assert all(got[k].tobytes() == want[k][perm].tobytes() for k in KEYS)
    for cubes in ("1", "4", "64"):
        monkeypatch.setenv("OGG_LOCATE_CUBES", cubes)
        got = run(lon, lat)
        assert same(got, want) and got["counts"]["cubes"] == int(cubes), cubes
        if int(cubes) < want["counts"]["cubes"]:
            assert got["counts"]["tests"] > want["counts"]["tests"]
    monkeypatch.delenv("OGG_LOCATE_CUBES")
    monkeypatch.setenv("OGG_LOCATE_BRUTE", "1")
    brute = run(lon[:4000], lat[:4000])
    valid = int((D.cells(want["cu"], *LI.shape_of(x))["sigma"] != 0).sum())
    assert brute["counts"]["cubes"] == 0 and brute["counts"]["large_cells"] == valid and brute["counts"]["tests"] == 4000 * valid
    assert all(brute[k].tobytes() == want[k][:4000].tobytes() for k in KEYS)
    monkeypatch.delenv("OGG_LOCATE_BRUTE")
    host = LOC.locate(x, y, lon, lat, periodic=periodic, fold=fold)
    assert same(host, want) and host["counts"] == want["counts"]
    assert LOC.locate(x, y, lon, lat)["periodic"] == periodic                           # the topology read from the grid


# ---- sampling --------------------------------------------------------------------------------------------------
def test_linear_field_on_the_interior(LOC):
    ny, nx = 9, 11
    g = sm.latlon_grid(ny, nx)
    j, i = np.indices((ny, nx))
    f = (3.0 * i + 5.0 * j)[None]
    lon, lat, c = LI.interior_points(g["x"], g["y"], np.random.default_rng(2), 3000, 0.0, 1.0)
    res = LI.check(LOC, g["x"], g["y"], lon, lat, False, False, field=f)
    inner = (res["cell_j"] > 0) & (res["cell_j"] < ny - 1) & (res["cell_i"] > 0) & (res["cell_i"] < nx - 1)
    want = 3.0 * (res["cell_i"] + res["s"] - 0.5) + 5.0 * (res["cell_j"] + res["t"] - 0.5)
    smp = res["samples"][0]
    assert inner.sum() > 1500 and np.all(smp["flags"][0][inner] == 1)
    assert np.abs(smp["values"][0] - want)[inner].max() <= 1e-12
    edge = (res["cell"] >= 0) & ~inner
    assert np.all(np.isin(smp["flags"][0][edge], (1, 2))) and np.any(smp["flags"][0][edge] == 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_field_across_the_seam_and_the_fold(LOC, dtype):
    x, y, (periodic, fold) = grid_of("full")
    ny, nx = LI.shape_of(x)
    f = np.full((2, ny, nx), 7.3, dtype)
    lon, lat, c = LI.interior_points(x, y, np.random.default_rng(9), 4000, 0.0, 1.0)
    ll, la = LI.line_points(x, y, fold)
    res = LI.check(LOC, x, y, np.concatenate([lon, ll]), np.concatenate([lat, la]), periodic, fold, field=f)
    smp = res["samples"][0]
    has = res["cell"] >= 0
    const = float(dtype(7.3))
    assert np.all(np.abs(smp["values"][:, has] - const) <= 4 * np.spacing(const))
    top, side = res["cell_j"] == ny - 1, (res["cell_i"] == 0) | (res["cell_i"] == nx - 1)
    assert top.sum() > 20 and side.sum() > 20 and np.all(smp["flags"][:, has & (res["cell_j"] > 0)] == 1)   # seam and fold: full stencils


def test_fold_symmetric_field_at_mirror_cells(LOC):
    """a field symmetric under the fold map (j, i) -> (j, nx - 1 - i) sampled at a point of cell (j, i) at (s, t) and at a point of
    its mirror cell at (1 - s, t) uses mirrored stencils with the same weights: the same values"""
    x, y, (periodic, fold) = grid_of("full")
    ny, nx = LI.shape_of(x)
    rng = np.random.default_rng(10)
    half = rng.random((ny, nx))
    f = (half + half[:, ::-1])[None]
    n = 3000
    cell = (rng.integers(ny - 6, ny, n) * nx + rng.integers(0, nx, n)).astype(np.int32)
    s, t = rng.random(n), rng.random(n)
    mirror = ((cell // nx) * nx + (nx - 1 - cell % nx)).astype(np.int32)
    from ocean_model_grid_generator_amd import _lib as L
    import ctypes
    out = []
    for c, ss in ((cell, s), (mirror, 1.0 - s)):
        p = LOC.params(ny, nx, n, periodic, fold, "bilinear", 1, np.float64)
        v, fl, cnt = np.empty((1, n)), np.empty((1, n), np.uint8), L.LocateCounts()
        ss = np.ascontiguousarray(ss)
        L.call("ogg_locate_sample", ctypes.byref(p), c.ctypes.data, ss.ctypes.data, t.ctypes.data, f.ctypes.data, None, v.ctypes.data,
               fl.ctypes.data, ctypes.byref(cnt))
        dv, dfl = D.sample(c, ss, t, f, None, ny, nx, periodic, fold)
        assert v.tobytes() == dv.tobytes() and fl.tobytes() == dfl.tobytes()
        out.append((v, fl))
    exact = np.abs(s - 0.5) == np.abs((1.0 - s) - 0.5)                              # 1 - s rounds for some s: fx differs in the last bit
    assert exact.sum() > 1000 and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][0][0][exact], out[1][0][0][exact]) and np.abs(out[0][0] - out[1][0]).max() <= 1e-14


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["bilinear", "cell"])
def test_mask_and_missing_values(LOC, dtype, mode):
    x, y, (periodic, fold) = grid_of("fold_only")
    ny, nx = LI.shape_of(x)
    rng = np.random.default_rng(13)
    f = (10.0 * rng.random((3, ny, nx))).astype(dtype)
    for k, v in enumerate((np.nan, -999.0, 1.0e20)):
        f[:, rng.random((ny, nx)) < 0.05] = v
    f[1][rng.random((ny, nx)) < 0.3] = -999.0
    wet = sm.wet_mask(ny, nx)
    lon, lat, c = LI.interior_points(x, y, np.random.default_rng(14), 6000, 0.0, 1.0)
    res = LI.check(LOC, x, y, np.concatenate([lon, [np.nan, 0.0]]), np.concatenate([lat, [0.0, -89.9]]), periodic, fold, field=f, wet=wet,
                   mode=mode, fills=(-999.0, 1.0e20))
    smp = res["samples"][0]
    cell = res["cell"]
    dry = (cell >= 0) & (wet.reshape(-1)[np.maximum(cell, 0)] == 0)
    assert dry.sum() > 100 and np.all(smp["flags"][:, dry] == 3) and np.all(smp["values"][:, dry] == 1.0e20)
    assert np.all(smp["flags"][:, cell < 0] == 0) and np.all(smp["values"][:, cell < 0] == 1.0e20) and (cell < 0).sum() >= 1
    used = smp["flags"] != 3
    assert np.all(np.isfinite(smp["values"])) and np.all(smp["values"][used & (smp["flags"] > 0)] <= 10.0)
    if mode == "bilinear":
        assert (smp["flags"] == 2).sum() > 500 and (smp["flags"] == 1).sum() > 500
    else:
        assert not np.any(smp["flags"] == 2) and (smp["flags"] == 1).sum() > 500
    # without the fill values the 1e20 and -999 count as data: other values, no fewer full stencils
    other = LOC.locate_dev(LI.to_device(x), LI.to_device(y), lon, lat, periodic=periodic, fold=fold, field=f, wet=wet, mode=mode)
    assert (other["samples"][0]["flags"] == 1).sum() > (smp["flags"] == 1).sum()


def test_refusals_on_the_device_path(LOC):
    g = sm.latlon_grid(4, 5)
    with pytest.raises(ValueError, match="the field ends in \\(4, 6\\), the grid has 4 x 5 model cells"):
        LOC.sample(g["x"], g["y"], [-30.0], [-20.0], np.zeros((4, 6)))
    with pytest.raises(ValueError, match="the wet mask is \\(5, 4\\), the model cells \\(4, 5\\)"):
        LOC.sample(g["x"], g["y"], [-30.0], [-20.0], np.zeros((4, 5)), wet=np.ones((5, 4)))
    with pytest.raises(ValueError, match="2 longitudes and 1 latitudes"):
        LOC.locate(g["x"], g["y"], [1.0, 2.0], [3.0])
    res = LOC.sample(g["x"], g["y"], [-29.0, 50.0], [-20.5, 0.0], np.arange(20.0).reshape(4, 5), mode="cell")
    assert res["cell"].tolist() == [1, -1] and res["samples"][0]["values"].tolist() == [1.0, 1.0e20]
    assert res["samples"][0]["flags"].tolist() == [1, 0]

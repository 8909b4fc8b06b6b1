"""CPU tests of point location: the definition alone (tests/locate_definition.py, numpy's unit vectors), the recorded fact behind
OGG_LOCATE_TOL, the coverage of the four topology cuts, a closed-form truth on a regular grid, and the host-side argument checks and
points-file parser of ocean_model_grid_generator_amd.locate.  tests/test_gpu_locate.py and tests/test_gpu_small_locate.py hold the
device to this definition bit for bit."""
import numpy as np
import pytest

import locate_definition as D
import small_meshes as sm


def shape_of(x):
    return (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2


def define(x, y, lon, lat, periodic=False, fold=False, tol=D.TOL):
    ny, nx = shape_of(x)
    cu = D.corner_table(x, y, periodic, fold)
    assert D.is_canonical(cu, ny, nx, periodic, fold)
    return D.locate(cu, D.unit(lon, lat), ny, nx, tol=tol)


# ---- the tolerance stands on a recorded fact -------------------------------------------------------------------
JITTERED = [(1.0, -10.0), (0.01, 60.0), (3.0, -88.0), (0.125, 80.0)]   # spacing, base latitude (degrees)


@pytest.mark.parametrize("spacing,lat0", JITTERED)
def test_worst_best_margin_at_vertices_and_edges(spacing, lat0):
    """Near a vertex the rounded half-plane tests of the cells around it can disagree in a pinwheel, so that no cell has m >= 0.  On
    four jittered meshes of 12 x 14 cells the queries are the interior corners, the edge midpoints and their 1-ulp neighbours, and the
    best key over ALL cells whose box holds the query is measured: some of the queries have no cell with m >= 0, and the worst best-m
    stays above -2^-53, a hundred times inside OGG_LOCATE_TOL = 2^-50."""
    x, y = D.jittered_mesh(spacing, lat0)
    ny, nx = shape_of(x)
    inner = np.zeros(x.shape, bool)
    inner[2:-2, 2:-2] = True
    inner[1::2, 1::2] = False          # corners and edge midpoints, not centres
    lon, lat = x[inner], y[inner]
    ul, ua = D.ulp_neighbours(lon, lat)
    lon, lat = np.concatenate([lon, ul]), np.concatenate([lat, ua])
    cell, _, _, m = define(x, y, lon, lat, tol=np.inf)
    assert np.all(cell >= 0)
    worst = float(m.min())
    print("spacing %g at %g: %d queries, %.1f%% with best m < 0, worst best-m %.3g" % (spacing, lat0, m.size, 100.0 * np.mean(m < 0), worst))
    assert worst > -2.0 ** -53
    # and with the tolerance every one of them has a cell, the same cell
    c2, _, _, m2 = define(x, y, lon, lat)
    assert np.array_equal(c2, cell) and m2.tobytes() == m.tobytes()


def test_edge_measure_is_antisymmetric_bit_for_bit():
    rng = np.random.default_rng(5)
    a, b, p = (D.unit(360 * rng.random(20000), 180 * rng.random(20000) - 90) for _ in range(3))
    t1, t2 = D.dot3(p, D.cross(a, b)), D.dot3(p, D.cross(b, a))
    assert (-t1).tobytes() == t2.tobytes()
    x, y = D.jittered_mesh(0.125, 80.0)
    g = D.cells(D.corner_table(x, y, False, False), *shape_of(x))
    nx = shape_of(x)[1]
    n = g["n"].reshape(-1, nx, 4, 3)
    assert (-n[:, :-1, 1]).tobytes() == np.ascontiguousarray(n[:, 1:, 3]).tobytes()     # E of a cell, W of its east neighbour
    assert (-n[:-1, :, 2]).tobytes() == np.ascontiguousarray(n[1:, :, 0]).tobytes()     # N of a cell, S of its north neighbour


def test_enumeration_equals_the_plain_matrix():
    x, y = D.jittered_mesh(3.0, -88.0)
    ny, nx = shape_of(x)
    lon, lat = D.mesh_queries(x, y)
    lon, lat = np.concatenate([lon, [np.nan, 0.0, np.inf, 200.0]]), np.concatenate([lat, [0.0, np.nan, 0.0, 0.0]])
    cu, qu = D.corner_table(x, y, False, False), D.unit(lon, lat)
    cell, _, _, m = D.locate(cu, qu, ny, nx, pairs=1000)
    c2, m2 = D.locate_matrix(cu, qu, ny, nx)
    assert np.array_equal(cell, c2) and m.tobytes() == m2.tobytes()
    assert np.all(cell[-4:] == -1) and np.all(np.isnan(m[-4:]))


# ---- the topology cuts -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cuts():
    return sm.topology_cuts()


def cut_queries(g, seed):
    """the mesh's own supergrid points (corners, edge midpoints, centres), their 1-ulp neighbours, and 5,000 random points north of
    the southern edge"""
    x, y = g["x"], g["y"]
    lon, lat = D.mesh_queries(x, y)
    rng = np.random.default_rng(seed)
    south = float(y[0].max())
    periodic = g["topology"][0]
    if periodic:   # with a fold the grid reaches the pole; without, up to its top row
        north = 89.99 if g["topology"][1] else float(y[-1].min()) - 0.01
        rl = 360.0 * rng.random(5000) - 300.0
        ra = south + 0.01 + (north - south - 0.01) * rng.random(5000)
    else:   # a cut in longitude: random points of the cells themselves
        ny, nx = shape_of(x)
        j, i = rng.integers(0, ny, 5000), rng.integers(0, nx, 5000)
        u = D.unit(x, y)
        w = rng.random((5000, 4)) + 0.05
        p = sum(w[:, k, None] * u[2 * j + dj, 2 * i + di] for k, (dj, di) in enumerate(((0, 0), (0, 2), (2, 2), (2, 0))))
        p /= np.linalg.norm(p, axis=1)[:, None]
        rl, ra = np.degrees(np.arctan2(p[:, 1], p[:, 0])), np.degrees(np.arcsin(np.clip(p[:, 2], -1, 1)))
    return np.concatenate([lon, rl]), np.concatenate([lat, ra])


@pytest.mark.parametrize("name", sorted(sm.CUTS))
def test_every_point_of_a_cut_gets_a_cell(cuts, name):
    g = cuts[name]
    periodic, fold = g["topology"]
    lon, lat = cut_queries(g, 11)
    cell, s, t, m = define(g["x"], g["y"], lon, lat, periodic, fold)
    assert np.all(cell >= 0), (int((cell < 0).sum()), lon[cell < 0][:5], lat[cell < 0][:5])
    assert np.all((s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)) and np.all(m >= -D.TOL)
    # a cell's own centre returns that cell
    ny, nx = shape_of(g["x"])
    centre = np.zeros(g["x"].shape, bool)
    centre[1::2, 1::2] = True
    k = np.nonzero(centre.reshape(-1))[0]
    assert np.array_equal(cell[k], np.arange(ny * nx))


def test_points_off_the_grid_and_not_finite_get_no_cell(cuts):
    """south, west, east and north of a regional grid (33W .. 0, 21S .. 3S: its southern edge bulges 0.0066 degrees to the south),
    north of the top row of the cut without a fold, and coordinates that are not finite.  (The cuts themselves reach the south pole.)"""
    g = sm.latlon_grid(9, 11)
    lon = np.array([-20.0, -10.0, -34.0, 0.5, -10.0, 160.0, np.nan, -10.0, np.inf, -np.inf, -20.0, -10.0])
    lat = np.array([-22.0, -21.5, -10.0, -10.0, -2.9, 10.0, -10.0, np.nan, -10.0, -10.0, np.inf, -np.inf])
    cell, s, t, m = define(g["x"], g["y"], lon, lat)
    assert np.all(cell == -1) and np.all(np.isnan(s)) and np.all(np.isnan(t)) and np.all(np.isnan(m))
    assert define(g["x"], g["y"], [-20.0, -10.0], [-20.5, -21.0])[0].tolist() == [4, 7]
    c = cuts["periodic_only"]
    top = float(c["y"][-1].max())
    cell = define(c["x"], c["y"], [0.0, 100.0, -250.0], [top + 1.0, 89.0, 90.0], True, False)[0]
    assert np.all(cell == -1)


# ---- closed-form truth -----------------------------------------------------------------------------------------
def test_regular_grid_closed_form():
    """Points at (i + alpha, j + beta) cells of a 3 x 2 degree grid, alpha, beta in {0.1, 0.5, 0.9}, return exactly (j, i), with s and
    t near alpha and beta.  The edges are great circles, not parallels: the edge between two corners 3 degrees apart on the grid's
    row of highest |latitude| (21 degrees) bulges by 3.28e-3 of the 2-degree cell height at its middle (measured below), which is
    more than 2e-3, so the bound is twice the measured bulge."""
    ny, nx = 9, 11
    g = sm.latlon_grid(ny, nx)
    x, y = g["x"], g["y"]
    row = int(np.argmax(np.abs(y[::2, 0]))) * 2
    a, b = D.unit(x[row, 0], y[row, 0]), D.unit(x[row, 2], y[row, 2])
    mid = (a + b) / np.linalg.norm(a + b)
    bulge = abs(np.degrees(np.arcsin(mid[2])) - y[row, 0]) / 2.0
    print("bulge of a 3-degree edge at latitude %g: %.3e of the cell height" % (y[row, 0], bulge))
    assert 3.2e-3 < bulge < 3.4e-3
    bound = 2.0 * bulge if bulge > 2e-3 else 2e-3
    fr = np.array([0.1, 0.5, 0.9])
    J, I, B, A = np.meshgrid(np.arange(ny), np.arange(nx), fr, fr, indexing="ij")
    lon, lat = (x[0, 0] + 3.0 * (I + A)).reshape(-1), (y[0, 0] + 2.0 * (J + B)).reshape(-1)
    cell, s, t, _ = define(x, y, lon, lat)
    assert np.array_equal(cell, (J * nx + I).reshape(-1))
    print("largest |s - alpha| %.3e, |t - beta| %.3e" % (np.abs(s - A.reshape(-1)).max(), np.abs(t - B.reshape(-1)).max()))
    assert np.abs(s - A.reshape(-1)).max() <= bound and np.abs(t - B.reshape(-1)).max() <= bound


# ---- sampling, on the definition -------------------------------------------------------------------------------
def test_sampling_definition_linear_and_flags():
    ny, nx = 6, 8
    j, i = np.indices((ny, nx))
    f = (3.0 * i + 5.0 * j)[None]
    rng = np.random.default_rng(2)
    cell = (rng.integers(1, ny - 1, 500) * nx + rng.integers(1, nx - 1, 500)).astype(np.int32)
    s, t = rng.random(500), rng.random(500)
    v, fl = D.sample(cell, s, t, f, None, ny, nx, False, False)
    want = 3.0 * (cell % nx + s - 0.5) + 5.0 * (cell // nx + t - 0.5)
    assert np.all(fl == 1) and np.abs(v[0] - want).max() < 1e-12
    wet = np.ones((ny, nx), np.uint8)
    wet[2, 3] = 0
    v, fl = D.sample(np.array([2 * nx + 3, 2 * nx + 4, 2 * nx + 4, -1]), np.array([0.5, 0.2, 0.7, np.nan]), np.array([0.5, 0.5, 0.5, np.nan]),
                     f, wet, ny, nx, False, False)
    assert list(fl[0]) == [3, 2, 1, 0] and v[0, 0] == D.FILL and v[0, 3] == D.FILL
    v, fl = D.sample(np.array([0, nx - 1]), np.array([0.2, 0.9]), np.array([0.1, 0.5]), f, None, ny, nx, False, False, mode=D.CELL)
    assert list(fl[0]) == [1, 1] and list(v[0]) == [0.0, 3.0 * (nx - 1)]


# ---- the package's host side -----------------------------------------------------------------------------------
def test_parameter_refusals():
    from ocean_model_grid_generator_amd import locate as LOC
    with pytest.raises(ValueError, match="mode must be one of bilinear, cell"):
        LOC.params(4, 4, 10, mode="nearest")
    with pytest.raises(ValueError, match="ny, nx >= 1 and ny \\* nx \\* 27 < 2\\^31"):
        LOC.params(0, 4, 10)
    with pytest.raises(ValueError, match="ny \\* nx \\* 27 < 2\\^31"):
        LOC.params(10000, 10000, 10)
    with pytest.raises(ValueError, match="-1 queries: 0 <= n < 2\\^31"):
        LOC.params(4, 4, -1)
    with pytest.raises(ValueError, match="at most 2 fill values"):
        LOC.params(4, 4, 1, fill_values=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="float32 or float64"):
        LOC.params(4, 4, 1, dtype=np.int32)
    p = LOC.params(4, 5, 7, periodic=True, fold=True, mode="cell", nrec=3, dtype=np.float32, fill_values=(-999.0,))
    assert (p.ny, p.nx, p.n, p.nrec, p.topology, p.mode, p.dtype, p.n_fill, p.fill[0]) == (4, 5, 7, 3, 3, 0, 0, 1, -999.0)


def test_main_flag_refusals():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    with pytest.raises(ValueError, match="--locate_mode must be bilinear or cell, not 'nearest'"):
        ogg.main(1.0, locate_points="p.txt", locate_mode="nearest")
    with pytest.raises(ValueError, match="--locate_file and --locate_mode need --locate_points"):
        ogg.main(1.0, locate_mode="cell")
    with pytest.raises(ValueError, match="--locate_file and --locate_mode need --locate_points"):
        ogg.main(1.0, locate_file="other.nc", path="functions")


def test_points_file_parser(tmp_path):
    from ocean_model_grid_generator_amd import locate as LOC
    from ocean_model_grid_generator_amd import netcdf3
    path = tmp_path / "points.txt"
    path.write_text("# moorings\n-140.5 0.25 TAO_140W   # on the equator\n\n 35 -60.0\n1e1 2e1 last\n")
    lon, lat, names = LOC.read_points(str(path))
    assert list(lon) == [-140.5, 35.0, 10.0] and list(lat) == [0.25, -60.0, 20.0] and names == ["TAO_140W", "", "last"]
    path.write_text("1 2\n3 4\n")
    assert LOC.read_points(str(path))[2] is None
    for text, msg in (("1 2 a b\n", "points.txt:1: 4 values: lon lat \\[name\\]"), ("1\n", "1 values"), ("# nothing\n", "no points"),
                      ("1 2\nx 3\n", "points.txt:2: two numbers are needed: x 3")):
        path.write_text(text)
        with pytest.raises(ValueError, match=msg):
            LOC.read_points(str(path))
    nc = tmp_path / "points.nc"
    ds = netcdf3.Dataset(str(nc), [("point", 3)])
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("point",), [], np.array([1.0, 2.0, 3.5]))
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("point",), [], np.array([-1.0, -2.0, 80.0]))
    ds.write()
    lon, lat, names = LOC.read_points(str(nc))
    assert list(lon) == [1.0, 2.0, 3.5] and list(lat) == [-1.0, -2.0, 80.0] and names is None


def test_written_file_and_summary(tmp_path):
    from ocean_model_grid_generator_amd import locate as LOC
    from ocean_model_grid_generator_amd import netcdf3
    cell = np.array([7, -1, 0], np.int32)
    counts = dict(zip(LOC.L.LOCATE_COUNT_FIELDS, (2, 1, 0, 0, 3, 30, 0, 0, 0, 0)))
    res = LOC.result(cell, np.array([0.25, np.nan, 1.0]), np.array([0.5, np.nan, 0.0]), np.array([0.01, np.nan, 0.0]), counts,
                     np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0]), (3, 5), True, False, names=["a", "", "gauge"])
    fld = LOC.Field(np.zeros((2, 3, 5), np.float32), name="temp", lead_dims=[("time", 2)])
    res["samples"].append({"name": "temp", "values": np.arange(6.0).reshape(2, 3), "flags": np.array([[1, 0, 2], [3, 0, 1]], np.uint8),
                           "mode": "bilinear", "field": fld, "counts": {"flag0": 2, "flag1": 2, "flag2": 1, "flag3": 1}})
    lines = LOC.summary_lines(res)
    assert "3 points on 5 x 3 cells (periodic): 2 located, 1 outside the grid, 0 not finite" in lines[0]
    assert "point 1 at lon 2.000000, lat 5.000000 is in no cell" in lines[1] and "temp (bilinear)" in lines[2]
    out = tmp_path / "p.nc"
    LOC.write_locate(str(out), res)
    h = netcdf3.read_header(str(out))
    assert h.vars["temp"].shape == (2, 3) and h.vars["temp_locate_flag"].shape == (2, 3) and h.vars["name"].shape == (3, 5)
    ints = {k: np.frombuffer(netcdf3.read_var_bytes(str(out), h, k, dtype=netcdf3.NC_INT), ">i4") for k in ("cell_j", "cell_i")}
    assert list(ints["cell_j"]) == [1, -1, 0] and list(ints["cell_i"]) == [2, -1, 0]
    assert netcdf3.read_doubles(str(out), names=("temp",))["temp"].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert netcdf3.read_var_bytes(str(out), h, "name", dtype=netcdf3.NC_CHAR) == b"a\0\0\0\0" + b"\0" * 5 + b"gauge"

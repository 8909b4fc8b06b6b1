"""CPU tests of the bilinear interpolation: the definition's own properties (tests/bilinear_definition.py: constants, a field linear in
latitude, an analytic field against the interpolation bound, the seam, the nodes, missing corners, the rotation), the library's
checks and refusals (no device work), main()'s flags and the file writer."""
import ctypes

import numpy as np
import pytest

import bilinear_definition as D

EPS = 2.0 ** -53


def edges(kind):
    """a regular 1-degree source, or the remap tests' source of non-uniform latitudes (not reaching the poles) with an odd lon0"""
    if kind == "regular":
        return 360.0 * np.arange(361) / 360, -90.0 + 180.0 * np.arange(181) / 180
    lat = 88.0 * np.sin(0.5 * np.pi * np.linspace(-1.0, 1.0, 121))
    return -17.3 + 360.0 * np.arange(251) / 250, lat


def random_points(n, seed, lat_max=90.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-300.0, 420.0, n), rng.uniform(-lat_max, lat_max, n)


# ---- the definition's properties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "gaussian"])
def test_constants_come_back_within_eight_roundings(kind):
    """at most three roundings per weight, one per product and three additions: 8 * 2^-53 * |c|, also where corners are missing"""
    lon, lat = edges(kind)
    x, y = random_points(2_000_000, 11)
    I, I1, wx, J, J1, wy = D.locate(x, y, lon, lat)
    assert np.all((wx >= 0) & (wx < 1)) and np.all((wy >= 0) & (wy <= 1))
    assert I.min() >= 0 and I.max() == lon.size - 2 and J.min() == 0 and J.max() == lat.size - 2
    c = 17.25
    f = np.full((1, lat.size - 1, lon.size - 1), c)
    v, fl = D.interpolate(x, y, lon, lat, f)
    worst = np.abs(v - c).max() / (EPS * c)
    print("constant, %s: %.2f units of 2^-53 |c|" % (kind, worst))
    assert np.all(fl == D.REMAPPED) and worst <= 8.0
    f[0][np.random.default_rng(5).random(f.shape[1:]) < 0.3] = np.nan
    v, fl = D.interpolate(x, y, lon, lat, f)
    got = fl[0] == D.REMAPPED
    assert 0.9 < got.mean() < 1.0 and np.all(v[0][~got] == D.FILL) and np.all(fl[0][~got] == D.UNFILLED)
    worst = np.abs(v[0][got] - c).max() / (EPS * c)
    print("constant with 30 %% missing, %s: %.2f units" % (kind, worst))
    assert worst <= 8.0


@pytest.mark.parametrize("kind", ["regular", "gaussian"])
def test_linear_in_latitude_and_the_clamps(kind):
    lon, lat = edges(kind)
    _, latc = D.centres(lon, lat)
    f = np.broadcast_to(latc[:, None], (1, latc.size, lon.size - 1)).copy()
    x, y = random_points(1_000_000, 12)
    v, _ = D.interpolate(x, y, lon, lat, f)
    inside = (y >= latc[0]) & (y <= latc[-1])
    worst = np.abs(v[0][inside] - y[inside]).max() / (EPS * 90.0)
    print("linear in latitude, %s: %.2f units of 2^-53 * 90" % (kind, worst))
    assert inside.sum() > 900_000 and worst <= 8.0
    # beyond the first and last centre: the clamped value (the weights in longitude still round: the same bound)
    assert np.abs(v[0][y < latc[0]] - latc[0]).max() <= 8.0 * EPS * 90.0 and np.abs(v[0][y > latc[-1]] - latc[-1]).max() <= 8.0 * EPS * 90.0
    assert (y < latc[0]).any() and (y > latc[-1]).any()


def test_analytic_field_stays_below_the_interpolation_bound():
    """sin(lon) cos(lat) on a regular 1-degree source: per direction the error of linear interpolation is at most h^2 / 8 times the
    second derivative (at most 1), and the cross term h^4 / 64: derived, not fitted"""
    h = np.radians(1.0)
    bound = h * h / 8 * 2 + h ** 4 / 64
    assert abs(bound - 7.6156e-5) < 1e-9
    lon, lat = edges("regular")
    lonc, latc = D.centres(lon, lat)
    f = (np.sin(np.radians(lonc))[None, :] * np.cos(np.radians(latc))[:, None])[None]
    x, y = random_points(3_000_000, 13, lat_max=89.5)
    v, fl = D.interpolate(x, y, lon, lat, f)
    err = np.abs(v[0] - np.sin(np.radians(x)) * np.cos(np.radians(y))).max()
    print("analytic field: %.4e (bound %.4e)" % (err, bound))
    assert np.all(fl == D.REMAPPED) and err < bound
    assert err > 0.9 * bound   # the points do reach the worst case: the bound is not slack


def test_seam_nodes_and_missing_corners():
    lon, lat = edges("gaussian")
    lonc, latc = D.centres(lon, lat)
    NA, NB = lonc.size, latc.size
    rng = np.random.default_rng(3)
    f = rng.standard_normal((2, NB, NA))
    # between the last and the first centre, on either side of the seam and a turn away
    xs = np.array([lonc[-1] + 0.3, lonc[0] - 0.3, lonc[0] - 0.3 + 360.0, lonc[-1] + 0.3 - 720.0])
    I, I1, wx, _, _, _ = D.locate(xs, np.zeros(4), lon, lat)
    assert np.all(I == NA - 1) and np.all(I1 == 0) and np.all((wx > 0) & (wx < 1))
    # on a node: that node's value, bit for bit (every node, every record)
    X, Y = np.meshgrid(lonc, latc)
    v, fl = D.interpolate(X, Y, lon, lat, f)
    assert v.tobytes() == f.tobytes() and np.all(fl == D.REMAPPED)
    v, _ = D.interpolate(X, Y, lon, lat, f.astype(np.float32))
    assert v.tobytes() == f.astype(np.float32).astype(np.float64).tobytes()
    # four missing corners: unfilled; one valid corner of non-zero weight: its value within one rounding of the division
    g = f.copy()
    g[:, 40:42, 100:102] = np.nan
    px, py = 0.5 * (lonc[100] + lonc[101]) + 0.1, 0.5 * (latc[40] + latc[41]) + 0.1
    v, fl = D.interpolate(np.array([px]), np.array([py]), lon, lat, g, fills=())
    assert np.all(fl[:, 0] == D.UNFILLED) and np.all(v[:, 0] == D.FILL)
    g[:, 41, 101] = f[:, 41, 101]
    v, fl = D.interpolate(np.array([px]), np.array([py]), lon, lat, g)
    assert np.all(fl[:, 0] == D.REMAPPED)
    assert np.all(np.abs(v[:, 0] - f[:, 41, 101]) <= 2 * EPS * np.abs(f[:, 41, 101]))
    # fill values are compared in the source's own type; a vector's corner is valid only where both components are
    g32 = f.astype(np.float32)
    g32[:, 40:42, 100:102] = np.float32(-999.0)
    v, fl = D.interpolate(np.array([px]), np.array([py]), lon, lat, g32, fills=(-999.0,))
    assert np.all(fl[:, 0] == D.UNFILLED)
    (u, w), fl = D.interpolate(np.array([px, px + 20]), np.array([py, py]), lon, lat, f, g)
    assert np.all(fl[:, 0] == D.REMAPPED) and np.all(fl[:, 1] == D.REMAPPED)
    assert np.all(np.abs(u[:, 0] - f[:, 41, 101]) <= 2 * EPS * np.abs(f[:, 41, 101]))
    # a mask: dry cells carry flag 0 and the fill value
    v, fl = D.interpolate(X[:2, :3], Y[:2, :3], lon, lat, f, mask=np.array([[1, 0, 1], [0, 1, 1]]))
    assert np.array_equal(fl[0], [[1, 0, 1], [0, 1, 1]]) and v[1, 0, 1] == D.FILL and v[1, 1, 0] == D.FILL


def test_rotation_keeps_the_speed_and_turns_back():
    rng = np.random.default_rng(4)
    n = 1_000_000
    U, V = rng.standard_normal(n) * 10, rng.standard_normal(n) * 10
    fl = np.full(n, D.REMAPPED, np.uint8)
    ug, vg = D.rotate(U, V, fl, np.ones(n), np.zeros(n))
    assert np.array_equal(ug, U) and np.array_equal(vg, V)
    ca, sa = D.rot(rng.uniform(-180.0, 180.0, n))
    ug, vg = D.rotate(U, V, fl, ca, sa)
    speed = np.abs(np.hypot(ug, vg) / np.hypot(U, V) - 1).max() / EPS
    ub, vb = D.rotate(ug, vg, fl, ca, -sa)
    back = (np.maximum(np.abs(ub - U), np.abs(vb - V)) / (np.abs(U) + np.abs(V))).max() / EPS
    print("rotation: speed %.2f, back %.2f units of 2^-53" % (speed, back))
    assert speed <= 8.0 and back <= 8.0
    fl[::2] = D.UNFILLED
    ug, vg = D.rotate(np.where(fl == D.UNFILLED, D.FILL, U), np.where(fl == D.UNFILLED, D.FILL, V), fl, ca, sa)
    assert np.all(ug[::2] == D.FILL) and np.all(vg[::2] == D.FILL)


# ---- the library's checks (no device in the machine) --------------------------------------------------------------------
def good_params(L, **kw):
    p = L.BilinearParams(ny=10, nx=20, m0=0, NA=36, NB=18, nrec=2, dtype=L.REMAP_FLOAT32, n_fill=1, points=L.BILINEAR_H, ncomp=1,
                         topology=0, fill_max=-1)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_struct_size_and_check_refusals():
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import bilinear as B
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["BILINEAR_PARAMS"]) == ctypes.sizeof(L.BilinearParams)
    B.check(good_params(L))
    B.check(good_params(L, points=L.BILINEAR_C, ncomp=2))
    B.check(good_params(L, points=L.BILINEAR_H, ncomp=2), has_mask=True)
    for kw, mask, text in ((dict(ny=0), False, "ny, nx >= 1"), (dict(nx=1 << 31), False, "ny, nx >= 1"), (dict(NA=0), False, "NA, NB >= 1"),
                           (dict(NA=1 << 20, NB=1 << 20), False, "NA \\* NB < 2\\^31"), (dict(nrec=0), False, "nrec >= 1"),
                           (dict(ny=40000, nx=40000, nrec=8), False, "2\\^32"), (dict(m0=-1), False, "first row"),
                           (dict(dtype=2), False, "source dtype 2"), (dict(n_fill=3), False, "3 fill values \\(at most 2\\)"),
                           (dict(points=4), False, "point kind 4"), (dict(points=-1), False, "point kind -1"),
                           (dict(ncomp=3), False, "3 components"), (dict(points=L.BILINEAR_C), False, "c points are for vectors"),
                           (dict(points=L.BILINEAR_U), True, "a mask belongs to the h points"),
                           (dict(points=L.BILINEAR_C, ncomp=2), True, "a mask belongs to the h points"),
                           (dict(topology=4), False, "topology flags 4")):
        with pytest.raises(ValueError, match=text):
            B.check(good_params(L, **kw), has_mask=mask)
    assert lib.ogg_bilinear_check(None, 0) == L.OGG_EARG
    # the entry points refuse before any device work
    p = good_params(L, points=7)
    assert lib.ogg_bilinear_dev(ctypes.byref(p), None, None, 0, *([None] * 12)) == L.OGG_EARG and b"point kind 7" in lib.ogg_last_error()
    assert lib.ogg_bilinear(ctypes.byref(p), *([None] * 8), 0, 0, *([None] * 8)) == L.OGG_EARG
    p = good_params(L)
    assert lib.ogg_bilinear_rotate_dev(ctypes.byref(p), None, 0, *([None] * 10), 1, None) == L.OGG_EARG
    assert b"a vector is needed" in lib.ogg_last_error()


def test_knobs_must_be_integers_in_range(monkeypatch):
    """the knobs are read when the call is set up, before any device work: a value that is no integer is refused, not read as 0"""
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    p = good_params(L)
    args = (ctypes.byref(p), 8, 8, 2 * p.nx + 1, 8, 8, 8, None, None, 8, 8, None, None, None, None, None)   # never dereferenced
    for knob, val in (("OGG_BILINEAR_BLOCKS", "abc"), ("OGG_BILINEAR_LDS", "abc"), ("OGG_BILINEAR_LDS", "1x"), ("OGG_BILINEAR_LDS", ""),
                      ("OGG_BILINEAR_LDS", "2"), ("OGG_BILINEAR_BLOCKS", "0"), ("OGG_BILINEAR_RECORDS", "-1")):
        monkeypatch.setenv(knob, val)
        assert lib.ogg_bilinear_dev(*args) == L.OGG_EARG, (knob, val)
        assert (knob + "=" + val).encode() in lib.ogg_last_error() and b"an integer" in lib.ogg_last_error()
        monkeypatch.delenv(knob)


def test_python_layer_refusals():
    from ocean_model_grid_generator_amd import bilinear as B
    from ocean_model_grid_generator_amd import remap as R
    lon, lat = 360.0 * np.arange(9) / 8, -90.0 + 180.0 * np.arange(5) / 4
    s = R.Source(np.zeros((4, 8), np.float32), lon, lat, name="u")
    x, y = np.meshgrid(np.linspace(0, 360, 9), np.linspace(-80, 80, 5))
    with pytest.raises(ValueError, match="c points are for vectors"):
        B.bilinear(x, y, s, points="c")
    with pytest.raises(ValueError, match="points must be one of"):
        B.bilinear(x, y, s, points="q")
    with pytest.raises(ValueError, match="a mask belongs to the h points"):
        B.bilinear(x, y, s, points="u", mask=np.ones((2, 4)))
    with pytest.raises(ValueError, match="the mask is"):
        B.bilinear(x, y, s, mask=np.ones((3, 4)))
    with pytest.raises(ValueError, match="angle_dx"):
        B.bilinear(x, y, s, s)
    with pytest.raises(ValueError, match="different grids"):
        B.bilinear(x, y, s, R.Source(np.zeros((4, 8), np.float32), lon + 1.0, lat), rotate=False)
    with pytest.raises(ValueError, match="the two components are"):
        B.bilinear(x, y, s, R.Source(np.zeros((4, 8), np.float64), lon, lat), rotate=False)
    with pytest.raises(ValueError, match="fill_max must be >= 0"):
        B.bilinear(x, y, s, fill_max=-2)


def test_main_flags_and_their_validation():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    a = ogg.build_parser().parse_args(["-r", "1", "--interp_source", "s.nc", "--interp_var", "t", "--interp_var", "s", "--interp_vector",
                                       "u", "v", "--interp_points", "u", "--interp_file", "i.nc", "--interp_no_fill", "--interp_fill_max",
                                       "3", "--interp_no_rotate"])
    assert (a.interp_source, a.interp_var, a.interp_vector, a.interp_points, a.interp_file) == ("s.nc", ["t", "s"], [["u", "v"]], "u", "i.nc")
    assert a.interp_no_fill and a.interp_fill_max == 3 and a.interp_no_rotate
    b = ogg.build_parser().parse_args(["-r", "1"])
    assert (b.interp_source, b.interp_var, b.interp_vector, b.interp_points, b.interp_file, b.interp_no_fill, b.interp_fill_max,
            b.interp_no_rotate) == (None, None, None, "h", "interp.nc", False, None, False)
    ogg._validate_interp_flags(None, None, None, "h", False)
    ogg._validate_interp_flags("s.nc", ["t"], [("u", "v")], "h", False)
    for args, text in ((("s.nc", None, None, "h", False), "nothing to interpolate"), ((None, ["t"], None, "h", False), "need --interp_source"),
                       (("s.nc", ["t"], None, "c", False), "c points are for vectors"),
                       (("s.nc", None, [("u", "v")], "c", True), "drop --skip_metrics"),
                       (("s.nc", None, [("u",)], "h", False), "two names"),
                       (("s.nc", ["t"], None, "h", False, False, -1), "--interp_fill_max must be >= 0")):
        with pytest.raises(ValueError, match=text):
            ogg._validate_interp_flags(*args)
    ogg._validate_interp_flags("s.nc", ["t"], None, "v", True)   # scalars work without the metrics
    for path in (None, "functions"):   # main() refuses before any device work, on both of its paths
        with pytest.raises(ValueError, match="nothing to interpolate"):
            ogg.main(1.0, interp_source="s.nc", path=path)


# ---- the writer -----------------------------------------------------------------------------------------------------------
def test_write_bilinear_reads_back(tmp_path):
    from ocean_model_grid_generator_amd import bilinear as B
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import remap as R
    lon, lat = 360.0 * np.arange(9) / 8, -90.0 + 180.0 * np.arange(5) / 4
    ny, nx = 3, 4
    rng = np.random.default_rng(8)
    depth = ("depth", netcdf3.NC_DOUBLE, [("units", "m")], np.array([5.0, 50.0]))
    t = R.Source(np.zeros((2, 4, 8), np.float32), lon, lat, name="temp", lead_dims=[("depth", 2)], coords=[depth], atts=[("units", "degC")])
    u = R.Source(np.zeros((4, 8)), lon, lat, name="uwnd")
    v = R.Source(np.zeros((4, 8)), lon, lat, name="vwnd")

    def fake(src, src2, points, rotated):
        arr = {}
        for sfx, kind in zip(("", "2"), B._kinds(points, src2 is not None)):
            shape = (src.nrec,) + B.point_shape(ny, nx, kind)
            arr["values" + sfx] = rng.standard_normal(shape)
            arr["flags" + sfx] = rng.integers(0, 4, shape).astype(np.uint8)
            arr["values" + sfx][arr["flags" + sfx] % 3 == 0] = B.FILL
        return B.result(arr, src, src2, points, True, True, points == "h", None, False, rotated)
    for points, rotated in (("h", True), ("c", False), ("u", True), ("v", True)):
        res = [((t,), fake(t, None, "h" if points == "c" else points, False)), ((u, v), fake(u, v, points, rotated))]
        if points == "c":
            res = res[1:]
        path = str(tmp_path / ("i_%s.nc" % points))
        B.write_bilinear(path, res)
        h = netcdf3.read_header(path)
        k1, k2 = B._kinds(points, True)
        for (srcs, r), names in zip(res, (("temp",), ("uwnd", "vwnd")) if points != "c" else (("uwnd", "vwnd"),)):
            for name, key, kind in zip(names, ("", "2"), (k1, k2)):
                var, flag = h.vars[name], h.vars[name + "_interp_flag"]
                lead = (2,) if name == "temp" else ()
                assert tuple(var.shape) == lead + B.point_shape(ny, nx, kind) == tuple(flag.shape)
                assert var.nc_type == netcdf3.NC_DOUBLE and flag.nc_type == netcdf3.NC_BYTE
                assert tuple(var.dims) == (("depth",) if lead else ()) + B._DIMS[kind]
                assert float(np.asarray(var.atts["_FillValue"]).reshape(-1)[0]) == 1e20 and var.atts["points"] == kind
                got = np.frombuffer(netcdf3.read_var_bytes(path, h, name), dtype=">f8").reshape(var.shape)
                assert got.astype("<f8").tobytes() == r["values" + key].tobytes()
                gf = np.frombuffer(netcdf3.read_var_bytes(path, h, name + "_interp_flag", dtype=netcdf3.NC_BYTE), dtype=np.int8)
                assert np.array_equal(gf.reshape(flag.shape), r["flags" + key])
                if name != "temp":
                    assert var.atts["grid_relative"] == ("true" if rotated else "false")
                    assert var.atts["vector_component"] == ("x" if key == "" else "y")
                else:
                    assert "grid_relative" not in var.atts and var.atts["units"] == "degC"
        if points != "c":
            assert np.array_equal(np.frombuffer(netcdf3.read_var_bytes(path, h, "depth"), dtype=">f8"), [5.0, 50.0])
    with pytest.raises(ValueError, match="asked for twice"):
        B.write_bilinear(str(tmp_path / "d.nc"), [((t,), fake(t, None, "h", False)), ((t,), fake(t, None, "h", False))])

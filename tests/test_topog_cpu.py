"""CPU tests of topography by refined sampling: the numpy definition (tests/topog_definition.py) on hand-computed cases, the exact
128-bit spread, the host-side merge of partial records, the NetCDF source reader, the topog.nc layout, and argument errors that
are caught before any device work."""
import ctypes

import numpy as np
import pytest

import topog_definition as td

from ocean_model_grid_generator_amd import _lib as L
from ocean_model_grid_generator_amd import netcdf3
from ocean_model_grid_generator_amd import topography as T


def latlon_grid(lon0, lat0, dlon, dlat, ni, nj):
    x, y = np.meshgrid(lon0 + dlon * np.arange(ni + 1), lat0 + dlat * np.arange(nj + 1))
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def test_constant_raster_has_zero_spread_and_exact_mean():
    raw = np.full((180, 360), -1234, dtype=np.int16)
    x, y = latlon_grid(-30.0, -40.0, 0.5, 0.5, 8, 6)
    rec = td.records(x, y, raw, -180.0, 1.0, -90.0, 1.0)
    assert np.all(rec["n"] == 4 * rec["R"] ** 2) and np.all(rec["n_missing"] == 0)
    res = T.fields_from_records(as_struct(rec), 1.0)
    assert np.all(res["height"] == -1234.0) and np.all(res["h_std"] == 0.0)
    assert np.all(res["depth"] == 1234.0) and np.all(res["wet_fraction"] == 1.0)
    assert np.all(res["h_min"] == -1234.0) and np.all(res["h_max"] == -1234.0)


def as_struct(rec):
    out = T.empty_records(rec["n"].shape)
    for f in td.RECORD_FIELDS:
        out[f] = rec[f]
    return out


def test_row_index_raster_gives_known_means():
    """S[js, is] = js on a 1-degree raster; a supergrid cell of the aligned 1-degree grid holds R x R samples, all in one row."""
    raw = np.repeat(np.arange(180, dtype=np.int16)[:, None], 360, axis=1)
    x, y = latlon_grid(0.0, -90.0, 1.0, 1.0, 360, 180)
    rec = td.records(x, y, raw, 0.0, 1.0, -90.0, 1.0, cells_="supergrid")
    assert np.all(rec["R"] == 2)
    res = T.fields_from_records(as_struct(rec), 1.0)
    np.testing.assert_array_equal(res["height"], np.repeat(np.arange(180.0)[:, None], 360, axis=1))
    model = td.model_records(rec)
    mres = T.fields_from_records(as_struct(model), 1.0)
    np.testing.assert_array_equal(mres["height"][:, 0], np.arange(90) * 2 + 0.5)
    np.testing.assert_array_equal(mres["h_std"][:, 0], np.full(90, 0.5))
    np.testing.assert_array_equal(mres["n_samples"], np.full((90, 180), 16))


def test_cell_straddling_the_dateline_is_unwrapped():
    c = td.cells(np.array([[179.5, -179.5], [179.5, -179.5]]), np.array([[0.0, 0.0], [1.0, 1.0]]), 1.0, 1.0)
    assert c["L01"][0, 0] == 180.5 and c["L11"][0, 0] == 180.5
    assert c["R"][0, 0] == 2 and c["pole"][0, 0] == 0
    raw = np.zeros((180, 360), dtype=np.int16)
    raw[:, 359] = 10   # 179 .. 180
    raw[:, 0] = 20     # -180 .. -179
    rec = td.records(np.array([[179.5, -179.5], [179.5, -179.5]]), np.array([[0.0, 0.0], [1.0, 1.0]]), raw, -180.0, 1.0, -90.0, 1.0,
                     cells_="supergrid")
    assert rec["n"][0, 0] == 4 and rec["sum"][0, 0] == 2 * 10 + 2 * 20 and rec["min"][0, 0] == 10 and rec["max"][0, 0] == 20


def polar_cap(n=8, lat=-85.0):
    """A ring of ordinary cells around the south pole (rows at lat and lat + 2): none of them encloses it."""
    ang = np.linspace(0.0, 360.0, n + 1)
    x = np.array([ang, ang])
    y = np.array([np.full(n + 1, lat), np.full(n + 1, lat + 2.0)])
    return x, y


def test_pole_enclosing_cell_is_detected():
    # one cell whose four corners sit around the pole at 90 degrees apart (longitudes 0, 90 / 270, 180 around the loop)
    x = np.array([[0.0, 90.0], [270.0, 180.0]])
    y = np.full((2, 2), -89.0)
    c = td.cells(x, y, 1.0, 1.0)
    assert c["pole"][0, 0] == -1
    assert c["R"][0, 0] == 256 and c["clamped"][0, 0]          # its unwrapped longitudes span 180 degrees
    raw = np.arange(180 * 360, dtype=np.int32).reshape(180, 360).astype(np.float64)
    rec = td.records(x, y, raw, -180.0, 1.0, -90.0, 1.0, quantum=1.0, cells_="supergrid", refine=4)
    # 4 x 4 samples on the southmost raster row at lon = 0 + 360 * (a + 0.5) / 4 = 45, 135, 225, 315 (is = 225, 315, 45, 135)
    assert rec["n"][0, 0] == 16 and rec["min"][0, 0] == 45 and rec["max"][0, 0] == 315
    assert rec["sum"][0, 0] == 4 * (45 + 135 + 225 + 315)
    # a ring of ordinary cells next to it: none encloses the pole
    xr, yr = polar_cap()
    assert np.all(td.cells(xr, yr, 1.0, 1.0)["pole"] == 0)
    # a corner AT the pole takes its row neighbour's longitude: the cell does not enclose it
    c = td.cells(np.array([[0.0, 90.0], [0.0, 90.0]]), np.array([[-90.0, -90.0], [-89.0, -89.0]]), 1.0, 1.0)
    assert c["pole"][0, 0] == 0


def test_refinement_formula_and_clamp():
    x, y = latlon_grid(0.0, 0.0, 0.3, 0.1, 1, 1)
    assert td.cells(x, y, 1.0, 1.0)["R"][0, 0] == 1                    # ceil(2 * 0.3) = 1
    assert td.cells(x, y, 0.25, 1.0)["R"][0, 0] == 3                   # ceil(2 * 0.3 / 0.25) = ceil(2.4)
    assert td.cells(x, y, 0.1, 1.0)["R"][0, 0] == 7                    # 2 * (0.3 / 0.1) = 6.000000000000001 in fp64
    assert td.cells(x, y, 1.0, 0.01)["R"][0, 0] == 20                  # the latitude span decides
    c = td.cells(x, y, 1e-4, 1.0)
    assert c["R"][0, 0] == 256 and c["clamped"][0, 0]
    c = td.cells(x, y, 1e-4, 1.0, refine=3)
    assert c["R"][0, 0] == 3 and not c["clamped"][0, 0]
    c = td.cells(x, y, 1.0, 1.0, oversample=1000.0)
    assert c["R"][0, 0] == 256 and c["clamped"][0, 0]


def test_exact_spread_against_python_integers():
    rng = np.random.default_rng(3)
    n = rng.integers(1, 262145, size=4000)
    q = rng.integers(-2 ** 21, 2 ** 21 + 1, size=4000)
    # sums of n samples of magnitude <= 2^21: realistic extremes and random mixtures
    s = np.where(rng.random(4000) < 0.5, n * q, (n * q) // 3)
    ss = np.abs(s) * (2 ** 21) // 1 + n * 7
    ss = np.maximum(ss, (s.astype(object) ** 2 // n.astype(object)).astype(np.int64) + 1)
    got = T.exact_variance_numerator(n, s, ss)
    want = np.array([float(int(a) * int(c) - int(b) * int(b)) for a, b, c in zip(n, s, ss)])
    np.testing.assert_array_equal(got, want)
    assert np.any([int(a) * int(c) >= 2 ** 64 for a, c in zip(n, ss)])   # the 128-bit branch was taken


def test_partial_rows_combine_exactly():
    rng = np.random.default_rng(7)
    raw = rng.integers(-6000, 3000, size=(90, 180)).astype(np.int16)
    x, y = latlon_grid(-100.0, -30.0, 0.7, 0.45, 10, 12)
    sg = td.records(x, y, raw, -180.0, 2.0, -90.0, 2.0, cells_="supergrid")
    whole = as_struct(td.model_records(sg))
    # bands of supergrid rows 0..4, 5..8, 9..11 (the first and second split model rows 2 and 4)
    parts = []
    for a, b in ((0, 5), (5, 9), (9, 12)):
        piece = {f: sg[f][a:b] for f in td.RECORD_FIELDS}
        if a % 2:
            piece = {f: np.concatenate([np.zeros_like(v[:1]) if f not in ("min", "max") else
                                        np.full_like(v[:1], np.iinfo(np.int32).max if f == "min" else np.iinfo(np.int32).min), v])
                     for f, v in piece.items()}
        if piece["n"].shape[0] % 2:
            piece = {f: np.concatenate([v, np.zeros_like(v[:1]) if f not in ("min", "max") else
                                        np.full_like(v[:1], np.iinfo(np.int32).max if f == "min" else np.iinfo(np.int32).min)])
                     for f, v in piece.items()}
        parts.append((a // 2, as_struct(td.model_records(piece))))
    got = T.assemble(parts[::-1], 6, 5)
    assert got.tobytes() == whole.tobytes()


def write_source(path, var, data, lon, lat, nc_type, atts=(), version=2):
    ds = netcdf3.Dataset(path, [("lat", len(lat)), ("lon", len(lon))])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "degrees_north")], np.asarray(lat))
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "degrees_east")], np.asarray(lon))
    ds.def_var(var, nc_type, ("lat", "lon"), list(atts), data)
    ds.write()


@pytest.mark.parametrize("nc_type,dtype", [(netcdf3.NC_SHORT, np.int16), (netcdf3.NC_FLOAT, np.float32), (netcdf3.NC_DOUBLE, np.float64)])
@pytest.mark.parametrize("fill", [None, -32767])
def test_netcdf_source_reader(tmp_path, nc_type, dtype, fill):
    lon = -179.5 + np.arange(360.0)        # centres
    lat = 89.5 - np.arange(180.0)          # north first
    data = (np.arange(180 * 360) % 5000 - 2500).reshape(180, 360).astype(dtype)
    if fill is not None:
        data[3, 4] = fill
    atts = [("units", "m")] + ([("_FillValue", float(fill) if dtype != np.int16 else int(fill))] if fill is not None else [])
    p = str(tmp_path / "src.nc")
    write_source(p, "elevation", data, lon, lat, nc_type, atts)
    s = T.read_source(p, "elevation")
    assert "centres" in s.note and s.data.dtype == dtype
    assert (s.lon0, s.dlon, s.lat0, s.dlat) == (-180.0, 1.0, -90.0, 1.0)
    np.testing.assert_array_equal(s.data, data[::-1])
    assert s.fill == (() if fill is None else (float(fill),))
    assert s.quantum == (1.0 if dtype == np.int16 else 0.01) and s.periodic
    # edges: coordinates on the lattice of the step
    p2 = str(tmp_path / "edges.nc")
    write_source(p2, "z", data[::-1], np.arange(360.0) - 180.0, np.arange(180.0) - 90.0, nc_type)
    s2 = T.read_source(p2, "z")
    assert "edges" in s2.note and (s2.lon0, s2.lat0) == (-180.0, -90.0)


def test_netcdf_source_reader_takes_lon_lat_order(tmp_path):
    """A variable stored (lon, lat) is transposed: the coordinates' units say which dimension is which, whatever their names."""
    data = (np.arange(180 * 360) % 777 - 300).reshape(180, 360).astype(np.int16)
    p = str(tmp_path / "t.nc")
    ds = netcdf3.Dataset(p, [("a", 360), ("b", 180)])
    ds.def_var("a", netcdf3.NC_DOUBLE, ("a",), [("units", "degrees_east")], -179.5 + np.arange(360.0))
    ds.def_var("b", netcdf3.NC_DOUBLE, ("b",), [("units", "degrees_north")], -89.5 + np.arange(180.0))
    ds.def_var("z", netcdf3.NC_SHORT, ("a", "b"), [], np.ascontiguousarray(data.T))
    ds.write()
    s = T.read_source(p, "z")
    np.testing.assert_array_equal(s.data, data)
    assert (s.lon0, s.dlon, s.lat0, s.dlat) == (-180.0, 1.0, -90.0, 1.0)
    q = str(tmp_path / "u.nc")   # neither units nor known names: refused rather than guessed
    ds = netcdf3.Dataset(q, [("a", 360), ("b", 180)])
    ds.def_var("a", netcdf3.NC_DOUBLE, ("a",), [], -179.5 + np.arange(360.0))
    ds.def_var("b", netcdf3.NC_DOUBLE, ("b",), [], -89.5 + np.arange(180.0))
    ds.def_var("z", netcdf3.NC_SHORT, ("a", "b"), [], np.ascontiguousarray(data.T))
    ds.write()
    with pytest.raises(ValueError, match="degrees_north"):
        T.read_source(q, "z")


def test_netcdf_source_reader_refuses(tmp_path):
    lon = np.arange(10.0)
    lon[5] += 1e-3
    p = str(tmp_path / "bad.nc")
    write_source(p, "elevation", np.zeros((4, 10), dtype=np.int16), lon, np.arange(4.0), netcdf3.NC_SHORT)
    with pytest.raises(ValueError, match="not uniform"):
        T.read_source(p)
    for magic in (b"CDF\x05", b"\x89HDF\r\n\x1a\n"):
        q = str(tmp_path / "other.nc")
        open(q, "wb").write(magic + b"\0" * 64)
        with pytest.raises(ValueError, match="nccopy -k 64-bit-offset"):
            T.read_source(q)
    with pytest.raises(KeyError, match="--var"):
        T.read_source(p, "depth")
    with pytest.raises(ValueError, match="source_box"):
        np.save(str(tmp_path / "a.npy"), np.zeros((2, 2), dtype=np.int16))
        T.read_source(str(tmp_path / "a.npy"))
    s = T.read_source(str(tmp_path / "a.npy"), box=(0.0, 1.0, 0.0, 1.0))
    assert s.shape == (2, 2) and not s.periodic


def test_topog_file_layout(tmp_path):
    rec = T.empty_records((4, 6))
    rec["n"][1:] = 9
    rec["sum"][1:] = -90
    rec["sumsq"][1:] = 900
    rec["min"][1:], rec["max"][1:], rec["n_wet"][1:], rec["R"][1:] = -10, -10, 9, 3
    res = T.result(rec, 0.5, 0.0, "model", None, 2.0)
    assert res["height"][0, 0] == T.FILL and res["height"][1, 0] == -5.0 and res["depth"][1, 0] == 5.0
    assert res["summary"]["n_samples"] == 18 * 9 and res["summary"]["n_empty_cells"] == 6
    p = str(tmp_path / "topog.nc")
    T.write_topog(p, res)
    h = netcdf3.read_header(p)
    assert h.version == 2 and h.dims == [("ny", 4), ("nx", 6)]
    for name in ("height", "depth", "h_std", "h_min", "h_max", "wet_fraction"):
        v = h.vars[name]
        assert v.nc_type == netcdf3.NC_DOUBLE and v.shape == (4, 6) and v.dims == ("ny", "nx")
        assert "units" in v.atts and "long_name" in v.atts and float(v.atts["_FillValue"][0]) == T.FILL
        got = np.frombuffer(netcdf3.read_var_bytes(p, h, name), dtype=">f8").reshape(4, 6)
        np.testing.assert_array_equal(got, res[name])
    v = h.vars["n_samples"]
    assert v.nc_type == netcdf3.NC_INT
    np.testing.assert_array_equal(np.frombuffer(netcdf3.read_var_bytes(p, h, "n_samples", dtype=netcdf3.NC_INT), dtype=">i4").reshape(4, 6),
                                  rec["n"])


def test_argument_errors():
    with pytest.raises(ValueError, match="ensure_nj_even"):
        T.check_args(8, 11, "model", None, 2.0)        # 7 x 10 supergrid cells
    T.check_args(8, 11, "supergrid", None, 2.0)
    with pytest.raises(ValueError, match="refine"):
        T.check_args(9, 11, "model", 257, 2.0)
    with pytest.raises(ValueError, match="quantum"):
        T.Source(np.zeros((2, 2)), 0.0, 1.0, 0.0, 1.0, quantum=0.0)
    with pytest.raises(ValueError, match="2\\^21"):
        td.quantise(np.array([[30000.0]]), quantum=0.01)
    # the library validates before any device work
    lib = L.load()
    band = L.TopogBand(nx=7, j0=0, n_cell_rows=4, cells=L.TOPOG_MODEL_CELLS, refine=0, oversample=2.0)
    band.x = band.y = band.x_next = band.y_next = 8
    src = L.TopogSource(data=8, dtype=L.TOPOG_INT16, Nx=360, Ny=180, lon0=0.0, dlon=1.0, lat0=-90.0, dlat=1.0, quantum=1.0)
    rc = lib.ogg_topog_band_dev(ctypes.byref(band), ctypes.byref(src), 8, 256, 8, None)
    assert rc == L.OGG_ESHAPE and b"even" in lib.ogg_last_error()
    band.nx, band.refine = 8, 300
    assert lib.ogg_topog_band_dev(ctypes.byref(band), ctypes.byref(src), 8, 256, 8, None) == L.OGG_EARG
    band.refine, src.dtype = 0, L.TOPOG_FLOAT32
    assert lib.ogg_topog_band_dev(ctypes.byref(band), ctypes.byref(src), 8, 256, 8, None) == L.OGG_EARG
    assert b"quantise" in lib.ogg_last_error()
    assert lib.ogg_abi_sizeof(L.ABI["TOPOG_RECORD"]) == L.TOPOG_RECORD.itemsize
    band.j0, band.n_cell_rows = 3, 4
    assert lib.ogg_topog_band_out_rows(ctypes.byref(band)) == 3    # model rows 1, 2, 3

"""CPU tests of the atmosphere x ocean exchange grid: the numpy definition (tests/xgrid_definition.py) on lat-lon grids with analytic
areas, conservation, a cap of cells at the pole, the longitude wrap, threshold and mask; the exchange-grid file layout; the C
structs and the argument checks the library makes before any device work; the command-line flags."""
import ctypes
import math

import numpy as np
import pytest

import xgrid_definition as xd

from ocean_model_grid_generator_amd import _lib as L
from ocean_model_grid_generator_amd import exchange_grid as X
from ocean_model_grid_generator_amd import netcdf3

RE = 6371.0e3


def latlon_supergrid(lon0, lat0, dlon, dlat, ni, nj):
    """A supergrid of ni x nj cells of dlon x dlat (model cells 2 dlon x 2 dlat)."""
    x, y = np.meshgrid(lon0 + dlon * np.arange(ni + 1), lat0 + dlat * np.arange(nj + 1))
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def rect_area(l1, l2, p1, p2):
    return RE * RE * (l2 - l1) * xd.D2R * (math.sin(p2 * xd.D2R) - math.sin(p1 * xd.D2R))


def test_aligned_latlon_grids_give_the_analytic_areas():
    x, y = latlon_supergrid(-40.0, -30.0, 1.0, 1.0, 40, 60)     # 2-degree model cells, lon -40 .. 0, lat -30 .. 30
    lon, lat = X.regular_atm(90, 45)                            # 4-degree atmosphere, lon 0 .. 360
    lst, a_poly, counts = xd.exchange_grid(x, y, lon, lat)
    want = []
    for m in range(30):
        for n in range(20):
            l1, p1 = -40.0 + 2 * n, -30.0 + 2 * m
            want.append((int((l1 + 360.0) // 4), int((p1 + 90.0) // 4), n, m))
    assert [e[:4] for e in lst] == want
    got = np.array([e[4] for e in lst])
    ref = np.array([rect_area(-40.0 + 2 * n, -38.0 + 2 * n, -30.0 + 2 * m, -28.0 + 2 * m) for m in range(30) for n in range(20)])
    assert np.max(np.abs(got / ref - 1)) <= 1e-14
    assert np.max(np.abs(a_poly.reshape(-1) / ref - 1)) <= 1e-14
    assert counts["candidates"] == counts["kept"] == 600 and counts["inverted"] == counts["pole_cells"] == 0


def test_offset_grids_conserve_area():
    x, y = latlon_supergrid(-40.3, -30.2, 1.0, 1.0, 40, 60)
    lon, lat = X.regular_atm(90, 45)
    lst, a_poly, _ = xd.exchange_grid(x, y, lon, lat, threshold=0.0)
    atm, ocn, area = xd.as_arrays(lst)
    per_ocn = np.bincount(ocn[:, 1] * 20 + ocn[:, 0], weights=area, minlength=600).reshape(30, 20)
    assert np.max(np.abs(per_ocn / a_poly - 1)) <= 1e-12
    per_atm = np.bincount(atm[:, 1] * 90 + atm[:, 0], weights=area, minlength=90 * 45).reshape(45, 90)
    n_full = 0
    for J in range(45):
        for I in range(90):
            l1, l2, p1, p2 = lon[I], lon[I + 1], lat[J], lat[J + 1]
            if l1 - 360.0 >= -40.3 and l2 - 360.0 <= -0.3 and p1 >= -30.2 and p2 <= 29.8:   # inside the ocean grid
                n_full += 1
                assert abs(per_atm[J, I] / rect_area(l1, l2, p1, p2) - 1) <= 1e-12
    assert n_full >= 50


def test_pole_fan_tiles_the_cap():
    """Model cells from 80 N to the pole whose top corners all lie at 90 N: each becomes a lon-lat rectangle up to the pole."""
    x, y = latlon_supergrid(-300.0, 80.0, 7.5, 5.0, 48, 2)
    lst, a_poly, counts = xd.exchange_grid(x, y, *X.regular_atm(36, 18), threshold=0.0)
    cap = 2 * math.pi * RE * RE * (1 - math.sin(80.0 * xd.D2R))
    assert counts["pole_cells"] == 24 and counts["pole_enclosing"] == counts["degenerate"] == counts["inverted"] == 0
    assert abs(np.sum(a_poly) / cap - 1) <= 1e-12
    assert abs(sum(e[4] for e in lst) / cap - 1) <= 1e-12
    # a point of the grid at the pole: four cells with one pole corner each, the polygons (L_before, 90), (L_after, 90)
    st, verts, npole = xd.polygon([0.0, 90.0, 45.0, 0.0], [88.0, 88.0, 90.0, 89.0])
    assert st == "ok" and npole == 1 and verts == [(0.0, 88.0), (90.0, 88.0), (90.0, 90.0), (0.0, 90.0), (0.0, 89.0)]
    st, _, _ = xd.polygon([0.0, 90.0, 180.0, 270.0], [89.0, 89.0, 89.0, 89.0])   # around the pole
    assert st == "pole"
    assert xd.polygon([0.0, 1.0, 2.0, 3.0], [90.0, 90.0, 90.0, 89.0])[0] == "degenerate"


def test_longitude_wrap():
    x, y = latlon_supergrid(-300.0, -20.0, 0.75, 1.0, 480, 12)   # the whole circle, lon -300 .. 60
    lon, lat = X.regular_atm(40, 30)
    lon = lon + 5.5                                               # a lon0 that is no multiple of the ocean spacing
    a, pa, _ = xd.exchange_grid(x, y, lon, lat, threshold=0.0)
    b, pb, _ = xd.exchange_grid(x + 360.0, y, lon, lat, threshold=0.0)
    assert [e[:4] for e in a] == [e[:4] for e in b]
    ra, rb = np.array([e[4] for e in a]), np.array([e[4] for e in b])
    # not 1e-14 of A_x: lam * pi / 180 rounds at |lam| up to 420 (half an ulp of 7.3 rad, 4.4e-16), and an edge's dlam^ of one 0.75
    # degree cell (0.013 rad) carries that from both ends -- 6.8e-14 of the cell, measured 3.4e-14 of A_poly and 1.0e-13 of the
    # smallest A_x.  The bound is four such roundings of A_poly.
    a_poly = np.array([pa[e[3], e[2]] for e in a])
    assert np.max(np.abs(ra - rb) / a_poly) <= 4 * 2.0 ** -53 * 420.0 / 0.75
    assert np.max(np.abs(pa / pb - 1)) <= 4 * 2.0 ** -53 * 420.0 / 0.75
    band = 2 * math.pi * RE * RE * (math.sin(-8.0 * xd.D2R) - math.sin(-20.0 * xd.D2R))
    assert abs(ra.sum() / band - 1) <= 1e-12


def test_threshold_and_mask():
    x, y = latlon_supergrid(-40.0000001, -30.2, 1.0, 1.0, 40, 20)   # slivers of 1e-7 degree at the atmosphere's lon edges
    lon, lat = X.regular_atm(90, 45)
    all_, a_poly, _ = xd.exchange_grid(x, y, lon, lat, threshold=0.0)
    kept, _, c = xd.exchange_grid(x, y, lon, lat)
    atm_area = lambda e: RE * RE * (lon[e[0] + 1] * xd.D2R - lon[e[0]] * xd.D2R) * (math.sin(lat[e[1] + 1] * xd.D2R) -  # noqa: E731
                                                                                     math.sin(lat[e[1]] * xd.D2R))
    want = [e for e in all_ if e[4] > 1e-6 * min(a_poly[e[3], e[2]], atm_area(e))]
    assert kept == want and len(kept) < len(all_) and c["candidates"] == len(all_)
    rng = np.random.default_rng(1)
    mask = (rng.random(a_poly.shape) < 0.6).astype(np.uint8)
    masked, _, cm = xd.exchange_grid(x, y, lon, lat, mask=mask)
    assert masked == [e for e in kept if mask[e[3], e[2]]]
    assert cm["masked"] == int(np.sum(mask == 0))


def test_xgrid_file_layout(tmp_path):
    atm = np.array([[3, 4], [5, 6], [0, 0]], dtype=np.int32)
    ocn = np.array([[1, 2], [1, 2], [7, 9]], dtype=np.int32)
    area = np.array([1.5e9, 2.5e9, 3.0])
    lon, lat = X.regular_atm(8, 8)
    res = X.result(atm, ocn, area, np.full((10, 8), 1e10), dict.fromkeys(L.XGRID_COUNT_FIELDS, 0), lon, lat, RE, 1e-6)
    p = str(tmp_path / "x.nc")
    X.write_xgrid(p, res)
    h = netcdf3.read_header(p)
    assert h.version == 2 and h.dims == [("ncells", 3), ("two", 2)]
    for name, want, sn in (("tile1_cell", atm + 1, "parent_cell_indices_in_mosaic1"), ("tile2_cell", ocn + 1, "parent_cell_indices_in_mosaic2")):
        v = h.vars[name]
        assert v.nc_type == netcdf3.NC_INT and v.dims == ("ncells", "two") and v.atts["standard_name"] == sn
        np.testing.assert_array_equal(np.frombuffer(netcdf3.read_var_bytes(p, h, name, dtype=netcdf3.NC_INT), dtype=">i4").reshape(3, 2), want)
    v = h.vars["xgrid_area"]
    assert v.nc_type == netcdf3.NC_DOUBLE and v.dims == ("ncells",)
    assert v.atts["standard_name"] == "exchange_grid_area" and v.atts["units"] == "m2"
    np.testing.assert_array_equal(np.frombuffer(netcdf3.read_var_bytes(p, h, "xgrid_area"), dtype=">f8"), area)
    # ocean_frac: the areas summed per atmosphere cell, in list order, over the cell's area
    assert res["ocean_frac"].shape == (8, 8)
    assert res["ocean_frac"][0, 0] == 3.0 / res["a_atm"][0, 0]


def test_structs_and_argument_checks_before_device_work():
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["XGRID_BAND"]) == ctypes.sizeof(L.XgridBand)
    assert lib.ogg_abi_sizeof(L.ABI["XGRID_ATM"]) == ctypes.sizeof(L.XgridAtm)
    assert lib.ogg_abi_sizeof(L.ABI["XGRID_COUNTS"]) == ctypes.sizeof(L.XgridCounts) == 64
    x, y = latlon_supergrid(0.0, -10.0, 1.0, 1.0, 8, 4)
    counts = L.XgridCounts()
    out = np.zeros(64)

    def run(lon, lat, nx=8, ny=4):
        lon, lat = np.ascontiguousarray(lon, dtype=np.float64), np.ascontiguousarray(lat, dtype=np.float64)
        band = L.XgridBand(nx=nx, ny=ny, j0=0, n_cell_rows=ny, Re=RE, threshold=1e-6)
        band.x, band.y = x.ctypes.data, y.ctypes.data
        atm = L.XgridAtm(lon=lon.ctypes.data, lat=lat.ctypes.data, NA=lon.size - 1, NB=lat.size - 1)
        return lib.ogg_xgrid(ctypes.byref(band), ctypes.byref(atm), 0, None, None, None, out.ctypes.data, ctypes.byref(counts))

    lon, lat = X.regular_atm(36, 18)
    for bad_lon, bad_lat, what in ((lon[::-1], lat, b"increase"), (lon * 0.5, lat, b"span 360"), (lon, lat * 1.01, b"leave"),
                                   (np.r_[lon[:3], lon[2], lon[4:]], lat, b"increase"), (lon, lat[::-1], b"increase")):
        assert run(bad_lon, bad_lat) == L.OGG_EARG, what
        assert what in lib.ogg_last_error()
    for nx, ny in ((7, 4), (8, 3)):
        assert run(lon, lat, nx, ny) == L.OGG_EARG and b"ensure_nj_even" in lib.ogg_last_error()
    with pytest.raises(ValueError, match="span 360"):
        X.exchange_grid(x, y, lon[:-1], lat)
    with pytest.raises(ValueError, match="ensure_nj_even"):
        X.exchange_grid(x[:4], y[:4], lon, lat)
    band = L.XgridBand(nx=8, ny=10, j0=3, n_cell_rows=4)
    assert (lib.ogg_xgrid_band_first_row(ctypes.byref(band)), lib.ogg_xgrid_band_out_rows(ctypes.byref(band)),
            lib.ogg_xgrid_band_next_rows(ctypes.byref(band))) == (2, 2, 2)     # model rows 2, 3 (cell rows 4, 6): rows 7, 8 after it
    band.j0, band.n_cell_rows = 4, 4
    assert (lib.ogg_xgrid_band_first_row(ctypes.byref(band)), lib.ogg_xgrid_band_out_rows(ctypes.byref(band)),
            lib.ogg_xgrid_band_next_rows(ctypes.byref(band))) == (2, 2, 1)
    band.j0, band.n_cell_rows = 5, 1
    assert lib.ogg_xgrid_band_out_rows(ctypes.byref(band)) == 0 and lib.ogg_xgrid_band_next_rows(ctypes.byref(band)) == 0


def test_command_line_flags():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    a = ogg.build_parser().parse_args(["-r", "2", "--xgrid_atm", "180", "90", "--xgrid_file", "xg.nc"])
    assert a.xgrid_atm == [180, 90] and a.xgrid_file == "xg.nc"
    a = ogg.build_parser().parse_args(["-r", "2"])
    assert a.xgrid_atm is None and a.xgrid_file == X.DEFAULT_FILE
    with pytest.raises(SystemExit):
        ogg.build_parser().parse_args(["-r", "2", "--xgrid_atm", "180"])
    lon, lat = X.regular_atm(180, 90)
    assert lon[0] == 0.0 and lon[-1] == 360.0 and lat[0] == -90.0 and lat[-1] == 90.0 and lon.size == 181

"""GPU tests of the conservative regrid to a lat-lon grid (csrc/ogg_regrid.hip, latlon_regrid.py, Supergrid.regrid_to_latlon): values,
covers, ocean_frac and n_entries bit for bit against the definition in tests/latlon_regrid_definition.py on the device's own exchange
list, for coarser and finer targets, float32 and fp64 fields with and without missing values and a wet mask, both normalisations; the
same bits for any rank count, run and knob; conservation and a remap round trip; main()'s fraction file on both paths and the file
command."""
import os
import subprocess
import sys

import numpy as np
import pytest

import latlon_regrid_definition as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "r1": dict(inverse_resolution=1.0, ensure_nj_even=True),
    "r2": dict(inverse_resolution=2.0, ensure_nj_even=True),
    "r2_dp": dict(inverse_resolution=2.0, lon_dp=80.0, lat_dp=-85.85, ensure_nj_even=True),
}


def target(kind):
    """a coarse regular target, a fine one, or one of non-uniform latitudes whose lon0 is no multiple of the grid's"""
    if kind == "coarse":
        return 360.0 * np.arange(73) / 72, -90.0 + 180.0 * np.arange(37) / 36
    if kind == "fine":
        return 360.0 * np.arange(721) / 720, -90.0 + 180.0 * np.arange(361) / 360
    lat = 89.0 * np.sin(0.5 * np.pi * np.linspace(-1.0, 1.0, 97))
    return -17.3 + 360.0 * np.arange(201) / 200, lat


def model_field(x, y, nrec, dtype, missing):
    """smooth records on the model cells; with ``missing`` NaN over a box of land and -999 where the records get deeper"""
    cx, cy = np.radians(x[1::2, 1::2]), np.radians(y[1::2, 1::2])
    f = np.stack([np.cos(cy) * (20 + r) + 3 * np.sin(3 * cx + r) * np.cos(2 * cy) for r in range(nrec)]).astype(dtype)
    if missing:
        lon, lat = x[1::2, 1::2] % 360, y[1::2, 1::2]
        box = (lon > 20) & (lon < 70) & (lat > -30) & (lat < 40)
        for r in range(nrec):
            f[r][box] = np.nan
            f[r][np.abs(lat) > 75 - 15 * r] = -999.0
    return f


def wet_of(x, y):
    cx, cy = x[1::2, 1::2] % 360, y[1::2, 1::2]
    land = ((cx > 100) & (cx < 140) & (cy > -20) & (cy < 30)) | ((cx > 250) & (cx < 300) & (cy > 10) & (cy < 60)) | (cy > 80)
    return (~land).astype(np.uint8)


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def device_grid(sg, name, world=1):
    plan = sg.SupergridPlan(**CONFIGS[name])
    ranks = []
    for r in range(world):
        ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
    for g in ranks:
        g.run_pass()
    return plan, ranks


def check_against_definition(res, lists, field, fills, normalize):
    want_v, want_c = D.regrid(lists["atm"], lists["ocn"], lists["area"], field.reshape((-1,) + field.shape[-2:]), lists["a_atm"], fills,
                              normalize)
    frac, n = D.static(lists["atm"], lists["area"], lists["a_atm"])
    assert res["values"].tobytes() == want_v.reshape(res["values"].shape).tobytes()
    assert res["cover"].tobytes() == want_c.reshape(res["cover"].shape).tobytes()
    assert res["ocean_frac"].tobytes() == frac.tobytes() and res["n_entries"].tobytes() == n.tobytes()
    assert res["ocean_frac"].tobytes() == lists["ocean_frac"].tobytes()   # the exchange grid's own host fraction
    assert res["cell_area"].tobytes() == lists["a_atm"].tobytes()


CASES = [("coarse", np.float32, True, True, 3, "area"), ("fine", np.float64, False, False, 1, "cell"),
         ("gaussian", np.float32, True, False, 2, "cell"), ("coarse", np.float64, False, True, 1, "area"),
         ("fine", np.float32, True, True, 2, "area")]


@pytest.mark.parametrize("name", ["r1", "r2", "r2_dp"])
def test_device_equals_definition(sg, name):
    plan, ranks = device_grid(sg, name)
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = out["x"], out["y"]
    for kind, dtype, missing, masked, nrec, normalize in CASES:
        lon, lat = target(kind)
        f = model_field(x, y, nrec, dtype, missing)
        fills = (-999.0,) if missing else ()
        from ocean_model_grid_generator_amd import latlon_regrid as G
        mask = wet_of(x, y) if masked else None
        res = g.regrid_to_latlon(cut, G.Field(f, fill=fills), (lon, lat), mask=mask, normalize=normalize, cover=True)
        lists = g.exchange_grid(cut, (lon, lat), mask=mask)
        check_against_definition(res, lists, f, fills, normalize)
        c = res["counts"]
        NB, NA = lat.size - 1, lon.size - 1
        assert c["entries"] == lists["area"].size and c["valid"] + c["empty"] == nrec * NA * NB
        assert c["cells"] == int((res["n_entries"] > 0).sum()) and c["max_entries"] == int(res["n_entries"].max())


def test_host_entry_and_static_sums_equal_the_device(sg):
    from ocean_model_grid_generator_amd import latlon_regrid as G
    plan, ranks = device_grid(sg, "r2")
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = out["x"], out["y"]
    lon, lat = target("gaussian")
    f = model_field(x, y, 2, np.float32, True)
    mask = wet_of(x, y)
    dev = g.regrid_to_latlon(cut, G.Field(f, fill=(-999.0,)), (lon, lat), mask=mask, cover=True)
    host = G.regrid_to_latlon(x, y, f, lon, lat, mask=mask, cover=True, fill_values=(-999.0,), Re=float(plan.Re))
    import torch
    xt, yt = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    one = G.regrid_to_latlon_dev(xt, yt, f, lon, lat, mask=mask, cover=True, fill_values=(-999.0,), Re=float(plan.Re))
    frac = G.latlon_fraction(x, y, lon, lat, mask=mask, Re=float(plan.Re))
    static = g.regrid_to_latlon(cut, None, (lon, lat), mask=mask)
    for k in ("values", "cover", "ocean_frac", "n_entries", "cell_area"):
        assert host[k].tobytes() == dev[k].tobytes() == one[k].tobytes(), k
    for k in ("ocean_frac", "n_entries", "cell_area"):
        assert frac[k].tobytes() == static[k].tobytes() == dev[k].tobytes(), k
    assert static["values"] is None and static["counts"]["valid"] == 0


def test_same_bits_for_any_rank_count(sg):
    from ocean_model_grid_generator_amd import latlon_regrid as G
    lon, lat = target("gaussian")
    want = None
    for world in (1, 2, 3):
        plan, ranks = device_grid(sg, "r2", world)
        cut = ranks[0].south_cut()
        out = sg.stitch(plan, [g.bands_to_host() for g in ranks])
        f = G.Field(model_field(out["x"], out["y"], 2, np.float32, True), fill=(-999.0,))
        mask = wet_of(out["x"], out["y"])
        res = ranks[0].regrid_to_latlon(cut, f, (lon, lat), mask=mask, cover=True)
        assert all(g.regrid_to_latlon(cut, f, (lon, lat), mask=mask) is None for g in ranks[1:])
        if want is None:
            want = res
        for k in ("values", "cover", "ocean_frac", "n_entries"):
            assert res[k].tobytes() == want[k].tobytes(), (world, k)
        assert res["summary"] == want["summary"]


def test_same_bits_on_two_runs_and_every_knob(sg, monkeypatch):
    from ocean_model_grid_generator_amd import latlon_regrid as G
    plan, ranks = device_grid(sg, "r1")
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    f = G.Field(model_field(out["x"], out["y"], 5, np.float32, True), fill=(-999.0,))
    for kind in ("coarse", "fine"):
        atm = target(kind)
        want = g.regrid_to_latlon(cut, f, atm, cover=True)
        again = g.regrid_to_latlon(cut, f, atm, cover=True)
        assert again["values"].tobytes() == want["values"].tobytes() and again["cover"].tobytes() == want["cover"].tobytes()
        for knob, vals in (("OGG_REGRID_RECORDS", ("1", "2", "8")), ("OGG_REGRID_LONG", ("0", "1", "7", "64", "1000000"))):
            for v in vals:
                monkeypatch.setenv(knob, v)
                res = g.regrid_to_latlon(cut, f, atm, cover=True)
                for k in ("values", "cover", "ocean_frac", "n_entries"):
                    assert res[k].tobytes() == want[k].tobytes(), (kind, knob, v, k)
                monkeypatch.delenv(knob)
    monkeypatch.setenv("OGG_REGRID_RECORDS", "3")
    with pytest.raises(Exception, match="OGG_REGRID_RECORDS"):
        g.regrid_to_latlon(cut, f, target("coarse"))


@pytest.mark.parametrize("nlon, nlat", [(1, 36), (1, 1), (3, 2)])
def test_zonal_and_one_cell_targets(sg, monkeypatch, nlon, nlat):
    """targets whose cells hold a large part of the list (a zonal mean, the whole globe in one cell): the same bits as the definition,
    on the whole-wavefront path and, with every cell forced onto it or off it, on the per-lane path"""
    from ocean_model_grid_generator_amd import latlon_regrid as G
    plan, ranks = device_grid(sg, "r2")
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = out["x"], out["y"]
    atm = G.X.regular_atm(nlon, nlat)
    f = model_field(x, y, 5, np.float32, True)
    lists = g.exchange_grid(cut, atm)
    n = np.bincount(lists["atm"][:, 1].astype(np.int64) * nlon + lists["atm"][:, 0], minlength=nlon * nlat)
    assert n.max() > 512, n.max()   # longer than OGG_REGRID_LONG's default: the whole-wavefront path
    want = None
    for long_n in (None, "0", str(int(n.max()))):
        if long_n is not None:
            monkeypatch.setenv("OGG_REGRID_LONG", long_n)
        for normalize in ("area", "cell"):
            res = g.regrid_to_latlon(cut, G.Field(f, fill=(-999.0,)), atm, normalize=normalize, cover=True)
            check_against_definition(res, lists, f, (-999.0,), normalize)
            if normalize == "area":
                want = res if want is None else want
                assert res["values"].tobytes() == want["values"].tobytes()
        assert res["counts"]["max_entries"] == n.max() and res["counts"]["cells"] == int((n > 0).sum())
        monkeypatch.delenv("OGG_REGRID_LONG", raising=False)
    frac = g.regrid_to_latlon(cut, None, atm, lists=lists)
    assert frac["ocean_frac"].tobytes() == lists["ocean_frac"].tobytes() and frac["n_entries"].tobytes() == n.astype(np.int32).tobytes()


def test_conservation_constant_field_and_remap_round_trip(sg):
    from ocean_model_grid_generator_amd import latlon_regrid as G
    from ocean_model_grid_generator_amd import remap as R
    plan, ranks = device_grid(sg, "r2")
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = out["x"], out["y"]
    lon, lat = target("coarse")
    lists = g.exchange_grid(cut, (lon, lat))
    ny, nx = lists["a_poly"].shape
    Ac = np.bincount(lists["ocn"][:, 1].astype(np.int64) * nx + lists["ocn"][:, 0], weights=lists["area"], minlength=ny * nx)
    f = model_field(x, y, 1, np.float64, False)
    res = g.regrid_to_latlon(cut, f, (lon, lat), normalize="cell")
    got = np.sum(res["values"][0] * res["cell_area"])
    want = np.sum(f[0].reshape(-1) * Ac)
    assert abs(got / want - 1) <= 1e-12, got / want - 1
    assert abs(res["summary"]["integral_latlon"][0] / res["summary"]["integral_model"][0] - 1) <= 1e-12
    # a constant field: a power of two is returned exactly (every product A_e * c is exact, so S = c W); any other constant within
    # the bound of two in-order sums of n terms, n eps relative each
    ok = res["n_entries"] > 0
    for c in (4.0, 3.75):
        const = g.regrid_to_latlon(cut, np.full((ny, nx), c), (lon, lat))
        bound = 4 * np.spacing(c) if c == 4.0 else 2.0 * res["n_entries"][ok] * np.finfo(float).eps * c
        assert np.all(np.abs(const["values"][ok] - c) <= bound) and np.all(const["values"][~ok] == D.FILL), c
    # a smooth lat-lon field remapped onto the model and regridded back keeps its global integral
    lc, pc = np.radians(0.5 * (lon[1:] + lon[:-1])), np.radians(0.5 * (lat[1:] + lat[:-1]))
    L2, P2 = np.meshgrid(lc, pc)
    h = (10 + np.cos(P2) * np.sin(2 * L2) + np.sin(P2))[None]
    onto = g.remap(cut, R.Source(h, lon, lat), fill=False)   # (cells without entries take no part in either direction)
    back = g.regrid_to_latlon(cut, onto["values"], (lon, lat), normalize="cell")
    model = np.sum(onto["values"][0].reshape(-1) * Ac)
    assert abs(np.sum(back["values"][0] * back["cell_area"]) / model - 1) <= 1e-12
    assert abs(np.sum(h[0] * lists["ocean_frac"] * lists["a_atm"]) / model - 1) <= 1e-12


def write_fields(path, x, y):
    """a 3-record float32 SST with an unlimited time axis and a fixed double field on the model cells, NetCDF-3"""
    from ocean_model_grid_generator_amd import netcdf3
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    f = model_field(x, y, 3, np.float32, True)
    f[np.isnan(f)] = 1e20
    ds = netcdf3.Dataset(str(path), [("time", 3), ("yh", ny), ("xh", nx)], record_dim="time")
    ds.def_var("time", netcdf3.NC_DOUBLE, ("time",), [("units", "days since 2000-01-01")], np.array([15.5, 45.0, 74.5]))
    ds.def_var("tos", netcdf3.NC_FLOAT, ("time", "yh", "xh"), [("units", "degC"), ("_FillValue", np.float32(1e20)),
                                                               ("missing_value", np.float32(-999.0))], f)
    ds.def_var("deptho", netcdf3.NC_DOUBLE, ("yh", "xh"), [("units", "m")], 1000.0 + 0.0 * f[0].astype(np.float64))
    ds.write()
    return str(path)


def test_main_fraction_file_and_file_command(sg, tmp_path, capsys):
    from ocean_model_grid_generator_amd import latlon_regrid as G
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from ocean_model_grid_generator_amd import netcdf3
    fr = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "f1", "f2", "x1", "x2", "t1", "t2", "out")}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, xgrid_atm=(72, 36))
    ogg.main(2.0, gridfilename=fr["grid"], xgrid_file=fr["x1"], xgrid_frac_file=fr["f1"], **kw)
    ogg.main(2.0, gridfilename=None, xgrid_file=fr["x2"], xgrid_frac_file=fr["f2"], path="functions", **kw)
    assert "latlon regrid:" in capsys.readouterr().out
    assert open(fr["f1"], "rb").read() == open(fr["f2"], "rb").read()
    h = netcdf3.read_header(fr["f1"])
    frac = np.frombuffer(netcdf3.read_var_bytes(fr["f1"], h, "ocean_frac"), dtype=">f8").reshape(36, 72)
    assert np.all(frac > 0.999) and np.all(frac < 1.001)   # no mask: every cell exchanges
    # the file command writes the field values Supergrid.regrid_to_latlon gives
    g = netcdf3.read_doubles(fr["grid"], names=("x", "y"))
    fields = write_fields(tmp_path / "fields.nc", g["x"], g["y"])
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.latlon_regrid", fr["grid"], fields, "--var", "tos",
                        "--var", "deptho", "--atm", "72", "36", "--cover", "-o", fr["out"]], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert "sum S" in r.stdout
    plan, ranks = device_grid(sg, "r2")
    cut = ranks[0].south_cut()
    shape = ((g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2)
    fld = G.read_field(fields, "tos", shape)
    want = ranks[0].regrid_to_latlon(cut, fld, G.X.regular_atm(72, 36), cover=True)
    h = netcdf3.read_header(fr["out"])
    assert h.vars["tos"].is_record and h.vars["tos"].shape[1:] == (36, 72)
    got = np.frombuffer(netcdf3.read_record_var_bytes(fr["out"], h, "tos"), dtype=">f8").reshape(want["values"].shape)
    assert got.astype(np.float64).tobytes() == want["values"].tobytes()
    cov = np.frombuffer(netcdf3.read_record_var_bytes(fr["out"], h, "tos_cover"), dtype=">f8").reshape(want["cover"].shape)
    assert cov.astype(np.float64).tobytes() == want["cover"].tobytes()
    assert np.any(want["values"] == D.FILL) or np.any(want["cover"] < 1)

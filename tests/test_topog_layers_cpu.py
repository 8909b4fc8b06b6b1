"""CPU tests of layered topography ("Layered topography" of include/ogg_hip.h): the numpy definition against Snyder's worked example
and the 50-digit truth file, its reduction to the single-source definition, the merge's properties, the library's refusals (before any
device work), the share of cells the GPU tests may leave out of their exact comparison, and the command-line surface."""
import ctypes

import numpy as np
import pytest

import small_grids as G
import topog_definition as D
import topog_layers_definition as TL
import topog_layers_inputs as TI

# E_def measured on this definition (test_definition_matches_the_truth_file prints it): 4.0e-9 m, 6.3e-6 of rho (the relative figure
# comes from within 1e-8 degrees of the pole, where phi = lat * pi / 180 rounds to 1e-16 of a quarter turn and rho is 1e-4 m)


def test_snyder_worked_example():
    """Map Projections: A Working Manual, p. 315: International ellipsoid, lat_ts = -71, lon0 = -100, the point (150 E, 75 S)"""
    p = TL.Stereo(-1, -71.0, -100.0, 6378388.0, np.sqrt(0.00672267), lat_gate=0.0)
    X, Y, ok = TL.project(p, 150.0, -75.0)
    assert bool(ok) and abs(float(X) - -1540033.6) <= 0.05 and abs(float(Y) - -560526.4) <= 0.05


def test_definition_matches_the_truth_file(capsys):
    cases = TL.truth_cases()
    assert len(cases) == 8 and sum(c[1].size for c in cases) == 4000
    assert {c[0].h for c in cases} == {1, -1} and {c[0].e == 0.0 for c in cases} == {True, False}
    em, er = TL.definition_error()
    with capsys.disabled():
        print("\nE_def of the numpy projection against the 50-digit truth: %.3g m, %.3g of rho" % (em, er))
    assert np.isfinite(em) and np.isfinite(er)


def test_gate_pole_and_nonfinite_points():
    p = TI.stereo("south_wgs84", lat_gate=60.0)
    lon = np.array([10.0, 10.0, 10.0, np.nan, np.inf, 10.0, 10.0])
    lat = np.array([-60.0, -59.999, -90.0, -70.0, -70.0, np.nan, -90.0 + 0.5e-10])
    X, Y, ok = TL.project(p, lon, lat)
    assert ok.tolist() == [True, False, True, False, False, False, True]
    assert X[2] == 0.0 and Y[2] == 0.0 and X[6] == 0.0 and Y[6] == 0.0 and not np.signbit(X[2]) and not np.signbit(Y[2])
    assert np.hypot(X[0], Y[0]) > 3.0e6


@pytest.mark.parametrize("kind", ["int16", "int16_fill2", "window", "float32_q0.01"])
def test_one_latlon_layer_is_the_single_source_definition(kind):
    r = G.raster(kind)
    ly = TL.layer(r["data"], r["box"], quantum=r["quantum"], fill=r["fill"])
    grids = [G.placed(name) for name in G.PLACEMENTS] + [G.beyond_pole_row(1), G.nonfinite_grid("x", "nan")[:2], G.nonfinite_grid("y", "pinf")[:2]]
    grids += [(x, y) for x, y, _ in G.pole_cells().values()]
    for x, y in grids:
        for cells in ("supergrid", "model"):
            if cells == "model" and ((x.shape[0] - 1) % 2 or (x.shape[1] - 1) % 2):
                continue
            for refine in (None, 3):
                want = D.records(x, y, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], refine=refine, cells_=cells)
                got = TL.records(x, y, [ly], refine=refine, cells_=cells)
                for f in D.RECORD_FIELDS:
                    np.testing.assert_array_equal(got[f], want[f], err_msg=f)
                np.testing.assert_array_equal(got["n_from"][0], want["n"])
                assert not got["n_from"][1:].any()


def test_merge_properties():
    x, y, layers = TI.two_layers()
    top, bottom = layers
    both = TL.records(x, y, layers, cells_="supergrid")
    n = both["n"]
    np.testing.assert_array_equal(both["n_from"].sum(axis=0), n)
    assert both["n_from"][0].sum() > 0 and both["n_from"][1].sum() > 0 and not both["n_missing"].any()
    # a first layer that is all fill reproduces the second alone (the refinement too: use one R for both)
    void = TL.layer(np.full((100, 100), -9999.0, dtype=np.float32), top["box"], top["proj"], quantum=0.01, fill=(-9999.0,))
    under = TL.records(x, y, [void, bottom], refine=5, cells_="supergrid")
    alone = TL.records(x, y, [bottom], refine=5, cells_="supergrid")
    for f in D.RECORD_FIELDS:
        np.testing.assert_array_equal(under[f], alone[f], err_msg=f)
    np.testing.assert_array_equal(under["n_from"][1], alone["n_from"][0])
    assert not under["n_from"][0].any()
    # two fully valid overlapping layers: swapping them changes only which one is read
    xi, yi, a = TI.placed("inside_south")
    g, gbox = TI.global_int16()
    b = TL.layer(g, gbox)
    ab, ba = TL.records(xi, yi, [a, b], refine=4, cells_="supergrid"), TL.records(xi, yi, [b, a], refine=4, cells_="supergrid")
    only_a, only_b = TL.records(xi, yi, [a], refine=4, cells_="supergrid"), TL.records(xi, yi, [b], refine=4, cells_="supergrid")
    for f in D.RECORD_FIELDS:
        np.testing.assert_array_equal(ab[f], only_a[f], err_msg=f)
        np.testing.assert_array_equal(ba[f], only_b[f], err_msg=f)
    assert not ab["n_from"][1].any() and not ba["n_from"][1].any()
    # q_mul scales sums and extremes exactly
    m = 7
    scaled = TL.records(xi, yi, [TL.layer(a["q"].astype(np.int16), a["box"], a["proj"], q_mul=m)], refine=4, cells_="supergrid")
    np.testing.assert_array_equal(scaled["sum"], m * only_a["sum"])
    np.testing.assert_array_equal(scaled["sumsq"], m * m * only_a["sumsq"])
    np.testing.assert_array_equal(scaled["min"], m * only_a["min"])
    np.testing.assert_array_equal(scaled["max"], m * only_a["max"])
    np.testing.assert_array_equal(scaled["n"], only_a["n"])
    with pytest.raises(ValueError, match="2\\^21"):
        TL.layer(a["q"].astype(np.int16), a["box"], a["proj"], q_mul=1 << 12)


def _one_layer(L, **kw):
    """a band and one projected layer that pass every check, with the fields of ``kw`` changed (proj_*: the projection's)"""
    data = np.zeros((4, 4), dtype=np.int16)
    x = np.zeros((3, 3))
    band = L.TopogBand(nx=2, j0=0, n_cell_rows=2, cells=L.TOPOG_SUPERGRID_CELLS, refine=2, oversample=2.0)
    band.x = band.y = band.x_next = band.y_next = x.ctypes.data
    layers = (L.TopogLayer * 4)()
    for ly in layers:
        ly.src = L.TopogSource(data=data.ctypes.data, dtype=L.TOPOG_INT16, n_fill=0, Nx=4, Ny=4, lon0=-2000.0, dlon=1000.0, lat0=-2000.0,
                               dlat=1000.0, quantum=1.0, wet_below=0.0)
        ly.kind, ly.q_mul = L.TOPOG_POLAR_STEREO, 1
        ly.proj = L.TopogProjection(h=-1, lon0=0.0, a=6378137.0, e=0.08, K=1.2e7, lat_gate=60.0)
    for k, v in kw.items():
        if k.startswith("proj_"):
            setattr(layers[0].proj, k[5:], v)
        elif k in ("dlon", "dlat"):
            setattr(layers[0].src, k, v)
        else:
            setattr(layers[0], k, v)
    return band, layers, (data, x)


@pytest.mark.parametrize("kw,n_layers,text", [
    ({}, 0, "n_layers = 0"), ({}, 5, "n_layers = 5"), (dict(kind=2), 1, "kind = 2"), (dict(proj_h=0), 1, "hemisphere h = 0"),
    (dict(proj_h=2), 1, "hemisphere h = 2"), (dict(proj_e=0.2), 1, "eccentricity"), (dict(proj_e=-0.01), 1, "eccentricity"),
    (dict(dlon=0.0), 1, "dX and dY must be positive"), (dict(dlat=-1.0), 1, "dX and dY must be positive"),
    (dict(proj_lat_gate=-80.5), 1, "lat_gate"), (dict(q_mul=0), 1, "q_mul = 0"), (dict(proj_K=0.0), 1, "K = 0")])
def test_library_refusals_need_no_device(kw, n_layers, text):
    """every argument is validated before any device work: OGG_EARG and a message, from every entry point that takes layers"""
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    band, layers, keep = _one_layer(L, **kw)
    out = np.zeros(4, dtype=L.TOPOG_MERGE_RECORD)
    rcs = [lib.ogg_topog_layers(ctypes.byref(band), n_layers, layers, out.ctypes.data)]
    msgs = [lib.ogg_last_error().decode()]
    rcs.append(lib.ogg_topog_layers_band_dev(ctypes.byref(band), n_layers, layers, 8, 256, 8, None))   # pointers never dereferenced
    msgs.append(lib.ogg_last_error().decode())
    assert rcs == [L.OGG_EARG, L.OGG_EARG] and all(text in m for m in msgs), msgs
    if any(k.startswith("proj_") for k in kw):
        rc = lib.ogg_topog_project_dev(ctypes.byref(layers[0].proj), 4, 8, 8, 8, 8, 8, None)
        assert rc == L.OGG_EARG and text in lib.ogg_last_error().decode()


def test_edge_condition_leaves_out_at_most_one_percent():
    """The GPU tests compare every field exactly except in cells holding a sample whose fractional index, in the definition's own
    evaluation, lies within delta = 64 * 1.5 * E_def (in elements) of an integer.  On every named input at most 1 % of the cells are
    left out; the patches and rasters are not commensurate so that it is so."""
    em, _ = TL.definition_error()
    worst = 0.0
    inputs = [(n,) + TI.named(n) for n in TI.NAMED] + [("strip%d" % s[0],) + s[1:] for s in TI.strips()]
    lists = [("two",) + TI.two_layers(), ("three",) + TI.three_layers(), ("four",) + TI.four_layers()]
    for name, x, y, ly in inputs + lists:
        layers = ly if isinstance(ly, list) else [ly]
        rec = TL.records(x, y, layers, cells_="supergrid", with_edge=True)
        delta = max(64.0 * 1.5 * em / l["box"][1] for l in layers if l["kind"] == TL.POLAR_STEREO)
        share = float(np.mean(rec["edge"] <= delta))
        worst = max(worst, share)
        assert share <= 0.01, (name, share)
        assert (rec["n"] + rec["n_missing"]).sum() > 0
    assert worst <= 0.01


def test_named_inputs_reach_what_they_are_named_for():
    rec = {n: TL.records(*TI.named(n)[:2], [TI.named(n)[2]], cells_="supergrid") for n in TI.NAMED}
    assert not rec["inside_south"]["n_missing"].any() and not rec["inside_north"]["n_missing"].any()
    for n in ("left_edge", "right_edge", "bottom_edge", "top_edge", "gate_south", "gate_north"):
        r = rec[n]
        assert (r["n"] == 0).any() and (r["n_missing"] == 0).any() and ((r["n"] > 0) & (r["n_missing"] > 0)).any(), n
    w = rec["wrong_hemisphere"]
    assert not w["n"].any() and (w["R"] == 1).all() and (w["n_missing"] == 1).all() and not w["n_clamped"].any()
    for n in ("pole_corner_south", "pole_corner_north"):
        assert not rec[n]["n_pole"].any() and not rec[n]["n_missing"].any() and (rec[n]["R"] > 1).all()
    for n, sign in (("pole_enclosing_south", -1), ("pole_enclosing_north", 1)):
        r, (x, y, ly) = rec[n], TI.named(n)
        assert r["n_pole"].sum() == 1 and r["n_missing"].sum() == 0
        fi, fj = int(np.floor((0.0 - ly["box"][0]) / ly["box"][1])), int(np.floor((0.0 - ly["box"][2]) / ly["box"][3]))
        assert r["min"][0, 0] == r["max"][0, 0] == ly["q"][fj, fi]     # every sample reads the element at (+0, +0)
    for n in ("nan", "pinf", "minf"):
        assert (rec[n]["n_missing"] > 0).sum() >= 4 and not rec[n]["n_clamped"].any()
    other = TL.records(*TI.pole_enclosing(1, "south_wgs84")[:2], [TI.pole_enclosing(1, "south_wgs84")[2]], cells_="supergrid")
    assert other["n"].sum() == 0 and other["n_pole"].sum() == 1     # the other hemisphere's layer is refused by its gate


def test_python_surface_without_a_device(tmp_path):
    from ocean_model_grid_generator_amd import netcdf3, ocean_grid_generator as ogg, topography as T
    p = T.PolarStereo.parse("stere:S,lat_ts=-71,lon0=0")
    ref = TI.stereo("south_wgs84")
    assert p.h == -1 and abs(p.K / ref.K - 1.0) < 1e-14 and abs(p.e - ref.e) < 1e-12 and str(T.PolarStereo.parse(str(p))) == str(p)
    sphere = T.PolarStereo.parse("stere:N,lat_ts=90,lon0=170,a=6371000,rf=0")
    assert sphere.e == 0.0 and sphere.K == 2.0 * 6371000.0
    with pytest.raises(ValueError, match="stere:N or stere:S"):
        T.PolarStereo.parse("utm:33")
    # the inverse behind the default gate against the definition's forward projection
    lat = np.array([-89.9, -80.0, -65.0, -50.0])
    X, Y, _ = TL.project(ref, 33.0, lat)
    np.testing.assert_allclose(p.pole_latitude(X, Y), -lat, rtol=0, atol=1e-9)
    data = np.zeros((200, 200), dtype=np.int16)
    s = T.Source(data, -100.0e3, 1000.0, -100.0e3, 1000.0, projection=p, name="bm")
    X, Y, _ = TL.project(ref, 45.0, -(s.lat_gate + 0.01))
    assert abs(float(np.hypot(X, Y)) - np.hypot(100.0e3, 100.0e3)) < 1.0 and not s.periodic
    with pytest.raises(ValueError, match="gate latitude"):
        T.Source(data, -2.0e8, 1000.0, -100.0e3, 1000.0, projection=p)
    with pytest.raises(ValueError, match="lat_gate belongs"):
        T.Source(data, -180.0, 1.8, -90.0, 0.9, lat_gate=50.0)
    # quanta and q_mul
    g = T.Source(np.zeros((180, 360), dtype=np.int16), -180.0, 1.0, -90.0, 1.0, name="gebco")
    f = T.Source(np.zeros((200, 200), dtype=np.float32), -100.0e3, 1000.0, -100.0e3, 1000.0, projection=p, name="bm")
    sl = T.as_sources([f, g])
    assert isinstance(sl, T.SourceList) and sl.quantum == 0.01 and sl.q_mul == [1, 100] and sl.names == ["bm", "gebco"]
    lay = sl.layers(sea_level=2.0)
    assert lay[0].kind == 1 and lay[1].kind == 0 and lay[1].q_mul == 100 and lay[0].src.wet_below == lay[1].src.wet_below == 200.0
    assert lay[0].proj.h == -1 and lay[0].proj.lat_gate == f.lat_gate
    with pytest.raises(ValueError, match="not an integer multiple"):
        T.SourceList([f, g.replace(quantum=0.015)])
    with pytest.raises(ValueError, match="1 .. 4 sources"):
        T.SourceList([g] * 5)
    assert T.as_sources(g) is g and T.as_sources([g]) is g and isinstance(T.as_sources(f), T.SourceList)
    # records of layers: empty, merged, assembled
    e = T.empty_records((2, 3), merge=True)
    assert T.has_layers(e) and e["min"][0, 0] == np.iinfo(np.int32).max and not e["n_from"].any()
    e2 = T.empty_records((2, 3), merge=True)
    e2["n_from"][..., 1] = 5
    T.merge_into(e, e2)
    T.merge_into(e, e2)
    assert (e["n_from"][..., 1] == 10).all()
    with pytest.raises(ValueError, match="do not combine"):
        T.merge_into(e, T.empty_records((2, 3)))
    assert T.record_words(merge=True) == 11
    # the plane fit is refused before any device work
    x, y = TI.patch(37.3, -84.1)
    with pytest.raises(ValueError, match="plane fit"):
        T.topography(x, y, [f, g], plane=True)
    for path in ("pass", "functions"):
        with pytest.raises(ValueError, match="--topog_roughness: the plane fit"):
            ogg.main(1.0, gridfilename=None, topog_source=["a.nc", "b.nc"], topog_roughness=True, path=path)
        with pytest.raises(ValueError, match="--topog_roughness: the plane fit"):
            ogg.main(1.0, gridfilename=None, topog_source="a.nc", topog_proj="stere:S,lat_ts=-71", topog_roughness=True, path=path)
    # flags
    a = ogg.build_parser().parse_args(["-r", "1", "--topog_source", "bm.nc", "--topog_source", "gebco.nc", "--topog_var", "bed", "--topog_var",
                                       "elevation", "--topog_proj", "stere:S,lat_ts=-71,lon0=0", "--topog_proj", "latlon"])
    assert a.topog_source == ["bm.nc", "gebco.nc"] and a.topog_var == ["bed", "elevation"] and a.topog_proj[1] == "latlon"
    b = ogg.build_parser().parse_args(["-r", "1"])
    assert b.topog_source is None and b.topog_var is None and b.topog_proj is None
    assert ogg.AnalysisFlags().topog_proj is None
    # one lat-lon --topog_source resolves to the Source of the single-source path; a CF grid mapping to a projected one
    srcf, bmf = str(tmp_path / "src.nc"), str(tmp_path / "bm.nc")
    z = (np.arange(90 * 180) % 500).astype(np.int16).reshape(90, 180)
    ds = netcdf3.Dataset(srcf, [("lat", 90), ("lon", 180)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], -90.0 + 2.0 * (np.arange(90) + 0.5))
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], -180.0 + 2.0 * (np.arange(180) + 0.5))
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], z)
    ds.write()
    one = ogg._topog_source(ogg.build_parser().parse_args(["-r", "1", "--topog_source", srcf]).topog_source, None, None)
    old = ogg._topog_source(srcf, "elevation")
    assert type(one) is T.Source and one.projection is None and one.data.tobytes() == old.data.tobytes() and \
        (one.lon0, one.dlon, one.lat0, one.dlat, one.quantum, one.fill) == (old.lon0, old.dlon, old.lat0, old.dlat, old.quantum, old.fill)
    bed = (np.arange(40 * 50) % 300).astype(np.float32).reshape(40, 50)
    ds = netcdf3.Dataset(bmf, [("y", 40), ("x", 50)])
    ds.def_var("x", netcdf3.NC_DOUBLE, ("x",), [("units", "m")], -12000.0 + 500.0 * np.arange(50))
    ds.def_var("y", netcdf3.NC_DOUBLE, ("y",), [("units", "m")], 9750.0 - 500.0 * np.arange(40))     # descending, as BedMachine's
    ds.def_var("mapping", netcdf3.NC_INT, (), [("grid_mapping_name", "polar_stereographic"), ("standard_parallel", -71.0),
                                               ("straight_vertical_longitude_from_pole", 0.0), ("semi_major_axis", 6378137.0),
                                               ("inverse_flattening", 298.257223563), ("latitude_of_projection_origin", -90.0)], 0)
    ds.def_var("bed", netcdf3.NC_FLOAT, ("y", "x"), [("grid_mapping", "mapping"), ("_FillValue", np.float32(-9999.0))], bed)
    ds.write()
    bm = T.read_source(bmf, "bed")
    assert bm.projection is not None and bm.projection.h == -1 and bm.projection.lat_ts == -71.0
    assert (bm.lon0, bm.dlon, bm.lat0, bm.dlat) == (-12250.0, 500.0, -10000.0, 500.0) and bm.fill == (-9999.0,)
    np.testing.assert_array_equal(bm.data, bed[::-1])
    both = ogg._topog_source([bmf, srcf], ["bed", "elevation"], None)
    assert isinstance(both, T.SourceList) and both.q_mul == [1, 100] and both.names == [bmf, srcf]
    same = T.read_sources([bmf, srcf], ["bed", "elevation"])
    assert [s.describe() for s in same.sources] == [s.describe() for s in both.sources]
    flagged = T.read_source(srcf, "elevation", projection="stere:N,lat_ts=70,lon0=-45")
    assert flagged.projection.h == 1 and flagged.dlon == 2.0


def test_file_flags_of_a_list(tmp_path):
    """One --quantum with several sources is the float sources' (an int16 metre raster keeps 1 m); one per source goes to each.
    --topog_proj latlon overrides a file's own grid mapping; --topog_roughness on one file with a polar stereographic mapping is
    refused with the other flags, before the grid is made."""
    from ocean_model_grid_generator_amd import netcdf3, ocean_grid_generator as ogg, topography as T
    srcf, bmf = str(tmp_path / "src.nc"), str(tmp_path / "bm.nc")
    ds = netcdf3.Dataset(srcf, [("lat", 90), ("lon", 180)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], -90.0 + 2.0 * (np.arange(90) + 0.5))
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], -180.0 + 2.0 * (np.arange(180) + 0.5))
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], np.zeros((90, 180), dtype=np.int16))
    ds.write()
    ds = netcdf3.Dataset(bmf, [("lat", 40), ("lon", 50)])     # named lat / lon, so that it also reads as a lat-lon raster
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "m")], -12.0 + 0.5 * np.arange(50))
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "m")], -80.0 + 0.5 * np.arange(40))
    ds.def_var("mapping", netcdf3.NC_INT, (), [("grid_mapping_name", "polar_stereographic"), ("standard_parallel", -71.0)], 0)
    ds.def_var("bed", netcdf3.NC_FLOAT, ("lat", "lon"), [("grid_mapping", "mapping")], np.zeros((40, 50), dtype=np.float32))
    ds.write()
    both = T.read_sources([bmf, srcf], ["bed", "elevation"], quantum=0.05)
    assert [s.quantum for s in both.sources] == [0.05, 1.0] and both.q_mul == [1, 20]
    both = T.read_sources([bmf, srcf], ["bed", "elevation"], quantum=[0.25, 0.5])
    assert [s.quantum for s in both.sources] == [0.25, 0.5] and both.q_mul == [1, 2]
    assert T.read_sources(srcf, quantum=0.5).quantum == T.read_sources(srcf, quantum=[0.5]).quantum == 0.5     # one source: as ever
    with pytest.raises(ValueError, match="3 quanta for 2 sources"):
        T.read_sources([bmf, srcf], ["bed", "elevation"], quantum=[1.0, 1.0, 1.0])
    # the file's own mapping, and latlon over it
    assert T.file_projection(bmf, "bed").lat_ts == -71.0 and T.file_projection(srcf) is None and T.file_projection("none.nc") is None
    assert T.read_source(bmf, "bed").projection is not None
    flat = T.read_source(bmf, "bed", projection="latlon")
    assert flat.projection is None and flat.dlon == 0.5
    assert type(ogg._topog_source(bmf, "bed", "latlon")) is T.Source and isinstance(ogg._topog_source(bmf, "bed"), T.SourceList)
    assert isinstance(T.read_sources(bmf, "bed"), T.SourceList) and type(T.read_sources(bmf, "bed", "latlon")) is T.Source
    # the plane fit and a mapped file: refused among the flags
    assert ogg._topog_layered(bmf, None, "bed") and not ogg._topog_layered(bmf, "latlon", "bed") and not ogg._topog_layered(srcf)
    for path in ("pass", "functions"):
        with pytest.raises(ValueError, match="--topog_roughness: the plane fit"):
            ogg.main(1.0, gridfilename=None, topog_source=bmf, topog_var="bed", topog_roughness=True, path=path)

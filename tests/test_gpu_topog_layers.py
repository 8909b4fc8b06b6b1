"""GPU tests of layered topography (csrc/ogg_topog.hip: topog_layers_kernel; topography.py): the device projection against the 50-digit
truth, one lat-lon layer against the single-source kernel bit for bit, projected layers and lists against the numpy definition
(tests/topog_layers_definition.py) exactly, every split into bands, a physical check that does not come from the definition, and
main() against the file command.

The exact comparison leaves out the cells that hold a sample whose fractional index, in the definition's evaluation, lies within
delta = 64 * 1.5 * E_def (in elements of that raster) of an integer: there the device's sine, cosine and series, a few ulp from
numpy's, may floor to the neighbouring element.  E_def comes from the truth file; at most 1 % of an input's cells may be left out
(tests/test_topog_layers_cpu.py shows the inputs stay within that), and those cells are still held to n + n_missing, R, n_pole and
n_clamped."""
import ctypes

import numpy as np
import pytest

import small_grids as G
import topog_layers_definition as TL
import topog_layers_inputs as TI

pytestmark = pytest.mark.gpu
K_REF = 1.5          # the rule of tests/test_gpu_truth.py: the device's error at most 1.5 times the definition's own
FIELDS = TL.RECORD_FIELDS


@pytest.fixture(scope="module")
def T(hip):
    from ocean_model_grid_generator_amd import topography
    return topography


@pytest.fixture(scope="module")
def e_def():
    return TL.definition_error()


def to_source(T, ly, name):
    """the product's Source of a definition layer"""
    p = ly["proj"]
    if p is None:
        return T.Source(ly["raw"], *ly["box"], fill=ly["fill"], quantum=ly["quantum"], name=name)
    proj = T.PolarStereo(p.h, p.lat_ts, p.lon0, p.a, e=p.e)
    assert proj.K == p.K
    return T.Source(ly["raw"], *ly["box"], fill=ly["fill"], quantum=ly["quantum"], projection=proj, lat_gate=p.lat_gate, name=name)


def to_list(T, layers):
    sl = T.SourceList([to_source(T, ly, "layer%d" % k) for k, ly in enumerate(layers)])
    assert sl.q_mul == [ly["q_mul"] for ly in layers]
    return sl


def assert_against_definition(got, want, layers, e_def, what=""):
    """every field exact outside the cells the module docstring leaves out; the rest of those cells' fields all the same"""
    delta = max(64.0 * K_REF * e_def[0] / ly["box"][1] for ly in layers if ly["kind"] == TL.POLAR_STEREO)
    out = want["edge"] <= delta
    assert out.mean() <= 0.01, (what, float(out.mean()))
    keep = ~out
    for f in FIELDS:
        np.testing.assert_array_equal(got[f].astype(np.int64)[keep], want[f][keep], err_msg="%s %s" % (what, f))
    for k in range(TL.MAX_SOURCES):
        np.testing.assert_array_equal(got["n_from"][..., k][keep], want["n_from"][k][keep], err_msg="%s n_from[%d]" % (what, k))
    np.testing.assert_array_equal(got["n"] + got["n_missing"], want["n"] + want["n_missing"], err_msg=what)
    for f in ("R", "n_pole", "n_clamped"):
        np.testing.assert_array_equal(got[f].astype(np.int64), want[f], err_msg="%s %s" % (what, f))
    np.testing.assert_array_equal(got["n_from"].sum(axis=-1), got["n"], err_msg=what)


def check(T, x, y, layers, e_def, what, cells="supergrid", refine=None, sea_level=0.0):
    got = T.topography(x, y, to_list(T, layers), cells=cells, refine=refine, sea_level=sea_level)
    want = TL.records(x, y, layers, refine=refine, cells_=cells, sea_level=sea_level, with_edge=True)
    assert_against_definition(got["records"], want, layers, e_def, what)
    return got, want


# ---- 1. the projection ------------------------------------------------------------------------------------------------
def test_device_projection_against_the_truth(T, hip, e_def, capsys):
    """ogg_topog_project_dev -- the sampling kernel's own projection function -- on the 4000 points of tests/golden/stereo_truth.npz:
    its largest error in metres and relative to rho at most 1.5 times the numpy definition's (E_def = 4.0e-9 m, 6.3e-6 of rho).
    Measured on an MI355X: 3.99e-9 m and 6.28e-6 of rho, 1.000 times E_def in both (the test prints the figures)."""
    import torch
    L = hip
    em = er = 0.0
    for case in TL.truth_cases():
        p, lon, lat = case[0], case[1], case[2]
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (lon, lat)]
        X, Y = torch.empty_like(d[0]), torch.empty_like(d[0])
        ok = torch.zeros(lon.size, dtype=torch.int32, device="cuda:0")
        desc = L.TopogProjection(h=p.h, lon0=p.lon0, a=p.a, e=p.e, K=p.K, lat_gate=p.lat_gate)
        L.call("ogg_topog_project_dev", ctypes.byref(desc), lon.size, d[0].data_ptr(), d[1].data_ptr(), X.data_ptr(), Y.data_ptr(),
               ok.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(ok.cpu().numpy().all())
        m, r = TL.truth_errors(X.cpu().numpy(), Y.cpu().numpy(), case)
        em, er = max(em, float(m.max())), max(er, float(r.max()))
    with capsys.disabled():
        print("\ndevice projection against the 50-digit truth: %.3g m (%.3f of E_def %.3g m), %.3g of rho (%.3f of E_def %.3g)"
              % (em, em / e_def[0], e_def[0], er, er / e_def[1], e_def[1]))
    assert em <= K_REF * e_def[0] and er <= K_REF * e_def[1]
    # the gate, the pole and points that are not finite, as the definition has them
    p = TI.stereo("south_wgs84", lat_gate=60.0)
    lon = np.array([10.0, 10.0, 10.0, np.nan, np.inf, 10.0, 10.0])
    lat = np.array([-60.0, -59.999, -90.0, -70.0, -70.0, np.nan, -90.0 + 0.5e-10])
    d = [torch.from_numpy(a).to("cuda:0") for a in (lon, lat)]
    X, Y, ok = torch.full_like(d[0], 7.0), torch.full_like(d[0], 7.0), torch.zeros(7, dtype=torch.int32, device="cuda:0")
    desc = L.TopogProjection(h=p.h, lon0=p.lon0, a=p.a, e=p.e, K=p.K, lat_gate=p.lat_gate)
    L.call("ogg_topog_project_dev", ctypes.byref(desc), 7, d[0].data_ptr(), d[1].data_ptr(), X.data_ptr(), Y.data_ptr(), ok.data_ptr(), None)
    torch.cuda.synchronize()
    wX, wY, wok = TL.project(p, lon, lat)
    assert ok.cpu().numpy().tolist() == wok.astype(int).tolist() == [1, 0, 1, 0, 0, 0, 1]
    Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
    assert Xh[2] == 0.0 and Yh[2] == 0.0 and Xh[6] == 0.0 and not np.signbit(Xh[2]) and not np.signbit(Yh[2]) and not Xh[[1, 3, 4, 5]].any()
    assert abs(Xh[0] - wX[0]) <= 1e-8 and abs(Yh[0] - wY[0]) <= 1e-8


# ---- 2. one lat-lon layer is the single-source kernel --------------------------------------------------------------------
def latlon_source(T, kind):
    if kind == "regional_fill2":
        r = G.raster("int16_fill2")
        return T.Source(np.ascontiguousarray(r["data"][G.WINDOW]), *G.WINDOW_BOX, fill=r["fill"])
    r = G.raster(kind)
    return T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])


@pytest.mark.parametrize("kind", ["int16", "regional_fill2", "float32_q0.01"])
def test_one_latlon_layer_is_the_single_source_kernel(T, kind):
    """periodic int16, regional int16 with two fill values, quantised float32: the merge records' base is ogg_topog's record byte for
    byte, n_from[0] = n; on placements inside, across the raster's edges and the date line, pole-enclosing cells and a NaN point"""
    src = latlon_source(T, kind)
    grids = [G.placed(n) for n in G.PLACEMENTS] + [G.nonfinite_grid("x", "nan")[:2], G.beyond_pole_row(-1)]
    grids += [(x, y) for x, y, _ in G.pole_cells().values()] + [G.shape_grid(n) for n in ("1x1", "1x65")]
    for x, y in grids:
        even = (x.shape[0] - 1) % 2 == 0 and (x.shape[1] - 1) % 2 == 0
        for cells in ("supergrid", "model") if even else ("supergrid",):
            for refine in (None, 3):
                one = T.topography(x, y, src, cells=cells, refine=refine, sea_level=-3.0)
                lay = T.topography(x, y, T.SourceList([src]), cells=cells, refine=refine, sea_level=-3.0)
                a, b = one["records"], lay["records"]
                assert b.dtype == hip_merge_dtype(T)
                for f in a.dtype.names:
                    assert a[f].tobytes() == b[f].tobytes(), (kind, cells, refine, f)
                np.testing.assert_array_equal(b["n_from"][..., 0], a["n"])
                assert not b["n_from"][..., 1:].any()
                for f in ("height", "h_std", "depth", "wet_fraction"):
                    assert one[f].tobytes() == lay[f].tobytes()


def hip_merge_dtype(T):
    from ocean_model_grid_generator_amd import _lib
    return _lib.TOPOG_MERGE_RECORD


# ---- 3. one projected layer against the definition -------------------------------------------------------------------------
@pytest.mark.parametrize("name", TI.NAMED)
def test_one_projected_layer(T, e_def, name):
    """north and south, ellipsoid and sphere, lon0 != 0; a patch inside the raster, across each of its edges, across the gate
    latitude, on the wrong hemisphere (every sample missing, R = 1), with the pole as a corner, around the pole; NaN and infinite
    points.  Supergrid and model cells."""
    x, y, ly = TI.named(name)
    got, want = check(T, x, y, [ly], e_def, name)
    if (x.shape[0] - 1) % 2 == 0 and (x.shape[1] - 1) % 2 == 0:
        check(T, x, y, [ly], e_def, name, cells="model", sea_level=250.0)
    if name == "wrong_hemisphere":
        assert not got["records"]["n"].any() and (got["records"]["R"] == 1).all()
    if name.startswith("pole_enclosing"):
        assert got["records"]["n_pole"].sum() == 1 and got["records"]["min"][0, 0] == got["records"]["max"][0, 0]


@pytest.mark.parametrize("refine", TI.REFINES)
def test_every_refine(T, e_def, refine):
    """R x R samples, R around the wavefront's 64: one lane's share is 1, 2 or more samples, and the last round is partial"""
    x, y, ly = TI.placed("left_edge")
    check(T, x[:5, :7], y[:5, :7], [ly], e_def, "refine %d" % refine, refine=refine)
    x, y, ly = TI.pole_enclosing(-1)
    check(T, x, y, [ly], e_def, "pole, refine %d" % refine, refine=refine)


def test_strips(T, e_def):
    """1 x n cells, n = 1 .. 129: records that are no multiple of the four a wavefront takes at a time, more than one workgroup"""
    for n, x, y, ly in TI.strips():
        check(T, x, y, [ly], e_def, "strip %d" % n)


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two_layers", "three_layers", "four_layers"])
def test_lists_against_the_definition(T, e_def, which):
    """a projected float32 raster with fill holes over a global int16 one (q_mul = 100); a projected layer over a projected layer of
    another plane over lat-lon; four layers: n_from against the definition, and model cells the integer combination of their four
    supergrid cells"""
    x, y, layers = getattr(TI, which)()
    got, want = check(T, x, y, layers, e_def, which, sea_level=-100.0)
    assert all(want["n_from"][k].sum() > 0 for k in range(len(layers)))
    assert got["source_names"] == ["layer%d" % k for k in range(len(layers))] and got["n_from"].shape == (len(layers),) + x[1:, 1:].shape
    np.testing.assert_array_equal(got["n_from"].sum(axis=0), got["records"]["n"])
    model, _ = check(T, x, y, layers, e_def, which + " model", cells="model", sea_level=-100.0)
    sg, md = got["records"], model["records"]
    blocks = lambda a: [a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]]   # noqa: E731
    for f in ("n", "n_missing", "n_wet", "sum", "sumsq", "n_pole", "n_clamped", "n_from"):
        np.testing.assert_array_equal(md[f], sum(blocks(sg[f])), err_msg=f)
    np.testing.assert_array_equal(md["min"], np.minimum.reduce(blocks(sg["min"])))
    np.testing.assert_array_equal(md["max"], np.maximum.reduce(blocks(sg["max"])))
    np.testing.assert_array_equal(md["R"], np.maximum.reduce(blocks(sg["R"])))


def test_a_value_beyond_the_limit_is_refused(T):
    """|q_mul * q| <= 2^21 of every stored value, sampled or not: an int16 raster of 300 under a float raster of quantum 1e-4 (q_mul =
    10000) fails the call; nothing is clamped"""
    x, y, top = TI.placed("inside_south")
    g = np.zeros((180, 360), dtype=np.int16)
    g[170, 5] = 300     # far from the patch
    srcs = [T.Source((0.1 * top["raw"]).astype(np.float32), *top["box"], quantum=1.0e-4, projection=to_source(T, top, "t").projection),
            T.Source(g, -180.0, 1.0, -90.0, 1.0)]
    from ocean_model_grid_generator_amd import _lib
    with pytest.raises(_lib.OggHipError, match="q_mul = 10000 times a stored value exceeds"):
        T.topography(x, y, srcs)
    with pytest.raises(ValueError, match="exceeds 2\\^21"):
        T.DeviceSourceList(T.SourceList(srcs), "cuda:0")


# ---- 5. bands -----------------------------------------------------------------------------------------------------------------
def test_every_split_into_bands(T, hip):
    """A 65-row patch on three layers, model cells (the last model row holds one supergrid row): every split into two bands and one
    into five, device pointers throughout (band_records_dev on a DeviceSourceList), assembled: the bytes of the unsplit call."""
    import torch
    L = hip
    _, _, layers = TI.three_layers()
    x, y = TI.patch(37.3, -84.1, ny=65, nx=8, dlat=0.011, dlon=0.6)
    dev = T.DeviceSourceList(to_list(T, layers), "cuda:0", sea_level=-50.0)
    xd, yd = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def run(edges, cells):
        pieces, keep = [], []
        for a, b in zip(edges[:-1], edges[1:]):
            band = L.TopogBand(nx=8, j0=a, n_cell_rows=b - a, cells=cells, refine=0, oversample=2.0)
            band.x, band.y, band.x_next, band.y_next = xd[a].data_ptr(), yd[a].data_ptr(), xd[b].data_ptr(), yd[b].data_ptr()
            m0, out, ws = T.band_records_dev(band, dev.desc, st, xd.device)
            assert out.shape[2] == 11
            pieces.append((m0, out))
            keep.append(ws)
        torch.cuda.synchronize()
        sh = 1 if cells == L.TOPOG_MODEL_CELLS else 0
        return T.assemble([(m0, T.records_to_host(out)) for m0, out in pieces], (65 + sh) >> sh, 8 >> sh)

    for cells in (L.TOPOG_MODEL_CELLS, L.TOPOG_SUPERGRID_CELLS):
        one = run((0, 65), cells)
        assert one.dtype == L.TOPOG_MERGE_RECORD and one["n"].sum() > 0 and (one["n_from"].sum(axis=(0, 1))[:3] > 0).all()
        for cut in range(1, 65):
            assert run((0, cut, 65), cells).tobytes() == one.tobytes(), cut
        assert run((0, 7, 20, 21, 48, 65), cells).tobytes() == one.tobytes()
    host = T.topography(x[:65], y[:65], to_list(T, layers), sea_level=-50.0)["records"]     # 64 rows: the host form, model cells
    assert host.tobytes() == run((0, 64), L.TOPOG_MODEL_CELLS)[:32].tobytes()


# ---- 6. a check that does not come from the definition ----------------------------------------------------------------------
def test_two_rasters_of_one_field_agree(T):
    """One smooth analytic field, h = A sin(X / a) cos(Y / b) of the south polar plane (X, Y), sampled onto a 0.02 degree lat-lon
    raster and onto a 1 km stereographic raster around 80 S.  Either topography reads, for every sample, the field at the centre of
    the element the sample falls in: off by at most G times half that element's diagonal (in the plane), G the field's largest
    gradient.  |grad h|^2 = A^2 (cos^2 u cos^2 v / a^2 + sin^2 u sin^2 v / b^2), u = X / a, v = Y / b, is linear in cos^2 u and in
    cos^2 v, so its maximum is at a corner of [0, 1]^2: G = A / min(a, b) = 0.02.  The cell means of the two topographies so differ
    by at most G (d1 + d2) / 2, d1 = 2.23 km the largest diagonal of a lat-lon element in the plane and d2 = 1.41 km that of a
    stereographic one, plus the two quantisations of 0.005 m: 36.5 m, within the G d1 = 44.6 m of one lat-lon element's diagonal.
    With the numpy definition the two differ by 0.52 m; a sphere in place of WGS84 gives 43.9 m and a standard parallel of 70 S
    40.5 m, both beyond the bound.
    The lat-lon raster is filled through the definition's projection (TL.project, held to the 50-digit truth by
    tests/test_topog_layers_cpu.py): the check is independent of the device code and of the definition's sampling and merge, not of
    that one function."""
    A, a, b = 1000.0, 50.0e3, 70.0e3
    G_max = A / min(a, b)
    field = lambda X, Y: A * np.sin(X / a) * np.cos(Y / b)   # noqa: E731
    p = TI.stereo("south_wgs84")
    x, y = TI.patch(32.0, -80.0, dlon=0.25, dlat=0.06)
    # the lat-lon raster: 29 .. 35 E, 81 .. 79 S
    lon = 29.0 + 0.02 * (np.arange(300) + 0.5)
    lat = -81.0 + 0.02 * (np.arange(100) + 0.5)
    Xc, Yc, _ = TL.project(p, lon[None, :], lat[:, None])
    ll = T.Source(field(Xc, Yc).astype(np.float32), 29.0, 0.02, -81.0, 0.02, name="latlon")
    Xe, Ye, _ = TL.project(p, (29.0 + 0.02 * np.arange(301))[None, :], (-81.0 + 0.02 * np.arange(101))[:, None])
    d1 = float(max(np.hypot(Xe[1:, 1:] - Xe[:-1, :-1], Ye[1:, 1:] - Ye[:-1, :-1]).max(),
                   np.hypot(Xe[1:, :-1] - Xe[:-1, 1:], Ye[1:, :-1] - Ye[:-1, 1:]).max()))
    # the stereographic raster: 1 km elements around the patch
    X0, Y0, _ = TL.project(p, 32.0, -80.0)
    N = 400
    bx, by = float(X0) - 200.37e3, float(Y0) - 199.61e3
    Xs, Ys = bx + 1000.0 * (np.arange(N) + 0.5), by + 1000.0 * (np.arange(N) + 0.5)
    st = T.Source(field(Xs[None, :], Ys[:, None]).astype(np.float32), bx, 1000.0, by, 1000.0, name="stereo",
                  projection=T.PolarStereo("S", -71.0, 0.0))
    d2 = float(np.hypot(1000.0, 1000.0))
    r1, r2 = T.topography(x, y, ll, refine=16), T.topography(x, y, st, refine=16)
    assert not r1["records"]["n_missing"].any() and not r2["records"]["n_missing"].any()
    bound = G_max * (d1 + d2) / 2.0 + 0.01
    assert bound <= G_max * d1     # no more than the largest gradient times one (lat-lon) element's diagonal
    diff = float(np.abs(r1["height"] - r2["height"]).max())
    assert diff <= bound, (diff, bound)
    assert float(np.abs(r1["height"]).max()) > 0.5 * A     # the field is there


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def write_latlon(path, data, box):
    from ocean_model_grid_generator_amd import netcdf3
    ds = netcdf3.Dataset(path, [("lat", data.shape[0]), ("lon", data.shape[1])])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], box[2] + box[3] * (np.arange(data.shape[0]) + 0.5))
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], box[0] + box[1] * (np.arange(data.shape[1]) + 0.5))
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], data)
    ds.write()


def write_stereo(path, data, box):
    """a float variable ``bed`` on x / y in metres, y descending, with a CF polar_stereographic grid mapping (BedMachine's layout)"""
    from ocean_model_grid_generator_amd import netcdf3
    Ny, Nx = data.shape
    ds = netcdf3.Dataset(path, [("y", Ny), ("x", Nx)])
    ds.def_var("x", netcdf3.NC_DOUBLE, ("x",), [("units", "m")], box[0] + box[1] * (np.arange(Nx) + 0.5))
    ds.def_var("y", netcdf3.NC_DOUBLE, ("y",), [("units", "m")], (box[2] + box[3] * (np.arange(Ny) + 0.5))[::-1])
    ds.def_var("mapping", netcdf3.NC_INT, (), [("grid_mapping_name", "polar_stereographic"), ("standard_parallel", -71.0),
                                               ("straight_vertical_longitude_from_pole", 0.0), ("semi_major_axis", 6378137.0),
                                               ("inverse_flattening", 298.257223563), ("latitude_of_projection_origin", -90.0)], 0)
    ds.def_var("bed", netcdf3.NC_FLOAT, ("y", "x"), [("grid_mapping", "mapping"), ("_FillValue", np.float32(-9999.0))], data[::-1])
    ds.write()


def test_main_with_two_sources_equals_the_file_command(T, hip, tmp_path, capsys):
    """main(topog_source=[polar, global]) on the 1 degree tripolar grid writes topog.nc; the file command on the written
    ocean_hgrid.nc writes the same bytes; n_from_source is there and depth agrees with it.  One lat-lon source gives one and the same
    file through the old spelling (a string), the new one (a list of one) and the file command."""
    from ocean_model_grid_generator_amd import netcdf3, ocean_grid_generator as ogg
    g, gbox = TI.global_int16()
    bed = TI.smooth_values(200, 200, amplitude=900.0)
    bed[50:80, 20:90] = -9999.0
    A, B = str(tmp_path / "polar.nc"), str(tmp_path / "global.nc")
    write_stereo(A, bed, (-1.0e6 + 123.0, 10000.0, -1.0e6 - 321.0, 10000.0))     # 2000 km around the south pole, 10 km elements
    write_latlon(B, g, gbox)
    grid, t1, t2 = (str(tmp_path / n) for n in ("hgrid.nc", "t1.nc", "t2.nc"))
    kw = dict(no_changing_meta=True, ensure_nj_even=True)
    ogg.main(1.0, gridfilename=grid, topog_source=[A, B], topog_var=["bed", "elevation"], topog_file=t1, topog_refine=4, **kw)
    out = capsys.readouterr().out
    assert "valid samples by source: %s" % A in out
    res = T.main([grid, A, B, "--var", "bed", "--var", "elevation", "--refine", "4", "-o", t2])
    capsys.readouterr()
    assert open(t1, "rb").read() == open(t2, "rb").read()
    h = netcdf3.read_header(t1)
    assert "n_from_source" in h.vars and h.vars["n_from_source"].shape[0] == 2 and A in h.gatts["sources"] and "stere:S" in h.gatts["sources"]
    nf = res["n_from"]
    assert nf.shape[0] == 2 and nf[0].sum() > 0 and nf[1].sum() > 0
    np.testing.assert_array_equal(nf.sum(axis=0), res["n_samples"])
    assert not nf[0][res["n_samples"].shape[0] // 2:].any()          # nothing polar north of the equator
    only_polar = (nf[1] == 0) & (nf[0] > 0)
    assert only_polar.any()
    xy = netcdf3.read_doubles(grid, names=("x", "y"))     # with one R for all, a cell read from the polar raster alone is that raster's
    alone = T.topography(xy["x"], xy["y"], T.read_source(A, "bed"), refine=4)
    np.testing.assert_array_equal(res["depth"][only_polar], alone["depth"][only_polar])
    np.testing.assert_array_equal(nf[0], alone["n_samples"])
    # one lat-lon source: the single-source file whatever the spelling
    o1, o2, o3 = (str(tmp_path / n) for n in ("o1.nc", "o2.nc", "o3.nc"))
    ogg.main(1.0, gridfilename=None, topog_source=B, topog_file=o1, **kw)
    ogg.main(1.0, gridfilename=None, topog_source=[B], topog_var=["elevation"], topog_file=o2, **kw)
    T.main([grid, B, "-o", o3])
    capsys.readouterr()
    assert open(o1, "rb").read() == open(o2, "rb").read() == open(o3, "rb").read()
    assert "n_from_source" not in netcdf3.read_header(o1).vars and "sources" not in netcdf3.read_header(o1).gatts


def test_same_bits_for_any_rank_count(T, hip):
    """Supergrid.topography on r2_dp with a polar raster over a global one, for 1, 2 and 4 ranks (every rank uploads every layer, rank
    0 gathers the merge records): the same record bytes, n_from and summary, and those of the host form on the stitched grid."""
    import ocean_model_grid_generator_amd.supergrid as sg
    from test_gpu_topog import device_grid
    g, gbox = TI.global_int16()
    bed = TI.index_values(200, 200)
    bed[50:80, 20:90] = -1
    polar = T.Source(bed, -1.0e6 + 123.0, 10000.0, -1.0e6 - 321.0, 10000.0, fill=(-1,), projection=T.PolarStereo("S", -71.0, 0.0), name="polar")
    sl = T.SourceList([polar, T.Source(g, *gbox, name="global")])
    dev = T.DeviceSourceList(sl, "cuda:0")
    want = None
    for world in (1, 2, 4):
        plan, ranks = device_grid(sg, "r2_dp", world=world)
        res = ranks[0].topography(ranks[0].south_cut(), dev)
        for other in ranks[1:]:
            assert other.topography(other.south_cut(), dev) is None
        if want is None:
            want = res
            out = sg.stitch(plan, [ranks[0].bands_to_host()])
            host = T.topography(out["x"], out["y"], sl)
            assert host["records"].tobytes() == res["records"].tobytes() and host["summary"] == res["summary"]
            assert res["n_from"][0].sum() > 0 and res["n_from"][1].sum() > 0 and res["records"].dtype == hip.TOPOG_MERGE_RECORD
        else:
            assert res["records"].tobytes() == want["records"].tobytes(), world
            assert res["n_from"].tobytes() == want["n_from"].tobytes() and res["summary"] == want["summary"]
    with pytest.raises(ValueError, match="plane fit"):
        ranks[0].topography(ranks[0].south_cut(), dev, plane=True)

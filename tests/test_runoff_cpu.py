"""CPU tests of the runoff mapping: the numpy definition (tests/runoff_definition.py) on hand-worked grids (a coastal cell seen only
through the seam or the fold, an exact distance tie, missing and all-zero sources, conservation), the record-variable reader against
scipy, the writer read back through scipy with an unlimited time axis, the library's struct sizes and refusals, and main()'s refusals."""
import ctypes

import numpy as np
import pytest

import runoff_definition as D


def test_coast_seen_only_through_the_seam_and_the_fold():
    wet = np.ones((4, 6), np.uint8)
    wet[1, 5] = 0                     # land on the east edge of row 1: its seam partner (1, 0) is coastal
    wet[3, 1] = 0                     # land on the top row: its fold partner (3, 6 - 1 - 1) = (3, 4) is coastal
    t = D.targets(wet, periodic=True, fold=True)
    assert t[1, 0] and t[3, 4]
    assert not t[1, 1] and not t[2, 0] and not t[3, 3]
    # the same cells are inland when the partners are wet; the open boundaries are coast without the topology
    t2 = D.targets(np.ones((4, 6), np.uint8), periodic=True, fold=True)
    assert t2[0].all() and not t2[1:].any()   # only the south edge, which has no neighbour beyond it
    t3 = D.targets(np.ones((4, 6), np.uint8), periodic=False, fold=False)
    assert t3[:, 0].all() and t3[:, -1].all() and t3[0].all() and t3[-1].all() and not t3[1:-1, 1:-1].any()
    assert np.array_equal(D.targets(wet, True, True, mode="wet"), wet != 0)


def test_exact_tie_goes_to_the_smaller_cell():
    tu = D.unit([-10.0, 10.0, 0.0], [0.0, 0.0, 11.0])
    tcell = np.array([3, 7, 11])
    su = D.unit([0.0], [0.0])         # exactly midway in longitude between cells 3 and 7, on the equator
    d = D.d2(su, tu)[0]
    assert d[0] == d[1] and d[2] > d[0]   # a bit-exact tie (cos and sin of -10 and +10 degrees mirror each other)
    c, dd = D.nearest(su, tu, tcell)
    assert c[0] == 3 and dd[0] == d[0]
    c, _ = D.nearest(su, tu[[1, 0, 2]][np.argsort([7, 3, 11])], np.array([3, 7, 11]))
    assert c[0] == 3


def test_missing_and_all_zero_sources_contribute_nothing():
    f = np.zeros((2, 2, 3), np.float32)
    f[0, 0, 0] = 1.0                  # mapped
    f[:, 0, 1] = np.nan               # missing in every record
    f[0, 0, 2], f[1, 0, 2] = -999.0, 0.0   # missing once, zero once: skipped
    f[1, 1, 0] = -999.0
    f[0, 1, 0] = 2.0                  # mapped, missing in record 1
    mapped, skipped, missing = D.classify(f, (-999.0,))
    assert mapped.tolist() == [True, False, False, True, False, False]
    assert skipped.tolist() == [False, False, True, False, True, True]
    assert missing.tolist() == [False, True, False, False, False, False]
    As = np.arange(1.0, 7.0)
    Ac = np.array([[4.0, 8.0]])
    v, n = D.accumulate(f, (-999.0,), np.array([0, 3]), np.array([1, 1]), As, Ac)
    assert n.tolist() == [[0, 2]]
    assert v[0, 0, 0] == 0.0 and np.signbit(v[0, 0, 0]) == False   # noqa: E712
    assert v[0, 0, 1] == (0.0 + 1.0 * 1.0 + 2.0 * 4.0) / 8.0 and v[1, 0, 1] == 0.0


def test_conservation_on_a_small_global_grid():
    # a 4 x 8 model grid of 45 degree cells, a 2-degree source with runoff on a "continent" next to a strip of land
    ny, nx = 4, 8
    lon_pts = np.linspace(0.0, 360.0, 2 * nx + 1)
    lat_pts = np.linspace(-90.0, 90.0, 2 * ny + 1)
    X, Y = np.meshgrid(lon_pts, lat_pts)
    Re = 6371.0e3
    sa = (Re * Re) * (np.radians(np.diff(lon_pts))[None, :]) * np.diff(np.sin(np.radians(lat_pts)))[:, None]
    wet = np.ones((ny, nx), np.uint8)
    wet[1:3, 2:4] = 0
    t = D.targets(wet, True, False)
    tcell = np.nonzero(t.reshape(-1))[0]
    tu = D.unit(X[1::2, 1::2].reshape(-1)[tcell], Y[1::2, 1::2].reshape(-1)[tcell])
    lon, lat = np.linspace(0.0, 360.0, 181), np.linspace(-90.0, 90.0, 91)
    rng = np.random.default_rng(0)
    f = np.where(rng.random((3, 90, 180)) < 0.2, rng.random((3, 90, 180)), 0.0)
    f[1, :10] = np.nan
    mapped, _, _ = D.classify(f)
    src = np.nonzero(mapped)[0]
    J, I = np.divmod(src, 180)
    su = D.unit(0.5 * (lon[I] + lon[I + 1]), 0.5 * (lat[J] + lat[J + 1]))
    ds = D.ds_of(lat)
    v, n, s, tg, _ = D.runoff(f, (), lon, lat, ds, Re, su, tu, tcell, sa)
    assert n.sum() == len(src) and np.all(n.reshape(-1)[~t.reshape(-1)] == 0)
    As = D.source_area(lon, ds, Re).reshape(-1)
    Ac = D.cell_area(sa)
    for r in range(3):
        fr = f[r].reshape(-1)
        ok = ~np.isnan(fr)
        want = np.sum(fr[ok] * As[ok])
        got = np.sum(v[r] * Ac)
        assert abs(got / want - 1.0) < 1e-12


def write_runoff_source(path, nrec=3, with_other_record_var=True):
    """a 2-degree runoff source with an unlimited time axis, written with scipy"""
    from scipy.io import netcdf_file
    lo, la = np.arange(180) * 2.0 + 1.0, np.arange(90) * 2.0 - 89.0
    with netcdf_file(str(path), "w", version=2) as nc:
        nc.createDimension("time", None)
        nc.createDimension("lat", 90)
        nc.createDimension("lon", 180)
        t = nc.createVariable("time", "d", ("time",))
        t.units = "days since 1900-01-01"
        a = nc.createVariable("lat", "d", ("lat",))
        a.units = "degrees_north"
        a[:] = la
        b = nc.createVariable("lon", "d", ("lon",))
        b.units = "degrees_east"
        b[:] = lo
        v = nc.createVariable("friver", "f", ("time", "lat", "lon"))
        v.units = "kg m-2 s-1"
        v._FillValue = np.float32(1e20)
        if with_other_record_var:
            w = nc.createVariable("licalvf", "d", ("time", "lat", "lon"))
            w.units = "kg m-2 s-1"
        rng = np.random.default_rng(1)
        for r in range(nrec):
            t[r] = 15.0 + 30.0 * r
            v[r] = np.where(rng.random((90, 180)) < 0.1, rng.random((90, 180)), 0.0).astype(np.float32)
            if with_other_record_var:
                w[r] = np.where(rng.random((90, 180)) < 0.05, 1e-3 * r, 0.0)


@pytest.mark.parametrize("two", [True, False])
def test_record_variable_reader_matches_scipy(tmp_path, two):
    from scipy.io import netcdf_file
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    p = tmp_path / "jra.nc"
    write_runoff_source(p, with_other_record_var=two)
    with netcdf_file(str(p), "r", mmap=False) as nc:
        want = {k: np.array(nc.variables[k][:]) for k in nc.variables}
    for var in ("friver", "licalvf") if two else ("friver",):
        src = RO.read_source(str(p), var)
        assert src.record_dim == "time" and src.lead_dims == [("time", 3)]
        assert np.array_equal(src.data, want[var]) and src.data.dtype == want[var].dtype.newbyteorder("=")
        assert src.coords[0][0] == "time" and np.array_equal(src.coords[0][3], want["time"])
    with pytest.raises(ValueError, match="record"):
        R.read_source(str(p), "friver")


def test_writer_reads_back_through_scipy_with_time_unlimited(tmp_path):
    from scipy.io import netcdf_file
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    p = tmp_path / "jra.nc"
    write_runoff_source(p)
    srcs = [RO.read_source(str(p), v) for v in ("friver", "licalvf")]
    ny, nx = 5, 6
    rng = np.random.default_rng(2)
    area = rng.random((ny, nx)) + 1.0
    results = []
    for src in srcs:
        res = {"values": rng.random((3, ny, nx)), "n_sources": rng.integers(0, 9, (ny, nx)).astype(np.int32), "area": area}
        results.append((src, res))
    out = tmp_path / "runoff.nc"
    RO.write_runoff(str(out), results)
    with netcdf_file(str(out), "r", mmap=False) as nc:
        assert nc.dimensions["time"] is None and nc.variables["friver"].dimensions == ("time", "ny", "nx")
        for src, res in results:
            assert np.array_equal(nc.variables[src.name][:], res["values"])
            assert nc.variables[src.name].units == b"kg m-2 s-1"
        assert np.array_equal(nc.variables["time"][:], [15.0, 45.0, 75.0])
        assert np.array_equal(nc.variables["area"][:], area) and nc.variables["area"].units == b"m2"
        assert np.array_equal(nc.variables["n_sources"][:], results[0][1]["n_sources"])
    # a source without a record dimension writes a file without one; the fixed-size layout is unchanged
    fixed = R.Source(np.ones((2, 90, 180)), np.linspace(0, 360, 181), np.linspace(-90, 90, 91), name="f",
                     lead_dims=[("month", 2)])
    RO.write_runoff(str(tmp_path / "fixed.nc"), [(fixed, {"values": np.zeros((2, ny, nx)), "n_sources": np.zeros((ny, nx), np.int32),
                                                          "area": area})])
    with netcdf_file(str(tmp_path / "fixed.nc"), "r", mmap=False) as nc:
        assert nc.dimensions["month"] == 2 and nc.variables["f"].shape == (2, ny, nx)


def test_struct_sizes_and_refusals():
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["RUNOFF_PARAMS"]) == ctypes.sizeof(L.RunoffParams) == 80
    assert lib.ogg_abi_sizeof(L.ABI["RUNOFF_COUNTS"]) == ctypes.sizeof(L.RunoffCounts) == 64

    def p(**kw):
        q = L.RunoffParams(ny=10, nx=20, NA=36, NB=18, nrec=2, dtype=L.REMAP_FLOAT32, n_fill=1, topology=3, targets=L.RUNOFF_COAST,
                           Re=6371e3)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    assert lib.ogg_runoff_check(ctypes.byref(p())) == L.OGG_OK
    assert lib.ogg_runoff_workspace_bytes(ctypes.byref(p())) > 0
    for bad, text in ((dict(ny=0), b"cells"), (dict(NA=1 << 16, NB=1 << 16), b"source cells"), (dict(nrec=0), b"records"),
                      (dict(dtype=2), b"dtype"), (dict(n_fill=3), b"fill values"), (dict(topology=4), b"topology"),
                      (dict(targets=2), b"targets"), (dict(Re=0.0), b"radius"), (dict(Re=float("nan")), b"radius")):
        q = p(**bad)
        assert lib.ogg_runoff_check(ctypes.byref(q)) == L.OGG_EARG and text in lib.ogg_last_error(), bad
        assert lib.ogg_runoff_workspace_bytes(ctypes.byref(q)) == -1


def test_knobs_must_be_integers_in_range(monkeypatch):
    """the knobs are read when a call is set up, before any device work: a value that is no integer in range is refused, not read as 0
    or as its numeric prefix"""
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    p = L.RunoffParams(ny=10, nx=20, NA=36, NB=18, nrec=2, dtype=L.REMAP_FLOAT32, n_fill=1, topology=3, targets=L.RUNOFF_COAST, Re=6371e3)
    args = (ctypes.byref(p), 8, 8, 1, 8, 1, 8, 1 << 40, 8, 8, 8, None)   # never dereferenced
    for knob, val in (("OGG_RUNOFF_BINS", "abc"), ("OGG_RUNOFF_BINS", "4x"), ("OGG_RUNOFF_BRUTE", ""), ("OGG_RUNOFF_BRUTE", "2"),
                      ("OGG_RUNOFF_BINS", "-1")):
        monkeypatch.setenv(knob, val)
        assert lib.ogg_runoff_search_dev(*args) == L.OGG_EARG, (knob, val)
        assert (knob + "=" + val).encode() in lib.ogg_last_error() and b"an integer" in lib.ogg_last_error()
        monkeypatch.delenv(knob)


def test_python_arguments_are_checked():
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    src = R.Source(np.ones((1, 18, 36), np.float32), np.linspace(0, 360, 37), np.linspace(-90, 90, 19))
    with pytest.raises(ValueError, match="targets"):
        RO.params(4, 8, src, targets="ocean")
    with pytest.raises(ValueError, match="wet mask"):
        RO._wet(None, (4, 8))
    with pytest.raises(ValueError, match="wet mask is"):
        RO._wet(np.ones((3, 8)), (4, 8))


def test_main_refuses_runoff_without_variables_or_topography():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    with pytest.raises(ValueError, match="--runoff_var"):
        ogg.main(1.0, gridfilename=None, runoff_source="r.nc", topog_source="t.nc")
    with pytest.raises(ValueError, match="--topog_source"):
        ogg.main(1.0, gridfilename=None, runoff_source="r.nc", runoff_var=["friver"])
    with pytest.raises(ValueError, match="--topog_source"):
        ogg.main(1.0, gridfilename=None, runoff_source="r.nc", runoff_var=["friver"], path="functions")
    a = ogg.build_parser().parse_args(["--inverse_resolution", "1", "--runoff_source", "r.nc", "--runoff_var", "friver", "--runoff_var",
                                       "licalvf", "--runoff_targets", "wet"])
    assert a.runoff_var == ["friver", "licalvf"] and a.runoff_targets == "wet" and a.runoff_file == "runoff.nc"

"""CPU tests of face topography (include/ogg_hip.h, "Face topography"): that the numpy definition of tests/topog_faces_definition.py
and the fixtures of tests/topog_faces_cases.py mean what they say (planted ridges tell u from v and a sill from a mean, closed forms
in Python integers, seam, fold, edges and the pole), that the mirrors of the records agree, and what the API refuses, writes and parses
before any device work.  The device is held to the same truths by tests/test_gpu_topog_faces.py."""
import ctypes
import os

import numpy as np
import pytest

import small_grids as G
import small_meshes as sm
import topog_faces_cases as C
import topog_faces_definition as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def FT():
    from ocean_model_grid_generator_amd import face_topography
    return face_topography


# ---- the definition and the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.PLANTED_KINDS)
def test_planted_ridge_tells_u_from_v_and_a_sill_from_a_mean(kind):
    x, y = C.planted_grid()
    rec = fd.records(x, y, C.planted(kind), *C.BOX, refine=C.PLANTED_R)
    C.assert_planted(kind, rec)
    # the cell mean knows nothing of it: the model cells on either side of the closed faces are deep
    import topog_definition as td
    mean = td.records(x, y, C.planted(kind), *C.BOX, refine=C.PLANTED_R)
    assert np.all(mean["sum"] / mean["n"] < -800.0)
    fam, row, col = ("v", 1, 1) if kind.startswith("row") else ("u", 1, 1)
    r = rec[fam][row, col]
    assert r["lo"] == C.RIDGE and r["q_min"] == C.FLOOR and r["n_dry_lines"] == r["n_lines"]


@pytest.mark.parametrize("kind", ["index_js", "index_is"])
@pytest.mark.parametrize("R", [2, 8, 32])
def test_closed_forms_in_python_integers(kind, R):
    x, y = C.closed_grid()
    r = G.raster(kind)
    C.assert_closed_forms(kind, R, fd.records(x, y, r["data"], *r["box"], refine=R))


@pytest.mark.parametrize("cut", list(sm.CUTS))
def test_seam_fold_and_edges_of_the_tripolar_cuts(cut):
    from ocean_model_grid_generator_amd import ocean_mask as M
    g = sm.topology_cuts()[cut]
    periodic, fold = g["topology"]
    assert M.detect_topology(g["x"], g["y"]) == (periodic, fold)
    r = G.raster("int16")
    rec = C.edge_records(g["x"], g["y"], r["data"], r["box"], M.topology_flags(periodic, fold), 2)
    ny, nx = g["x"].shape[0] - 1, g["x"].shape[1] - 1
    C.assert_edges(lambda fam, row, col: rec[fam, row, col], ny, nx, periodic, fold)


def test_pole_block_and_pole_corners():
    r = G.raster("int16")
    x, y = G.pole_block()
    rec = fd.records(x, y, r["data"], *r["box"], refine=4)
    pole = {("u", 0, 0): True, ("u", 0, 1): False, ("v", 0, 0): True, ("v", 1, 0): False}     # cell (0, 0) alone encloses the pole
    for (fam, row, col), is_pole in pole.items():
        f = rec[fam][row, col]
        assert bool(f["flags"] & fd.F_POLE) == is_pole, (fam, row, col)
        if is_pole:
            assert (f["n"], f["n_missing"], f["n_lines"], f["n_lines_missing"], f["n_dry_lines"], f["ridge_sum"]) == (0,) * 6
            assert (f["lo"], f["hi"], f["q_min"], f["R"]) == (fd.INT_MAX, fd.INT_MIN, fd.INT_MAX, 4)
        else:
            assert f["n_lines"] == 8 and f["n"] == 2 * 16
    # cells with pole corners are sampled like any other: the top point row of this grid lies at 90N
    x, y = G.grid(2, 2, lon0=30.0, lat0=88.0, d=1.0)
    assert np.all(y[-1] == 90.0)
    rec = fd.records(x, y, r["data"], *r["box"], refine=4)
    for fam in ("u", "v"):
        assert not np.any(rec[fam]["flags"] & fd.F_POLE) and np.all(rec[fam]["n_lines"] == 8)


def test_blocks_with_different_refinements_take_the_largest():
    """a sheared grid whose cells get different R by the spans: a block's cells are all sampled at its largest"""
    import topog_definition as td
    x, y = C.mixed_grid()
    r = G.raster("int16")
    c = td.cells(x, y, r["box"][1], r["box"][3])
    assert len(np.unique(c["R"])) > 1
    rec = fd.records(x, y, r["data"], *r["box"])
    mixed = 0
    for col in range(4):
        cells, _ = fd.block("u", 0, col, 4, 6, 0)
        Rs = {int(c["R"][j, i]) for _, j, i, _ in cells}
        mixed += len(Rs) > 1
        f = rec["u"][0, col]
        assert f["R"] == max(Rs) and f["n"] + f["n_missing"] == len(cells) * max(Rs) ** 2
    assert mixed


def test_shifted_and_mirrored_grids_give_the_same_records():
    """on the 1/8 degree lattice with a power-of-two R every position is exact: a grid stated 360 degrees away gives the same bytes,
    and a grid mirrored in the meridian 0 over the raster mirrored with it gives the records in mirrored order"""
    r = G.raster("int16")
    x, y = G.grid(4, 4, lon0=-2.0, lat0=-4.0)
    a = fd.records(x, y, r["data"], *r["box"], refine=4)
    b = fd.records(x + 360.0, y, r["data"], *r["box"], refine=4)
    m = fd.records(np.ascontiguousarray(-x[:, ::-1]), y, np.ascontiguousarray(r["data"][:, ::-1]), *r["box"], refine=4)
    for fam in ("u", "v"):
        assert a[fam].tobytes() == b[fam].tobytes()
        assert a[fam].tobytes() == np.ascontiguousarray(m[fam][:, ::-1]).tobytes()


# ---- mirrors -----------------------------------------------------------------------------------------------------------------------
def test_mirror_records(FT):
    from ocean_model_grid_generator_amd import _lib as L
    assert L.TOPOG_FACE_RECORD == fd.RECORD and fd.RECORD.itemsize == 56
    lib = L.load()
    # the record is OGG_TOPOG_FACE_WORDS int64 words at the header's byte offsets, not a struct of the header: no new ABI code
    header = open(os.path.join(ROOT, "include", "ogg_hip.h")).read()
    assert "#define OGG_TOPOG_FACE_WORDS %d\n" % L.TOPOG_FACE_WORDS in header and 8 * L.TOPOG_FACE_WORDS == fd.RECORD.itemsize
    offsets = {"n": 0, "n_missing": 8, "ridge_sum": 16, "n_lines": 24, "n_lines_missing": 28, "n_dry_lines": 32, "lo": 36, "hi": 40,
               "q_min": 44, "R": 48, "n_clamped": 52, "flags": 54}
    assert {f: fd.RECORD.fields[f][1] for f in fd.FIELDS} == offsets
    assert "52 n_clamped, 54 flags" in header and not any("FACE" in k for k in L.ABI)
    assert lib.ogg_abi_sizeof(len(L.ABI)) == -1
    assert (L.FACE_ONE_SIDED, L.FACE_POLE, L.FACE_SEAM, L.FACE_FOLD) == (fd.F_ONE_SIDED, fd.F_POLE, fd.F_SEAM, fd.F_FOLD)
    assert (L.MASK_PERIODIC, L.MASK_FOLD) == (fd.PERIODIC, fd.FOLD)
    assert FT.FILL == 1.0e20


# ---- API behaviour -----------------------------------------------------------------------------------------------------------------
def test_argument_refusals(FT):
    from ocean_model_grid_generator_amd import _lib as L, topography as T
    FT.params(2, 2, 0)
    FT.params(4, 6, (True, True), refine=256, u_rows=(1, 2), v_rows=(3, 3))
    for kw, text in ((dict(ny=3, nx=2), "2 x 2 supergrid cells"), (dict(ny=2, nx=5), "2 x 2 supergrid cells"), (dict(ny=0, nx=2), "supergrid cells"),
                     (dict(ny=4, nx=4, u_rows=(1, 3)), "u-face rows"), (dict(ny=4, nx=4, u_rows=(2, 1)), "u-face rows"),
                     (dict(ny=4, nx=4, v_rows=(0, 4)), "v-face rows"), (dict(ny=4, nx=4, v_rows=(-1, 2)), "v-face rows"),
                     (dict(ny=2, nx=2, topology=4), "topology"), (dict(ny=2, nx=2, refine=257), "refine"),
                     (dict(ny=2, nx=2, refine=0), "refine"), (dict(ny=2, nx=2, oversample=0.0), "oversample"),
                     (dict(ny=2, nx=2, ld=2), "row stride")):
        kw.setdefault("topology", 0)
        with pytest.raises(ValueError, match=text):
            FT.params(**kw)
    # the library's own check: refine outside 0 .. 256, and a float source on the device entry
    lib = L.load()
    p = FT.FaceParams(2, 2, 3, 0, -1, 2.0, (0, 1), (0, 2))
    src = T.Source(np.zeros((4, 8), dtype=np.float32), -180.0, 45.0, -90.0, 45.0).descriptor()
    assert lib.ogg_topog_faces_check(*p.args(), ctypes.byref(src), 0) == L.OGG_EARG and b"refine" in lib.ogg_last_error()
    p.grid.refine = 0
    assert lib.ogg_topog_faces_check(*p.args(), ctypes.byref(src), 0) == L.OGG_OK
    assert lib.ogg_topog_faces_check(*p.args(), ctypes.byref(src), 1) == L.OGG_EARG and b"dtype" in lib.ogg_last_error()
    assert lib.ogg_topog_faces_dev(*p.args(), ctypes.byref(src), None, 0, None, None, None) == L.OGG_EARG     # before any device work
    p.grid.j0 = 2     # the grid is the whole stitched grid, not a band of it
    assert lib.ogg_topog_faces_check(*p.args(), ctypes.byref(src), 0) == L.OGG_EARG and b"whole stitched grid" in lib.ogg_last_error()
    # a list of sources and a projected source
    s = T.Source(np.zeros((4, 8), dtype=np.int16), -180.0, 45.0, -90.0, 45.0)
    x, y = G.grid(2, 2)
    with pytest.raises(ValueError, match="not made from a list"):
        FT.face_topography(x, y, [s, s])
    with pytest.raises(ValueError, match="not made from a list"):
        FT.face_topography(x, y, T.Source(np.zeros((4, 4), dtype=np.int16), -1e5, 5e4, -1e5, 5e4, projection=T.PolarStereo.parse("stere:N,lat_ts=70,lon0=0")))
    with pytest.raises(ValueError, match="2-D of one shape"):
        FT.face_topography(x, y[:-1], s)


def test_file_layout(FT, tmp_path):
    from ocean_model_grid_generator_amd import netcdf3, topography as T
    x, y = C.planted_grid()
    src = T.Source(C.planted("row_gap"), *C.BOX, name="planted")
    rec = fd.records(x, y, src.data, *C.BOX, refine=C.PLANTED_R, sea_level=-10.0)
    res = FT.result(rec["u"], rec["v"], src, -10.0, C.PLANTED_R, 2.0, 0)
    assert res["u"]["depth_max"][0, 1] == 1000.0 and res["u"]["depth_min"][0, 1] == -50.0
    assert res["v"]["depth_max"][1, 1] == -50.0 and res["v"]["open_fraction"][1, 1] == 0.0 and res["v"]["open_fraction"][1, 0] == 2.0 / 16.0
    assert res["v"]["depth_ave"][1, 0] == -((14 * 50 - 2 * 1000) / 16.0)
    path = str(tmp_path / "faces.nc")
    FT.write_topog_faces(path, res)
    h = netcdf3.read_header(path)
    assert dict(h.dims) == {"ny": 2, "nx": 2, "nyq": 3, "nxq": 3}
    want = {"u": ("ny", "nxq"), "v": ("nyq", "nx")}
    names = []
    for fam, dims in want.items():
        for name, key in (("depth%s_max", "depth_max"), ("depth%s_min", "depth_min"), ("depth%s_ave", "depth_ave"),
                          ("open_fraction_%s", "open_fraction")):
            v = h.vars[name % fam]
            assert v.dims == dims and v.nc_type == netcdf3.NC_DOUBLE
            got = np.frombuffer(netcdf3.read_var_bytes(path, h, name % fam), dtype=">f8").reshape(v.shape)
            assert np.array_equal(got, res[fam][key]), name % fam
            names.append(name % fam)
        for name, key, t in (("n_lines_%s", "n_lines", netcdf3.NC_INT), ("flag_%s", "flag", netcdf3.NC_BYTE)):
            v = h.vars[name % fam]
            assert v.dims == dims and v.nc_type == t
            got = np.frombuffer(netcdf3.read_var_bytes(path, h, name % fam, t), dtype=netcdf3.NUMPY_DTYPE[t]).reshape(v.shape)
            assert np.array_equal(got, res[fam][key]), name % fam
            names.append(name % fam)
        assert "sill" in h.vars["depth%s_max" % fam].atts["long_name"].lower()
    assert sorted(h.vars) == sorted(names)
    assert float(h.gatts["sea_level"][0]) == -10.0 and int(h.gatts["refine"][0]) == C.PLANTED_R and int(h.gatts["topology"][0]) == 0
    assert "planted" in h.gatts["source"] and float(h.gatts["oversample"][0]) == 2.0
    # a face without a line is filled
    rec["u"]["n_lines"][0, 0] = 0
    assert FT.fields_from_records(rec["u"], 1.0)["depth_max"][0, 0] == FT.FILL
    assert any("closed" in line for line in FT.summary_lines(res))


def test_flags_are_refused_before_any_work(FT, tmp_path):
    import ocean_model_grid_generator_amd.ocean_grid_generator as ogg
    from ocean_model_grid_generator_amd import topography as T
    check = lambda **f: ogg._validate_all((), 0.0, -99.0, True, ogg.AnalysisFlags(**f))   # noqa: E731
    assert ogg.AnalysisFlags().topog_faces_file is None
    a = ogg.build_parser().parse_args(["-r", "1", "--topog_faces_file", "f.nc"]) if hasattr(ogg, "build_parser") else None
    assert a is None or a.topog_faces_file == "f.nc"
    s = T.Source(np.zeros((4, 8), dtype=np.int16), -180.0, 45.0, -90.0, 45.0)
    check(topog_faces_file="f.nc", topog_source=s)
    with pytest.raises(ValueError, match="--topog_faces_file needs --topog_source"):
        check(topog_faces_file="f.nc")
    with pytest.raises(ValueError, match="--topog_faces_file: .*not made from a list"):
        check(topog_faces_file="f.nc", topog_source=[s, s])
    with pytest.raises(ValueError, match="--topog_faces_file: .*projected source"):
        check(topog_faces_file="f.nc", topog_source="no_such_file.nc", topog_proj="stere:S,lat_ts=-71,lon0=0")
    # the file command: no file is read before the refusal
    with pytest.raises(SystemExit):
        T.main(["grid.nc", "--faces", "f.nc"])
    with pytest.raises(ValueError, match="--faces: .*not made from a list"):
        T.main(["no_grid.nc", "a.nc", "b.nc", "--faces", "f.nc"])
    with pytest.raises(ValueError, match="--faces: .*projected source"):
        T.main(["no_grid.nc", "a.nc", "--source_proj", "stere:S,lat_ts=-71,lon0=0", "--faces", "f.nc"])

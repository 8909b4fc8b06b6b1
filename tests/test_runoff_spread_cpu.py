"""CPU tests of the runoff spreading: the numpy definition (tests/runoff_spread_definition.py) on hand cases with known answers, its
latitude-window pruning against the unpruned loop, conservation within the bound that its roundings give, classes that keep two
basins apart, the refusals of the flags of main() and of the file command, and the ABI mirrors of the two new structs.  No device
call is made here."""
import ctypes
import math

import numpy as np
import pytest

import runoff_spread_definition as D
import small_meshes as sm


def mesh(ny, nx, seed=0, **kw):
    """a small lat-lon mesh as the definition takes it: u, A, candidates, a wet set with holes"""
    g = sm.latlon_grid(ny, nx, **kw)
    lon, lat = D.centres(g["x"], g["y"])
    A = D.cell_area(g["area"])
    rng = np.random.default_rng(seed)
    wet = (rng.random(ny * nx) < 0.8).astype(np.uint8)
    return D.unit(lon, lat), A, wet, D.candidates(A, wet, lon, lat), rng


def field(rng, cand, nrec, prob):
    load = (cand & (rng.random(cand.size) < prob)).astype(np.int32)
    v = np.where(load > 0, rng.random((nrec, cand.size)) * 1e-4, 0.0)
    return v, load


MESHES = [dict(ny=1, nx=1), dict(ny=1, nx=2), dict(ny=3, nx=3), dict(ny=129, nx=1, dlat=1.0, lat0=-64.5),
          dict(ny=2, nx=1, dlon=360.0, dlat=10.0), dict(ny=3, nx=2, dlon=180.0, dlat=10.0), dict(ny=5, nx=7, lat0=50.0, fold=True),
          dict(ny=16, nx=32, lon0=0.0, lat0=-88.0, dlon=11.25, dlat=11.0), dict(ny=40, nx=80, lon0=0.0, lat0=-88.0, dlon=4.5, dlat=4.4)]


@pytest.mark.parametrize("kw", MESHES, ids=lambda k: "%dx%d" % (k["ny"], k["nx"]))
def test_pruned_and_unpruned_definitions_give_the_same_bytes(kw):
    u, A, wet, cand, rng = mesh(seed=kw["ny"], **kw)
    v, load = field(rng, cand, 2, 0.3)
    cls = (np.arange(cand.size) % 3).astype(np.int32)
    for km in (50.0, 300.0, 1000.0, 2500.0, 25000.0):
        for shape in (D.UNIFORM, D.BIWEIGHT):
            for c in (None, cls):
                a = D.spread(v, A, u, cand, load, D.radius2(km), shape, c, prune=False)
                b = D.spread(v, A, u, cand, load, D.radius2(km), shape, c, prune=True)
                for k in ("out", "n_mouths", "mouth_cell", "mouth_n", "mouth_W"):
                    assert a[k].tobytes() == b[k].tobytes(), (km, shape, k)
                assert a["counts"] == b["counts"]


def test_one_mouth_on_a_1x1_grid():
    u, A = np.array([[1.0, 0.0, 0.0]]), np.array([3.0e9])
    v = np.array([[0.1], [-0.0], [np.nan]])
    r = D.spread(v, A, u, np.array([True]), np.array([1]), 0.01, D.BIWEIGHT)
    assert r["mouth_W"].tolist() == [1 << 24] and r["mouth_n"].tolist() == [1] and r["n_mouths"].tolist() == [1]
    assert r["out"][0, 0] == (0.1 * 3.0e9) / 3.0e9 and np.isnan(r["out"][2, 0])
    assert r["out"][1, 0] == 0.0 and not np.signbit(r["out"][1, 0])   # +0.0 + (-0.0 * 1.0) is +0.0
    assert r["counts"] == dict(candidates=1, mouths=1, pairs=1, max_receivers=1, loaded=1, max_mouths=1)


def test_two_equal_cells_share_a_uniform_spread_in_halves():
    u = D.unit(np.array([0.0, 1.0]), np.array([0.0, 0.0]))
    A = np.array([2.0e9, 2.0e9])
    r = D.spread(np.array([[0.3, 0.0]]), A, u, np.array([True, True]), np.array([1, 0]), D.radius2(300.0), D.UNIFORM)
    assert r["mouth_W"].tolist() == [1 << 25] and r["mouth_n"].tolist() == [2]
    half = ((0.3 * 2.0e9) * 0.5) / 2.0e9
    assert r["out"].tolist() == [[half, half]] and r["n_mouths"].tolist() == [1, 1]


def test_a_receiver_on_the_rim_counts_with_weight_zero():
    u = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])     # d2 = 2 exactly
    A = np.array([1.0e9, 1.0e9])
    r = D.spread(np.array([[0.5, 7.0]]), A, u, np.array([True, True]), np.array([1, 0]), 2.0, D.BIWEIGHT)
    assert r["mouth_n"].tolist() == [2] and r["mouth_W"].tolist() == [1 << 24] and r["n_mouths"].tolist() == [1, 1]
    assert r["out"][0, 0] == (0.5 * 1.0e9) / 1.0e9 and r["out"][0, 1] == 0.0 and not np.signbit(r["out"][0, 1])
    inside = D.spread(np.array([[0.5, 7.0]]), A, u, np.array([True, True]), np.array([1, 0]), np.nextafter(2.0, 0.0), D.BIWEIGHT)
    assert inside["mouth_n"].tolist() == [1] and inside["n_mouths"].tolist() == [1, 0]


def test_the_area_ratio_is_capped_at_256():
    u = D.unit(np.array([0.0, 0.5]), np.array([0.0, 0.0]))
    A = np.array([1.0e6, 1.0e9])
    r = D.spread(np.array([[1.0, 0.0]]), A, u, np.array([True, True]), np.array([1, 0]), D.radius2(300.0), D.UNIFORM)
    assert r["mouth_W"].tolist() == [257 << 24]
    F = 1.0 * 1.0e6
    assert r["out"].tolist() == [[(F * (1.0 / 257.0)) / 1.0e6, (F * (256.0 / 257.0)) / 1.0e9]]


def test_a_mouth_that_is_no_candidate_is_refused():
    u, A, wet, cand, rng = mesh(3, 3, seed=1)
    cand[:] = True
    cand[4] = cand[7] = False
    load = np.zeros(9, np.int32)
    load[[2, 4, 7]] = 1
    with pytest.raises(ValueError, match="mouth cell 4 "):
        D.spread(np.zeros((1, 9)), A, u, cand, load, 0.1, D.BIWEIGHT)


@pytest.mark.parametrize("km", [300.0, 1000.0, 2500.0])
@pytest.mark.parametrize("shape", [D.UNIFORM, D.BIWEIGHT])
def test_conservation_within_the_bound_of_its_roundings(km, shape):
    """|fsum(out A) - fsum(v A)| <= (max_mouths + 8) 2^-52 fsum(|v| A): each s is rounded once; each product, the division by A_t and
    the multiplication back add one rounding each; a left-to-right sum of k terms adds (k - 1) / 2 ulp."""
    u, A, wet, cand, rng = mesh(40, 80, seed=0, lon0=0.0, lat0=-88.0, dlon=4.5, dlat=4.4)
    A = A * (1.0 + 0.3 * rng.random(A.size))
    v, load = field(rng, cand, 3, 0.2)
    v[1] = -v[1]
    r = D.spread(v, A, u, cand, load, D.radius2(km), shape, prune=True)
    for rec, (defect, total) in enumerate(D.conservation(r["out"], v, A, r["mouth_cell"])):
        print("R = %g km, shape %d, record %d: defect %.3g of 2^-52 sum |v| A; max_mouths %d"
              % (km, shape, rec, defect / (2.0 ** -52 * total), r["counts"]["max_mouths"]))
        assert defect <= (r["counts"]["max_mouths"] + 8) * 2.0 ** -52 * total
    assert r["counts"]["max_mouths"] > 1 and (r["mouth_W"] > 0).all()


def test_classes_keep_two_basins_apart_across_a_one_cell_isthmus():
    ny, nx = 5, 9
    g = sm.latlon_grid(ny, nx, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    lon, lat = D.centres(g["x"], g["y"])
    A, u = D.cell_area(g["area"]), D.unit(lon, lat)
    wet = np.ones((ny, nx), np.uint8)
    wet[:, 4] = 0                                    # the isthmus
    cls = np.where(np.arange(nx) < 4, 1, 2)[None, :].repeat(ny, 0).reshape(-1).astype(np.int32)
    cand = D.candidates(A, wet, lon, lat)
    load = np.zeros((ny, nx), np.int32)
    load[2, 3] = load[1, 5] = 1
    v = np.zeros((1, ny * nx))
    v[0, 2 * nx + 3], v[0, 1 * nx + 5] = 1.0, 2.0
    free = D.spread(v, A, u, cand, load, D.radius2(300.0), D.BIWEIGHT)
    kept = D.spread(v, A, u, cand, load, D.radius2(300.0), D.BIWEIGHT, cls)
    west = (np.arange(ny * nx) % nx) < 4
    assert free["n_mouths"].max() == 2 and kept["n_mouths"].max() == 1
    m = kept["mouth_cell"]
    for k in range(2):   # each basin holds its own mouth's flux and nothing else
        side = west if m[k] % nx < 4 else ~west
        one = D.spread(np.where(np.arange(ny * nx) == m[k], v, 0.0), A, u, cand, (np.arange(ny * nx) == m[k]).astype(np.int32),
                       D.radius2(300.0), D.BIWEIGHT, cls)
        assert not one["out"][0][~side].any() and kept["out"][0][side].tobytes() == one["out"][0][side].tobytes()
    assert kept["counts"]["pairs"] < free["counts"]["pairs"]


# ---- the package's host side ---------------------------------------------------------------------------------------
def test_radius_and_parameters():
    from ocean_model_grid_generator_amd import runoff as RO
    assert RO.radius2(300.0, D.RE) == D.radius2(300.0) and RO.radius2(1e9) == 4.0
    s = math.sin(0.5 * (300.0 * 1e3 / D.RE))
    assert RO.radius2(300.0, D.RE) == (2 * s) * (2 * s)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="radius"):
            RO.radius2(bad)
    with pytest.raises(ValueError, match="shape"):
        RO.spread_params(3, 3, 1, 0.1, shape="gauss")
    for r2 in (0.0, -1.0, 4.0000001, float("nan")):
        with pytest.raises(ValueError, match="r2"):
            RO.spread_params(3, 3, 1, r2)
    with pytest.raises(ValueError, match="nrec"):
        RO.spread_params(3, 3, 0, 0.1)
    assert RO.spread_params(3, 3, 2, 4.0, "uniform", True).use_classes == 1


def test_the_workspace_grows_with_the_pairs_and_the_limit_names_P(monkeypatch):
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import runoff as RO
    lib = L.load()
    p = RO.spread_params(16, 32, 1, 0.1)
    w0, w1 = lib.ogg_spread_workspace_bytes(ctypes.byref(p), 0), lib.ogg_spread_workspace_bytes(ctypes.byref(p), 1000)
    assert 0 < w0 < w1 and w1 - w0 >= 16000
    assert lib.ogg_spread_workspace_bytes(ctypes.byref(p), L.SPREAD_MAX_PAIRS) == -1
    assert b"P = %d" % L.SPREAD_MAX_PAIRS in lib.ogg_last_error()
    monkeypatch.setenv("OGG_SPREAD_MAX_PAIRS_TEST", "1000")
    assert lib.ogg_spread_workspace_bytes(ctypes.byref(p), 999) > 0 and lib.ogg_spread_workspace_bytes(ctypes.byref(p), 1000) == -1
    assert b"P = 1000" in lib.ogg_last_error()
    monkeypatch.setenv("OGG_SPREAD_MAX_PAIRS_TEST", str(1 << 31))   # the knob can only lower the limit
    assert lib.ogg_spread_workspace_bytes(ctypes.byref(p), 999) == -1 and b"OGG_SPREAD_MAX_PAIRS_TEST" in lib.ogg_last_error()


def test_default_load():
    from ocean_model_grid_generator_amd import runoff as RO
    v = np.zeros((2, 2, 3))
    v[0, 0, 1], v[1, 1, 2], v[0, 1, 0], v[1, 0, 0] = 1.0, -2.0, np.nan, -0.0
    assert RO.default_load(v).tolist() == [[0, 1, 0], [0, 0, 1]]


def test_main_refuses_bad_spread_flags_before_any_device_work():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    run = dict(runoff_source="r.nc", runoff_var=["friver"], topog_source="t.nc")
    for path in ("pass", "functions"):
        with pytest.raises(ValueError, match="--runoff_spread_km needs --runoff_source"):
            ogg.main(1.0, gridfilename=None, runoff_spread_km=300.0, path=path)
        for km in (0.0, -5.0, float("nan")):
            with pytest.raises(ValueError, match="--runoff_spread_km must be a positive"):
                ogg.main(1.0, gridfilename=None, runoff_spread_km=km, path=path, **run)
        with pytest.raises(ValueError, match="--runoff_spread_shape must be"):
            ogg.main(1.0, gridfilename=None, runoff_spread_km=300.0, runoff_spread_shape="gauss", path=path, **run)
        with pytest.raises(ValueError, match="--runoff_spread_by_basin needs --runoff_spread_km"):
            ogg.main(1.0, gridfilename=None, runoff_spread_by_basin=True, path=path, **run)
        with pytest.raises(ValueError, match="--runoff_spread_by_basin needs --basin_codes_file and --basin_rules"):
            ogg.main(1.0, gridfilename=None, runoff_spread_km=300.0, runoff_spread_by_basin=True, path=path, **run)
        with pytest.raises(ValueError, match="--runoff_spread_by_basin needs --basin_codes_file and --basin_rules"):
            ogg.main(1.0, gridfilename=None, runoff_spread_km=300.0, runoff_spread_by_basin=True, basin_codes_file="b.nc", path=path, **run)
    a = ogg.build_parser().parse_args(["-r", "1", "--runoff_spread_km", "250", "--runoff_spread_shape", "uniform", "--runoff_spread_by_basin"])
    assert (a.runoff_spread_km, a.runoff_spread_shape, a.runoff_spread_by_basin) == (250.0, "uniform", True)
    d = ogg.build_parser().parse_args(["-r", "1"])
    assert (d.runoff_spread_km, d.runoff_spread_shape, d.runoff_spread_by_basin) == (None, "biweight", False)


def test_the_file_command_refuses_bad_spread_flags_before_it_reads_a_file():
    from ocean_model_grid_generator_amd import runoff as RO
    base = ["nogrid.nc", "nosource.nc", "--var", "friver", "--mask", "nomask.nc"]
    with pytest.raises(ValueError, match="need --spread_km"):
        RO.main(base + ["--spread_shape", "uniform"])
    with pytest.raises(ValueError, match="need --spread_km"):
        RO.main(base + ["--spread_classes", "b.nc"])
    for km in ("0", "-3", "nan"):
        with pytest.raises(ValueError, match="--spread_km must be a positive"):
            RO.main(base + ["--spread_km", km])
    with pytest.raises(ValueError, match="--spread_classes takes a file and at most one variable"):
        RO.main(base + ["--spread_km", "300", "--spread_classes", "b.nc", "basin", "extra"])
    with pytest.raises(SystemExit):
        RO.main(base + ["--spread_km", "300", "--spread_shape", "gauss"])


def test_abi_mirrors_of_the_spread_structs():
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    assert L.ABI["SPREAD_PARAMS"] == 40 and L.ABI["SPREAD_COUNTS"] == 41 and len(L.ABI) == 42
    assert lib.ogg_abi_sizeof(40) == ctypes.sizeof(L.SpreadParams) == 40
    assert lib.ogg_abi_sizeof(41) == ctypes.sizeof(L.SpreadCounts) == 8 * len(L.SPREAD_COUNT_FIELDS) == 64
    assert lib.ogg_abi_sizeof(42) == -1
    assert [f for f, _ in L.SpreadParams._fields_] == ["ny", "nx", "nrec", "shape", "use_classes", "r2"]
    for name in ("ogg_spread_check", "ogg_spread_sets_dev", "ogg_spread_count_dev", "ogg_spread_pairs_dev", "ogg_spread_apply_dev",
                 "ogg_runoff_spread"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert "ogg_spread_workspace_bytes" in L.LONG_GETTERS

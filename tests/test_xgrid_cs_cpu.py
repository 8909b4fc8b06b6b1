"""CPU tests of the cubed-sphere exchange grid: ogg_xgrid_cs_check_atm (host only), the definition of tests/xgrid_cs_definition.py
(conservation, the 50-digit truth, the zoo's branches), cubed_sphere_from_corners, the six-file writer and main()'s refusals.  No
device work."""
import os

import numpy as np
import pytest

import xgrid_cs_definition as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "tests", "golden", "xgrid_cs_truth.npz")


@pytest.fixture(scope="module")
def XC():
    from ocean_model_grid_generator_amd import exchange_grid_cs
    return exchange_grid_cs


def check(XC, t, frames):
    from ocean_model_grid_generator_amd import _lib as L
    t = np.ascontiguousarray(t, dtype=np.float64)
    desc = XC.atm_desc({"N": t.size - 1, "frames": frames}, t.ctypes.data)
    return L.load().ogg_xgrid_cs_check_atm(desc)


def test_check_atm_accepts_both_spacings_and_a_turned_cube(XC):
    for N in (1, 2, 3, 5, 48):
        for sp in XC.SPACINGS:
            atm = XC.cubed_sphere_atm(N, sp)
            t = atm["t"]
            assert t[0] == -1.0 and t[-1] == 1.0 and np.all(np.diff(t) > 0) and atm["N"] == N
            assert N % 2 or t[N // 2] == 0.0
            # symmetric up to the rounding of tan's argument (an ulp of pi / 4, times a slope of at most 2) and of tan itself, each side
            np.testing.assert_allclose(t, -t[::-1], rtol=0, atol=8e-16)
    assert check(XC, XC.table(48), XC.default_frames(-10.0)) == 0
    XC.cubed_sphere_atm(48, "edge_equidistant", lon_shift=-10.0)
    # the two spacings differ, and the edge-equidistant one has equal arcs along a face's edge (xi = t, eta = +-1)
    assert np.max(np.abs(XC.table(5) - XC.table(5, "edge_equidistant"))) > 1e-3
    arcs = np.diff(np.arctan(XC.table(5, "edge_equidistant") / np.sqrt(2.0)))
    np.testing.assert_allclose(arcs, arcs[0], rtol=1e-14)
    np.testing.assert_allclose(np.diff(np.arctan(XC.table(5))), np.pi / 10, rtol=1e-14)


def test_check_atm_refusals(XC):
    from ocean_model_grid_generator_amd import _lib as L
    fr = XC.default_frames()
    ok = XC.table(4)
    assert check(XC, ok, fr) == 0
    bad_tables = [np.array([-1.0, 0.0, 0.5]), np.array([-0.5, 0.0, 1.0]), np.array([-1.0, 0.3, 0.2, 1.0]), np.array([-1.0, 0.2, 0.2, 1.0]),
                  np.array([-1.0, np.nan, 1.0])]
    for t in bad_tables:
        assert check(XC, t, fr) == L.OGG_EARG, t
    left = fr.copy()
    left[2, 0] = -left[2, 0]           # e_u reversed: e_u x e_v = -e_n
    skew = fr.copy()
    skew[1, 0] = skew[1, 0] + 1e-6 * skew[1, 1]
    equal = fr.copy()
    equal[3] = equal[1]                # two equal normals (and no face at 270 E)
    long_ = fr.copy()
    long_[4] = long_[4] * (1 + 1e-9)
    turned = fr.copy()                 # a frame turned about its own normal: orthonormal, but e_u is no face's normal
    c, s = np.cos(0.3), np.sin(0.3)
    turned[0, 0], turned[0, 1] = c * fr[0, 0] + s * fr[0, 1], -s * fr[0, 0] + c * fr[0, 1]
    for bad in (left, skew, equal, long_, turned):
        assert check(XC, ok, bad) == L.OGG_EARG
        with pytest.raises(ValueError):
            XC.cubed_sphere_atm(4, frames=bad)
    assert b"cubed-sphere" in L.load().ogg_last_error()
    # N = 0 and N = 4097
    desc = XC.atm_desc({"N": 0, "frames": fr}, ok.ctypes.data)
    assert L.load().ogg_xgrid_cs_check_atm(desc) == L.OGG_EARG
    big = np.linspace(-1.0, 1.0, 4098)
    assert check(XC, big, fr) == L.OGG_EARG
    assert check(XC, np.linspace(-1.0, 1.0, 4097), fr) == 0
    for N in (0, 4097):
        with pytest.raises(ValueError):
            XC.cubed_sphere_atm(N)
    with pytest.raises(ValueError):
        XC.cubed_sphere_atm(4, "equidistant")
    # a cube in any rotation is accepted
    a, b = 0.4, -1.1
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    assert check(XC, ok, fr @ (Rz @ Rx).T) == 0


def test_atmosphere_areas_cover_the_sphere(XC):
    for N in (1, 2, 3, 5, 12, 48):
        for sp in XC.SPACINGS:
            t = XC.table(N, sp)
            a = XC.atm_area(t, 1.0)
            assert abs(6.0 * a.sum() / (4.0 * np.pi) - 1.0) <= 1e-14
            if N <= 5:   # the vectorised form and the definition's statements agree
                np.testing.assert_allclose(a, cd.a_atm_table(t, 1.0), rtol=4e-16)


def conservation(XC, x, y, atm):
    lst, a_poly, counts, _ = cd.exchange_grid_cs(x, y, atm["t"], atm["frames"], Re=1.0, threshold=0.0)
    A = cd.a_poly_array(a_poly)
    fij, ocn, area = cd.as_arrays(lst)
    ny, nx = A.shape
    per = np.bincount(ocn[:, 1] * nx + ocn[:, 0], weights=area, minlength=ny * nx).reshape(ny, nx)
    frac, _ = XC.ocean_frac(fij, area, atm["t"], 1.0)
    return counts, float(np.max(np.abs(per / A - 1))), frac, float(area.sum())


@pytest.mark.parametrize("lon0", [0.0, -283.7])
def test_definition_conserves_on_the_coarse_global_mesh(XC, lon0):
    """24 x 12 cells of 15 degrees with pole corners: per cell and per atmosphere cell within 1e-14, globally within 1e-13"""
    x, y = cd.regional(lon0, -90.0, 15.0, 15.0, 24, 12)
    for N in (1, 2, 3, 5, 12):
        for sp in XC.SPACINGS:
            counts, e_ocn, frac, total = conservation(XC, x, y, XC.cubed_sphere_atm(N, sp))
            assert counts["degenerate"] == counts["wide"] == counts["inverted"] == 0
            assert e_ocn <= 1e-14, (N, sp, e_ocn)
            assert np.max(np.abs(frac - 1)) <= 1e-14, (N, sp)
            assert abs(total / (4 * np.pi) - 1) <= 1e-13


@pytest.mark.parametrize("centre", [(45.0, 35.2643896828), (0.0, 0.0), (44.0, 89.0)])
def test_definition_conserves_on_fine_patches(XC, centre):
    """12 x 12 patches of 1/4 and 1/8 degree cells across a cube corner, at a face centre and at the pole: per cell within 1.5e-13"""
    for d in (0.25, 0.125):
        x, y = cd.regional(centre[0] - 6 * d, centre[1] - 6 * d, d, d, 12, 12)
        y = np.minimum(y, 90.0)   # (the polar patch stops at the pole: its last rows are triangles and collapsed cells)
        for N in (96, 384):
            atm = XC.cubed_sphere_atm(N, "equiangular" if N == 96 else "edge_equidistant")
            lst, a_poly, counts, status = cd.exchange_grid_cs(x, y, atm["t"], atm["frames"], Re=1.0, threshold=0.0)
            A = cd.a_poly_array(a_poly)
            _, ocn, area = cd.as_arrays(lst)
            per = np.bincount(ocn[:, 1] * 12 + ocn[:, 0], weights=area, minlength=144).reshape(12, 12)
            ok = A > 0
            assert ok.sum() >= 100 and counts["wide"] == counts["degenerate"] == 0
            assert np.max(np.abs(per[ok] / A[ok] - 1)) <= 1.5e-13, (centre, d, N)


@pytest.fixture(scope="module")
def zoo_definition(XC):
    """the definition on every case of the truth file: {case: (list, A_poly, counts, statuses)}"""
    t = np.load(TRUTH)
    zoo = cd.zoo()
    out = {}
    for case in t["cases"].tolist():
        name, c = case.split("/")
        N, sp = int(c[1:-1]), {"e": "equiangular", "d": "edge_equidistant"}[c[-1]]
        x, y, _ = zoo[name]
        out[case] = cd.exchange_grid_cs(x, y, XC.table(N, sp), XC.default_frames(), Re=6371.0e3)
    return t, out


def test_definition_stays_within_its_recorded_error_of_the_truth(zoo_definition):
    t, runs = zoo_definition
    e_poly = e_piece = 0.0
    n = 0
    for k, case in enumerate(t["cases"].tolist()):
        lst, a_poly, _, _ = runs[case]
        ap = t["a_poly"][t["cell_off"][k]:t["cell_off"][k + 1]]
        ref = cd.a_poly_array(a_poly).reshape(-1)
        np.testing.assert_array_equal(np.isnan(ref), np.isnan(ap[:, 0]))
        pos = ap[:, 0] > 0
        if pos.any():
            e_poly = max(e_poly, float(np.max(np.abs((ref[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0])))
        nx = len(a_poly[0])
        got = {e[:5]: e[5] for e in lst}
        sl = slice(t["piece_off"][k], t["piece_off"][k + 1])
        for p, (hi, lo) in zip(t["pieces"][sl].tolist(), t["area"][sl].tolist()):
            if tuple(p) in got:
                e_piece = max(e_piece, abs((got[tuple(p)] - hi) - lo) / ap[p[4] * nx + p[3], 0])
                n += 1
    assert n >= 0.99 * t["pieces"].shape[0] > 2000
    # the same statements on the same libm give the same figures; another libm may differ by a rounding or two
    assert e_poly <= 1.5 * float(t["eref_poly"]) and e_piece <= 1.5 * float(t["eref_piece"])
    assert float(t["eref_poly"]) < 1e-13 and float(t["eref_piece"]) < 1e-13


def test_every_zoo_input_reaches_its_branch(zoo_definition):
    t, runs = zoo_definition
    zoo = cd.zoo()
    assert set(c.split("/")[0] for c in runs) == set(zoo)
    for case, (lst, a_poly, counts, status) in runs.items():
        name, c = case.split("/")
        N = int(c[1:-1])
        expect = zoo[name][2]
        assert set(status.values()) == {expect}, case
        if expect == "ok":
            assert counts["kept"] > 0 and counts["face_candidates"] >= counts["cells"], case
        else:
            assert counts["kept"] == 0 and counts[expect] == counts["cells"] == 1, case
            assert (a_poly[0][0] is None) == (expect != "inverted"), case
        faces = sorted(set(e[2] for e in lst))
        if name == "cube_corner":
            assert faces == [0, 1, 4] and counts["face_candidates"] == 3, case
        if name == "edge_on_xi_0" and N % 2 == 0:   # the west edge lies on a grid line: the column west of it has no candidate
            assert min(e[0] for e in lst) == N // 2 and counts["candidates"] == len(set((e[0], e[1]) for e in lst)), case
        if name == "edge_on_face_boundary":         # xi = 1 of face 0 within a rounding: candidates on faces 0 and 1, pieces on face 1
            assert counts["face_candidates"] == 2 and 1 in faces, case
        if name.startswith("pole_") or name == "south_pole_two":
            assert faces == [5 if name == "south_pole_two" else 4], case
        if case == "big_25/C96e":
            assert counts["candidates"] > 300 and counts["kept"] > 300
        if name == "bow_tie":   # the lobes cancel in part: A_poly is a third of what the pieces of the larger lobe sum to
            assert counts["kept"] >= 1
    assert cd.zoo()["regional_1x129"][0].shape == (3, 259)


def test_from_corners_round_trips_and_refuses_a_displaced_tile(XC):
    for atm in (XC.cubed_sphere_atm(5), XC.cubed_sphere_atm(6, "edge_equidistant"), XC.cubed_sphere_atm(4, lon_shift=-10.0),
                XC.cubed_sphere_atm(1)):
        lon, lat = XC.cubed_sphere_corners(atm)
        assert lon.shape == (6, atm["N"] + 1, atm["N"] + 1)
        back = XC.cubed_sphere_from_corners(lon, lat)
        np.testing.assert_allclose(back["t"], atm["t"], rtol=0, atol=1e-14)
        np.testing.assert_allclose(back["frames"], atm["frames"], rtol=0, atol=1e-14)
        assert back["t"][0] == -1.0 and back["t"][-1] == 1.0
        # the tiles in another order and with i and j swapped are another, equally valid cube: the frames follow the input
        perm = XC.cubed_sphere_from_corners(lon[[1, 0, 3, 2, 5, 4]], lat[[1, 0, 3, 2, 5, 4]])
        np.testing.assert_allclose(perm["frames"], atm["frames"][[1, 0, 3, 2, 5, 4]], rtol=0, atol=1e-14)
        with pytest.raises(ValueError):   # i and j swapped on every tile: left-handed frames
            XC.cubed_sphere_from_corners(lon.transpose(0, 2, 1), lat.transpose(0, 2, 1))
    lon, lat = XC.cubed_sphere_corners(XC.cubed_sphere_atm(6))
    moved = lat.copy()
    moved[2, 3, 2] += 1e-6 * 180.0 / np.pi
    with pytest.raises(ValueError, match="tile 3"):
        XC.cubed_sphere_from_corners(lon, moved)
    with pytest.raises(ValueError):
        XC.cubed_sphere_from_corners(lon[:5], lat[:5])
    # a conformal (non-gnomonic) spacing on one axis only is no cube of this kind
    other = XC.cubed_sphere_atm(6, "edge_equidistant")
    lon2, lat2 = XC.cubed_sphere_corners(other)
    mixed_lon, mixed_lat = lon.copy(), lat.copy()
    mixed_lon[4], mixed_lat[4] = lon2[4], lat2[4]
    with pytest.raises(ValueError):
        XC.cubed_sphere_from_corners(mixed_lon, mixed_lat)


def fake_result(XC, atm, fij, ocn, area, shape):
    counts = {f: 0 for f in cd.COUNT_FIELDS}
    counts["kept"] = len(area)
    return XC.result(np.asarray(fij, np.int32).reshape(-1, 3), np.asarray(ocn, np.int32).reshape(-1, 2), np.asarray(area, np.float64),
                     np.ones(shape), counts, atm, 1.0, 0.0)


def read_xgrid(path):
    from ocean_model_grid_generator_amd import netcdf3
    h = netcdf3.read_header(path)
    assert [d[0] for d in h.dims] == ["ncells", "two"] and set(h.vars) == {"tile1_cell", "tile2_cell", "xgrid_area"}
    n = h.dims[0][1]
    if n == 0:   # (the classic format has no fixed dimension of length 0: ncells reads as the record dimension with no record)
        return np.zeros((0, 2), ">i4"), np.zeros((0, 2), ">i4"), np.zeros(0, ">f8")
    return (np.frombuffer(netcdf3.read_var_bytes(path, h, "tile1_cell", dtype=netcdf3.NC_INT), dtype=">i4").reshape(n, 2),
            np.frombuffer(netcdf3.read_var_bytes(path, h, "tile2_cell", dtype=netcdf3.NC_INT), dtype=">i4").reshape(n, 2),
            np.frombuffer(netcdf3.read_var_bytes(path, h, "xgrid_area"), dtype=">f8"))


def test_six_file_writer_partitions_stably_and_writes_empty_tiles(XC, tmp_path):
    atm = XC.cubed_sphere_atm(3)
    rng = np.random.default_rng(3)
    n = 40
    fij = np.stack([rng.integers(0, 3, n), rng.integers(0, 3, n), rng.choice([0, 1, 4], n)], axis=1)   # tiles 3, 4 and 6 stay empty
    ocn = np.stack([rng.integers(0, 7, n), np.sort(rng.integers(0, 5, n))], axis=1)
    area = rng.random(n)
    res = fake_result(XC, atm, fij, ocn, area, (5, 7))
    assert res["ocean_frac"].shape == res["land_frac"].shape == res["a_atm"].shape == (6, 3, 3)
    np.testing.assert_array_equal(res["land_frac"], 1.0 - res["ocean_frac"])
    k = (fij[:, 2] * 3 + fij[:, 1]) * 3 + fij[:, 0]
    np.testing.assert_array_equal(res["ocean_frac"].reshape(-1) * res["a_atm"].reshape(-1), np.bincount(k, weights=area, minlength=54))
    paths = XC.write_xgrid_cs(str(tmp_path / "atmos_mosaic_tile%dXocean_mosaic_tile1.nc"), res)
    assert [os.path.basename(p) for p in paths] == ["atmos_mosaic_tile%dXocean_mosaic_tile1.nc" % k for k in range(1, 7)]
    for f, p in enumerate(paths):
        t1, t2, a = read_xgrid(p)
        sel = fij[:, 2] == f
        assert (a.size == 0) == (f in (2, 3, 5))
        np.testing.assert_array_equal(t1, fij[sel][:, :2] + 1)     # (I + 1, J + 1), in list order
        np.testing.assert_array_equal(t2, ocn[sel] + 1)
        assert a.astype("<f8").tobytes() == area[sel].tobytes()
    XC.write_frac_cs(str(tmp_path / "frac.nc"), res)
    from ocean_model_grid_generator_amd import netcdf3
    got = netcdf3.read_doubles(str(tmp_path / "frac.nc"), names=("ocean_frac", "land_frac", "area", "t", "frames"))
    np.testing.assert_array_equal(got["ocean_frac"], res["ocean_frac"])
    np.testing.assert_array_equal(got["frames"].reshape(6, 3, 3), atm["frames"])
    for bad in ("no_tile_number.nc", "two_%d_%d.nc"):
        with pytest.raises(ValueError):
            XC.write_xgrid_cs(str(tmp_path / bad), res)


def test_main_flags_and_refusals():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    a = ogg.AnalysisFlags()
    assert a.xgrid_cs is None and a.xgrid_cs_spacing == "equiangular" and a.xgrid_cs_lon_shift == 0.0
    assert a.xgrid_cs_file == "atmos_mosaic_tile%dXocean_mosaic_tile1.nc" and a.xgrid_cs_frac_file is None
    ns = ogg.build_parser().parse_args(["-r", "1", "--xgrid_cs", "48", "--xgrid_cs_spacing", "edge_equidistant", "--xgrid_cs_lon_shift",
                                        "-10", "--xgrid_cs_frac_file", "f.nc"])
    assert (ns.xgrid_cs, ns.xgrid_cs_spacing, ns.xgrid_cs_lon_shift, ns.xgrid_cs_frac_file) == (48, "edge_equidistant", -10.0, "f.nc")

    def validate(**flags):
        ogg._validate_all((), 0.0, -99.0, flags.pop("skip_metrics", False), ogg.AnalysisFlags(**flags))

    validate(xgrid_cs=48, skip_metrics=True)
    validate(xgrid_cs=48, xgrid_atm=(180, 90), xgrid_file="other.nc")
    validate(xgrid_cs=48, xgrid_atm=(180, 90), xgrid_cs_file="cs_tile%d.nc")
    with pytest.raises(ValueError, match="--xgrid_file"):   # the default names: tile 1's file is --xgrid_file
        validate(xgrid_cs=48, xgrid_atm=(180, 90))
    with pytest.raises(ValueError, match="--xgrid_cs_frac_file needs --xgrid_cs"):
        validate(xgrid_cs_frac_file="f.nc")
    with pytest.raises(ValueError, match="%d"):
        validate(xgrid_cs=48, xgrid_cs_file="one_name.nc")
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="--xgrid_cs must be"):
            validate(xgrid_cs=bad)
    with pytest.raises(ValueError, match="--xgrid_cs_spacing"):
        validate(xgrid_cs=4, xgrid_cs_spacing="conformal")

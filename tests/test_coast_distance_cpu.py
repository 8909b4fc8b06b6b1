"""CPU tests of the distance to the coast: the definition (tests/coast_distance_definition.py) held to truths that do not come from
it (a closed form, symmetry, the neighbour rules, ties), the hand-made inputs of tests/coast_inputs.py checked to reach the branches
they are named for, the host side of coast_distance.py on the definition's output, and the flag validation of main().  No device
compute is done here."""
import ctypes

import numpy as np
import pytest

import coast_distance_definition as D
import coast_inputs as CI
import small_meshes as SM

RE = SM.RE


def test_one_land_cell_gives_the_haversine_distance():
    g = SM.latlon_grid(9, 13)
    wet = np.ones((9, 13), np.uint8)
    wet[4, 6] = 0
    fl, n, d2, _ = D.define(g["x"], g["y"], wet, False, False)
    lon, lat = D.centres(g["x"], g["y"])
    c = 4 * 13 + 6
    assert np.all(n[wet != 0] == c)
    from ocean_model_grid_generator_amd import coast_distance as CD
    dist = CD.distance_of(d2, n, RE)
    want = D.haversine(lon, lat, lon[4, 6], lat[4, 6], RE)
    q = wet != 0
    assert np.max(np.abs(dist[q] - want[q]) / want[q]) <= 1e-9
    # the land cell's answer is one of its four wet face neighbours (the nearest: a neighbour along the closer spacing)
    assert n[4, 6] in (c - 13, c + 13, c - 1, c + 1) and dist[4, 6] == dist.min()
    assert set(D.sets(fl)[0]) == {c} and set(D.sets(fl)[1]) == {c - 13, c + 13, c - 1, c + 1}


def test_land_column_on_a_periodic_band_is_nearest_in_the_querys_own_row():
    """Two rows at latitudes -+5 on a band round the globe.  A point at latitude phi is nearer to (psi = phi, dlon) than to
    (psi = -phi, dlon) for every dlon, since cos d = sin phi sin psi + cos phi cos psi cos dlon differs between the two by the sign
    of the first term alone; so the nearest cell of a land column is the one in the query's own row.  (With more rows this is false
    on a sphere: the foot of the perpendicular on a meridian lies poleward of the query, at 90 degrees of longitude and more at the
    band's edge.)"""
    g = SM.latlon_grid(2, 36, lon0=0.0, lat0=-10.0, dlon=10.0, dlat=10.0)
    wet = np.ones((2, 36), np.uint8)
    wet[:, 20] = 0
    _, n, d2, _ = D.define(g["x"], g["y"], wet, True, False, sides="wet")
    j = np.arange(2)[:, None] * np.ones((1, 36), int)
    q = wet != 0
    assert np.all(n[q] // 36 == j[q]) and np.all(n[q] % 36 == 20)
    # symmetric about the land column, across the seam too
    for k in range(1, 18):
        assert np.allclose(d2[:, (20 + k) % 36], d2[:, (20 - k) % 36], rtol=1e-12)


def test_neighbour_rules():
    w = np.ones((3, 6), np.uint8)
    w[1, 0] = 0
    assert not D.coastal(w, False, False)[1, 5] and D.coastal(w, True, False)[1, 5]      # the seam neighbour: only with periodic
    w = np.ones((3, 6), np.uint8)
    w[2, 1] = 0
    assert not D.coastal(w, False, False)[2, 4] and D.coastal(w, False, True)[2, 4]      # the fold partner: only with fold
    assert not D.coastal(w, False, True)[1, 4]                                           # and only on the top row
    ny, nx, _ = SM.SHAPES["fold_5x7"]
    for mid in (0, 1):   # the middle cell of an odd-width fold is its own partner: not thereby coastal
        w = np.full((ny, nx), 1 - mid, np.uint8)
        w[ny - 1, nx // 2] = mid
        w[ny - 2, nx // 2] = w[ny - 1, nx // 2 - 1] = w[ny - 1, nx // 2 + 1] = mid
        c = D.coastal(w, False, True)
        assert not c[ny - 1, nx // 2] and c[ny - 1, nx // 2 - 1]
    # the grid's edge is no coast (unlike the runoff mapping's coastal targets)
    import runoff_definition as RD
    w = np.ones((4, 5), np.uint8)
    assert not D.coastal(w, False, False).any() and RD.targets(w, False, False).sum() == 14
    w[:] = 0
    assert not D.coastal(w, False, False).any()


def test_empty_opposite_sets_give_no_answer():
    g = SM.latlon_grid(4, 5)
    for v in (0, 1):
        fl, n, d2, _ = D.define(g["x"], g["y"], np.full((4, 5), v, np.uint8), False, False)
        assert np.all(n == -1) and np.all(np.isposinf(d2)) and not (fl & D.F_COAST).any()


def test_exact_tie_goes_to_the_smaller_cell():
    c = CI.exact_tie()
    fl, n, d2, u = D.define(c["x"], c["y"], c["wet"], c["periodic"], c["fold"])
    assert u[6].tobytes() == u[8].tobytes()                       # the branch: two targets at one point
    q = c["wet"].reshape(-1) != 0
    assert D.d2(u[q], u[[6]]).tobytes() == D.d2(u[q], u[[8]]).tobytes()
    assert np.all(n[c["wet"] != 0] == 6)
    assert n[1, 1] in (1, 5, 7, 11) and n[1, 3] in (3, 7, 9, 13)   # a land cell is never its own answer


def test_pole_near_ties():
    c = CI.pole_near_ties()
    fl, n, d2, u = D.define(c["x"], c["y"], c["wet"], c["periodic"], c["fold"])
    top = u[16:24]
    assert len({t.tobytes() for t in top}) > 1 and np.max(np.abs(top - top[0])) < 1e-15   # the branch: distinct within an ulp of 1
    L, W = D.sets(fl)
    assert list(L) == list(range(16, 24)) and list(W) == list(range(8, 16))
    # each answer really is the key's minimum, found here one target at a time
    for qc in range(16):
        dd = D.d2(u[[qc]], top)[0]
        k = min(range(8), key=lambda t: (dd[t], t))
        assert n.flat[qc] == 16 + k and d2.flat[qc] == dd[k]


def test_an_invalid_centre_is_neither_query_nor_target_but_still_a_neighbour():
    c = CI.invalid_centres()
    fl, n, d2, _ = D.define(c["x"], c["y"], c["wet"], c["periodic"], c["fold"])
    assert not fl[1, 2] & D.F_VALID and not fl[2, 4] & D.F_VALID and fl[1, 2] & D.F_COAST     # the branch
    L, W = D.sets(fl)
    assert list(L) == [18] and 8 not in L                                   # the invalid land cell is no target
    assert {2, 7, 9, 14} <= set(W)                                          # yet its wet neighbours are coastal through its wet byte
    assert n[1, 2] == -1 and n[2, 4] == -1 and np.isposinf(d2[1, 2]) and np.isposinf(d2[2, 4])
    ok = (fl & D.F_VALID) != 0
    assert np.all(n[ok & (c["wet"] != 0)] == 18) and np.all(n[ok] != 8) and np.all(n[ok] != 16)


def test_sides_select_the_queries():
    c = CI.seam_band()
    _, both, d_both, _ = D.define(c["x"], c["y"], c["wet"], True, False)
    _, wet, d_wet, _ = D.define(c["x"], c["y"], c["wet"], True, False, sides="wet")
    _, land, d_land, _ = D.define(c["x"], c["y"], c["wet"], True, False, sides="land")
    w = c["wet"] != 0
    assert np.array_equal(wet[w], both[w]) and np.all(wet[~w] == -1) and np.all(np.isposinf(d_wet[~w]))
    assert np.array_equal(land[~w], both[~w]) and np.all(land[w] == -1) and np.all(np.isposinf(d_land[w]))
    assert np.all(both >= 0)
    # the coast across the seam: the first column's answer is the land column, two cells away through the seam
    assert np.all(both[:, 0] % 36 == 34) and np.all(both[:, 0] // 36 == np.arange(8))


def test_named_inputs_reach_their_branches():
    c = CI.random_centres()
    fl, n, d2, u = D.define(c["x"], c["y"], c["wet"], False, False)
    for bit in (0, 1):   # every tile's ball covers more than a hemisphere, and pass 2's bound U + 2 r >= 2 r reaches every target
        targets = u[D.sets(fl)[1 - bit]]
        for _, _, r, m in CI.tile_balls(u, fl, bit):
            assert r * r > 1.0 + m @ m and np.sqrt(((targets - m) ** 2).sum(axis=1).max()) <= 2.0 * r
    c = CI.antipodal()
    fl, n, d2, u = D.define(c["x"], c["y"], c["wet"], False, False)
    assert list(D.sets(fl)[0]) == [0] and n[0, 1] == 0 and 4.0 - d2[0, 1] < 1e-15
    c = CI.seam_band()
    fl, n, d2, u = D.define(c["x"], c["y"], c["wet"], True, False)
    (_, _, r0, _), = [b for b in CI.tile_balls(u, fl, 1) if b[:2] == (0, 0)]
    assert r0 > 0.5 and d2[0, 0] < 0.2            # the first tile's coast is nearer than its own far corner, and lies across the seam
    for k in (31, 32, 33):
        c = CI.coast_of(k)
        assert len(D.sets(D.flags(c["x"], c["y"], c["wet"], False, False))[0]) == k


def test_result_and_file_on_the_definitions_output(tmp_path):
    """the host side of coast_distance.py: metres from d2, the fill, the cell indices, the summary's farthest wet cell, the file"""
    from scipy.io import netcdf_file
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import coast_distance as CD
    c = CI.invalid_centres()
    fl, n, d2, _ = D.define(c["x"], c["y"], c["wet"], False, False)
    counts = dict.fromkeys(L.COAST_COUNT_FIELDS, 0)
    counts.update(queries=22, answered=22, tests=44)
    res = CD.result(n, d2, fl, counts, c["x"], c["y"], "both", False, False, RE)
    assert np.all(res["distance"][n < 0] == 1e20) and np.all(res["nearest_j"][n < 0] == -1) and np.all(res["nearest_i"][n < 0] == -1)
    ok = n >= 0
    assert np.array_equal(res["nearest_j"][ok] * 6 + res["nearest_i"][ok], n[ok])
    assert res["distance"][ok].tobytes() == (RE * (2 * np.arcsin(np.minimum(1, 0.5 * np.sqrt(d2[ok]))))).tobytes()
    f = res["summary"]["farthest"]
    sel = ok & (c["wet"] != 0)
    assert f["km"] * 1000.0 == pytest.approx(res["distance"][sel].max()) and d2[f["j"], f["i"]] == d2[sel].max()
    assert res["summary"]["tests_per_query"] == 2.0 and len(CD.summary_lines(res)) == 2
    path = str(tmp_path / "cd.nc")
    CD.write_coast_distance(path, res)
    with netcdf_file(path, "r", mmap=False) as nc:
        assert nc.variables["distance"]._FillValue == 1e20 and nc.variables["distance"].shape == (4, 6)
        assert np.array_equal(nc.variables["distance"][:], res["distance"]) and np.array_equal(nc.variables["nearest_i"][:], res["nearest_i"])
        assert np.array_equal(nc.variables["wet"][:], c["wet"]) and np.array_equal(nc.variables["coast"][:], res["coast"])


def test_abi_refuses_bad_parameters_and_knobs(monkeypatch):
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import coast_distance as CD
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["COAST_PARAMS"]) == ctypes.sizeof(L.CoastParams)
    assert lib.ogg_abi_sizeof(L.ABI["COAST_COUNTS"]) == ctypes.sizeof(L.CoastCounts)
    with pytest.raises(ValueError, match="sides"):
        CD.params(4, 8, sides="ocean")
    for bad in (dict(ny=0, nx=4, topology=0, sides=3), dict(ny=1 << 16, nx=1 << 15, topology=0, sides=3), dict(ny=4, nx=4, topology=4, sides=3),
                dict(ny=4, nx=4, topology=0, sides=0), dict(ny=4, nx=4, topology=0, sides=4)):
        p = L.CoastParams(**bad)
        assert lib.ogg_coast_check(ctypes.byref(p)) == L.OGG_EARG and lib.ogg_last_error().startswith(b"coast distance:")
        assert lib.ogg_coast_workspace_bytes(ctypes.byref(p)) == -1
    p = CD.params(10, 20, "both", True, True)
    assert lib.ogg_coast_workspace_bytes(ctypes.byref(p)) > 0
    with pytest.raises(ValueError, match="wet mask"):
        CD._wet(None, (4, 8))
    args = (ctypes.byref(p), 8, 8, 8, 8, 1, 8, 8, 1, 8, 1 << 40, 8, 8, 8, None)   # never dereferenced
    for knob, val in (("OGG_COAST_BRUTE", "2"), ("OGG_COAST_CUBES", "129"), ("OGG_COAST_CUBES", "4x"), ("OGG_COAST_TILE_X", "0"),
                      ("OGG_COAST_TILE_Y", "257"), ("OGG_COAST_CHUNK", "513"), ("OGG_COAST_CHUNK", "")):
        monkeypatch.setenv(knob, val)
        assert lib.ogg_coast_search_dev(*args) == L.OGG_EARG, (knob, val)
        assert (knob + "=" + val).encode() in lib.ogg_last_error() and b"an integer" in lib.ogg_last_error()
        monkeypatch.delenv(knob)
    monkeypatch.setenv("OGG_COAST_TILE_X", "32")
    monkeypatch.setenv("OGG_COAST_TILE_Y", "16")
    assert lib.ogg_coast_search_dev(*args) == L.OGG_EARG and b"at most 256 cells in a tile" in lib.ogg_last_error()


def test_main_refuses_bad_coast_distance_flags():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    for path in (None, "functions"):
        with pytest.raises(ValueError, match="--coast_distance_file needs --topog_source"):
            ogg.main(1.0, gridfilename=None, coast_distance_file="cd.nc", path=path)
        with pytest.raises(ValueError, match="--coast_distance_sides must be"):
            ogg.main(1.0, gridfilename=None, coast_distance_file="cd.nc", topog_source="t.nc", coast_distance_sides="coast", path=path)
        with pytest.raises(ValueError, match="--coast_distance_sides needs --coast_distance_file"):
            ogg.main(1.0, gridfilename=None, coast_distance_sides="wet", path=path)
    # the metrics are not needed: --skip_metrics passes the validation (and the missing raster is then what stops the run)
    ogg._validate_all((), 0.0, -99.0, True, ogg.AnalysisFlags(coast_distance_file="cd.nc", topog_source="t.nc"))
    a = ogg.build_parser().parse_args(["-r", "1", "--topog_source", "t.nc", "--coast_distance_file", "cd.nc", "--coast_distance_sides", "land"])
    assert a.coast_distance_file == "cd.nc" and a.coast_distance_sides == "land"
    b = ogg.build_parser().parse_args(["-r", "1"])
    assert b.coast_distance_file is None and b.coast_distance_sides == "both"
    assert ogg.AnalysisFlags().coast_distance_file is None and ogg.AnalysisFlags().coast_distance_sides == "both"

"""GPU tests of the basin codes (csrc/ogg_basin.hip, basin_codes.py, Supergrid.basin_codes): code, rule and the rule records bit for
bit against the sequential floods of tests/basin_definition.py run on the device's own unit vectors: regular grids around the 64 x 32
tile, a serpentine channel through every tile, diagonal contact, longitudes stated a turn away, invalid centres, every status, the
rule limits, random masks under random overlapping rules, the knobs, a rule over the whole sphere against the ocean mask's component
of its seed cell, the seed cell against the ocean mask's seed lookup, and main(), the function-level path, the file command and
Supergrid.basin_codes writing the same bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import basin_definition as D
import small_meshes as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE = sm.RE
FULL = (-180.0, 180.0, -90.0, 90.0)


@pytest.fixture(scope="module")
def BC(hip):
    from ocean_model_grid_generator_amd import basin_codes as m
    return m


def to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def device_units(lon, lat):
    """the device's unit vectors of the points (lon, lat), through the coast step's sets launch: the centres of a row of cells"""
    from ocean_model_grid_generator_amd import coast_distance as CD
    lon, lat = np.asarray(lon, np.float64).reshape(-1), np.asarray(lat, np.float64).reshape(-1)
    x, y = np.zeros((3, 2 * lon.size + 1)), np.zeros((3, 2 * lon.size + 1))
    x[1, 1::2], y[1, 1::2] = lon, lat
    return CD.coast_distance_dev(to(x), to(y), np.ones((1, lon.size), np.uint8), periodic=False, fold=False, keep_lists=True)["u"]


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("code", "rule", "records"))


def run(BC, x, y, wet, rules, periodic, fold, host=False, **kw):
    """the device result, checked against the definition: code, rule, records and counts"""
    wet = np.ascontiguousarray(wet, dtype=np.uint8)
    res = BC.basin_codes_dev(to(x), to(y), wet, rules, periodic=periodic, fold=fold, Re=RE, **kw)
    lon, lat = D.centres(x, y)
    u = device_units(lon, lat)
    su = device_units([r[1] for r in rules], [r[2] for r in rules])
    code, rule, rec = D.basin_codes(x, y, wet, [r[:7] for r in rules], periodic, fold, u, su, BC.seed_max_d2(kw.get("seed_max_distance"), RE))
    assert np.array_equal(res["code"], code) and np.array_equal(res["rule"], rule)
    assert res["code"].dtype == np.uint8 and res["rule"].dtype == np.int16
    for f in D.RECORD.names:
        assert np.array_equal(res["records"][f], rec[f]), (f, res["records"][f][:20], rec[f][:20])
    c = res["counts"]
    assert (c["wet"], c["coded"], c["uncoded"]) == (int(wet.astype(bool).sum()), int((code != 0).sum()),
                                                     int(wet.astype(bool).sum() - (code != 0).sum()))
    assert c["passes"] == len(BC.plan(rules)) - 1 and int(rec["cells"].sum()) == c["coded"]
    if host:
        h = BC.basin_codes(x, y, wet, rules, periodic=periodic, fold=fold, Re=RE, **kw)
        assert same(h, res) and h["summary"] == res["summary"]
    return res


def cell_box(g, j0, j1, i0, i1, pad=0.25):
    """(lon_w, lon_e, lat_s, lat_n) holding the centres of the cells (j0 .. j1, i0 .. i1) of a regular grid and no others"""
    x, y = g["x"], g["y"]
    dx, dy = x[0, 2] - x[0, 0], y[2, 0] - y[0, 0]
    return (float(x[1, 2 * i0 + 1] - pad * dx), float(x[1, 2 * i1 + 1] + pad * dx), float(y[2 * j0 + 1, 1] - pad * dy),
            float(y[2 * j1 + 1, 1] + pad * dy))


def centre(g, j, i):
    return float(g["x"][2 * j + 1, 2 * i + 1]), float(g["y"][2 * j + 1, 2 * i + 1])


# ---- regular grids around the tile ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("nx", [1, 2, 63, 64, 65, 129])
def test_regular_grids_around_the_tile(BC, ny, nx):
    g = sm.latlon_grid(ny, nx, lon0=-33.0, lat0=-21.0, dlon=1.0, dlat=1.0)
    ie, iw = (3 * nx) // 5, (2 * nx) // 5
    rules = [(1,) + centre(g, 0, 0) + cell_box(g, 0, ny - 1, 0, ie),                      # the western three fifths
             (2,) + centre(g, ny - 1, nx - 1) + cell_box(g, 0, ny - 1, iw, nx - 1),       # the eastern three fifths: they overlap
             (3,) + centre(g, ny // 2, nx // 2) + FULL,
             (1,) + centre(g, 0, nx - 1) + cell_box(g, 0, ny // 2, 0, nx - 1)]            # a second flood of code 1
    j, i = np.indices((ny, nx))
    wall = np.ones((ny, nx), np.uint8)
    wall[:, nx // 2] = 0
    for wet in (np.ones((ny, nx), np.uint8), ((i + j) % 2 == 0).astype(np.uint8), wall):
        res = run(BC, g["x"], g["y"], wet, rules, False, False, host=(ny, nx) == (33, 65))
    if nx > 2:   # behind the wall the western flood stops, the eastern one takes its side
        assert np.all(res["code"][:, :nx // 2] == 1) and np.all(res["code"][:, nx // 2 + 1:] == 2) and np.all(res["code"][:, nx // 2] == 0)


# ---- a serpentine channel through every tile -----------------------------------------------------------------------
def serpentine():
    ny, nx = 65, 129
    g = sm.latlon_grid(ny, nx, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    wet = np.zeros((ny, nx), np.uint8)
    wet[0::2] = 1
    for j in range(1, ny, 2):
        wet[j, nx - 1 if (j // 2) % 2 == 0 else 0] = 1
    rules = [(1, 0.5, 0.5, -180.0, 180.0, -90.0, 32.0),      # stops at the box edge, half way: rows 0 .. 31
             (2, 128.5, 64.5) + FULL,                       # seeded at the far end: the rest
             (3, 64.5, 0.5) + FULL]                         # seeded in rule 0's part
    return g, wet, rules


def test_serpentine_channel_cut_half_way(BC):
    g, wet, rules = serpentine()
    res = run(BC, g["x"], g["y"], wet, rules, False, False)
    assert np.array_equal(res["code"][:32], wet[:32]) and np.array_equal(res["code"][32:], 2 * wet[32:])
    r = res["records"]
    assert r["status"].tolist() == [0, 0, 3] and r["blocking_rule"].tolist() == [-1, -1, 0]
    assert r["cells"].tolist() == [int(wet[:32].sum()), int(wet[32:].sum()), 0] and res["counts"]["uncoded"] == 0 and res["counts"]["passes"] == 3


def test_two_classes_of_one_pass_do_not_unite(BC):
    """two rows of water joined only through the box of the OTHER rule of the pass: the first rule's flood must not reach its own
    box's cells of the second row through them; its box's east edge lies exactly on a column of centres, which belongs to it"""
    g = sm.latlon_grid(5, 20, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    wet = np.zeros((5, 20), np.uint8)
    wet[1] = wet[3] = 1
    wet[2, 15] = 1
    rules = [(1, 0.5, 1.5, 0.0, 10.5, 0.0, 5.0), (2, 19.5, 1.5, 11.0, 20.0, 0.0, 5.0)]
    res = run(BC, g["x"], g["y"], wet, rules, False, False, host=True)
    assert res["counts"]["passes"] == 1 and res["records"]["cells"].tolist() == [11, 19]
    assert np.all(res["code"][1, :11] == 1) and np.all(res["code"][3, :11] == 0) and np.all(res["code"][[1, 3], 11:] == 2)
    assert res["summary"]["uncoded_largest"] == [{"cells": 11, "root": 60, "j": 3, "i": 0, "lon": 0.5, "lat": 3.5}]


def test_diagonal_contact_does_not_connect(BC):
    g = sm.latlon_grid(4, 4, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    wet = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], np.uint8)
    res = run(BC, g["x"], g["y"], wet, [(7, 0.5, 0.5) + FULL], False, False, host=True)
    assert np.array_equal(res["code"], 7 * np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8))
    assert res["summary"]["uncoded_bodies"] == 1 and res["summary"]["uncoded_largest"][0]["cells"] == 4
    assert res["summary"]["uncoded_largest"][0]["root"] == 10


# ---- longitudes -----------------------------------------------------------------------------------------------------
def test_grid_stated_a_turn_away_from_the_boxes(BC):
    for turn in (360.0, -720.0):
        g = sm.latlon_grid(6, 40, lon0=10.0 + turn, lat0=0.0, dlon=1.0, dlat=1.0)
        rules = [(1, 12.5, 2.5, 10.0, 30.0, 0.0, 6.0), (2, 45.5 - 2 * turn, 2.5, 30.0 - 2 * turn, 50.0 - 2 * turn, 0.0, 6.0)]
        res = run(BC, g["x"], g["y"], np.ones((6, 40), np.uint8), rules, False, False)
        assert np.all(res["code"][:, :20] == 1) and np.all(res["code"][:, 20:] == 2)


def test_box_across_the_seam_of_a_periodic_band(BC):
    g = sm.latlon_grid(8, 36, lon0=-180.0, lat0=-20.0, dlon=10.0, dlat=5.0)
    wet = np.ones((8, 36), np.uint8)
    rules = [(4, 165.0, -2.5, 150.0, 210.0, -20.0, 20.0)]
    res = run(BC, g["x"], g["y"], wet, rules, True, False, host=True)
    assert np.all(res["code"][:, 33:] == 4) and np.all(res["code"][:, :3] == 4) and np.all(res["code"][:, 3:33] == 0)
    res = run(BC, g["x"], g["y"], wet, rules, False, False)   # without the seam the flood stays east
    assert np.all(res["code"][:, 33:] == 4) and np.all(res["code"][:, :33] == 0) and res["counts"]["uncoded"] == 8 * 33


# ---- invalid centres ------------------------------------------------------------------------------------------------
def test_invalid_centres_are_never_coded_block_the_flood_and_are_no_seed_cells(BC):
    g = sm.latlon_grid(5, 7, lon0=0.0, lat0=0.0, dlon=1.0, dlat=2.0)
    wet = np.zeros((5, 7), np.uint8)
    wet[2] = 1
    wet[4, 6] = 1
    g["x"][5, 7] = np.nan        # the centre of cell (2, 3): the only link between the row's two halves
    g["y"][9, 13] = np.inf       # the wet cell (4, 6)
    rules = [(1, 0.5, 5.0) + FULL,
             (2, 3.6, 5.0) + FULL,      # nearest to the NaN centre's place: the nearest VALID centre is (2, 4)'s
             (3, 6.5, 9.0) + FULL]      # at the infinite centre's place: the nearest valid one is land
    res = run(BC, g["x"], g["y"], wet, rules, False, False, host=True)
    assert res["code"][2].tolist() == [1, 1, 1, 0, 2, 2, 2] and res["code"][4, 6] == 0 and res["counts"]["uncoded"] == 2
    assert res["records"]["seed_cell"].tolist()[:2] == [14, 18] and res["records"]["status"].tolist() == [0, 0, 1]
    # no valid cell at all: there is no seed cell
    g["x"][1::2, 1::2] = np.nan
    res = run(BC, g["x"], g["y"], wet, rules[:1], False, False)
    assert res["records"]["status"].tolist() == [5] and res["records"]["seed_cell"].tolist() == [-1] and not res["code"].any()


# ---- the statuses ---------------------------------------------------------------------------------------------------
def test_every_status(BC):
    g = sm.latlon_grid(6, 8, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    wet = np.ones((6, 8), np.uint8)
    wet[0, 0] = 0
    rules = [(1, 0.5, 0.5) + FULL,                          # 1: the seed cell is land
             (2, 2.3, 2.5, 2.0, 2.4, 2.0, 3.0),             # 2: the seed is in its box, the seed cell's centre (2.5, 2.5) is not
             (3, 4.5, 4.5) + FULL,                          # 0: takes every wet cell
             (4, 1.5, 1.5) + FULL,                          # 3: rule 2 took the seed cell
             (5, 100.0, 50.0) + FULL]                       # 4: 90 degrees away
    res = run(BC, g["x"], g["y"], wet, rules, False, False, host=True, seed_max_distance=500.0e3)
    r = res["records"]
    assert r["status"].tolist() == [1, 2, 0, 3, 4] and r["blocking_rule"].tolist() == [-1, -1, -1, 2, -1] and r["cells"].tolist() == [0, 0, 47, 0, 0]
    assert r["seed_cell"].tolist()[:4] == [0, 18, 36, 9]
    res = run(BC, g["x"], g["y"], wet, rules, False, False)   # without the limit the far seed has a seed cell: rule 2 took it
    assert res["records"]["status"].tolist() == [1, 2, 0, 3, 3]
    lines = "\n".join(BC.summary_lines(res))
    assert "rule 0 (code 1) took nothing: the seed cell is land" in lines and "rule 3 (code 4) took nothing: the seed cell was taken by rule 2" in lines
    assert "code 3: 47 cells" in lines and "0 wet cells in 0 bodies of water have no code" in lines


# ---- the rule limits ------------------------------------------------------------------------------------------------
def one_cell_rules(g, n, nx):
    return [(1 + k % 255,) + centre(g, k // nx, k % nx) + cell_box(g, k // nx, k // nx, k % nx, k % nx) for k in range(n)]


@pytest.mark.parametrize("n, side, passes", [(255, 16, 1), (256, 16, 2), (4096, 64, 17)])
def test_rule_limits(BC, n, side, passes):
    g = sm.latlon_grid(side, side, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)
    res = run(BC, g["x"], g["y"], np.ones((side, side), np.uint8), one_cell_rules(g, n, side), False, False)
    assert res["counts"]["passes"] == passes and res["counts"]["coded"] == n
    assert np.array_equal(res["rule"].reshape(-1)[:n], np.arange(n)) and np.all(res["records"]["cells"] == 1)


# ---- random masks and rules -----------------------------------------------------------------------------------------
def random_case(seed):
    rng = np.random.default_rng(seed)
    ny, nx = 70, 150
    g = sm.latlon_grid(ny, nx, lon0=-180.0, lat0=-70.0, dlon=2.4, dlat=2.0)
    wet = (rng.random((ny, nx)) < 0.62).astype(np.uint8)   # just above the site-percolation threshold: large ragged bodies
    rules = []
    while len(rules) < 12:
        w, s = 0.25 * rng.integers(-800, 800), 0.25 * rng.integers(-300, 200)
        W, H = float(rng.choice([30.0, 90.0, 200.0, 360.0])), float(rng.choice([20.0, 60.0, 140.0]))
        box = (w, w + W, s, min(90.0, s + H))
        for _ in range(int(rng.integers(1, 4))):   # several seeds in one box, under shared codes
            rules.append((int(rng.integers(1, 6)), box[0] + W * rng.random(), box[2] + (box[3] - box[2]) * rng.random()) + box)
    return g, wet, rules[:12], bool(seed % 2), bool(seed % 4 >= 2)


@pytest.mark.parametrize("seed", range(20))
def test_random_masks_under_random_rules(BC, seed):
    g, wet, rules, periodic, fold = random_case(seed)
    res = run(BC, g["x"], g["y"], wet, rules, periodic, fold, host=seed == 0)
    assert res["counts"]["coded"] > 500 and res["counts"]["passes"] <= 12


def test_knobs_change_no_bit(BC, monkeypatch):
    cases = [random_case(s) for s in (1, 2, 3)] + [serpentine() + (False, False)]
    want = [BC.basin_codes_dev(to(g["x"]), to(g["y"]), wet, rules, periodic=p, fold=f, Re=RE) for g, wet, rules, p, f in cases]
    assert any(w["counts"]["passes"] < len(c[2]) for w, c in zip(want, cases))   # some rules do share a pass
    for env in (dict(OGG_BASIN_BATCH="0"), dict(OGG_BASIN_TILE_ROWS="1"), dict(OGG_BASIN_TILE_ROWS="7"), dict(OGG_BASIN_TILE_ROWS="32"),
                dict(OGG_BASIN_TILE_ROWS="64"), dict(OGG_BASIN_BATCH="0", OGG_BASIN_TILE_ROWS="7")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for (g, wet, rules, p, f), w in zip(cases, want):
            res = BC.basin_codes_dev(to(g["x"]), to(g["y"]), wet, rules, periodic=p, fold=f, Re=RE)
            assert same(res, w), env
            assert res["counts"]["passes"] == (len(rules) if env.get("OGG_BASIN_BATCH") == "0" else w["counts"]["passes"])
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setenv("OGG_BASIN_TILE_ROWS", "65")
    with pytest.raises(Exception, match="OGG_BASIN_TILE_ROWS=65"):
        BC.basin_codes_dev(to(cases[0][0]["x"]), to(cases[0][0]["y"]), cases[0][1], cases[0][2], periodic=True, fold=False)


# ---- the ocean mask's components ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [None, "1"])
@pytest.mark.parametrize("periodic,fold", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("shape", [(33, 129), (1, 65), (5, 7)])   # (5, 7): an odd fold narrower than a tile
def test_one_rule_over_the_sphere_floods_a_component_of_the_ocean_mask(BC, monkeypatch, shape, periodic, fold, rows):
    """both callers of the shared labelling agree: the flood of a rule whose box is the sphere is the ocean mask's component of the
    seed cell, cell for cell, with the size the mask's component list gives it"""
    from test_gpu_ocean_mask import lib_mask
    if rows:
        monkeypatch.setenv("OGG_MASK_TILE_ROWS", rows)
        monkeypatch.setenv("OGG_BASIN_TILE_ROWS", rows)
    ny, nx = shape
    g = sm.latlon_grid(ny, nx, lon0=-33.0, lat0=-21.0, dlon=1.0, dlat=1.0)
    wet = (np.random.default_rng(1000 * ny + nx).random(shape) < 0.5927).astype(np.uint8)
    cells = np.flatnonzero(wet)
    j, i = divmod(int(cells[cells.size // 2]), nx)   # the seed: the centre of the middle wet cell
    res = run(BC, g["x"], g["y"], wet, [(1,) + centre(g, j, i) + FULL], periodic, fold)
    comps = np.zeros(ny * nx, np.int64)
    root, _, _, counts = lib_mask(np.where(wet != 0, 100.0, 0.0), periodic, fold, components=comps)
    assert res["records"]["seed_cell"][0] == j * nx + i and root[j, i] >= 0
    assert np.array_equal(res["code"], (root == root[j, i]).astype(np.uint8))
    size = {2**31 - 1 - int(e & 0xFFFFFFFF): int(e >> 32) for e in comps[:counts["components"]]}
    assert res["records"]["cells"][0] == size[int(root[j, i])]


# ---- the seed cell --------------------------------------------------------------------------------------------------
def test_seed_cells_are_those_of_the_ocean_mask(BC, hip):
    import torch
    from ocean_model_grid_generator_amd import ocean_mask as M
    L = hip
    g = sm.latlon_grid(6, 8, lon0=-4.0, lat0=-3.0, dlon=1.0, dlat=1.0)   # centres at -3.5 .. 3.5 x -2.5 .. 2.5
    g["x"][7, 11], g["y"][7, 11] = g["x"][7, 3], g["y"][7, 3]           # the cells (3, 1) and (3, 5) hold one centre
    rng = np.random.default_rng(8)
    seeds = [(0.0, 0.5), (0.0, -1.5), (-2.5, 0.5), (-2.4, 0.6), (3.5, 2.5), (40.0, 60.0), (179.0, -89.0)] + \
        [(float(a), float(b)) for a, b in zip(rng.uniform(-5, 5, 20), rng.uniform(-4, 4, 20))]
    rules = [(1, s[0], s[1]) + FULL for s in seeds]
    res = run(BC, g["x"], g["y"], np.ones((6, 8), np.uint8), rules, False, False)
    rec = res["records"]
    # (0, 0.5) is equidistant from the centres (-0.5, 0.5) and (0.5, 0.5), to the bit: the smaller cell wins
    u = device_units(*D.centres(g["x"], g["y"])).reshape(6, 8, 3)
    su = device_units([0.0], [0.5])[0]
    d2 = lambda a: ((a[0] - su[0]) * (a[0] - su[0]) + (a[1] - su[1]) * (a[1] - su[1])) + (a[2] - su[2]) * (a[2] - su[2])   # noqa: E731
    assert d2(u[3, 3]) == d2(u[3, 4]) and rec["seed_cell"][0] == 3 * 8 + 3 and rec["seed_cell"][1] == 1 * 8 + 3
    assert rec["seed_cell"][2] == 3 * 8 + 1 and rec["seed_cell"][3] == 3 * 8 + 1   # identical centres: cell 25, not 29
    p = M.params(6, 8, False, False)
    ll = to(np.array(seeds, np.float64))
    out = torch.empty(2 * len(seeds), dtype=torch.int64, device="cuda:0")
    dx, dy = to(g["x"]), to(g["y"])
    L.call("ogg_mask_seed_dev", ctypes.byref(p), dx.data_ptr(), dy.data_ptr(), 17, len(seeds), ll.data_ptr(), out.data_ptr(),
           torch.cuda.current_stream().cuda_stream)
    out = out.cpu().numpy()
    assert np.array_equal(out[1::2], rec["seed_cell"]) and np.array_equal(out[0::2], rec["d2_bits"])


# ---- paths ----------------------------------------------------------------------------------------------------------
RULES_TEXT = """# three rules on the synthetic continents
1 -150 -60 -180 180 -90 -35 southern     # the ring south of 35S
9   25   5   15  35  -5  15 lake         # the lake inside the continent
2 -150   0 -180 180 -90  90 world        # what is left, the sea behind the sill with it
"""


def test_main_function_level_file_command_and_supergrid_write_the_same_bytes(BC, hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import LAKE, read, synthetic_raster, centres_in
    src, rf = str(tmp_path / "src.nc"), str(tmp_path / "rules.txt")
    synthetic_raster(src)
    open(rf, "w").write(RULES_TEXT)
    names = ("grid", "topog", "t2", "b1", "b2", "b3", "b4", "tm", "tm2", "mask", "mask2", "m1", "m2", "m3")
    f = {k: str(tmp_path / (k + ".nc")) for k in names}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src, basin_rules=rf)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], basin_codes_file=f["b1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], basin_codes_file=f["b2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert out.count("basin codes: code 9 (lake)") == 2 and out.index("topography:") < out.index("basin codes:")
    lines = [ln for ln in out.splitlines() if "basin codes:" in ln]
    assert lines[:len(lines) // 2] == lines[len(lines) // 2:] and " m2" in lines[1]   # the same digits on both paths, with areas

    def command(*args):
        r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.basin_codes", f["grid"], "--rules", rf] + list(args),
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout
    assert [ln for ln in command("--topog", f["topog"], "-o", f["b3"]).splitlines() if "basin codes:" in ln] == lines[:len(lines) // 2]
    b1 = open(f["b1"], "rb").read()
    assert b1 == open(f["b2"], "rb").read() and b1 == open(f["b3"], "rb").read()
    # Supergrid.basin_codes on the generated grid
    from test_gpu_runoff import stitched
    import ocean_model_grid_generator_amd.supergrid as sg
    wet = (read(f["topog"], "depth") > 0).astype(np.uint8)
    g = netcdf3.read_doubles(f["grid"], names=("x", "y"))
    for world in (1, 2):   # (the grid of main(1.0, ensure_nj_even=True)); rank 0 holds the result whatever the rank count
        plan, ranks, cut, _ = stitched(sg, "r1", world)
        res = ranks[0].basin_codes(cut, wet, BC.read_rules(rf))
        assert all(r.basin_codes(cut, wet, BC.read_rules(rf)) is None for r in ranks[1:])
        BC.write_basin_codes(f["b4"], res)
        assert open(f["b4"], "rb").read() == b1
        assert [ln for ln in BC.summary_lines(res)] == lines[:len(lines) // 2]
    # the file holds what the definition gives on the grid and wet set as written
    rules = [tuple(BC.read_rules(rf).table[k][n] for n in D.FIELDS) for k in range(3)]
    code, rule, rec = D.basin_codes(g["x"], g["y"], wet, rules, True, True)
    assert np.array_equal(read(f["b1"], "basin"), code) and np.array_equal(read(f["b1"], "rule"), rule) and np.array_equal(read(f["b1"], "wet"), wet)
    lake = centres_in(g["x"], g["y"], LAKE)
    assert lake.sum() > 20 and np.all(code[lake] == 9) and rec["status"].tolist() == [0, 0, 0] and np.all(code[wet != 0] != 0)
    h = netcdf3.read_header(f["b1"])
    assert h.vars["basin"].atts["flag_values"].tolist() == [0, 1, 2, 9] and h.vars["basin"].atts["flag_meanings"] == "none southern world lake"
    assert h.gatts["rule_0001"].split()[0] == "9" and h.gatts["rule_0001"].split()[-1] == "lake" and int(h.gatts["n_rules"][0]) == 3
    # with --ocean_mask_file the edited wet set is used: the lake is land there, and the rule seeded in it says so
    mk = dict(kw, mask_min_depth=10.0, skip_metrics=True)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm"], ocean_mask_file=f["mask"], basin_codes_file=f["m1"], **mk)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm2"], ocean_mask_file=f["mask2"], basin_codes_file=f["m2"], path="functions", **mk)
    out = capsys.readouterr().out
    assert out.count("rule 1 (code 9) took nothing: the seed cell is land") == 2 and " m2" not in out.split("basin codes:", 1)[1].split("\n")[1]
    command("--mask", f["mask"], "-o", f["m3"])
    bm = open(f["m1"], "rb").read()
    assert bm == open(f["m2"], "rb").read() and bm == open(f["m3"], "rb").read() and bm != b1
    mask = read(f["mask"], "mask")
    assert np.array_equal(read(f["m1"], "wet"), (mask != 0).astype(np.int8)) and not np.any(read(f["m1"], "basin") == 9)
    assert np.all(read(f["m1"], "basin")[lake] == 0)

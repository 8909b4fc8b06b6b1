"""CPU tests of the hand-made grids and rasters of tests/small_grids.py: that every named input reaches the branch it is named for,
using only the numpy definitions (tests/topog_definition.py, oracle/quality_oracle.py); and the two points the definition of
topography settles: a sample that is not finite is MISSING, and a regional raster is met on its own longitude branch."""
import numpy as np
import pytest

import small_grids as G
import topog_definition as td
from oracle import quality_oracle as qo
from test_gpu_quality import delta_tolerance

SWEEP = (1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256)


def records(x, y, kind, **kw):
    r = G.raster(kind)
    kw.setdefault("cells_", "supergrid")
    return td.records(x, y, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], **kw)


# ---- topography: every named case reaches its branch -----------------------------------------------------------
def test_coordinates_are_on_the_eighth_degree_lattice():
    grids = [G.shape_grid(n) for n in G.TOPOG_SHAPES] + [G.placed(n) for n in G.PLACEMENTS] + [G.beyond_pole_row(s) for s in (1, -1)]
    grids += list(G.odd_cells().values()) + [v[:2] for k, v in G.pole_cells().items() if "block" not in k]
    for x, y in grids:
        assert np.array_equal(x * 8, np.rint(x * 8)) and np.array_equal(y * 8, np.rint(y * 8))


def test_pole_cells_set_the_pole_flag_where_claimed():
    for name, (x, y, n_pole) in G.pole_cells().items():
        c = td.cells(x, y, 0.25, 0.25)
        assert int(np.sum(c["pole"] != 0)) == n_pole, name
        if n_pole:
            assert int(c["pole"].reshape(-1)[np.flatnonzero(c["pole"])[0]]) == (1 if "north" in name else -1), name
            assert c["pole"].reshape(-1)[0] != 0 and (c["pole"].size == 1 or not np.any(c["pole"].reshape(-1)[1:])), name
        else:   # a corner on the pole: the substitution of its row neighbour's longitude is what the cell is for
            on = np.abs(y) >= 90.0 - td.POLE_EPS
            assert on.sum() == (2 if "row" in name else 1), name
            L = np.array([[c["L00"][0, 0], c["L01"][0, 0]], [c["L10"][0, 0], c["L11"][0, 0]]])
            if "row" in name:     # both corners of a row: the two substitutions swap
                r = int(name[-1])
                assert L[r, 0] == x[r, 1] and L[r, 1] == x[r, 0], name
            else:
                r, k = np.argwhere(on)[0]
                assert L[r, k] == x[r, 1 - k], name
        rec = records(x, y, "int16")
        assert rec["n_pole"].sum() == n_pole and np.all(rec["n"] > 0), name


def test_odd_cells_are_what_their_names_say():
    odd = G.odd_cells()
    for name, (x, y) in odd.items():
        c = td.cells(x, y, 0.25, 0.25)
        # exactly 180 degrees: every corner unwraps to the west of x00 and the winding sum is -360, so the cell counts as enclosing
        # a pole (the northern one by its latitudes) and samples the polar row
        assert int(c["pole"][0, 0]) == (1 if name == "wide_180" else 0), name
        span = max(c[k][0, 0] for k in ("L00", "L01", "L10", "L11")) - min(c[k][0, 0] for k in ("L00", "L01", "L10", "L11"))
        if name == "point":
            assert c["R"][0, 0] == 1 and not c["clamped"][0, 0]
        if name == "wide_180":
            assert c["L01"][0, 0] == -180.0 and span == 180.0 and c["clamped"][0, 0]
        if name == "wider_200":
            assert c["L01"][0, 0] == -160.0 and span == 160.0
        if name == "clockwise":
            a = (x[0, 1] - x[0, 0]) * (y[1, 0] - y[0, 0]) - (x[1, 0] - x[0, 0]) * (y[0, 1] - y[0, 0])
            assert a < 0
        rec = records(x, y, "int16")
        assert rec["n"][0, 0] == rec["R"][0, 0] ** 2, name


def test_placements_miss_from_the_right_cause():
    home = records(*G.placed("home"), "window")
    assert np.all(home["n_missing"] == 0) and np.all(home["n"] == home["R"] ** 2)
    for name in ("across_window_lon0", "across_window_east"):     # columns outside the window: the west / east cells lose samples
        r = records(*G.placed(name), "window")
        lost = r["n_missing"] > 0
        assert lost.any() and not lost.all(), name
        assert lost[:, 0].all() != lost[:, -1].all(), name
    for name in ("above_window", "below_window"):                  # rows outside the window
        r = records(*G.placed(name), "window")
        lost = r["n_missing"] > 0
        assert np.array_equal(lost, np.broadcast_to(lost[:, :1], lost.shape)) and lost.any() and not lost.all(), name
    r = records(*G.placed("across_180"), "int16")                  # the seam of a periodic raster loses nothing
    assert np.all(r["n_missing"] == 0)


def test_latitude_clamp_is_hit():
    """A periodic raster that stops at 60 degrees: rows beyond it read its edge row (valid samples), a regional one loses them."""
    r60 = G.raster("band60")
    for name, edge_row in (("above_band60", -1), ("below_band60", 0)):
        x, y = G.placed(name)
        rec = records(x, y, "band60")
        assert np.all(rec["n_missing"] == 0), name
        c = td.cells(x, y, 0.25, 0.25)
        flat = {k: v.reshape(-1) for k, v in c.items()}
        idx = np.arange(flat["R"].size)
        lon, lat = td.sample_positions(flat, int(flat["R"][0]), idx)
        fj = np.floor((lat - r60["box"][2]) / r60["box"][3])
        assert (fj < 0).any() or (fj > r60["data"].shape[0] - 1).any(), name
        # the outermost cell row lies wholly beyond the raster: every sample of it is one of the edge row's values
        row = rec["min"][edge_row], rec["max"][edge_row]
        assert row[0].min() >= r60["data"][edge_row].min() and row[1].max() <= r60["data"][edge_row].max()
    for sign in (1, -1):
        x, y = G.beyond_pole_row(sign)
        assert np.abs(y).max() == 95.0
        assert np.all(records(x, y, "int16")["n_missing"] == 0)
        assert np.all(records(x, y, "window")["n"] == 0)


def test_fills_are_hit():
    x, y = G.placed("home")
    plain, one, two = (records(x, y, k) for k in ("int16", "int16_fill1", "int16_fill2"))
    assert np.all(plain["n_missing"] == 0)
    assert one["n_missing"].sum() > 0 and two["n_missing"].sum() > one["n_missing"].sum()
    assert two["max"].max() < 32767 and two["min"].min() > -32768
    for kind in G.FLOAT_RASTERS:
        r = G.raster(kind)
        d = r["data"]
        assert np.isnan(d).any() and (d == d.dtype.type(-999.0)).any() and (d == d.dtype.type(1.0e20)).any()
        rec = records(x, y, kind)
        assert rec["n_missing"].sum() > 0 and rec["n"].sum() > 0, kind


def test_float_rasters_sit_on_ties_and_limits():
    for kind in ("float32_q0.5", "float64_q0.5"):
        r = G.raster(kind)
        d = r["data"].astype(np.float64)
        ok = np.isfinite(d) & (d != -999.0) & (np.abs(d) < 1e19)
        t = d[ok] / 0.5
        on_tie = np.abs(t - np.floor(t) - 0.5) == 0.0
        assert on_tie.sum() >= ok.sum() - 2          # all but the two planted limits
    for kind in G.FLOAT_RASTERS:
        r = G.raster(kind)
        q, quantum = td.quantise(r["data"], r["quantum"], r["fill"])
        assert [int(q[e]) for e in G.LIMIT_ELEMENTS] == [2 ** 21, -2 ** 21], kind
        rec = records(*G.limit_grid(), kind)
        assert rec["max"][0, 0] == 2 ** 21 and rec["min"][1, 0] == -2 ** 21, kind
        for bad in ((2 ** 21 + 1) * quantum, -(2 ** 21 + 1) * quantum, np.inf, -np.inf):
            d = r["data"].copy()
            d[G.LIMIT_ELEMENTS[0]] = bad
            with pytest.raises(ValueError, match="2\\^21"):
                td.quantise(d, r["quantum"], r["fill"])


def test_small_rasters_are_hit_by_the_home_grids():
    x, y = G.placed("home")
    for kind in ("1x1_global", "1x1_regional", "nx1", "ny1"):
        rec = records(x, y, kind)
        assert rec["n"].sum() > 0, kind
        if kind != "1x1_global":
            assert rec["n_missing"].sum() > 0, kind      # smaller than the grid: part of every grid lies outside
    assert G.raster("nx1")["data"].shape[1] == 1 and G.raster("ny1")["data"].shape[0] == 1


def lane_walk(R):
    """The kernel's walk over the flattened samples of one cell, in Python: lane l takes f = l, l + 64, ... and carries (a, b) along
    with step_a = 64 % R, step_b = 64 // R and the carry a >= R.  Returns ((a, b) of every visit, whether the carry was taken)."""
    seen, carried = [], False
    for lane in range(min(64, R * R)):
        f, a, b = lane, lane % R, lane // R
        while f < R * R:
            seen.append((a, b))
            f, a, b = f + 64, a + 64 % R, b + 64 // R
            if a >= R:
                a, b, carried = a - R, b + 1, True
    return seen, carried


def test_refine_sweep_covers_the_carry_and_more_than_a_wavefront():
    carry, no_carry = [], []
    for R in SWEEP:
        seen, carried = lane_walk(R)
        assert sorted(seen) == sorted((a, b) for b in range(R) for a in range(R)), R
        (carry if carried else no_carry).append(R)
    assert set(no_carry) >= {1, 2, 8, 32, 64} and set(carry) >= {3, 7, 31, 33, 63, 65, 96, 127, 128, 129, 255, 256}
    assert any(R > 64 for R in SWEEP) and any(64 % R == R - 1 for R in SWEEP) and any(64 % R == 1 for R in SWEEP)


# ---- topography: truths that do not come from the definition ---------------------------------------------------
@pytest.mark.parametrize("kind", G.INDEX_RASTERS)
def test_index_rasters_closed_forms_hold_for_the_definition(kind):
    x, y = G.grid(6, 8)
    for R in (2, 8, 16):
        rec = records(x, y, kind, refine=R)
        for j in range(6):
            for i in range(8):
                n, s, ss, mn, mx = G.index_truth(kind, int(x[j, i] * 8), int(y[j, i] * 8), R)
                got = tuple(int(rec[f][j, i]) for f in ("n", "sum", "sumsq", "min", "max"))
                assert got == (n, s, ss, mn, mx), (R, j, i)
    x, y = G.grid(1, 4, lon0=178.0)     # across the raster's seam: is wraps
    rec = records(x, y, kind, refine=8)
    for i in range(4):
        assert tuple(int(rec[f][0, i]) for f in ("n", "sum", "sumsq", "min", "max")) == G.index_truth(kind, int(x[0, i] * 8), int(y[0, i] * 8), 8)


def test_capacity_closed_form_holds_for_the_definition():
    x, y = G.grid(2, 2)
    for kind, sign in (("const_p", 1), ("const_m", -1)):
        rec = records(x, y, kind, refine=256, cells_="model")
        want = {"n": 2 ** 18, "n_missing": 0, "sum": sign * 2 ** 39, "sumsq": 2 ** 60, "min": sign * 2 ** 21, "max": sign * 2 ** 21, "R": 256}
        for f, v in want.items():
            assert int(rec[f][0, 0]) == v, (kind, f)


def test_mirror_and_shift_hold_for_the_definition():
    x, y = G.placed("home")
    for kind in ("int16", "window"):
        want = records(x, y, kind, refine=8)
        for sj, si in ((1, -1), (-1, 1), (-1, -1)):
            got = records(np.ascontiguousarray(x[::sj, ::si]), np.ascontiguousarray(y[::sj, ::si]), kind, refine=8)
            for f in td.RECORD_FIELDS:
                np.testing.assert_array_equal(got[f], want[f][::sj, ::si], err_msg=f)


# ---- the two settled points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "band60", "window", "float64_q0.5"])
@pytest.mark.parametrize("coord", ["x", "y"])
@pytest.mark.parametrize("value", ["nan", "pinf", "minf"])
def test_a_point_that_is_not_finite_makes_its_cells_missing(kind, coord, value):
    """A cell with one corner that is not finite: n = 0, every sample MISSING, R clamped to 256; its neighbours are untouched."""
    x, y, cells = G.nonfinite_grid(coord, value)
    rec = records(x, y, kind)
    clean = records(*G.placed("home"), kind)
    hit = np.zeros(rec["n"].shape, dtype=bool)
    for j, i in cells:
        hit[j, i] = True
        assert (rec["n"][j, i], rec["n_missing"][j, i], rec["n_clamped"][j, i], rec["R"][j, i]) == (0, 65536, 1, 256), (j, i)
        assert rec["n_wet"][j, i] == 0 and rec["sum"][j, i] == 0 and rec["n_pole"][j, i] == 0
    for f in td.RECORD_FIELDS:
        np.testing.assert_array_equal(rec[f][~hit], clean[f][~hit], err_msg=f)


@pytest.mark.parametrize("kind", G.REGIONAL_KINDS + ("int16", "band60", "float32_q0.01"))
def test_records_do_not_depend_on_the_longitude_branch(kind):
    """x -> x + 360 k and lon0 -> lon0 +- 360 leave every record as it is, for regional rasters as for periodic ones."""
    x, y = G.placed("home")
    r = G.raster(kind)
    want = records(x, y, kind)
    assert want["n"].sum() > 0
    for k in (-2, -1, 1, 10):
        got = records(x + 360.0 * k, y, kind)
        for f in td.RECORD_FIELDS:
            np.testing.assert_array_equal(got[f], want[f], err_msg="%s k=%d" % (f, k))
    for shift in (-360.0, 360.0):
        box = (r["box"][0] + shift,) + r["box"][1:]
        got = td.records(x, y, r["data"], *box, quantum=r["quantum"], fill=r["fill"], cells_="supergrid")
        for f in td.RECORD_FIELDS:
            np.testing.assert_array_equal(got[f], want[f], err_msg="%s lon0 %+g" % (f, shift))


def test_the_window_stated_a_turn_away_is_the_same_raster():
    x, y = G.placed("home")
    want = records(x, y, "window")
    assert want["n"].sum() == 48 * 81     # R = ceil(2 * 1.125 / 0.25) = 9 with the shear
    big = records(x, y, "int16")       # the window is a cut of the big raster: inside it both give the same records
    for f in td.RECORD_FIELDS:
        np.testing.assert_array_equal(want[f], big[f], err_msg=f)
    for kind in ("window_p360", "window_m360"):
        got = records(x, y, kind)
        for f in td.RECORD_FIELDS:
            np.testing.assert_array_equal(got[f], want[f], err_msg=kind + " " + f)


# ---- quality grids ---------------------------------------------------------------------------------------------
def near_edges(g):
    """the number of corners whose delta lies within delta_tolerance of a bin edge (the ``near`` of check_against_oracle)"""
    delta, tol = qo.corner_delta(g["x"], g["y"], G.RE), delta_tolerance(g["x"], g["y"])
    ok = ~np.isnan(delta)
    return sum(int(np.sum(np.abs(delta[ok] - e) <= tol[ok])) for e in qo.BIN_EDGES_DEG)


def test_quality_pairs_cover_the_tile_edges():
    assert len(G.QUALITY_PAIRS) >= 12 and (1, 1) in G.QUALITY_PAIRS
    assert {p[0] for p in G.QUALITY_PAIRS} == {1, 2, 31, 32, 33, 64, 65}
    assert {p[1] for p in G.QUALITY_PAIRS} == {1, 2, 126, 127, 128, 253, 254, 255}
    for ny, nx in G.QUALITY_PAIRS:
        g = G.quality_shape(ny, nx)
        assert g["x"].shape == (ny + 1, nx + 1) and g["dx"].shape == (ny + 1, nx) and g["dy"].shape == (ny, nx + 1)
        assert g["area"].shape == (ny, nx) and g["dx"].min() > 1.0 and g["dy"].min() > 1.0


def test_no_corner_of_a_quality_grid_lies_near_a_bin_edge():
    grids = [G.seven_bins_grid(), G.planted_base()] + [G.quality_shape(*p) for p in G.QUALITY_PAIRS]
    for g in grids:
        assert near_edges(g) == 0
    for j, i in ((0, 0), (5, 126), (5, 127), (31, 7), (32, 7), (39, 139)):    # the moved points of the planted-delta test
        g = G.planted_base()
        g["x"][j, i] += 0.1
        assert near_edges(g) == 0


def test_seven_bins_grid_fills_every_bin():
    g = G.seven_bins_grid()
    assert g["x"].shape == (34, 141)
    sec = qo.grid_section(g["x"], g["y"], g["dx"], g["dy"], g["area"], Re=G.RE)
    h = sec["corner"]["histogram"]
    assert len(h) == 7 and all(c > 0 for c in h), h
    assert sum(h) + sec["corner"]["n_degenerate"] == sec["corner"]["n"]

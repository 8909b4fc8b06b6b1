"""GPU tests of the grid-quality report (csrc/ogg_quality.hip) on the hand-made grids of tests/small_grids.py, against the numpy
definition in oracle/quality_oracle.py: grids narrower and shorter than one tile of 127 columns by 32 rows and grids that end one
column or row before, on and after a tile edge; extrema planted on the tile edges; ties across tiles and sections; degenerate and
non-finite values; a grid that fills every bin of the corner histogram; and every split of a grid into sections, with planted seams."""
import copy

import numpy as np
import pytest

import small_grids as G
from oracle import quality_oracle as qo
from test_gpu_quality import check_against_oracle

pytestmark = pytest.mark.gpu
RE = G.RE
FIELDS = ("x", "y", "dx", "dy", "area")


@pytest.fixture(scope="module")
def Q(hip):
    from ocean_model_grid_generator_amd import grid_quality
    return grid_quality


def oracle(g, metrics=True):
    with np.errstate(all="ignore"):
        return qo.grid_section(*[g[k] for k in (FIELDS if metrics else FIELDS[:2])], Re=RE)


def report(Q, g, metrics=True, **kw):
    return Q.grid_quality(*[g[k] for k in (FIELDS if metrics else FIELDS[:2])], Re=RE, **kw)


def check(Q, g, metrics=True):
    """the device's whole-grid section of g against the oracle's; returns both"""
    got, want = report(Q, g, metrics)["grid"], oracle(g, metrics)
    with np.errstate(all="ignore"):
        check_against_oracle(got, want, g["x"], g["y"])
    return got, want


def where(e):
    return (e["j"], e["i"])


# ---- shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", G.QUALITY_PAIRS)
def test_shapes_around_the_tile_edges(Q, ny, nx):
    import torch
    g = G.quality_shape(ny, nx)
    for metrics in (True, False):
        got, want = check(Q, g, metrics)
        assert got["corner"]["histogram"] == want["corner"]["histogram"]
        d = [torch.from_numpy(g[k]).to("cuda:0") for k in (FIELDS if metrics else FIELDS[:2])]
        assert Q.grid_quality_dev(*d, Re=RE) == report(Q, g, metrics)
    assert got["dx"] is None and got["rx_max"] is None


# ---- planted extrema -------------------------------------------------------------------------------------------
# rows and columns of the 41 x 141 points of planted_base(): the first and last of the grid, the last a tile owns and the first of the next
ROWS = {"dx": (0, 31, 32, 40), "dy": (0, 31, 32, 39), "area": (0, 31, 32, 39)}
COLS = {"dx": (0, 126, 127, 139), "dy": (0, 126, 127, 140), "area": (0, 126, 127, 139)}


@pytest.mark.parametrize("field", ["dx", "dy", "area"])
def test_planted_sizes(Q, field):
    """the largest and the smallest dx, dy and area, one value edited at a time: the last point row (dx), the column i = nx (dy), the
    rows and columns on either side of a tile edge"""
    base = G.planted_base()
    hi, lo = 10.0 * base[field].max(), 0.1 * base[field].min()
    for j in ROWS[field]:
        for i in COLS[field]:
            for which, v in (("max", hi), ("min", lo)):
                g = copy.deepcopy(base)
                g[field][j, i] = v
                got, want = check(Q, g)
                assert where(want[field][which]) == (j, i) and want[field][which]["value"] == v
                assert got[field][which] == want[field][which]


def test_planted_ratios_and_aspect(Q):
    base = G.planted_base()
    nx = 140
    for j in (0, 31, 32, 40):          # rx at column i: dx[j, i + 1] ten times and dx[j, i + 2] three times their size; i = nx - 1 pairs
        for i in (0, 126, 127, nx - 2, nx - 1):   # with dx[j, 0]
            g = copy.deepcopy(base)
            g["dx"][j, (i + 1) % nx] *= 10.0
            g["dx"][j, (i + 2) % nx] *= 3.0
            got, want = check(Q, g)
            assert where(want["rx_max"]) == (j, i) and got["rx_max"] == want["rx_max"]
    for j in (0, 30, 31, 32, 38):      # ry at row j: dy[j + 1] against dy[j]; j = 31 reads the next tile's first row
        for i in (0, 126, 127, 140):
            g = copy.deepcopy(base)
            g["dy"][j + 1, i] *= 10.0
            if j + 2 < 40:
                g["dy"][j + 2, i] *= 3.0
            got, want = check(Q, g)
            assert where(want["ry_max"]) == (j, i) and got["ry_max"] == want["ry_max"]
    for j in (0, 31, 32, 39):          # aspect of cell (j, i): both of its dy a hundredth
        for i in (0, 126, 127, 139):
            g = copy.deepcopy(base)
            g["dy"][j, i] *= 0.01
            g["dy"][j, i + 1] *= 0.01
            got, want = check(Q, g)
            assert where(want["aspect_ratio_max"]) == (j, i) and got["aspect_ratio_max"] == want["aspect_ratio_max"]


def test_planted_delta(Q):
    """one point moved a tenth of a degree east: the largest corner angle lies next to it, whichever tile that is"""
    for j, i in ((0, 0), (5, 126), (5, 127), (31, 7), (32, 7), (39, 139)):
        for metrics in (True, False):
            g = G.planted_base()
            g["x"][j, i] += 0.1
            got, want = check(Q, g, metrics)
            gm, wm = got["corner"]["delta_max_deg"], want["corner"]["delta_max_deg"]
            assert where(gm) == where(wm) and (gm["lon"], gm["lat"]) == (wm["lon"], wm["lat"])
            assert abs(wm["j"] - j) <= 1 and abs(wm["i"] - i) <= 1
            assert got["corner"]["histogram"] == want["corner"]["histogram"]


# ---- ties ------------------------------------------------------------------------------------------------------
TIES = [((3, 9), (3, 5)), ((4, 2), (3, 100)), ((5, 130), (5, 3)), ((2, 130), (5, 3)), ((33, 1), (2, 130)), ((35, 130), (33, 131))]


@pytest.mark.parametrize("field,which", [("dx", "max"), ("dy", "min"), ("area", "max"), ("area", "min")])
def test_ties_go_to_the_smallest_j_i(Q, field, which):
    """the same extreme value at two places: inside one workgroup, in two tiles side by side, in two tiles one above the other, and in
    two sections"""
    base = G.planted_base()
    v = 10.0 * base[field].max() if which == "max" else 0.1 * base[field].min()
    for a, b in TIES:
        g = copy.deepcopy(base)
        g[field][a], g[field][b] = v, v
        got, want = check(Q, g)
        assert where(want[field][which]) == min(a, b) and got[field][which] == want[field][which]
    g = copy.deepcopy(base)
    g[field][25, 3], g[field][10, 130] = v, v
    rep = report(Q, g, sections=[("A", 0), ("B", 20)])
    assert where(rep["grid"][field][which]) == (10, 130) and where(rep["A"][field][which]) == (10, 130)
    assert where(rep["B"][field][which]) == (25, 3)
    assert rep["grid"] == report(Q, g)["grid"]


# ---- degenerate and non-finite values --------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_values_that_are_not_finite(Q, field):
    """NaN, +inf and -inf in each of x, y, dx, dy and area, inside a tile and on its edges: counts and extrema as the oracle's (a NaN
    is no extremum and no degenerate size; a corner with a NaN point is degenerate)"""
    for v in (np.nan, np.inf, -np.inf):
        for j, i in ((3, 5), (31, 126), (32, 127)):
            g = G.planted_base()
            g[field][j, i] = v
            got, want = check(Q, g)
            if field in ("x", "y"):
                assert want["corner"]["n_degenerate"] == 3 and got["corner"]["histogram"] == want["corner"]["histogram"]
                check(Q, g, metrics=False)


def test_degenerate_sizes_zero_areas_and_coincident_points(Q):
    g = G.planted_base()
    for j, i in ((3, 5), (31, 126), (32, 127), (40, 0)):
        g["dx"][j, i] = 5.0e-4                       # below 1 mm
    for j, i in ((2, 7), (31, 127), (32, 140), (39, 0)):
        g["dy"][j, i] = 9.99e-4
    g["dy"][7, 7] = 1.0e-3                           # exactly 1 mm is no degenerate size
    for j, i in ((0, 0), (31, 126), (32, 127), (39, 139)):
        g["area"][j, i] = 0.0
    g["area"][9, 9] = -0.0
    for j, i in ((10, 10), (31, 127), (39, 140)):    # coincident points: a point takes its western neighbour's place,
        g["x"][j, i], g["y"][j, i] = g["x"][j, i - 1], g["y"][j, i - 1]
    g["x"][33, 0], g["y"][33, 0] = g["x"][32, 0], g["y"][32, 0]      # ... and one its southern neighbour's
    got, want = check(Q, g)
    assert (want["dx"]["n_degenerate"], want["dy"]["n_degenerate"], want["area"]["n_zero"]) == (4, 4, 5)
    assert want["corner"]["n_degenerate"] == 4


def test_all_nan_fields_and_infinite_ratios(Q):
    for field in ("dx", "dy", "area"):
        g = G.planted_base()
        g[field][:] = np.nan
        got, want = check(Q, g)
        assert want[field]["min"] is None and want[field]["max"] is None and got[field] == want[field]
    g = G.planted_base()
    g["dx"][3, 5:8] = np.inf                          # inf / inf: no ratio; inf / finite: an infinite one
    g["dy"][31:34, 126] = np.inf
    got, want = check(Q, g)
    assert want["rx_max"]["value"] == np.inf and where(want["rx_max"]) == (3, 4)
    assert want["ry_max"]["value"] == np.inf and where(want["ry_max"]) == (30, 126)


# ---- the histogram ---------------------------------------------------------------------------------------------
def test_seven_bins(Q):
    """a grid with a corner in every bin and none within the tolerance of an edge (tests/test_small_grids_cpu.py): the histogram is
    the oracle's, count for count"""
    g = G.seven_bins_grid()
    for metrics in (True, False):
        got, want = check(Q, g, metrics)
        h = got["corner"]["histogram"]
        assert h == want["corner"]["histogram"] and all(c > 0 for c in h)
        assert sum(h) + got["corner"]["n_degenerate"] == got["corner"]["n"] == 33 * 140


# ---- sections and seams ----------------------------------------------------------------------------------------
def shifted(sec, dj):
    """a section's report with dj added to the row of every extremum"""
    out = copy.deepcopy(sec)

    def walk(d):
        if isinstance(d, dict):
            if "j" in d and "value" in d:
                d["j"] += dj
            for v in d.values():
                walk(v)
    walk(out)
    return out


def oracle_of_section(g, j0, j1, last):
    """The oracle's report of the section of point rows j0 .. j1 - 1, rows counted from j0.  A section that is not the last also owns
    the cell row between its last point row and the next section's first (corners, dy, area and aspect reach into row j1, the dy
    ratio into cell row j1 where that exists), but not the dx of row j1."""
    sl = lambda k, a, b: np.ascontiguousarray(g[k][a:b])
    c1 = j1 - 1 if last else j1                      # cell rows j0 .. c1 - 1, point rows j0 .. c1
    with np.errstate(all="ignore"):
        out = qo.grid_section(sl("x", j0, c1 + 1), sl("y", j0, c1 + 1), sl("dx", j0, c1 + 1), sl("dy", j0, c1), sl("area", j0, c1), Re=RE)
        if not last:
            own = qo.grid_section(sl("x", j0, j1), sl("y", j0, j1), sl("dx", j0, j1), sl("dy", j0, j1 - 1), sl("area", j0, j1 - 1), Re=RE)
            out["dx"], out["rx_max"] = own["dx"], own["rx_max"]
            if j1 < g["dy"].shape[0]:
                up = qo.grid_section(sl("x", j0, j1 + 2), sl("y", j0, j1 + 2), sl("dx", j0, j1 + 2), sl("dy", j0, j1 + 1), sl("area", j0, j1 + 1), Re=RE)
                out["ry_max"] = up["ry_max"]
    return out, sl("x", j0, c1 + 1), sl("y", j0, c1 + 1)


def check_sections(Q, g, starts, whole):
    names = ["S%d" % k for k in range(len(starts))]
    rep = report(Q, g, sections=list(zip(names, starts)))
    assert rep["grid"] == whole
    ends = list(starts[1:]) + [g["x"].shape[0]]
    for k, name in enumerate(names):
        last = k == len(names) - 1
        want, xs, ys = oracle_of_section(g, starts[k], ends[k], last)
        if last and ends[k] - starts[k] == 1:      # one point row and no cell: only dx and its ratio are there
            assert shifted(rep[name], -starts[k]) == want
            continue
        with np.errstate(all="ignore"):
            check_against_oracle(shifted(rep[name], -starts[k]), want, xs, ys)
    assert [jt["j"] for jt in rep["joints"]] == list(starts[1:])


@pytest.mark.parametrize("shear", [0.0, 0.5])
def test_every_split_into_two_sections_and_some_into_three(Q, shear):
    """65 point rows: the merged whole-grid section does not depend on the split, and every section is the oracle's on its slice"""
    g = G.quality_grid(64, 128, shear=shear)
    g["dx"][40, 100] *= 3.0          # something for the extrema to find away from row 0
    g["dy"][20, 127] *= 0.3
    whole = report(Q, g)["grid"]
    with np.errstate(all="ignore"):
        check_against_oracle(whole, oracle(g), g["x"], g["y"])
    for j1 in range(1, 65):
        check_sections(Q, g, (0, j1), whole)
    for a, b in ((1, 2), (1, 64), (31, 32), (32, 33), (32, 64), (20, 41), (33, 63), (63, 64)):
        check_sections(Q, g, (0, a, b), whole)


@pytest.mark.parametrize("j1", [1, 32, 33, 64])
def test_planted_seams(Q, j1):
    """the row a section dropped against the first row of the next: equal but for one point a known chord away, at the columns on
    either side of a tile edge and at i = nx.  The value is Re |P(seam) - P(first row)| from numpy, to the rounding of the unit vectors'
    components (a few 2^-53 each, 64 allowed as in delta_tolerance) times Re."""
    g = G.quality_grid(64, 128, shear=0.5)
    for i0 in (0, 126, 127, 128):
        for other in (None, 5):
            sx, sy = g["x"][j1].copy(), g["y"][j1].copy()
            sx[i0] += 1.0 / 64
            sy[i0] -= 1.0 / 128
            if other is not None:    # a smaller gap elsewhere does not win
                sx[other] += 1.0 / 256
            chord = np.linalg.norm(G.unit_vectors(sx[i0], sy[i0]) - G.unit_vectors(g["x"][j1, i0], g["y"][j1, i0]))
            for metrics in (True, False):
                rep = report(Q, g, metrics, sections=[("lower", 0), ("upper", j1)], seams=[(sx, sy)])
                (jt,) = rep["joints"]
                s = jt["seam_m"]
                assert (jt["lower"], jt["upper"], jt["j"]) == ("lower", "upper", j1)
                assert (s["j"], s["i"], s["lon"], s["lat"]) == (j1, i0, g["x"][j1, i0], g["y"][j1, i0])
                assert abs(s["value"] - RE * chord) <= RE * 64 * 2.0 ** -53
                assert (jt["ry"] is None) == (not metrics or j1 == 64)     # no cell row above the last point row: no dy to compare
    rep = report(Q, g, sections=[("lower", 0), ("upper", j1)], seams=[(g["x"][j1].copy(), g["y"][j1].copy())])
    s = rep["joints"][0]["seam_m"]
    assert (s["value"], s["j"], s["i"]) == (0.0, j1, 0)     # no gap anywhere: a tie of zeros, to the first column

"""Hand-made meshes and sources for tests/test_small_meshes_cpu.py and tests/test_gpu_small_meshes.py: cells, topologies and shapes the
grid generator never makes.  A plain module of builders (numpy only): a zoo of named cells in a one-row supergrid, four cuts of a
golden tripolar grid that are periodic and folded, folded only, periodic only and neither, regular regional grids of a few cells, and
sources with missing-value regions placed against the left column and the top row of a grid."""
import os

import numpy as np

RE = 6371.0e3
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_small_r0.25_even.npz")
TRUTH = os.path.join(HERE, "golden", "xgrid_truth.npz")
NAN = float("nan")

# (name, corner longitudes C0..C3, corner latitudes C0..C3): C0 south-west, C1 south-east, C2 north-east, C3 north-west of a
# well-formed cell.  The expected class of each is in ZOO_STATUS.
SPECIMENS = [
    ("ordinary", (9.0, 11.0, 11.0, 9.0), (11.0, 11.0, 13.0, 13.0)),               # inside the atmosphere cell 8..12 x 10..14
    ("on_edges", (16.0, 20.0, 20.0, 16.0), (14.0, 14.0, 18.0, 18.0)),             # exactly one atmosphere cell
    ("seam", (358.0, 362.0, 362.0, 358.0), (20.0, 20.0, 23.0, 23.0)),
    ("seam_m720", (-362.0, -358.0, -358.0, -362.0), (20.0, 20.0, 23.0, 23.0)),
    ("seam_p360", (718.0, 722.0, 722.0, 718.0), (20.0, 20.0, 23.0, 23.0)),
    ("north_corner", (30.0, 34.0, 34.0, 30.0), (86.0, 86.0, 90.0, 88.0)),
    ("south_corner", (40.0, 44.0, 44.0, 40.0), (-90.0, -87.0, -85.0, -86.0)),
    ("two_adjacent", (50.0, 54.0, 54.0, 50.0), (85.0, 85.0, 90.0, 90.0)),
    ("two_opposite", (70.0, 74.0, 74.0, 70.0), (-90.0, 0.0, 90.0, 0.0)),          # six vertices: the strip 70..74 from pole to pole
    ("three_poles", (80.0, 84.0, 84.0, 80.0), (87.0, 90.0, 90.0, 90.0)),
    ("four_poles", (90.0, 94.0, 94.0, 90.0), (90.0, 90.0, 90.0, 90.0)),
    ("enclosing", (0.0, 90.0, 180.0, 270.0), (89.0, 89.0, 89.0, 89.0)),
    ("clockwise", (100.0, 100.0, 102.0, 102.0), (10.0, 12.0, 12.0, 10.0)),
    ("point", (110.0, 110.0, 110.0, 110.0), (30.0, 30.0, 30.0, 30.0)),
    ("parallel", (120.0, 122.0, 122.0, 120.0), (40.0, 40.0, 40.0, 40.0)),
    ("bow_tie", (130.0, 134.0, 130.0, 134.0), (10.0, 10.0, 13.0, 16.0)),
    ("eps_inside", (140.0, 144.0, 144.0, 140.0), (86.0, 86.0, 90.0 - 5.0e-11, 88.0)),   # within POLE_EPS: a pole corner
    ("eps_outside", (150.0, 154.0, 154.0, 150.0), (86.0, 86.0, 90.0 - 2.0e-10, 88.0)),  # just outside: an ordinary corner
    ("nan_lat", (160.0, 164.0, 164.0, 160.0), (20.0, 20.0, NAN, 24.0)),
    ("nan_lon", (170.0, 174.0, NAN, 170.0), (-20.0, -20.0, -16.0, -16.0)),
    ("long", (181.0, 353.0, 353.0, 181.0), (75.0, 75.0, 87.0, 87.0)),              # 172 degrees wide: 44 x 4 atmosphere cells
]
# name -> (class, pole corners counted by pole_cells, kept entries against zoo_atmosphere() at threshold 0)
ZOO_STATUS = {
    "ordinary": ("ok", 0, 1), "on_edges": ("ok", 0, 1), "seam": ("ok", 0, 4), "seam_m720": ("ok", 0, 4), "seam_p360": ("ok", 0, 4),
    "north_corner": ("ok", 1, 2), "south_corner": ("ok", 1, 2), "two_adjacent": ("ok", 2, 4), "two_opposite": ("ok", 2, 90),
    "three_poles": ("degenerate", 3, 0), "four_poles": ("degenerate", 4, 0), "enclosing": ("pole", 0, 0),
    "clockwise": ("inverted", 0, 0), "point": ("inverted", 0, 0), "parallel": ("inverted", 0, 0),
    "bow_tie": ("ok", 0, 2),          # the larger lobe is counter-clockwise: a net positive area, clipped like any polygon
    "eps_inside": ("ok", 1, 1), "eps_outside": ("ok", 0, 2), "nan_lat": ("inverted", 0, 0), "nan_lon": ("inverted", 0, 0),
    "long": ("ok", 0, 176),
}


def zoo_atmosphere(kind="regular"):
    """the zoo's atmospheres: 90 x 45 regular cells of 4 degrees; non-uniform latitudes and a lon0 that is no multiple of anything;
    a single column (NA = 1); a single row (NB = 1)"""
    if kind == "regular":
        return 360.0 * np.arange(91) / 90, -90.0 + 180.0 * np.arange(46) / 45
    if kind == "gaussian":
        lat = 90.0 * np.sin(0.5 * np.pi * np.linspace(-1.0, 1.0, 41))
        lat[0], lat[-1] = -90.0, 90.0
        return -17.3 + 360.0 * np.arange(73) / 72, lat
    if kind == "one_column":
        return np.array([-20.0, 340.0]), -90.0 + 180.0 * np.arange(7) / 6
    if kind == "one_row":
        return 5.0 + 360.0 * np.arange(9) / 8, np.array([-90.0, 90.0])
    raise KeyError(kind)


def _midpoints(x):
    """the odd rows and columns of a supergrid from its even (corner) points: means of the two or four corners around them"""
    x[0::2, 1::2] = (x[0::2, 0:-1:2] + x[0::2, 2::2]) / 2.0
    x[1::2, 0::2] = (x[0:-1:2, 0::2] + x[2::2, 0::2]) / 2.0
    x[1::2, 1::2] = (x[1::2, 0:-1:2] + x[1::2, 2::2]) / 2.0
    return x


def cell_zoo():
    """x, y (3 x (2 nx + 1)) of one row of nx = 2 * len(SPECIMENS) - 1 model cells and {name: model column}: the even cells are the
    specimens, the odd cells between them whatever the shared corners make."""
    ns = len(SPECIMENS)
    nx = 2 * ns - 1
    x, y = np.zeros((3, 2 * nx + 1)), np.zeros((3, 2 * nx + 1))
    where = {}
    for k, (name, cx, cy) in enumerate(SPECIMENS):
        where[name] = 2 * k
        x[0, 4 * k], x[0, 4 * k + 2], x[2, 4 * k + 2], x[2, 4 * k] = cx
        y[0, 4 * k], y[0, 4 * k + 2], y[2, 4 * k + 2], y[2, 4 * k] = cy
    return _midpoints(x), _midpoints(y), where


def zoo_mask(nx):
    """a mask over the zoo's row that leaves out some specimens and some of the cells between them"""
    m = np.ones((1, nx), np.uint8)
    m[0, [1, 4, 10, 16, 23, 32, 38]] = 0
    return m


# ---- topologies ------------------------------------------------------------------------------------------------
CUTS = {"full": ((slice(None), slice(None)), (True, True)), "fold_only": ((slice(None), slice(8, -8)), (False, True)),
        "periodic_only": ((slice(None, -12), slice(None)), (True, False)), "neither": ((slice(None, -12), slice(8, -8)), (False, False))}


def topology_cuts():
    """{name: dict(x, y, area, angle_dx, topology)} of the four cuts of the golden 135 x 181 point tripolar grid"""
    g = np.load(GOLDEN)
    out = {}
    for name, ((sj, si), topo) in CUTS.items():
        x = np.ascontiguousarray(g["x"][sj, si])
        y = np.ascontiguousarray(g["y"][sj, si])
        ang = np.ascontiguousarray(g["angle_dx"][sj, si])
        area = np.ascontiguousarray(g["area"][:x.shape[0] - 1, (si.start or 0):(si.start or 0) + x.shape[1] - 1])
        out[name] = dict(x=x, y=y, area=area, angle_dx=ang, topology=topo)
    return out


# ---- shapes ----------------------------------------------------------------------------------------------------
def latlon_grid(ny, nx, lon0=-33.0, lat0=-21.0, dlon=3.0, dlat=2.0, fold=False):
    """A regular supergrid of ny x nx model cells of dlon x dlat degrees from (lon0, lat0): dict(x, y, area, angle_dx).  dlon * nx =
    360 gives a periodic band.  ``fold``: the top point row is bent onto itself reversed (point i takes the longitude of point
    nx - i on the left half's side), which detect_topology takes for a fold; with odd nx the middle cell is its own neighbour."""
    x, y = np.meshgrid(lon0 + 0.5 * dlon * np.arange(2 * nx + 1), lat0 + 0.5 * dlat * np.arange(2 * ny + 1))
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if fold:
        n = 2 * nx
        for i in range(n // 2 + 1, n + 1):
            x[-1, i] = x[-1, n - i]
    s = np.sin(np.radians(y[:, 0]))
    area = RE * RE * np.radians(0.5 * dlon) * np.tile((s[1:] - s[:-1])[:, None], (1, 2 * nx))
    return dict(x=x, y=y, area=np.ascontiguousarray(area), angle_dx=np.zeros_like(x))


SHAPES = {"1x1": (1, 1, {}), "1x63": (1, 63, {}), "1x64": (1, 64, {}), "1x65": (1, 65, {}), "129x1": (129, 1, dict(dlat=1.0, lat0=-64.5)),
          "3x3": (3, 3, {}), "band_2x1": (2, 1, dict(dlon=360.0, dlat=10.0)), "band_2x2": (2, 2, dict(dlon=180.0, dlat=10.0)),
          "band_3x1": (3, 1, dict(dlon=360.0, dlat=10.0)), "band_3x2": (3, 2, dict(dlon=180.0, dlat=10.0)),
          "fold_5x7": (5, 7, dict(fold=True, lat0=50.0))}
# what detect_topology makes of them (the others: (False, False)).  The three top points of the 2 x 2 band are lon0, lon0 + 180 and
# lon0 + 360: a row that maps onto itself reversed, so the band counts as folded too.
SHAPE_TOPOLOGY = {"band_2x1": (True, False), "band_2x2": (True, True), "band_3x1": (True, False), "band_3x2": (True, True),
                  "fold_5x7": (False, True)}


def shape_grid(name):
    ny, nx, kw = SHAPES[name]
    return latlon_grid(ny, nx, **kw)


# ---- sources ---------------------------------------------------------------------------------------------------
SOURCE_SHAPES = {"1x1": (1, 1), "1x5": (1, 5), "3x2": (3, 2), "7x1": (7, 1), "over_lds": (8000, 400), "nonuniform": (40, 24),
                 "regular": (90, 45)}


def source_edges(kind):
    """lon (NA + 1) and lat (NB + 1) edges of the source shapes (NA, NB); "nonuniform": latitudes bunched at the equator, not reaching
    the poles, and a lon0 that is no multiple of the spacing"""
    NA, NB = SOURCE_SHAPES[kind]
    if kind == "nonuniform":
        return -17.3 + 360.0 * np.arange(NA + 1) / NA, 88.0 * np.sin(0.5 * np.pi * np.linspace(-1.0, 1.0, NB + 1))
    if kind == "regular":
        return 360.0 * np.arange(NA + 1) / NA, -90.0 + 180.0 * np.arange(NB + 1) / NB
    lon = -300.0 + 360.0 * np.arange(NA + 1) / NA
    lon[-1] = lon[0] + 360.0
    return lon, -90.0 + 180.0 * np.arange(NB + 1) / NB


def smooth_field(lon, lat, nrec, dtype):
    lc, pc = np.radians(0.5 * (lon[1:] + lon[:-1])), np.radians(0.5 * (lat[1:] + lat[:-1]))
    L, P = np.meshgrid(lc, pc)
    return np.stack([np.cos(P) * (20 + r) + 3 * np.sin(3 * L + r) * np.cos(2 * P) + 0.25 * r for r in range(nrec)]).astype(dtype)


def cells_holding(lon, lat, px, py):
    """bool (NB, NA): the source cells that hold one of the points (px, py)"""
    NA, NB = lon.size - 1, lat.size - 1
    px, py = np.asarray(px, np.float64).reshape(-1), np.asarray(py, np.float64).reshape(-1)
    ok = np.isfinite(px) & np.isfinite(py)
    t = lon[0] + np.mod(px[ok] - lon[0], 360.0)
    I = np.clip(np.searchsorted(lon, t, side="right") - 1, 0, NA - 1)
    J = np.clip(np.searchsorted(lat, py[ok], side="right") - 1, 0, NB - 1)
    m = np.zeros((NB, NA), bool)
    m[J, I] = True
    return m


def edge_region(x, y, columns=2, rows=2):
    """the supergrid points of the model cells of the left ``columns`` columns (all rows) and of the top ``rows`` rows over the left
    half of the columns: where the sources below are missing and the runoff tests' land lies"""
    nxp = x.shape[1]
    sel = np.zeros(x.shape, bool)
    sel[:, :2 * columns + 1] = True
    sel[x.shape[0] - 1 - 2 * rows:, :(nxp // 2) + 1] = True
    return x[sel], y[sel]


def source_for(x, y, kind="nonuniform", nrec=1, dtype=np.float64, two_fills=False):
    """(data (nrec, NB, NA), lon, lat, fills) of a smooth source that is missing where the left columns and the left half of the top
    rows of the grid x, y lie (edge_region), more of it in later records.  With ``two_fills`` the missing cells hold, in turn, NaN, the
    fill value -999 and the fill value 1e20; otherwise NaN."""
    lon, lat = source_edges(kind)
    f = smooth_field(lon, lat, nrec, dtype)
    for r in range(nrec):
        px, py = edge_region(x, y, columns=2 + r % 2, rows=2 + r % 3)
        m = cells_holding(lon, lat, px, py)
        if two_fills:
            J, I = np.nonzero(m)
            for k, v in enumerate((np.nan, -999.0, 1.0e20)):
                f[r][J[k::3], I[k::3]] = v
        else:
            f[r][m] = np.nan
    return f, lon, lat, ((-999.0, 1.0e20) if two_fills else ())


def source_with_holes(x, y, nrec=1, dtype=np.float64):
    """(data, lon, lat, fills) of the smooth "regular" source (4-degree cells) with one hole per record: the cells whose centres lie
    within 1.01 cells of one h point of the grid x, y, so that all four nodes around that point are missing and the point is left to
    the fill, while an h point 10 degrees away keeps all of its nodes.  Record r takes the point (j, i) = ((r + 1) % ny, r % nx).  On
    grids of one or two columns, where the left-column region of source_for() is the whole grid, this leaves points to fill from."""
    lon, lat = source_edges("regular")
    f = smooth_field(lon, lat, nrec, dtype)
    lc, pc = 0.5 * (lon[1:] + lon[:-1]), 0.5 * (lat[1:] + lat[:-1])
    xh, yh = x[1::2, 1::2], y[1::2, 1::2]
    ny, nx = xh.shape
    for r in range(nrec):
        px, py = xh[(r + 1) % ny, r % nx], yh[(r + 1) % ny, r % nx]
        dl = np.abs(np.mod(lc - px + 180.0, 360.0) - 180.0)
        f[r][np.ix_(np.abs(pc - py) <= 1.01 * 4.0, dl <= 1.01 * 4.0)] = np.nan
    return f, lon, lat, ()


def synthetic_flags(ny, nx, nrec, seed):
    """values and flags (nrec, ny, nx) for the fill step alone: a third remapped (flag 1), a tenth dry (0), the rest unfilled (3,
    value 1e20)"""
    rng = np.random.default_rng(seed)
    u = rng.random((nrec, ny, nx))
    fl = np.where(u < 0.33, 1, np.where(u < 0.43, 0, 3)).astype(np.uint8)
    fl[:, 0, 0] = 1
    v = np.where(fl == 1, 10.0 * rng.random((nrec, ny, nx)), 1.0e20)
    return v, fl


def wet_mask(ny, nx):
    """a wet mask of ny x nx model cells with land touching the left column and the top row (and, on grids large enough, an island)"""
    wet = np.ones((ny, nx), np.uint8)
    wet[ny // 4: ny // 2 + 1, 0: max(1, nx // 16)] = 0
    wet[ny - max(1, ny // 16):, nx // 8: nx // 3 + 1] = 0
    if ny > 8 and nx > 8:
        wet[ny // 2 + 2: ny // 2 + 5, nx // 2: nx // 2 + 3] = 0
    if not wet.any():
        wet[0, 0] = 1
    return wet

"""Hand-made grids and rasters for tests/test_small_grids_cpu.py, tests/test_gpu_small_topog.py and tests/test_gpu_small_quality.py:
inputs for topography by refined sampling and for the grid-quality report that the grid generator never makes.  A plain module of
builders (numpy only), next to tests/small_meshes.py, whose cell zoo it reuses.

Topography grids are (x, y) point arrays of ny x nx SUPERGRID cells.  Unless a builder says otherwise every coordinate is a multiple
of 1/8 degree, so that with a power-of-two refinement every bilinear weight, every sample position and every raster index is exact in
fp64: results can then be stated in closed form, and mirrored or shifted grids must give identical records."""
import functools

import numpy as np

from small_meshes import NAN, RE, SPECIMENS

INF = float("inf")
GLOBAL_BOX = (-180.0, 0.25, -90.0, 0.25)            # the 720 x 1440 rasters
WINDOW = (slice(320, 440), slice(1120, 1320))       # rows, columns of the big raster: 100E .. 150E, 10S .. 20N
WINDOW_BOX = (100.0, 0.25, -10.0, 0.25)
HOME = dict(lon0=104.0, lat0=-4.0)                  # where the shapes sit: inside the window


# ---- topography grids ------------------------------------------------------------------------------------------
def grid(ny, nx, lon0=104.0, lat0=-4.0, d=1.0, shear=False):
    """x, y ((ny + 1) x (nx + 1)) of ny x nx supergrid cells of d x d degrees from (lon0, lat0); ``shear``: x += j / 8."""
    x, y = np.meshgrid(lon0 + d * np.arange(nx + 1), lat0 + d * np.arange(ny + 1))
    if shear:
        x = x + np.arange(ny + 1)[:, None] / 8.0
    return np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)


# name -> (ny, nx, keywords of grid()), in supergrid cells
TOPOG_SHAPES = {"1x1": (1, 1, {}), "2x2": (2, 2, {}), "1x63": (1, 63, {}), "1x64": (1, 64, {}), "1x65": (1, 65, {}), "5x3": (5, 3, {}),
                "6x8s": (6, 8, dict(shear=True)), "129x1": (129, 1, dict(lat0=-64.5))}


def shape_grid(name, **kw):
    ny, nx, k = TOPOG_SHAPES[name]
    return grid(ny, nx, **dict(k, **kw))


# where the sheared 6 x 8 grid is put: name -> keywords of grid()
PLACEMENTS = {
    "home": {},
    "across_180": dict(lon0=176.0),                 # 176 .. 184.75: the seam of the global rasters (lon0 = -180)
    "across_window_lon0": dict(lon0=96.0),          # 96 .. 104.75: the west edge of the window
    "across_window_east": dict(lon0=146.0),
    "m360": dict(lon0=104.0 - 360.0), "p360": dict(lon0=104.0 + 360.0), "m720": dict(lon0=104.0 - 720.0),
    "p720": dict(lon0=104.0 + 720.0), "p3600": dict(lon0=104.0 + 3600.0),
    "above_window": dict(lat0=17.0),                # 17 .. 23: across the window's top (20N)
    "below_window": dict(lat0=-13.0),
    "above_band60": dict(lat0=57.0),                # across 60N, where the -60 .. 60 periodic raster stops
    "below_band60": dict(lat0=-63.0),
}


def placed(name):
    return grid(6, 8, shear=True, **PLACEMENTS[name])


def beyond_pole_row(sign=1):
    """One hand-made row of four cells whose far point row lies at |y| = 95, past the pole."""
    x, y = grid(1, 4, lon0=104.0, lat0=85.0, d=2.0)
    y[1] = 95.0
    return (x, y) if sign > 0 else (x, np.ascontiguousarray(-y[::-1]))


def _cell(cx, cy):
    """a one-cell grid from the corners C0 (south-west), C1 (south-east), C2 (north-east), C3 (north-west)"""
    return np.array([[cx[0], cx[1]], [cx[3], cx[2]]], dtype=np.float64), np.array([[cy[0], cy[1]], [cy[3], cy[2]]], dtype=np.float64)


def pole_block():
    """3 x 3 points on a plane tangent at the north pole, (u, v) in {-1, 1, 3} x {-1, 1, 3} (1 unit = 1 degree of colatitude): of
    the 2 x 2 cells exactly the first encloses the pole.  Not on the 1/8-degree lattice."""
    u, v = np.meshgrid(np.array([-1.0, 1.0, 3.0]), np.array([-1.0, 1.0, 3.0]))
    return np.ascontiguousarray(np.degrees(np.arctan2(v, u))), np.ascontiguousarray(90.0 - np.hypot(u, v))


def pole_cells():
    """{name: (x, y, number of pole-enclosing supergrid cells)}: cells that enclose a pole or touch it with one or two corners."""
    out = {"south_enclosing": (np.array([[0.0, 90.0], [270.0, 180.0]]), np.full((2, 2), -89.0), 1),
           "north_enclosing": (np.array([[0.0, 90.0], [270.0, 180.0]]), np.full((2, 2), 89.0), 1)}
    x, y = pole_block()
    out["north_block"] = (x, y, 1)
    out["south_block"] = (x, -y, 1)
    for r in (0, 1):
        for c in (0, 1):
            x, y = grid(1, 1, lon0=30.0, lat0=88.0, d=1.0)
            y[r, c] = 90.0
            out["north_corner_%d%d" % (r, c)] = (x, y, 0)
            out["south_corner_%d%d" % (r, c)] = (x, -y, 0)
        x, y = grid(1, 1, lon0=50.0, lat0=86.0, d=2.0)
        y[r, :] = 90.0
        out["north_row_%d" % r] = (x, y, 0)
        out["south_row_%d" % r] = (x, -y, 0)
    return out


def odd_cells():
    """{name: (x, y)} of one-cell grids: clockwise, collapsed to a point (R = 1), a bow-tie, exactly 180 degrees wide (the unwrap
    takes +180 for -180), and wider than 180 degrees (unwrapped the short way round)."""
    zoo = {n: (cx, cy) for n, cx, cy in SPECIMENS}
    out = {n: _cell(*zoo[n]) for n in ("clockwise", "point", "bow_tie")}
    out["wide_180"] = _cell((0.0, 180.0, 180.0, 0.0), (10.0, 10.0, 12.0, 12.0))
    out["wider_200"] = _cell((0.0, 200.0, 200.0, 0.0), (10.0, 10.0, 12.0, 12.0))
    return out


NONFINITE = {"nan": NAN, "pinf": INF, "minf": -INF}
NONFINITE_POINT = (3, 4)    # corner 11 of cell (2, 3), 10 of (2, 4), 01 of (3, 3) and 00 of (3, 4): each position once


def nonfinite_grid(coord, value):
    """the sheared 6 x 8 grid at home with one point's x or y replaced: (x, y, the four cells that have it as a corner)"""
    x, y = placed("home")
    (x if coord == "x" else y)[NONFINITE_POINT] = NONFINITE[value]
    j, i = NONFINITE_POINT
    return x, y, [(j - 1, i - 1), (j - 1, i), (j, i - 1), (j, i)]


# ---- rasters ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    z = np.random.default_rng(20240607).integers(-6000, 6000, size=(720, 1440)).astype(np.int16)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _float_base(quantum):
    """360 x 720 values (0.5 degree, periodic) every one of which lies exactly half-way between two integer steps where quantum
    is a power of two ((k + 0.5) * quantum); and the masks of NaN, first and second fill"""
    rng = np.random.default_rng(77)
    k = rng.integers(-4000, 4000, size=(360, 720))
    v = (k + 0.5) * quantum
    u = rng.random((360, 720))
    return v, (u < 0.03), (u >= 0.03) & (u < 0.06), (u >= 0.06) & (u < 0.09)


def raster(kind):
    """dict(data, box=(lon0, dlon, lat0, dlat), fill, quantum) of the raster ``kind`` (RASTER_KINDS, INDEX_RASTERS, or
    "const_p" / "const_m")."""
    fill, quantum = (), None
    big = _big()
    if kind == "int16":
        data, box = big, GLOBAL_BOX
    elif kind in ("int16_fill1", "int16_fill2"):
        data, box = big.copy(), GLOBAL_BOX
        u = np.random.default_rng(5).random(big.shape)
        data[u < 0.05] = -32768
        fill = (-32768.0,)
        if kind == "int16_fill2":
            data[u > 0.95] = 32767
            fill = (-32768.0, 32767.0)
    elif kind == "band60":              # periodic, but only 60S .. 60N: latitudes beyond it are clamped to its edge rows
        data, box = np.ascontiguousarray(big[120:600]), (-180.0, 0.25, -60.0, 0.25)
    elif kind == "1x1_global":
        data, box = np.array([[-1234]], dtype=np.int16), (-180.0, 360.0, -90.0, 180.0)
    elif kind == "1x1_regional":
        data, box = np.array([[777]], dtype=np.int16), (105.0, 3.0, -2.0, 3.0)
    elif kind == "nx1":
        data, box = np.ascontiguousarray(big[:16, :1]), (104.0, 5.0, -4.0, 0.5)
    elif kind == "ny1":
        data, box = np.ascontiguousarray(big[:1, :16]), (102.0, 0.5, -3.0, 4.0)
    elif kind in ("window", "window_p360", "window_m360"):
        data = np.ascontiguousarray(big[WINDOW])
        box = (WINDOW_BOX[0] + {"window": 0.0, "window_p360": 360.0, "window_m360": -360.0}[kind],) + WINDOW_BOX[1:]
    elif kind.startswith("float"):      # float32_q0.5, float64_q0.01, ...
        dtype, q = kind.split("_q")
        quantum = float(q)
        v, m_nan, m_f0, m_f1 = _float_base(quantum)
        data = v.astype(np.float32 if dtype == "float32" else np.float64)
        data[m_nan], data[m_f0], data[m_f1] = np.nan, -999.0, 1.0e20
        data[LIMIT_ELEMENTS[0]], data[LIMIT_ELEMENTS[1]] = 2.0 ** 21 * quantum, -(2.0 ** 21) * quantum   # the largest |q| accepted
        box, fill = (-180.0, 0.5, -90.0, 0.5), (-999.0, 1.0e20)
    elif kind in INDEX_RASTERS:
        js, is_ = np.meshgrid(np.arange(720), np.arange(1440), indexing="ij")
        data, box = {"index_js": js, "index_is": is_ % 251, "index_sum": js + is_}[kind].astype(np.int16), GLOBAL_BOX
    elif kind in ("const_p", "const_m"):
        data = np.full((1, 1), 2.0 ** 21 if kind == "const_p" else -(2.0 ** 21))
        box, quantum = (-180.0, 360.0, -90.0, 180.0), 1.0
    else:
        raise KeyError(kind)
    return dict(data=data, box=box, fill=fill, quantum=quantum)


LIMIT_ELEMENTS = ((100, 568), (101, 568))    # 104E .. 104.5E, 40S .. 39S of the float rasters: +-2^21 * quantum


def limit_grid():
    """two cells, one over each of LIMIT_ELEMENTS"""
    return grid(2, 1, lon0=104.0, lat0=-40.0, d=0.5)


INDEX_RASTERS = ("index_js", "index_is", "index_sum")
FLOAT_RASTERS = ("float32_q0.5", "float32_q0.01", "float64_q0.5", "float64_q0.01")
RASTER_KINDS = ("int16", "int16_fill1", "int16_fill2", "band60", "1x1_global", "1x1_regional", "nx1", "ny1", "window", "window_p360",
                "window_m360") + FLOAT_RASTERS
REGIONAL_KINDS = ("1x1_regional", "nx1", "ny1", "window", "window_p360", "window_m360")


def index_value(kind, js, is_):
    return {"index_js": js, "index_is": is_ % 251, "index_sum": js + is_}[kind]


def index_truth(kind, lon8, lat8, R):
    """Python-integer record (n, sum, sumsq, min, max) of one d = 1 degree supergrid cell whose south-west corner is (lon8 / 8,
    lat8 / 8) degrees, both multiples of 1/4 degree, over an index raster (0.25 degree from -180, -90), R a power of two >= 2:
    sample a sits (2 a + 1) / (2 R) degrees east of the corner, i.e. (4 a + 2) // R quarter-degree columns."""
    assert lon8 % 2 == 0 and lat8 % 2 == 0 and R >= 2 and R & (R - 1) == 0
    i0, j0 = ((lon8 + 180 * 8) // 2) % 1440, (lat8 + 90 * 8) // 2
    vals = [index_value(kind, j0 + (4 * b + 2) // R, (i0 + (4 * a + 2) // R) % 1440) for b in range(R) for a in range(R)]
    return len(vals), sum(vals), sum(v * v for v in vals), min(vals), max(vals)


# ---- grids for the quality report ------------------------------------------------------------------------------
def unit_vectors(x, y):
    lam, phi = np.deg2rad(x), np.deg2rad(y)
    return np.stack((np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)), axis=-1)


def metrics_from_chords(x, y):
    """dx (nyp x nx), dy (ny x nxp) as chord lengths in metres and area (ny x nx) as the product of the mean sides"""
    P = unit_vectors(x, y)
    dx = RE * np.linalg.norm(P[:, 1:] - P[:, :-1], axis=-1)
    dy = RE * np.linalg.norm(P[1:, :] - P[:-1, :], axis=-1)
    area = 0.25 * (dx[:-1] + dx[1:]) * (dy[:, :-1] + dy[:, 1:])
    return np.ascontiguousarray(dx), np.ascontiguousarray(dy), np.ascontiguousarray(area)


def quality_grid(ny, nx, shear=0.0, lon0=10.0, lat0=-20.0, d=0.25):
    """dict(x, y, dx, dy, area) of ny x nx cells of d degrees; column i is displaced east by shear[i] * (y - lat0) (a number: every
    column alike, a sheared grid; zero: a lat-lon grid)"""
    j, i = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    s = np.broadcast_to(np.asarray(shear, dtype=np.float64), (nx + 1,))
    x = np.ascontiguousarray(lon0 + d * i + s[None, :] * (d * j))
    y = np.ascontiguousarray(lat0 + d * j.astype(np.float64))
    dx, dy, area = metrics_from_chords(x, y)
    return dict(x=x, y=y, dx=dx, dy=dy, area=area)


# (ny, nx) in cells: every nx of {1, 2, 126, 127, 128, 253, 254, 255} around the 127-column tiles and every ny of {1, 2, 31, 32, 33,
# 64, 65} around the 32-row tiles
QUALITY_PAIRS = [(1, 1), (1, 127), (2, 2), (2, 254), (31, 126), (31, 255), (32, 127), (32, 128), (33, 253), (33, 1), (64, 128), (64, 126),
                 (65, 2), (65, 255)]


def quality_shape(ny, nx):
    """the grid of a pair: every second pair sheared"""
    k = QUALITY_PAIRS.index((ny, nx))
    return quality_grid(ny, nx, shear=0.5 if k % 2 else 0.0)


# The chord along a parallel leaves its point (dlon / 2) sin(lat) off due east, so a lat-lon grid of 0.25 degrees is orthogonal on the
# equator only (bin 0, below 1e-6 degrees), 5e-4 degrees off one row away from it (bin 1) and 1e-3 .. 0.1 degrees off elsewhere (bin
# 2); these shears put the corners of their columns into the bins above 0.1, 1, 5 and 20 degrees
SEVEN_SHEARS = (0.0, 0.0, 8.0e-3, 5.0e-2, 0.2, 1.0, 0.0)


def seven_bins_grid(ny=33, group=20):
    """33 x 140 cells from 1S, row 4 on the equator, in seven groups of 20 columns, each group with its own shear: two tiles
    across, two down, and every bin of the delta histogram occupied"""
    shear = np.repeat(np.asarray(SEVEN_SHEARS), group)
    shear = np.concatenate([shear, shear[-1:]])
    return quality_grid(ny, shear.size - 1, shear=shear, lat0=-1.0)


def planted_base():
    """40 x 140 cells (41 x 141 points): columns 0 .. 126 and rows 0 .. 31 are the first tile; sheared a little so no two metrics tie"""
    return quality_grid(40, 140, shear=0.125)

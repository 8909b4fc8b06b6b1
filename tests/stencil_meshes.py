"""The meshes of the generic stencil's truth fixtures (plain numpy and the numpy oracle; used by scripts/truth_table.py --groups stencil, which
STORES each mesh beside its truth -- the caps come out of tan / atan / acos, whose last bit is the host's -- and by the tests, which read the
stored bits and hold this builder to them).

  bipolar    a bipolar cap of 257 x 12 points: the fold row (the top row, where columns i and Ni - i coincide), the two pole points at exactly
             90 degrees (top row, columns 64 and 192), the seam (columns 0 and 256 are the same meridian, 360 degrees apart) and the kernel's
             column-tile edge 255 | 256
  dpole      a displaced-pole cap of 261 x 12 points: the pole row (row 0, every point the displaced pole itself: dx and the angle are exactly 0) and longitudes unwrapped below -300
  turns      a smooth curvilinear mesh of 515 x 8 points whose longitudes are moved by whole turns, -720 .. +720 degrees, point by point
  edge       259 x 9 points: rows at exactly -90 and +90 degrees and 1e-10 degrees inside them, an equator row of +0.0 and -0.0 in pairs, two
             rows with the same latitudes (dy is exactly +0.0 where their longitudes agree too: the even columns), and two columns (100, 101)
             that hold the same point in every row (dx there is exactly +0.0)

WINDOWS are rectangles of these meshes, each a mesh of its own (the one-sided angle at its first and last column, and the rows its last cell
row needs, are the window's): shapes (1, 2) .. (7, 513), row counts on either side of each tile height in use, widths on either side of the
kernel's 256-column tile.
"""
import numpy as np

from oracle import ogg_oracle as orc

MESHES = ("bipolar", "dpole", "turns", "edge")
# name -> (mesh, first row, first column, rows, columns)
WINDOWS = {"w1x2": ("bipolar", 11, 64, 1, 2),            # the fold row at a pole point
           "w2x2": ("dpole", 0, 0, 2, 2),                # the pole row
           "w2x3": ("turns", 0, 100, 2, 3),
           "w1x257": ("bipolar", 11, 0, 1, 257),         # the fold row alone
           "w3x255": ("dpole", 0, 3, 3, 255),
           "w3x256": ("turns", 2, 0, 3, 256),
           "w3x257": ("edge", 6, 0, 3, 257),             # the rows up to +90 degrees
           "w3x258": ("turns", 5, 1, 3, 258),
           "w7x513": ("turns", 1, 1, 7, 513)}
WINDOW_SHAPES = [(1, 2), (2, 2), (2, 3), (1, 257), (3, 255), (3, 256), (3, 257), (3, 258), (7, 513)]
ZERO_DX_COLUMNS = (100, 101)
ZERO_DY_ROWS = (4, 5)


def bipolar():
    x, y, _, _ = orc.generate_bipolar_cap_mesh(256, 11, 65.0, -300.0, ensure_nj_even=False)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def dpole():
    x, y, _, _ = orc.generate_displaced_pole_grid(260, 11, -300.0, -78.0, 80.0, 0.2)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def turns():
    nj, ni = 8, 515
    rng = np.random.default_rng(720)
    u = np.arange(ni)[None, :] / (ni - 1.0)
    v = np.arange(nj)[:, None] / (nj - 1.0)
    x = -300.0 + 340.0 * u + 9.0 * np.sin(2.0 * np.pi * (u + 0.37 * v)) + 4.0 * v
    y = -70.0 + 150.0 * v + 6.0 * np.cos(2.0 * np.pi * (1.5 * u + v)) + 3.0 * u
    k = rng.integers(-2, 3, size=(nj, ni))
    k[0, :5] = (-2, 2, 0, -2, 2)                          # the extremes side by side: 1440 degrees between two neighbours
    return np.ascontiguousarray(x + 360.0 * k), np.ascontiguousarray(y + 0.0 * u)


def edge():
    ni = 259
    rng = np.random.default_rng(90)
    lat = np.array([-90.0, -(90.0 - 1e-10), -60.0, 0.0, 20.0, 20.0, 60.0, 90.0 - 1e-10, 90.0])
    x = np.tile(-300.0 + np.arange(ni) * (360.0 / (ni - 1.0)), (lat.size, 1))
    y = np.tile(lat[:, None], (1, ni))
    x[2] += rng.uniform(-0.3, 0.3, ni)
    y[2] += rng.uniform(-0.3, 0.3, ni)
    x[6] += rng.uniform(-0.3, 0.3, ni)
    y[6] += rng.uniform(-0.3, 0.3, ni)
    y[3, np.arange(ni) % 4 >= 2] = -0.0                   # +0.0, +0.0, -0.0, -0.0, ... along the equator: N = y[i+1] - y[i-1] is -0.0 at every other point
    noise = rng.uniform(-0.2, 0.2, ni)
    y[4] += noise
    y[5] += noise                                         # the same latitudes in rows 4 and 5, point by point
    x[5, 1::2] += 0.125                                   # ... and the same longitudes at the even columns only
    x[:, ZERO_DX_COLUMNS[1]] = x[:, ZERO_DX_COLUMNS[0]]
    y[:, ZERO_DX_COLUMNS[1]] = np.where(y[:, ZERO_DX_COLUMNS[0]] == 0.0, y[:, ZERO_DX_COLUMNS[1]], y[:, ZERO_DX_COLUMNS[0]])   # the equator keeps its -0.0
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


BUILDERS = {"bipolar": bipolar, "dpole": dpole, "turns": turns, "edge": edge}


def window(meshes, name):
    """(x, y) of the window `name`, contiguous copies, from {mesh: (x, y)}."""
    m, j0, i0, nj, ni = WINDOWS[name]
    x, y = meshes[m]
    assert j0 + nj <= x.shape[0] and i0 + ni <= x.shape[1], (name, x.shape)
    return np.ascontiguousarray(x[j0:j0 + nj, i0:i0 + ni]), np.ascontiguousarray(y[j0:j0 + nj, i0:i0 + ni])


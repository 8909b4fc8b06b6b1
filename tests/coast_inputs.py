"""Hand-made inputs of the distance-to-the-coast tests (tests/test_coast_distance_cpu.py checks on the CPU that each reaches the branch
it is named for; tests/test_gpu_small_coast.py runs them on the device): grids from tests/small_meshes.py whose cell centres, the
(odd, odd) supergrid points, are written directly.  A plain module of builders (numpy only).  Each returns dict(x, y, wet, periodic,
fold)."""
import numpy as np

import small_meshes as SM


def _case(g, wet, periodic=False, fold=False):
    return dict(x=g["x"], y=g["y"], wet=np.ascontiguousarray(wet, dtype=np.uint8), periodic=periodic, fold=fold)


def exact_tie():
    """3 x 5 cells, two land cells (1, 1) and (1, 3) whose centres hold identical (lon, lat): every wet cell is exactly as far from
    the one as from the other, and the smaller cell, 6, wins"""
    g = SM.latlon_grid(3, 5)
    wet = np.ones((3, 5), np.uint8)
    wet[1, 1] = wet[1, 3] = 0
    for i in (1, 3):
        g["x"][3, 2 * i + 1], g["y"][3, 2 * i + 1] = -25.5, -18.0
    return _case(g, wet)


def pole_near_ties():
    """3 x 8 cells whose top row is land with every centre at latitude 90 and its own longitude: cos(90 D) is 6e-17, not 0, so the
    eight centres differ in the 17th digit only"""
    g = SM.latlon_grid(3, 8, lat0=78.0, dlat=4.0, dlon=45.0, lon0=-180.0)
    g["y"][5, 1::2] = 90.0
    wet = np.ones((3, 8), np.uint8)
    wet[2] = 0
    return _case(g, wet, periodic=True)


def invalid_centres():
    """4 x 6 cells: the land cell (1, 2) has a NaN longitude and the wet cell (2, 4) an infinite latitude; (3, 0) is ordinary land"""
    g = SM.latlon_grid(4, 6)
    wet = np.ones((4, 6), np.uint8)
    wet[1, 2] = wet[3, 0] = 0
    g["x"][3, 5] = np.nan
    g["y"][5, 9] = np.inf
    return _case(g, wet)


def random_centres(seed=5, ny=20, nx=24):
    """ny x nx cells with centres scattered uniformly over the sphere and a random half of them wet: index neighbours are not
    neighbours on the sphere, and every tile's ball covers more than a hemisphere"""
    rng = np.random.default_rng(seed)
    g = SM.latlon_grid(ny, nx)
    g["x"][1::2, 1::2] = rng.uniform(-180.0, 180.0, (ny, nx))
    g["y"][1::2, 1::2] = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, (ny, nx))))
    return _case(g, rng.random((ny, nx)) < 0.5)


def seam_band():
    """a periodic band of 8 x 36 cells of 10 degrees whose only land is the column next to last: for the cells of the first columns
    the coast lies across the seam, 350 degrees away in index space and 20 degrees away on the sphere"""
    g = SM.latlon_grid(8, 36, lon0=-180.0, lat0=-20.0, dlon=10.0, dlat=5.0)
    wet = np.ones((8, 36), np.uint8)
    wet[:, 34] = 0
    return _case(g, wet, periodic=True)


def antipodal():
    """1 x 4 cells: the only land cell, 0, at (10, 20); the wet cell 1 at its antipode (190, -20), d2 next to 4"""
    g = SM.latlon_grid(1, 4)
    g["x"][1, 1::2] = [10.0, 190.0, 100.0, -80.0]
    g["y"][1, 1::2] = [20.0, -20.0, 0.0, 45.0]
    return _case(g, [[0, 1, 1, 1]])


def coast_of(n, ny=12, nx=40):
    """ny x nx cells with exactly n coastal land cells: n isolated land cells on every other column of every other row"""
    g = SM.latlon_grid(ny, nx, dlon=1.0, dlat=1.0)
    wet = np.ones((ny, nx), np.uint8)
    spots = [(j, i) for j in range(1, ny - 1, 2) for i in range(1, nx - 1, 2)]
    assert n <= len(spots)
    for j, i in spots[:n]:
        wet[j, i] = 0
    return _case(g, wet)


CASES = {"exact_tie": exact_tie, "pole_near_ties": pole_near_ties, "invalid_centres": invalid_centres, "random_centres": random_centres,
         "seam_band": seam_band, "antipodal": antipodal}


def tile_balls(u, fl, wet_bit, TY=16, TX=16):
    """the radius of every tile's ball as the search forms it: the queries (valid, wet bit ``wet_bit``) of each tile of TY x TX cells,
    m the middle of their bounding box, r the largest |p - m|.  [(tile j, tile i, r, m)] of the tiles that hold a query."""
    ny, nx = fl.shape
    u = np.asarray(u).reshape(ny, nx, 3)
    out = []
    for tj in range(0, ny, TY):
        for ti in range(0, nx, TX):
            f = fl[tj:tj + TY, ti:ti + TX]
            q = ((f & 4) != 0) & ((f & 1) == wet_bit)
            if q.any():
                p = u[tj:tj + TY, ti:ti + TX][q]
                m = 0.5 * (p.min(axis=0) + p.max(axis=0))
                out.append((tj // TY, ti // TX, float(np.sqrt(((p - m) ** 2).sum(axis=1).max())), m))
    return out

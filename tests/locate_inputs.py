"""What tests/test_gpu_locate.py and tests/test_gpu_small_locate.py share: the device's point location held to the definition of
tests/locate_definition.py on the device's own corner table and query vectors, bit for bit and at every point, and query sets on the
special lines of a grid.  Test infrastructure only."""
import numpy as np

import locate_definition as D

MODES = {"cell": D.CELL, "bilinear": D.BILINEAR}


def shape_of(x):
    return (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def check(LOC, x, y, lon, lat, periodic, fold, field=None, wet=None, mode="bilinear", fills=(), xy_dev=None):
    """locate_dev (and with ``field`` the sample step) on the grid x, y and the points lon, lat, every output compared with the
    definition: cu canonical and within a few ulp of numpy's, cell, s, t, m, values and flags bit for bit, the counts."""
    ny, nx = shape_of(x)
    lon, lat = np.asarray(lon, np.float64).reshape(-1), np.asarray(lat, np.float64).reshape(-1)
    dx, dy = xy_dev if xy_dev is not None else (to_device(x), to_device(y))
    res = LOC.locate_dev(dx, dy, lon, lat, periodic=periodic, fold=fold, keep_vectors=True, field=field, wet=wet, mode=mode,
                         fill_values=fills)
    cu, qu = res["cu"], res["qu"]
    assert D.is_canonical(cu, ny, nx, periodic, fold)
    want_cu = D.corner_table(x, y, periodic, fold)
    ok = np.isfinite(want_cu).all(axis=1)
    assert np.array_equal(np.isfinite(cu).all(axis=1), ok) and np.max(np.abs(cu[ok] - want_cu[ok]), initial=0.0) <= 4e-16
    want_qu = D.unit(lon, lat)
    okq = np.isfinite(want_qu).all(axis=1)
    assert np.array_equal(np.isfinite(qu).all(axis=1), okq) and np.max(np.abs(qu[okq] - want_qu[okq]), initial=0.0) <= 4e-16
    cell, s, t, m = D.locate(cu, qu, ny, nx)
    bad = np.nonzero(res["cell"] != cell)[0]
    assert bad.size == 0, (bad[:5], res["cell"][bad[:5]], cell[bad[:5]], lon[bad[:5]], lat[bad[:5]])
    for k, v in (("s", s), ("t", t), ("margin", m)):
        assert res[k].tobytes() == v.tobytes(), (k, np.nonzero(~((res[k] == v) | (np.isnan(res[k]) & np.isnan(v))))[0][:5])
    assert np.array_equal(res["cell_j"], np.where(cell >= 0, cell // nx, -1)) and np.array_equal(res["cell_i"], np.where(cell >= 0, cell % nx, -1))
    c = res["counts"]
    assert (c["located"], c["outside"], c["invalid"]) == (int((cell >= 0).sum()), int(((cell < 0) & okq).sum()), int((~okq).sum()))
    if field is not None:
        f = field.records if hasattr(field, "records") else np.asarray(field).reshape((-1, ny, nx))
        v, fl = D.sample(cell, s, t, f, wet, ny, nx, periodic, fold, MODES[mode], fills)
        smp = res["samples"][0]
        assert smp["flags"].reshape(fl.shape).tobytes() == fl.tobytes()
        assert smp["values"].reshape(v.shape).tobytes() == v.tobytes()
        assert [smp["counts"]["flag%d" % k] for k in range(4)] == [int((fl == k).sum()) for k in range(4)]
    return res


def interior_points(x, y, rng, n, lo=0.05, hi=0.95):
    """n points inside random cells of the grid, built from the corners' unit vectors with bilinear weights (a, b) in [lo, hi]^2:
    lon, lat, cell.  (Cells with a corner that is not finite are not drawn.)"""
    ny, nx = shape_of(x)
    u = D.unit(x, y)
    good = np.nonzero(np.isfinite(u[0::2, 0::2]).all(axis=2)[:-1, :-1].reshape(-1) & np.isfinite(u[2::2, 2::2]).all(axis=2).reshape(-1) &
                      np.isfinite(u[0:-2:2, 2::2]).all(axis=2).reshape(-1) & np.isfinite(u[2::2, 0:-2:2]).all(axis=2).reshape(-1))[0]
    c = rng.choice(good, n)
    j, i = c // nx, c % nx
    a, b = lo + (hi - lo) * rng.random(n), lo + (hi - lo) * rng.random(n)
    p = (((1 - a) * (1 - b))[:, None] * u[2 * j, 2 * i] + (a * (1 - b))[:, None] * u[2 * j, 2 * i + 2] +
         (a * b)[:, None] * u[2 * j + 2, 2 * i + 2] + ((1 - a) * b)[:, None] * u[2 * j + 2, 2 * i])
    p /= np.linalg.norm(p, axis=1)[:, None]
    return np.degrees(np.arctan2(p[:, 1], p[:, 0])), np.degrees(np.arcsin(np.clip(p[:, 2], -1.0, 1.0))), c


def line_points(x, y, fold):
    """points on the seam meridian (the first point column, its own points and the middles between them in latitude), on the fold line
    (the top point row) when there is one, and the singular points of a cap: the two ends and the middle of the top row"""
    lon = [x[:, 0], x[:, 0], 0.5 * (x[:-1, 0] + x[1:, 0]), x[:, -1]]
    lat = [y[:, 0], y[:, 0] + 1e-9, 0.5 * (y[:-1, 0] + y[1:, 0]), y[:, -1]]
    if fold:
        n = x.shape[1] - 1
        lon += [x[-1], x[-1], x[-1, [0, n // 2, n]], x[-1, [0, n // 2, n]] + 1e-7]
        lat += [y[-1], y[-1] - 1e-9, y[-1, [0, n // 2, n]], y[-1, [0, n // 2, n]]]
    return np.concatenate(lon), np.concatenate(lat)


def cube_of(v, G):
    return np.clip(np.floor((v + 1.0) * (0.5 * G)).astype(np.int64), 0, G - 1)


def large_cells(cu, ny, nx, G, max_touch=27):
    """bool (nc,): the cells that can hold a point and whose box touches more than max_touch cubes of a grid of G^3"""
    g = D.cells(cu, ny, nx)
    ok = g["sigma"] != 0
    lo, hi = np.where(ok[:, None], g["lo"], 0.0), np.where(ok[:, None], g["hi"], 0.0)
    touch = np.prod(cube_of(hi, G) - cube_of(lo, G) + 1, axis=1)
    return ok & (touch > max_touch)

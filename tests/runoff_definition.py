"""The runoff mapping of include/ogg_hip.h ("Runoff mapping") written out in numpy, for the tests: the target set, the mapped sources,
the nearest target by brute force over (d2, cell), and the in-order sums.  Every operation is an elementwise IEEE fp64 operation, so
each value is formed by the same additions in the same order as the definition says.  Test infrastructure only: the unit vectors and
ds_J may be the device's own (the device's sin / cos need not round as the host's do)."""
import numpy as np

D2R = np.pi / 180.0


def targets(wet, periodic, fold, mode="coast"):
    """bool (ny, nx): the target cells"""
    w = np.asarray(wet) != 0
    if mode == "wet":
        return w.copy()
    ny, nx = w.shape
    land = np.zeros((ny + 2, nx + 2), bool)   # padded: a missing neighbour counts as land
    land[1:-1, 1:-1] = ~w
    land[0, 1:-1] = True
    land[-1, 1:-1] = True
    land[1:-1, 0] = ~w[:, -1] if periodic else True
    land[1:-1, -1] = ~w[:, 0] if periodic else True
    if fold:
        land[-1, 1:-1] = ~w[-1, ::-1]
    coast = land[:-2, 1:-1] | land[2:, 1:-1] | land[1:-1, :-2] | land[1:-1, 2:]
    return w & coast


def unit(lon, lat):
    """(n, 3) unit vectors of lon, lat in degrees, as the definition forms them"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    cl = np.cos(lat * D2R)
    return np.stack([cl * np.cos(lon * D2R), cl * np.sin(lon * D2R), np.sin(lat * D2R)], axis=-1)


def classify(f, fills=()):
    """mapped, skipped, missing (bool, NB * NA) of the records f (nrec, NB, NA)"""
    f = np.asarray(f)
    fr = f.reshape(f.shape[0], -1)
    ok = ~np.isnan(fr)
    for fv in fills:
        ok &= fr != f.dtype.type(fv)
    anyv = ok.any(axis=0)
    nz = (ok & (fr != 0)).any(axis=0)
    return nz, anyv & ~nz, ~anyv


def d2(su, tu):
    """(ns, nt) squared chordal distances, (dx dx + dy dy) + dz dz"""
    dx = su[:, None, 0] - tu[None, :, 0]
    dy = su[:, None, 1] - tu[None, :, 1]
    dz = su[:, None, 2] - tu[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(su, tu, tcell, chunk=256):
    """for every source the target cell with the smallest (d2, cell), and that d2 (tcell ascending: argmin's first is the smaller
    cell)"""
    tcell = np.asarray(tcell)
    assert np.all(np.diff(tcell) > 0)
    out_c = np.empty(len(su), np.int64)
    out_d = np.empty(len(su), np.float64)
    for k in range(0, len(su), chunk):
        d = d2(su[k:k + chunk], tu)
        a = np.argmin(d, axis=1)
        out_c[k:k + chunk] = tcell[a]
        out_d[k:k + chunk] = d[np.arange(len(a)), a]
    return out_c, out_d


def source_area(lon, lat_ds, Re):
    """A_s (NB, NA) = ((Re Re) (a_I+1 D - a_I D)) ds_J"""
    lon = np.asarray(lon, np.float64)
    return (Re * Re) * (lon[1:] * D2R - lon[:-1] * D2R)[None, :] * np.asarray(lat_ds)[:, None]


def ds_of(lat):
    b1, b2 = np.asarray(lat[:-1]) * D2R, np.asarray(lat[1:]) * D2R
    return 2.0 * np.cos((b1 + b2) / 2.0) * np.sin((b2 - b1) / 2.0)


def cell_area(area):
    a = np.asarray(area, np.float64)
    return (a[0::2, 0::2] + a[1::2, 1::2]) + (a[0::2, 1::2] + a[1::2, 0::2])


def accumulate(f, fills, src_cell, target, As, Ac):
    """values (nrec, ny, nx) and n_sources (ny, nx): src_cell ascending, target the cell of each, As (NB * NA), Ac (ny, nx)"""
    f = np.asarray(f)
    nrec = f.shape[0]
    ny, nx = Ac.shape
    ncell = ny * nx
    fr = f.reshape(nrec, -1)
    src_cell, target = np.asarray(src_cell, np.int64), np.asarray(target, np.int64)
    order = np.argsort(target, kind="stable")   # by cell, ascending source within a cell
    tc, sc = target[order], src_cell[order]
    count = np.bincount(tc, minlength=ncell)
    start = np.zeros(ncell, np.int64)
    first = np.r_[True, tc[1:] != tc[:-1]] if tc.size else np.zeros(0, bool)
    start[tc[first]] = np.nonzero(first)[0]
    S = np.zeros((nrec, ncell))
    for t in range(int(count.max()) if tc.size else 0):   # the t-th source of every cell, left to right
        cs = np.nonzero(count > t)[0]
        e = sc[start[cs] + t]
        v = fr[:, e]
        ok = ~np.isnan(v)
        for fv in fills:
            ok &= v != f.dtype.type(fv)
        p = v.astype(np.float64) * As.reshape(-1)[e][None, :]
        S[:, cs] = np.where(ok, S[:, cs] + p, S[:, cs])
    values = np.zeros((nrec, ncell))
    has = count > 0
    values[:, has] = S[:, has] / Ac.reshape(-1)[has]
    return values.reshape(nrec, ny, nx), count.reshape(ny, nx).astype(np.int32)


def runoff(f, fills, lon, lat, ds, Re, su, tu, tcell, area):
    """the whole definition on given unit vectors (su of the mapped sources in ascending order, tu / tcell of the targets): values,
    n_sources, mapped source cells, their targets and d2"""
    mapped, _, _ = classify(f, fills)
    src = np.nonzero(mapped)[0]
    assert len(src) == len(su)
    if len(src):
        tgt, dd = nearest(su, tu, tcell)
    else:
        tgt, dd = np.zeros(0, np.int64), np.zeros(0)
    As = source_area(lon, ds, Re)
    v, n = accumulate(f, fills, src, tgt, As, cell_area(area))
    return v, n, src, tgt, dd

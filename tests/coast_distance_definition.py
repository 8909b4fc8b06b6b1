"""The distance to the coast of include/ogg_hip.h ("Distance to the coast") written out in numpy, for the tests: the flag bytes, the
two coastal sets and the nearest member of the opposite set by brute force over (d2, cell).  Unit vectors, d2 and the nearest search are
the runoff definition's (tests/runoff_definition.py), as the header says they are.  Test infrastructure only: the unit vectors may be
the device's own (the device's sin / cos need not round as the host's do)."""
import numpy as np

from runoff_definition import d2, nearest, unit   # noqa: F401

F_WET, F_COAST, F_VALID = 1, 2, 4
WET, LAND = 1, 2
SIDES = {"wet": WET, "land": LAND, "both": WET | LAND}


def centres(x, y):
    """lon, lat (ny, nx) of the cell centres: supergrid points (2j+1, 2i+1)"""
    return np.asarray(x)[1::2, 1::2], np.asarray(y)[1::2, 1::2]


def coastal(wet, periodic, fold):
    """bool (ny, nx): the cells with a face neighbour of the other wetness; a neighbour that does not exist is no neighbour"""
    w = np.asarray(wet) != 0
    c = np.zeros(w.shape, bool)
    c[1:] |= w[1:] != w[:-1]
    c[:-1] |= w[:-1] != w[1:]
    c[:, 1:] |= w[:, 1:] != w[:, :-1]
    c[:, :-1] |= w[:, :-1] != w[:, 1:]
    if periodic:
        c[:, 0] |= w[:, 0] != w[:, -1]
        c[:, -1] |= w[:, -1] != w[:, 0]
    if fold:
        c[-1] |= w[-1] != w[-1, ::-1]
    return c


def flags(x, y, wet, periodic, fold):
    """uint8 (ny, nx): bit 0 wet, bit 1 coastal, bit 2 valid"""
    lon, lat = centres(x, y)
    valid = np.isfinite(lon) & np.isfinite(lat)
    return ((np.asarray(wet) != 0) * F_WET + coastal(wet, periodic, fold) * F_COAST + valid * F_VALID).astype(np.uint8)


def sets(fl):
    """the cells of L (valid coastal land) and of W (valid coastal wet), each ascending"""
    f = np.asarray(fl).reshape(-1)
    member = (f & (F_COAST | F_VALID)) == (F_COAST | F_VALID)
    return np.nonzero(member & ((f & F_WET) == 0))[0], np.nonzero(member & ((f & F_WET) != 0))[0]


def queries(fl, sides="both"):
    """the wet and the land cells that are queried (valid and of a selected side), each ascending"""
    f = np.asarray(fl).reshape(-1)
    valid = (f & F_VALID) != 0
    wet = (f & F_WET) != 0
    s = SIDES[sides]
    return (np.nonzero(valid & wet)[0] if s & WET else np.zeros(0, np.int64),
            np.nonzero(valid & ~wet)[0] if s & LAND else np.zeros(0, np.int64))


def coast_distance(u, fl, sides="both", only=None, chunk=256):
    """nearest (int32) and d2 (fp64), (ny, nx), from the unit vectors u (ny * nx, 3) of every cell and the flag bytes: -1 and +inf
    for a cell that is not queried, is invalid, or whose opposite set is empty.  ``only``: cells (flat) to which the queries are
    restricted (the others keep -1 and +inf)."""
    shape = np.asarray(fl).shape
    u = np.asarray(u).reshape(-1, 3)
    L, W = sets(fl)
    qw, ql = queries(fl, sides)
    out_c = np.full(u.shape[0], -1, np.int32)
    out_d = np.full(u.shape[0], np.inf)
    for q, t in ((qw, L), (ql, W)):
        if only is not None:
            q = np.intersect1d(q, np.asarray(only))
        if q.size and t.size:
            c, d = nearest(u[q], u[t], t, chunk)
            out_c[q] = c
            out_d[q] = d
    return out_c.reshape(shape), out_d.reshape(shape)


def define(x, y, wet, periodic, fold, sides="both"):
    """flags, nearest, d2 of a supergrid x, y with numpy's own unit vectors"""
    fl = flags(x, y, wet, periodic, fold)
    lon, lat = centres(x, y)
    with np.errstate(invalid="ignore"):
        u = unit(lon.reshape(-1), lat.reshape(-1))
    n, d = coast_distance(u, fl, sides)
    return fl, n, d, u


def haversine(lon1, lat1, lon2, lat2, Re):
    """the great-circle distance by the haversine formula (metres)"""
    a1, b1, a2, b2 = (np.radians(v) for v in (lon1, lat1, lon2, lat2))
    h = np.sin((b2 - b1) / 2) ** 2 + np.cos(b1) * np.cos(b2) * np.sin((a2 - a1) / 2) ** 2
    return 2.0 * Re * np.arcsin(np.sqrt(h))

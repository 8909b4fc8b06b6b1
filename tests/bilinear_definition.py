"""The bilinear interpolation of include/ogg_hip.h ("Bilinear interpolation") written out in numpy, for the tests: the locate step by
np.searchsorted(..., side="right") - 1 on the source's cell centres, the masked weighted sums in corner order, and the rotation of a
vector's components.  Every operation is an elementwise IEEE fp64 operation, so each value is formed by the same operations in the
same order as the definition says.  The fill is remap_definition.fill.  Test infrastructure only."""
import numpy as np

from remap_definition import DRY, FILL, FILLED, REMAPPED, UNFILLED, fill  # noqa: F401

OFFSETS = {"h": (1, 1), "u": (1, 0), "v": (0, 1)}


def points(a, kind):
    """the h, u or v points of a supergrid field ((2 ny + 1) x (2 nx + 1))"""
    oy, ox = OFFSETS[kind]
    return a[oy::2, ox::2]


def centres(lon_edges, lat_edges):
    lon, lat = np.asarray(lon_edges, dtype=np.float64), np.asarray(lat_edges, dtype=np.float64)
    return (lon[:-1] + lon[1:]) / 2.0, (lat[:-1] + lat[1:]) / 2.0


def locate(x, y, lon_edges, lat_edges):
    """I, I1, wx, J, J1, wy of the points (x, y), each of x's shape"""
    lonc, latc = centres(lon_edges, lat_edges)
    NA, NB = lonc.size, latc.size
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    c = lonc - lonc[0]
    t = x - lonc[0]
    t = t - 360.0 * np.floor(t / 360.0)
    t = np.where((t >= 0.0) & (t < 360.0), t, 0.0)
    I = np.maximum(np.searchsorted(c, t, side="right") - 1, 0)
    I1 = (I + 1) % NA
    c1 = np.where(I + 1 < NA, c[np.minimum(I + 1, NA - 1)], c[0] + 360.0)
    wx = (t - c[I]) / (c1 - c[I])
    below, above = y <= latc[0], y >= latc[NB - 1]
    J = np.clip(np.searchsorted(latc, y, side="right") - 1, 0, max(NB - 2, 0))
    J1 = np.minimum(J + 1, NB - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        wy = np.where(J1 > J, (y - latc[J]) / (latc[J1] - latc[J]), 0.0)
    J = np.where(below, 0, np.where(above, NB - 1, J))
    J1 = np.where(below, 0, np.where(above, NB - 1, J1))
    wy = np.where(below | above, 0.0, wy)
    return I, I1, wx, J, J1, wy


def _missing(v, fills):
    m = np.isnan(v)
    for fv in fills:
        m |= v == v.dtype.type(fv)
    return m


def interpolate(x, y, lon_edges, lat_edges, f, f2=None, fills=(), mask=None):
    """values, flags ((nrec,) + x.shape) of f (nrec, NB, NA) at the points (x, y); with f2 a vector: (values, values2), flags"""
    I, I1, wx, J, J1, wy = locate(x, y, lon_edges, lat_edges)
    f = np.asarray(f)
    ux, uy = 1.0 - wx, 1.0 - wy
    ws = (ux * uy, wx * uy, ux * wy, wx * wy)
    corners = ((J, I), (J, I1), (J1, I), (J1, I1))
    shape = (f.shape[0],) + np.shape(x)
    W, n = np.zeros(shape), np.zeros(shape, dtype=np.int64)
    fs = [f] if f2 is None else [f, np.asarray(f2)]
    S = [np.zeros(shape) for _ in fs]
    for w, (jj, ii) in zip(ws, corners):
        vs = [g[:, jj, ii] for g in fs]
        ok = np.ones(shape, dtype=bool)
        for v in vs:
            ok &= ~_missing(v, fills)
        wb = np.broadcast_to(w, shape)
        W = np.where(ok, W + wb, W)
        for k, v in enumerate(vs):
            with np.errstate(invalid="ignore", over="ignore"):
                S[k] = np.where(ok, S[k] + wb * v.astype(np.float64), S[k])
        n += ok
    nolat = np.broadcast_to(np.isnan(np.asarray(y, dtype=np.float64)), shape)   # a NaN latitude: no corners, whatever locate() clipped to
    full, part = (n == 4) & ~nolat, (n > 0) & (n < 4) & (W > 0) & ~nolat
    flags = np.where(full | part, REMAPPED, UNFILLED).astype(np.uint8)
    out = []
    for s in S:
        with np.errstate(invalid="ignore", divide="ignore"):
            out.append(np.where(full, s, np.where(part, s / W, FILL)))
    if mask is not None:
        dry = np.broadcast_to(np.asarray(mask) == 0, shape)
        flags = np.where(dry, DRY, flags).astype(np.uint8)
        out = [np.where(dry, FILL, v) for v in out]
    return (out[0], flags) if f2 is None else ((out[0], out[1]), flags)


def rot(angle_deg):
    """numpy's cosine and sine of angle_dx (the device's come from sincospi(a / 180): compared within a bound, not bit for bit)"""
    a = np.radians(np.asarray(angle_deg, dtype=np.float64))
    return np.cos(a), np.sin(a)


def rotate(U, V, flags, ca, sa):
    """(ug, vg) = (U ca + V sa, V ca - U sa) where the flag is REMAPPED or FILLED; the fill value elsewhere"""
    ok = (flags == REMAPPED) | (flags == FILLED)
    with np.errstate(invalid="ignore", over="ignore"):
        ug = np.where(ok, U * ca + V * sa, U)
        vg = np.where(ok, V * ca - U * sa, V)
    return ug, vg

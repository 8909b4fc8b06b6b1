"""The numpy definition of plane-fit topography (include/ogg_hip.h, "Plane-fit topography"), restated operation for operation on top
of tests/topog_definition.py (its cells, sample_positions and sample_values), used by tests/test_topog_plane_cpu.py and
tests/test_gpu_topog_plane.py.  Three parts: the integer plane records of a grid or of a band of its rows; the host outputs from
those integers in Python integers and Python floats (``fields``); and an exact-rational solver (``rational_fit``), the independent
truth for a, b and h2.  Slow, so for small grids only."""
from fractions import Fraction

import numpy as np

import topog_definition as td

MAX_OFFSET = 1 << 15
MOMENTS = ("sx", "sy", "sxx", "sxy", "syy", "sxq", "syq", "n_far")
FIELDS = td.RECORD_FIELDS + MOMENTS
FILL = 1.0e20
RE = 6371.0e3
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


# ---- the integer records ---------------------------------------------------------------------------------------
def origin_points(x, y, cells_, j0=0):
    """(xO, yO), one per supergrid cell of the band whose point rows are x, y (its first cell row is row j0 of the whole grid): the
    centre (2 jm + 1, 2 im + 1) of the model cell it belongs to, or its own P00."""
    ny, nx = x.shape[0] - 1, x.shape[1] - 1
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    if cells_ == "model":
        jo, io = 2 * ((j + j0) // 2) + 1 - j0, 2 * (i // 2) + 1     # a row of the band, or the one that follows it: 0 .. ny
    else:
        jo, io = j, i
    return x[jo, io], y[jo, io]


def origin_indices(xO, yO, Nx, Ny, lon0, dlon, lat0, dlat):
    """(fI0, fJ0, has): the origin's raster column and row as integral doubles, and whether the cell has an origin"""
    periodic = abs(Nx * dlon - 360.0) <= 1e-9
    inv_dlon, inv_dlat = 1.0 / dlon, 1.0 / dlat
    with np.errstate(invalid="ignore", over="ignore"):
        has = np.isfinite(xO) & np.isfinite(yO)
        fJ0 = np.floor((yO - lat0) * inv_dlat)
        if periodic:
            fI0 = np.floor((xO - lon0) * inv_dlon)
            has &= np.abs(fI0) < 4.0e15
            fJ0 = np.clip(fJ0, 0.0, Ny - 1.0)
        else:
            fI0 = np.floor(((xO - lon0) % 360.0) * inv_dlon)
        has &= ~(np.isnan(fI0) | np.isnan(fJ0))
    return fI0, fJ0, has


def sample_indices(Nx, Ny, lon0, dlon, lat0, dlat, lon, lat):
    """(fi, fj) of every sample as integral doubles: the unreduced column (before mod Nx on a periodic source, after the branch
    mapping on a regional one) and the row (after the clamp on a periodic source).  Only those of valid samples are used."""
    periodic = abs(Nx * dlon - 360.0) <= 1e-9
    inv_dlon, inv_dlat = 1.0 / dlon, 1.0 / dlat
    with np.errstate(invalid="ignore", over="ignore"):
        fj = np.floor((lat - lat0) * inv_dlat)
        if periodic:
            fi = np.floor((lon - lon0) * inv_dlon)
            fj = np.clip(fj, 0.0, Ny - 1.0)
        else:
            fi = np.floor(((lon - lon0) % 360.0) * inv_dlon)
    return fi, fj


def offsets(fi, fj, fI0, fJ0, has, pole, Nx, periodic):
    """(dI, dJ, near) of samples with indices fi, fj (integral doubles) against the origin indices fI0, fJ0 of their cell: near is
    False for a FAR sample (an offset beyond MAX_OFFSET or not a number, a pole-enclosing cell, a cell without origin)"""
    hN = float(Nx // 2)
    with np.errstate(invalid="ignore", over="ignore"):
        dI = (np.mod(fi - fI0 + hN, float(Nx)) - hN) if periodic else fi - fI0
        dJ = fj - fJ0
        near = (np.abs(dI) <= MAX_OFFSET) & (np.abs(dJ) <= MAX_OFFSET) & has & (pole == 0)
    return dI, dJ, near


def supergrid_records(x, y, q, lon0, dlon, lat0, dlat, refine=None, oversample=2.0, wet_below=0.0, cells_="supergrid", j0=0):
    """Plane records of every supergrid cell of a band (a dict of int64 arrays ny x nx, FIELDS); the origin is that of the output
    cell (``cells_``) the supergrid cell belongs to."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = td.supergrid_records(x, y, q, lon0, dlon, lat0, dlat, refine, oversample, wet_below)
    with np.errstate(invalid="ignore"):
        c = td.cells(x, y, dlon, dlat, refine, oversample)
    shape = c["R"].shape
    Ny, Nx = q.shape
    periodic = abs(Nx * dlon - 360.0) <= 1e-9
    fI0, fJ0, has = (a.reshape(-1) for a in origin_indices(*origin_points(x, y, cells_, j0), Nx, Ny, lon0, dlon, lat0, dlat))
    for f in MOMENTS:
        out[f] = np.zeros(shape, dtype=np.int64)
    o = {f: out[f].reshape(-1) for f in MOMENTS}
    flat = {k: v.reshape(-1) for k, v in c.items()}
    for R in np.unique(flat["R"]):
        all_idx = np.nonzero(flat["R"] == R)[0]
        chunk = max(1, 2_000_000 // int(R * R))
        for s0 in range(0, all_idx.size, chunk):
            idx = all_idx[s0:s0 + chunk]
            with np.errstate(invalid="ignore"):
                lon, lat = td.sample_positions(flat, int(R), idx)
            pole = flat["pole"][idx]
            v, miss = td.sample_values(q, lon0, dlon, lat0, dlat, lon, lat, pole)
            ok = ~miss
            fi, fj = sample_indices(Nx, Ny, lon0, dlon, lat0, dlat, lon, lat)
            dI, dJ, near = offsets(fi, fj, *(a[idx][:, None, None] for a in (fI0, fJ0, has)), pole[:, None, None], Nx, periodic)
            far = ok & ~near
            use = ok & near
            di, dj = np.where(use, dI, 0.0).astype(np.int64), np.where(use, dJ, 0.0).astype(np.int64)
            vq = np.where(use, v, 0).astype(np.int64)
            for f, a in (("sx", di), ("sy", dj), ("sxx", di * di), ("sxy", di * dj), ("syy", dj * dj), ("sxq", di * vq), ("syq", dj * vq),
                         ("n_far", far.astype(np.int64))):
                o[f][idx] = a.sum(axis=(1, 2))
    return out


def _empty_rows(like, n):
    out = {}
    for f, v in like.items():
        out[f] = np.full((n,) + v.shape[1:], INT32_MAX if f == "min" else (INT32_MIN if f == "max" else 0), dtype=np.int64)
    return out


def model_records(sg, j0=0):
    """2 x 2 blocks of the supergrid records of a band whose first row is row j0 of the whole grid: the (partial, where the band holds
    one of a model row's two supergrid rows) records of model rows j0 >> 1 .. (j0 + n - 1) >> 1."""
    n = sg["n"].shape[0]
    parts = ([_empty_rows(sg, 1)] if j0 % 2 else []) + [sg] + ([_empty_rows(sg, 1)] if (j0 + n) % 2 else [])
    sg = {f: np.concatenate([p[f] for p in parts]) for f in sg}
    out = {}
    for f, a in sg.items():
        blocks = [a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]]
        if f == "min":
            out[f] = np.minimum.reduce(blocks)
        elif f in ("max", "R"):
            out[f] = np.maximum.reduce(blocks)
        else:
            out[f] = blocks[0] + blocks[1] + blocks[2] + blocks[3]
    return out


def records(x, y, raw, lon0, dlon, lat0, dlat, refine=None, oversample=2.0, quantum=None, sea_level=0.0, cells_="model", fill=(), j0=0):
    """Plane records of the band whose point rows are x, y (the whole grid when j0 = 0 and they are all its rows)."""
    q, quantum = td.quantise(raw, quantum, fill)
    sg = supergrid_records(x, y, q, lon0, dlon, lat0, dlat, refine, oversample, float(sea_level) / quantum, cells_, j0)
    return model_records(sg, j0) if cells_ == "model" else sg


def add_records(a, b):
    """the exact combination of two record dicts of one shape"""
    out = {}
    for f in a:
        out[f] = np.minimum(a[f], b[f]) if f == "min" else (np.maximum(a[f], b[f]) if f in ("max", "R") else a[f] + b[f])
    return out


# ---- the host outputs, from Python integers --------------------------------------------------------------------
def centred(r):
    """Cxx, Cxy, Cyy, Cxq, Cyq, Cqq of one record (a dict of Python integers), exact"""
    n, s, ss, sx, sy = r["n"], r["sum"], r["sumsq"], r["sx"], r["sy"]
    return (n * r["sxx"] - sx * sx, n * r["sxy"] - sx * sy, n * r["syy"] - sy * sy, n * r["sxq"] - sx * s, n * r["syq"] - sy * s,
            n * ss - s * s)


def cell(rec, j, i):
    return {f: int(rec[f][j, i]) for f in FIELDS}


def cell_latitudes(y, cells_):
    y = np.asarray(y, dtype=np.float64)
    if cells_ == "model":
        return y[1::2, 1::2]
    with np.errstate(invalid="ignore"):
        return (y[:-1, :-1] + y[:-1, 1:] + y[1:, :-1] + y[1:, 1:]) / 4.0


def fields(rec, quantum, lat_c, dlon, dlat):
    """h2, plane_a, plane_b, slope_east, slope_north, plane_flag: every centred moment a Python integer rounded once by float(), then
    the header's fp64 sequence in Python floats, cell by cell."""
    shape = rec["n"].shape
    out = {k: np.full(shape, FILL) for k in ("h2", "plane_a", "plane_b", "slope_east", "slope_north")}
    flag = np.zeros(shape, dtype=np.int8)
    q = float(quantum)
    for j in range(shape[0]):
        for i in range(shape[1]):
            r = cell(rec, j, i)
            n = r["n"]
            if n == 0:
                continue
            Cxx, Cxy, Cyy, Cxq, Cyq, Cqq = (float(v) for v in centred(r))
            d = Cxx * Cyy - Cxy * Cxy
            flag[j, i] = 3 if r["n_far"] > 0 else (2 if (n < 3 or not d > 0.0) else 1)
            nn = float(n) * float(n)
            if flag[j, i] != 1:
                out["h2"][j, i] = Cqq / nn * (q * q)
                continue
            a = (Cxq * Cyy - Cyq * Cxy) / d
            b = (Cyq * Cxx - Cxq * Cxy) / d
            r_ = Cqq - a * Cxq - b * Cyq
            out["h2"][j, i] = max(0.0, r_) / nn * (q * q)
            out["plane_a"][j, i], out["plane_b"][j, i] = a, b
    fitted = flag == 1
    lat = np.asarray(lat_c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        east = out["plane_a"] * q / (dlon * np.pi / 180.0 * RE * np.cos(lat * np.pi / 180.0))
        north = out["plane_b"] * q / (dlat * np.pi / 180.0 * RE)
        polar = ~(np.abs(lat) < 90.0 - td.POLE_EPS)
    out["slope_east"] = np.where(fitted & ~polar, east, FILL)
    out["slope_north"] = np.where(fitted, north, FILL)
    out["plane_flag"] = flag
    return out


# ---- the independent truth -------------------------------------------------------------------------------------
def rational_fit(r):
    """(a, b, h2 in quanta^2, variance about the mean in quanta^2) of one record as Fractions, from the normal equations solved in
    exact rationals; None when the determinant is zero or n = 0"""
    if r["n"] == 0:
        return None
    Cxx, Cxy, Cyy, Cxq, Cyq, Cqq = centred(r)
    det = Cxx * Cyy - Cxy * Cxy
    if det == 0:
        return None
    a, b = Fraction(Cxq * Cyy - Cyq * Cxy, det), Fraction(Cyq * Cxx - Cxq * Cxy, det)
    nn = r["n"] * r["n"]
    return a, b, (Cqq - a * Cxq - b * Cyq) / nn, Fraction(Cqq, nn)


def brute_fit(dI, dJ, q):
    """the same from the samples themselves (lists of Python integers), by the normal equations of q ~ c + a dI + b dJ: a check of
    the moments' algebra that does not go through them"""
    n = len(q)
    mx, my, mq = Fraction(sum(dI), n), Fraction(sum(dJ), n), Fraction(sum(q), n)
    X, Y, Q = [v - mx for v in dI], [v - my for v in dJ], [v - mq for v in q]
    sxx, sxy, syy = sum(v * v for v in X), sum(u * v for u, v in zip(X, Y)), sum(v * v for v in Y)
    sxq, syq = sum(u * v for u, v in zip(X, Q)), sum(u * v for u, v in zip(Y, Q))
    det = sxx * syy - sxy * sxy
    a, b = (sxq * syy - syq * sxy) / det, (syq * sxx - sxq * sxy) / det
    return a, b, sum((w - a * u - b * v) ** 2 for u, v, w in zip(X, Y, Q)) / n


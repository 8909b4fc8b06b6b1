"""Numpy definition of the grid-quality report (include/ogg_hip.h, "Grid-quality report"), for the tests only: the package never
imports it.  Written from the definitions, literally: both quotients of every ratio, the corner angle as atan2(|A' x B'|, A'.B')
and its distance from 90 degrees.  Ties of an extremum go to the smallest (j, i) (the first index numpy's argmin / argmax finds in
C order).  It returns the "grid" section of the report, in the report's own layout."""
import numpy as np

DEGENERATE_M = 1.0e-3
BIN_EDGES_DEG = (1.0e-6, 1.0e-3, 0.1, 1.0, 5.0, 20.0)


def unit_vectors(x, y):
    lam, phi = np.deg2rad(x), np.deg2rad(y)
    return np.stack((np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)), axis=-1)


def corner_delta(x, y, Re):
    """delta (degrees) at the SW corner of every cell, ny x nx; NaN where a chord is degenerate."""
    P = unit_vectors(x, y)
    p0, pe, pn = P[:-1, :-1], P[:-1, 1:], P[1:, :-1]
    A, B = pe - p0, pn - p0
    ok = (Re * np.linalg.norm(A, axis=-1) >= DEGENERATE_M) & (Re * np.linalg.norm(B, axis=-1) >= DEGENERATE_M)
    Ap = A - np.sum(A * p0, axis=-1, keepdims=True) * p0
    Bp = B - np.sum(B * p0, axis=-1, keepdims=True) * p0
    theta = np.degrees(np.arctan2(np.linalg.norm(np.cross(Ap, Bp), axis=-1), np.sum(Ap * Bp, axis=-1)))
    return np.where(ok, np.abs(theta - 90.0), np.nan)


def _ext(v, x, y, which):
    """{value, j, i, lon, lat} of the max / min of v over its non-NaN entries (None if there are none)."""
    if not np.any(~np.isnan(v)):
        return None
    k = np.nanargmax(v) if which == "max" else np.nanargmin(v)
    j, i = np.unravel_index(k, v.shape)
    return {"value": float(v[j, i]), "j": int(j), "i": int(i), "lon": float(x[j, i]), "lat": float(y[j, i])}


def ratio(p, q):
    return np.maximum(p / q, q / p)


def grid_section(x, y, dx=None, dy=None, area=None, Re=6371.0e3):
    """The "grid" section of the report of a stitched supergrid."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nan = np.nan
    delta = corner_delta(x, y, Re)
    good = delta[~np.isnan(delta)]
    edges = np.asarray(BIN_EDGES_DEG)
    out = {"corner": {"delta_max_deg": _ext(delta, x, y, "max"), "n": int(delta.size), "n_degenerate": int(np.isnan(delta).sum()),
                      "histogram": [int(c) for c in np.bincount(np.searchsorted(edges, good, side="right"), minlength=len(edges) + 1)]}}
    if dx is None:
        out.update({k: None for k in ("dx", "dy", "area", "aspect_ratio_max", "rx_max", "ry_max")})
        return out
    dx, dy, area = (np.asarray(a, np.float64) for a in (dx, dy, area))
    dx_ok, dy_ok = dx >= DEGENERATE_M, dy >= DEGENERATE_M
    out["dx"] = {"min": _ext(np.where(dx_ok, dx, nan), x, y, "min"), "max": _ext(dx, x, y, "max"), "n": int(dx.size),
                 "n_degenerate": int((dx < DEGENERATE_M).sum())}
    out["dy"] = {"min": _ext(np.where(dy_ok, dy, nan), x, y, "min"), "max": _ext(dy, x, y, "max"), "n": int(dy.size),
                 "n_degenerate": int((dy < DEGENERATE_M).sum())}
    out["area"] = {"min": _ext(np.where(area != 0, area, nan), x, y, "min"), "max": _ext(area, x, y, "max"), "n": int(area.size),
                   "n_zero": int((area == 0).sum())}
    a = (dx[:-1, :] + dx[1:, :]) / 2
    b = (dy[:, :-1] + dy[:, 1:]) / 2
    ok = dx_ok[:-1, :] & dx_ok[1:, :] & dy_ok[:, :-1] & dy_ok[:, 1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["aspect_ratio_max"] = _ext(np.where(ok, ratio(a, b), nan), x, y, "max")
        right = np.roll(dx, -1, axis=1)                    # dx[j, i+1], dx[j, 0] for i = nx-1
        out["rx_max"] = _ext(np.where(dx_ok & np.roll(dx_ok, -1, axis=1), ratio(right, dx), nan), x, y, "max")
        ry = np.where(dy_ok[:-1] & dy_ok[1:], ratio(dy[1:], dy[:-1]), nan)
        out["ry_max"] = _ext(ry, x, y, "max")
    return out

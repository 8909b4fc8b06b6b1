#!/usr/bin/env python3
"""Extended-precision TRUTH for the exchange grid's areas on the cell zoo of tests/small_meshes.py.

CPU only (mpmath, 50 digits):

    python scripts/xgrid_truth.py      ->  tests/golden/xgrid_truth.npz

What "truth" means here: the exact area of the polygons the definition (include/ogg_hip.h, "Atmosphere x ocean exchange grid";
tests/xgrid_definition.py) builds from the fp64 corners -- edges straight in (lambda, phi), the vertices of xgrid_definition.polygon
-- with every operation and every transcendental exact, pi included, rounded once at the end:

    A = -Re^2 sum over the edges of dlam * (mean of sin(phi) - sin(phi_r) along the edge),
    mean = (cos(phi_1) - cos(phi_2)) / (phi_2 - phi_1) - sin(phi_r), or sin(phi_1) - sin(phi_r) on a parallel,

and the same for every piece, clipped by the same Sutherland-Hodgman passes in mpmath against the edges of zoo_atmosphere("regular").
|fp64 definition - truth| is the definition's own rounding error, the yardstick the device is held to
(tests/test_gpu_small_meshes.py): a kernel no further from the truth than 1.5 times that cannot be told from the definition on
another libm.

Stored: cells (model column of every cell with a finite A_poly), a_poly (hi, lo), pairs (I, J, n, m) of every piece the definition
keeps at threshold 0, area (hi, lo), with hi = fp64(truth) and lo = fp64(truth - hi); and the definition's distance from the truth
relative to A_poly, as measured when the file was made (eref_poly, eref_piece; eref_poly_rest, eref_piece_rest over every cell
but the bow-tie).
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import small_meshes as sm  # noqa: E402
import xgrid_definition as xd  # noqa: E402

mp.mp.dps = 50
OUT = os.path.join(ROOT, "tests", "golden", "xgrid_truth.npz")


def M(v):
    """fp64 -> mpf, exactly"""
    return mp.mpf(float(v))


def split(t):
    hi = float(t)
    return hi, float(t - M(hi))


def area(verts):
    """the exact area of a polygon of (lambda, phi) in degrees (mpf), edges straight in (lambda, phi)"""
    if not verts:
        return mp.mpf(0)
    d = mp.pi / 180
    pr = mp.sin(verts[0][1] * d)
    s = mp.mpf(0)
    n = len(verts)
    for k in range(n):
        (l1, p1), (l2, p2) = verts[k], verts[(k + 1) % n]
        if l1 == l2:
            continue
        p1, p2 = p1 * d, p2 * d
        mean = mp.sin(p1) - pr if p1 == p2 else (mp.cos(p1) - mp.cos(p2)) / (p2 - p1) - pr
        s += (l2 - l1) * d * mean
    return -(M(sm.RE) ** 2) * s


def _inside(S, v, c):
    return (v[0] >= c, v[0] <= c, v[1] >= c, v[1] <= c)[S]


def _cross(S, a, b, c):
    if S < 2:
        return (c, a[1] + (c - a[0]) * (b[1] - a[1]) / (b[0] - a[0]))
    return (a[0] + (c - a[1]) * (b[0] - a[0]) / (b[1] - a[1]), c)


def clip(verts, clo, chi, blo, bhi):
    """xgrid_definition.clip in exact arithmetic"""
    for S, c in ((0, clo), (1, chi), (2, blo), (3, bhi)):
        if not verts:
            return []
        n = len(verts)
        out = [verts[0]] if _inside(S, verts[0], c) else []
        for k in range(n):
            a, b = verts[k], verts[(k + 1) % n]
            if _inside(S, a, c) != _inside(S, b, c):
                out.append(_cross(S, a, b, c))
            if k + 1 < n and _inside(S, b, c):
                out.append(b)
        verts = out
    return verts


def table():
    """the arrays of tests/golden/xgrid_truth.npz"""
    x, y, _ = sm.cell_zoo()
    lon, lat = sm.zoo_atmosphere("regular")
    lst, a_def, _ = xd.exchange_grid(x, y, lon, lat, Re=sm.RE, threshold=0.0)
    nx = a_def.shape[1]
    polys, cells, a_poly = {}, [], []
    for n in range(nx):
        if not np.isfinite(a_def[0, n]):
            continue
        cx = [float(x[0, 2 * n]), float(x[0, 2 * n + 2]), float(x[2, 2 * n + 2]), float(x[2, 2 * n])]
        cy = [float(y[0, 2 * n]), float(y[0, 2 * n + 2]), float(y[2, 2 * n + 2]), float(y[2, 2 * n])]
        _, verts, _ = xd.polygon(cx, cy)
        polys[n] = [(M(l), M(p)) for l, p in verts]
        cells.append(n)
        a_poly.append(split(area(polys[n])))
    pairs, areas = [], []
    for I, J, n, m, _ in lst:
        lmin = min(v[0] for v in polys[n])
        s = 360 * mp.floor((lmin - M(lon[I])) / 360)   # the turn that brings the atmosphere column onto the polygon
        best = None
        for k in (s - 360, s, s + 360):
            a = area(clip(polys[n], M(lon[I]) + k, M(lon[I + 1]) + k, M(lat[J]), M(lat[J + 1])))
            best = a if best is None or a > best else best
        pairs.append((I, J, n, m))
        areas.append(split(best))
    out = {"dps": np.array(mp.mp.dps), "cells": np.array(cells, np.int32), "a_poly": np.array(a_poly),
           "pairs": np.array(pairs, np.int32).reshape(-1, 4), "area": np.array(areas)}
    ap = out["a_poly"]
    got = a_def[0, out["cells"]]
    pos = ap[:, 0] > 0
    out["eref_poly"] = np.array(np.max(np.abs((got[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0]))
    scale = a_def[0, out["pairs"][:, 2]]
    ar = out["area"]
    e_piece = np.abs((np.array([e[4] for e in lst]) - ar[:, 0]) - ar[:, 1]) / scale
    out["eref_piece"] = np.array(np.max(e_piece))
    # the same without the bow-tie, whose cancelling lobes carry ten times the error of any other cell
    bow = sm.cell_zoo()[2]["bow_tie"]
    rest = pos & (out["cells"] != bow)
    out["eref_poly_rest"] = np.array(np.max(np.abs((got[rest] - ap[rest, 0]) - ap[rest, 1]) / ap[rest, 0]))
    out["eref_piece_rest"] = np.array(np.max(e_piece[out["pairs"][:, 2] != bow]))
    return out


def main():
    out = table()
    np.savez_compressed(OUT, **out)
    print("%d cells, %d pieces; definition vs truth: A_poly %.3e, pieces %.3e of A_poly" % (
        out["cells"].size, out["pairs"].shape[0], float(out["eref_poly"]), float(out["eref_piece"])))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""The atmosphere x ocean exchange grid of include/ogg_hip.h written out directly: a loop over ocean cells and their candidates, in
plain Python floats (fp64, no fused multiply-add).  Test infrastructure only: the GPU tests compare the device's lists with it."""
import math

import numpy as np

POLE_EPS = 1.0e-10
D2R = math.pi / 180.0


def mod360(x):
    return x % 360.0   # Python's float % has numpy's semantics: the sign of the divisor


def wrap180(d):
    return mod360(d + 180.0) - 180.0


def polygon(cx, cy):
    """(status, vertices, n pole corners) of one cell from its corners C0..C3: status 'ok', 'degenerate' or 'pole'."""
    pc = [abs(v) >= 90.0 - POLE_EPS for v in cy]
    npole = sum(pc)
    if npole >= 3:
        return "degenerate", [], npole
    L = [cx[0] + wrap180(v - cx[0]) for v in cx]
    verts = []
    for k in range(4):
        if not pc[k]:
            verts.append((L[k], cy[k]))
        elif not pc[(k + 3) % 4]:
            lb = L[(k + 3) % 4]
            la = L[(k + 2) % 4] if pc[(k + 1) % 4] else L[(k + 1) % 4]
            p = 90.0 if cy[k] > 0.0 else -90.0
            verts += [(lb, p), (la, p)]
    w = 0.0
    for k in range(len(verts)):
        w = w + wrap180(verts[(k + 1) % len(verts)][0] - verts[k][0])
    return ("pole" if abs(w) > 180.0 else "ok"), verts, npole


def efun(h):
    if abs(h) < 0.1:
        h2 = h * h
        return h2 * (1.0 / 6.0 - h2 * (1.0 / 120.0 - h2 * (1.0 / 5040.0 - h2 / 362880.0)))
    return 1.0 - math.sin(h) / h


def gfun(p1, p2, pr):
    pm, h = (p1 + p2) / 2.0, (p2 - p1) / 2.0
    return 2.0 * math.cos((pm + pr) / 2.0) * math.sin((pm - pr) / 2.0) - math.sin(pm) * efun(h)


def area(verts, Re):
    if not verts:
        return 0.0
    lam = [v[0] * D2R for v in verts]
    phi = [v[1] * D2R for v in verts]
    pr = phi[0]
    s = 0.0
    n = len(verts)
    for k in range(n):
        k1 = (k + 1) % n
        s = s + (lam[k1] - lam[k]) * gfun(phi[k], phi[k1], pr)
    return -(Re * Re) * s


def _inside(S, v, c):
    return (v[0] >= c, v[0] <= c, v[1] >= c, v[1] <= c)[S]


def _cross(S, a, b, c):
    if S < 2:
        e, f = (a, b) if a <= b else (b, a)        # tuples compare lexicographically on (lam, phi)
        return (c, e[1] + (c - e[0]) * ((f[1] - e[1]) / (f[0] - e[0])))
    e, f = (a, b) if (a[1], a[0]) <= (b[1], b[0]) else (b, a)
    return (e[0] + (c - e[1]) * ((f[0] - e[0]) / (f[1] - e[1])), c)


def clip(verts, clo, chi, blo, bhi):
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


def exchange_grid(x, y, lon, lat, mask=None, Re=6371.0e3, threshold=1.0e-6, rows=None):
    """(list of (I, J, n, m, A_x) in the canonical order, A_poly (ny/2 x nx/2, NaN for degenerate / pole-enclosing cells), counts
    dict).  ``rows``: the model rows to do (default all; A_poly of the others stays NaN)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    NA, NB = lon.size - 1, lat.size - 1
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    a_poly = np.full((ny, nx), np.nan)
    counts = dict(cells=0, pole_cells=0, pole_enclosing=0, inverted=0, degenerate=0, masked=0, candidates=0, kept=0)
    out = []
    dsin = [2.0 * math.cos((float(lat[J]) * D2R + float(lat[J + 1]) * D2R) / 2.0) *
            math.sin((float(lat[J + 1]) * D2R - float(lat[J]) * D2R) / 2.0) for J in range(NB)]
    lonl, latl = [float(v) for v in lon], [float(v) for v in lat]
    for m in (range(ny) if rows is None else rows):
        for n in range(nx):
            cx = [float(x[2 * m, 2 * n]), float(x[2 * m, 2 * n + 2]), float(x[2 * m + 2, 2 * n + 2]), float(x[2 * m + 2, 2 * n])]
            cy = [float(y[2 * m, 2 * n]), float(y[2 * m, 2 * n + 2]), float(y[2 * m + 2, 2 * n + 2]), float(y[2 * m + 2, 2 * n])]
            counts["cells"] += 1
            masked = mask is not None and mask[m, n] == 0
            counts["masked"] += int(masked)
            st, verts, npole = polygon(cx, cy)
            if st == "degenerate":
                counts["degenerate"] += 1
                continue
            counts["pole_cells"] += int(npole > 0)
            if st == "pole":
                counts["pole_enclosing"] += 1
                continue
            A = area(verts, Re)
            a_poly[m, n] = A
            if not A > 0:
                counts["inverted"] += 1
                continue
            if masked:
                continue
            lmin, lmax = min(v[0] for v in verts), max(v[0] for v in verts)
            pmin, pmax = min(v[1] for v in verts), max(v[1] for v in verts)
            Js = [J for J in range(NB) if latl[J] < pmax and latl[J + 1] > pmin]
            kf = math.floor((lmin - lonl[0]) / 360.0)
            cols = []
            for k in range(kf - 2, kf + 3):
                s = 360.0 * k
                cols += [(I, s) for I in range(NA) if lonl[I] + s < lmax and lonl[I + 1] + s > lmin]
            counts["candidates"] += len(Js) * len(cols)
            for J in Js:
                for I, s in cols:
                    poly = clip(verts, lonl[I] + s, lonl[I + 1] + s, latl[J], latl[J + 1])
                    ax = area(poly, Re)
                    a_atm = (Re * Re) * (lonl[I + 1] * D2R - lonl[I] * D2R) * dsin[J]
                    if ax > 0.0 and ax > threshold * min(A, a_atm):
                        out.append((I, J, n, m, ax))
    counts["kept"] = len(out)
    return out, a_poly, counts


def as_arrays(lst):
    """(atm (n, 2) = (I, J), ocn (n, 2) = (n, m), area) of a list of exchange_grid()."""
    if not lst:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0)
    a = np.array([(e[0], e[1]) for e in lst], dtype=np.int32)
    o = np.array([(e[2], e[3]) for e in lst], dtype=np.int32)
    return a, o, np.array([e[4] for e in lst])

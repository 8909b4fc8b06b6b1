"""The cubed-sphere exchange grid of include/ogg_hip.h ("Exchange grid with a cubed-sphere atmosphere") written out directly: a loop
over ocean cells, candidate faces and their candidates, in plain Python floats (fp64, no fused multiply-add).  The arithmetic goes
through a small backend object, so scripts/xgrid_cs_truth.py runs the same statements in mpmath at 50 digits.  Test infrastructure
only: the tests compare the device's lists with it."""
import math

import numpy as np

COS_WIDE = 0.86602540378443864676
W_MIN = 0.05
COUNT_FIELDS = ("cells", "degenerate", "wide", "inverted", "masked", "face_candidates", "candidates", "kept")


class F64:
    """fp64: Python floats and the math module"""
    D = math.pi / 180.0
    one = 1.0
    num = staticmethod(float)
    cos, sin, sqrt, atan2 = math.cos, math.sin, math.sqrt, math.atan2


def mod360(x):
    return x % 360.0   # Python's float % has numpy's semantics: the sign of the divisor; exact


def unit_vector(x, y, M=F64):
    lam, phi = M.num(mod360(float(x))) * M.D, M.num(float(y)) * M.D
    cp = M.cos(phi)
    return (cp * M.cos(lam), cp * M.sin(lam), M.sin(phi))


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def omega3(a, b, c, M=F64):
    u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    v = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    return 2 * M.atan2(dot(a, n), 1 + dot(a, b) + dot(b, c) + dot(c, a))


def _r(p, M):
    return M.sqrt(1 + p[0] * p[0] + p[1] * p[1])


def _d(p, q, rp, rq):
    return (p[0] * q[0] + p[1] * q[1] + 1) / (rp * rq)


def omega2(a, b, c, M=F64):
    ra, rb, rc = _r(a, M), _r(b, M), _r(c, M)
    num = ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) / (ra * rb * rc)
    return 2 * M.atan2(num, 1 + _d(a, b, ra, rb) + _d(b, c, rb, rc) + _d(c, a, rc, ra))


def fan_area(verts, Re, M=F64):
    """A_x of a clipped polygon in (xi, eta): the fan from vertex 0"""
    s = M.num(0.0)
    for k in range(1, len(verts) - 1):
        s = s + omega2(verts[0], verts[k], verts[k + 1], M)
    return (Re * Re) * s


def a_atm(t, J, I, Re, M=F64):
    c00, c10, c11, c01 = (t[I], t[J]), (t[I + 1], t[J]), (t[I + 1], t[J + 1]), (t[I], t[J + 1])
    return (Re * Re) * (omega2(c00, c10, c11, M) + omega2(c00, c11, c01, M))


def a_atm_table(t, Re=6371.0e3):
    """A_atm (N x N) in fp64"""
    tl = [float(v) for v in t]
    N = len(tl) - 1
    return np.array([[a_atm(tl, J, I, Re) for I in range(N)] for J in range(N)])


def _inside(S, v, c):
    return (v[0] >= c, v[0] <= c, v[1] >= c, v[1] <= c)[S]


def _cross(S, a, b, c):
    if S < 2:
        e, f = (a, b) if (a[0], a[1]) <= (b[0], b[1]) else (b, a)
        return (c, e[1] + (c - e[0]) * ((f[1] - e[1]) / (f[0] - e[0])))
    e, f = (a, b) if (a[1], a[0]) <= (b[1], b[0]) else (b, a)
    return (e[0] + (c - e[1]) * ((f[0] - e[0]) / (f[1] - e[1])), c)


def clip(verts, clo, chi, blo, bhi):
    """the Sutherland-Hodgman of the lat-lon section (tests/xgrid_definition.py has the same statements), on (xi, eta)"""
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


def cell_status(cx, cy, Re, M=F64):
    """(status 'ok' / 'degenerate' / 'wide' / 'inverted', A_poly or None, the four unit vectors)"""
    if not all(math.isfinite(float(v)) for v in list(cx) + list(cy)):
        return "degenerate", None, None
    P = [unit_vector(cx[k], cy[k], M) for k in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            if dot(P[i], P[j]) < COS_WIDE:
                return "wide", None, P
    A = (Re * Re) * (omega3(P[0], P[1], P[2], M) + omega3(P[0], P[2], P[3], M))
    return ("ok" if A > 0 else "inverted"), A, P


def face_polygon(P, frame, M=F64):
    """the gnomonic polygon of a cell on a face, or None when the face is no candidate"""
    eu, ev, en = frame[0:3], frame[3:6], frame[6:9]
    w = [dot(p, en) for p in P]
    if not all(v > W_MIN for v in w):
        return None
    return [(dot(P[k], eu) / w[k], dot(P[k], ev) / w[k]) for k in range(4)]


def exchange_grid_cs(x, y, t, frames, mask=None, Re=6371.0e3, threshold=1.0e-6, rows=None, M=F64):
    """(list of (I, J, f, n, m, A_x) in the canonical order, A_poly (ny/2 x nx/2 of M's numbers, None where DEGENERATE or WIDE),
    counts dict, statuses).  ``rows``: the model rows to do (default all)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    tl = [M.num(float(v)) for v in np.asarray(t, dtype=np.float64)]
    fr = [[M.num(float(v)) for v in np.asarray(f, dtype=np.float64).reshape(9)] for f in frames]
    N = len(tl) - 1
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    a_poly = [[None] * nx for _ in range(ny)]
    counts = {f: 0 for f in COUNT_FIELDS}
    status = {}
    aatm = {}
    out = []
    ReM = M.num(float(Re))
    thr = M.num(float(threshold))
    for m in (range(ny) if rows is None else rows):
        for n in range(nx):
            cx = [x[2 * m, 2 * n], x[2 * m, 2 * n + 2], x[2 * m + 2, 2 * n + 2], x[2 * m + 2, 2 * n]]
            cy = [y[2 * m, 2 * n], y[2 * m, 2 * n + 2], y[2 * m + 2, 2 * n + 2], y[2 * m + 2, 2 * n]]
            counts["cells"] += 1
            masked = mask is not None and mask[m, n] == 0
            counts["masked"] += int(masked)
            st, A, P = cell_status(cx, cy, ReM, M)
            status[(m, n)] = st
            a_poly[m][n] = A
            if st != "ok":
                counts[st] += 1
                continue
            if masked:
                continue
            for f in range(6):
                poly = face_polygon(P, fr[f], M)
                if poly is None:
                    continue
                counts["face_candidates"] += 1
                xs, es = [v[0] for v in poly], [v[1] for v in poly]
                xmin, xmax, emin, emax = min(xs), max(xs), min(es), max(es)
                Js = [J for J in range(N) if tl[J] < emax and tl[J + 1] > emin]
                Is = [I for I in range(N) if tl[I] < xmax and tl[I + 1] > xmin]
                counts["candidates"] += len(Js) * len(Is)
                for J in Js:
                    for I in Is:
                        if tl[I] <= xmin and xmax <= tl[I + 1] and tl[J] <= emin and emax <= tl[J + 1]:
                            ax = A
                        else:
                            ax = fan_area(clip(poly, tl[I], tl[I + 1], tl[J], tl[J + 1]), ReM, M)
                        if (J, I) not in aatm:
                            aatm[(J, I)] = a_atm(tl, J, I, ReM, M)
                        if ax > 0 and ax > thr * min(A, aatm[(J, I)]):
                            out.append((I, J, f, n, m, ax))
    counts["kept"] = len(out)
    return out, a_poly, counts, status


def a_poly_array(a_poly):
    """A_poly as a float array, NaN where None"""
    return np.array([[np.nan if v is None else float(v) for v in row] for row in a_poly])


def as_arrays(lst):
    """(atm (n, 3) = (I, J, f), ocn (n, 2) = (n, m), area) of a list of exchange_grid_cs()."""
    if not lst:
        return np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int32), np.zeros(0)
    a = np.array([e[0:3] for e in lst], dtype=np.int32)
    o = np.array([e[3:5] for e in lst], dtype=np.int32)
    return a, o, np.array([float(e[5]) for e in lst])


# ---- the zoo: named grids, each (x, y) of a stitched supergrid ((2 ny + 1) x (2 nx + 1)) ------------------------------
def regional(lon0, lat0, dlon, dlat, nx, ny):
    """a regular regional supergrid of nx x ny model cells from (lon0, lat0), cells dlon x dlat degrees"""
    xs = lon0 + 0.5 * dlon * np.arange(2 * nx + 1)
    ys = lat0 + 0.5 * dlat * np.arange(2 * ny + 1)
    return np.broadcast_to(xs, (2 * ny + 1, 2 * nx + 1)).copy(), np.broadcast_to(ys[:, None], (2 * ny + 1, 2 * nx + 1)).copy()


def one_cell(corners):
    """the supergrid of one model cell of corners C0 .. C3 = [(x, y)] * 4 (the mid points are never read: they hold the means)"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = corners
    x = np.array([[x0, (x0 + x1) / 2, x1], [(x0 + x3) / 2, (x0 + x1 + x2 + x3) / 4, (x1 + x2) / 2], [x3, (x3 + x2) / 2, x2]])
    y = np.array([[y0, (y0 + y1) / 2, y1], [(y0 + y3) / 2, (y0 + y1 + y2 + y3) / 4, (y1 + y2) / 2], [y3, (y3 + y2) / 2, y2]])
    return x, y


CORNER_LAT = 35.264389682754654   # the cube corner of the default frames: (45, asin(1 / sqrt 3))


def zoo():
    """name -> (x, y, the status every cell of it must have, or None for 'ok' with pieces)"""
    z = {}
    for nx, ny in ((1, 1), (3, 2), (63, 1), (64, 1), (65, 1), (129, 1)):
        z["regional_%dx%d" % (ny, nx)] = regional(30.25, 20.5, 0.5, 0.75, nx, ny) + ("ok",)
    z["cube_corner"] = one_cell([(43.0, 33.0), (47.0, 33.0), (47.0, 37.5), (43.0, 37.5)]) + ("ok",)
    z["edge_on_xi_0"] = one_cell([(0.0, -3.0), (4.0, -3.0), (4.0, 2.0), (0.0, 2.0)]) + ("ok",)        # its west edge is xi = 0 of face 0
    z["edge_on_face_boundary"] = one_cell([(45.0, -3.0), (49.0, -3.0), (49.0, 2.0), (45.0, 2.0)]) + ("ok",)   # xi = 1 of face 0
    z["big_25"] = one_cell([(-12.0, -6.0), (13.0, -6.0), (13.0, 6.0), (-12.0, 6.0)]) + ("ok",)   # 25 degrees long, 27.7 corner to corner
    z["wide_31"] = one_cell([(0.0, -2.0), (31.0, -2.0), (31.0, 2.0), (0.0, 2.0)]) + ("wide",)
    z["nan_corner"] = one_cell([(10.0, 10.0), (12.0, 10.0), (np.nan, 12.0), (10.0, 12.0)]) + ("degenerate",)
    z["clockwise"] = one_cell([(10.0, 10.0), (10.0, 12.0), (12.0, 12.0), (12.0, 10.0)]) + ("inverted",)
    z["collapsed"] = one_cell([(10.0, 10.0), (10.0, 10.0), (10.0, 10.0), (10.0, 10.0)]) + ("inverted",)
    z["bow_tie"] = one_cell([(10.0, 10.0), (12.0, 10.0), (10.0, 12.0), (11.0, 12.25)]) + ("ok",)   # the lobes' areas 2 : 1
    # pole corners: one (each position) and two (each adjacent pair), north and south
    for k in range(4):
        ring = [(100.0, 88.0), (130.0, 88.0), (130.0, 89.0), (100.0, 89.0)]
        ring = ring[-k:] + ring[:-k] if k else ring
        c = list(ring)
        c[(2 + k) % 4] = (c[(2 + k) % 4][0], 90.0)
        z["pole_one_%d" % k] = one_cell(c) + ("ok",)
        c = list(ring)
        c[(2 + k) % 4] = (c[(2 + k) % 4][0], 90.0)
        c[(3 + k) % 4] = (c[(3 + k) % 4][0], 90.0)
        z["pole_two_%d" % k] = one_cell(c) + ("ok",)
    z["south_pole_two"] = one_cell([(200.0, -90.0), (220.0, -90.0), (220.0, -89.0), (200.0, -89.0)]) + ("ok",)
    return z

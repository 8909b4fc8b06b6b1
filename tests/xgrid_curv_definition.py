"""The curvilinear-source exchange grid of include/ogg_hip.h ("Exchange grid with a curvilinear source grid") written out directly: a
loop over model cells and their candidate source cells, in plain Python floats (fp64, no fused multiply-add).  The arithmetic goes
through the backend object M of tests/xgrid_cs_definition.py, so the same statements run in mpmath.  The candidates are the pairs
whose padded boxes meet; ``brute=True`` does that test on every pair in a plain double loop, the default finds them with numpy over the
boxes of all source cells at once.  Test infrastructure only: the tests compare the device's lists with it."""
import math

import numpy as np

import xgrid_cs_definition as cd
from xgrid_cs_definition import F64, dot, omega3

PAD0 = 2.0 ** -40
# every count of ogg_xgrid_curv_counts that the definition fixes (src_large is the index's own)
COUNT_FIELDS = ("cells", "degenerate", "wide", "inverted", "masked", "src_cells", "src_degenerate", "src_wide", "src_reversed", "src_flat",
                "src_masked", "candidates", "kept")


def normal(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def measure(p, n):
    return (p[0] * n[0] + p[1] * n[1]) + p[2] * n[2]


def fan4(P, Re, M=F64):
    return (Re * Re) * (omega3(P[0], P[1], P[2], M) + omega3(P[0], P[2], P[3], M))


def source_status(cx, cy, Re, M=F64):
    """(status 'ok' / 'degenerate' / 'wide' / 'flat', A_src or None, the oriented corner vectors, reversed)"""
    st, A, Q = cd.cell_status(cx, cy, Re, M)
    if st in ("degenerate", "wide"):
        return st, None, None, False
    reversed_ = False
    if st == "inverted":
        if A < 0:
            Q = [Q[0], Q[3], Q[2], Q[1]]
            A = fan4(Q, Re, M)
            reversed_ = True
        st = "ok" if A > 0 else "flat"
    return st, A, Q, reversed_ and st == "ok"


def padded_box(P):
    """(lo, hi) of four corner vectors: point location's box"""
    L2 = 0.0
    for v in range(4):
        for w in range(v + 1, 4):
            dx, dy, dz = P[v][0] - P[w][0], P[v][1] - P[w][1], P[v][2] - P[w][2]
            L2 = max(L2, (dx * dx + dy * dy) + dz * dz)
    pad = 0.25 * L2 + PAD0
    return ([min(p[a] for p in P) - pad for a in range(3)], [max(p[a] for p in P) + pad for a in range(3)])


def crossing(a, da, b, db, M=F64):
    (e, de), (f, df) = ((a, da), (b, db)) if tuple(a) <= tuple(b) else ((b, db), (a, da))
    t = de / (de - df)
    w = (e[0] + t * (f[0] - e[0]), e[1] + t * (f[1] - e[1]), e[2] + t * (f[2] - e[2]))
    r = M.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return (w[0] / r, w[1] / r, w[2] / r)


def edge_measure(v, Q, normals, e):
    """T(v; Q_e, Q_e+1), exactly 0 when v is one of the edge's own ends (shared corners)"""
    if tuple(v) == tuple(Q[e]) or tuple(v) == tuple(Q[(e + 1) % 4]):
        return 0 * v[0]
    return measure(v, normals[e])


def clip(verts, Q, normals, M=F64):
    """the Sutherland-Hodgman of the lat-lon section on unit vectors: a pass per half-space T >= 0"""
    for e in range(4):
        if not verts:
            return []
        d = [edge_measure(v, Q, normals, e) for v in verts]
        nv = len(verts)
        out = [verts[0]] if d[0] >= 0 else []
        for k in range(nv):
            j = (k + 1) % nv
            if (d[k] >= 0) != (d[j] >= 0):
                out.append(crossing(verts[k], d[k], verts[j], d[j], M))
            if k + 1 < nv and d[j] >= 0:
                out.append(verts[j])
        verts = out
    return verts


def fan_area(verts, Re, M=F64):
    s = M.num(0.0)
    for k in range(1, len(verts) - 1):
        s = s + omega3(verts[0], verts[k], verts[k + 1], M)
    return (Re * Re) * s


def overlap(P, A, Q, normals, Re, M=F64):
    """(A_x, the number of vertices of the clipped polygon, or None when the cell lies inside all four half-spaces)"""
    if all(edge_measure(p, Q, normals, e) >= 0 for e in range(4) for p in P):
        return A, None
    v = clip(list(P), Q, normals, M)
    return (fan_area(v, Re, M) if len(v) >= 3 else M.num(0.0)), len(v)


def exchange_grid_curv(x, y, sx, sy, mask=None, src_mask=None, Re=6371.0e3, threshold=1.0e-6, rows=None, brute=False, M=F64):
    """(list of (I, J, n, m, A_x) in the canonical order, A_poly (list of lists, None where DEGENERATE or WIDE), A_src (NB x NA,
    likewise), counts dict, target statuses {(m, n)}, source statuses {(J, I)}: 'ok' / 'reversed' / ..., the largest number of
    vertices of a clipped polygon, the candidates of every valid unmasked model cell {(m, n)})"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    sx, sy = np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64)
    NB, NA = sx.shape[0] - 1, sx.shape[1] - 1
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    ReM, thr = M.num(float(Re)), M.num(float(threshold))
    counts = {f: 0 for f in COUNT_FIELDS}
    a_src = [[None] * NA for _ in range(NB)]
    src_status, src = {}, {}
    slo, shi = np.full((NB * NA, 3), np.inf), np.full((NB * NA, 3), -np.inf)
    for J in range(NB):
        for I in range(NA):
            cx = [sx[J, I], sx[J, I + 1], sx[J + 1, I + 1], sx[J + 1, I]]
            cy = [sy[J, I], sy[J, I + 1], sy[J + 1, I + 1], sy[J + 1, I]]
            st, A, Q, rev = source_status(cx, cy, ReM, M)
            counts["src_cells"] += 1
            masked = src_mask is not None and src_mask[J, I] == 0
            counts["src_masked"] += int(masked)
            a_src[J][I] = A
            src_status[(J, I)] = "reversed" if rev else st
            if st != "ok":
                counts["src_" + st] += 1
                continue
            counts["src_reversed"] += int(rev)
            if masked:
                continue
            q = J * NA + I
            lo, hi = padded_box([[float(c) for c in p] for p in Q])
            slo[q], shi[q] = lo, hi
            src[q] = (A, Q, [normal(Q[e], Q[(e + 1) % 4]) for e in range(4)])
    a_poly = [[None] * nx for _ in range(ny)]
    status, out, nvmax, ncand = {}, [], 0, {}
    for m in (range(ny) if rows is None else rows):
        for n in range(nx):
            cx = [x[2 * m, 2 * n], x[2 * m, 2 * n + 2], x[2 * m + 2, 2 * n + 2], x[2 * m + 2, 2 * n]]
            cy = [y[2 * m, 2 * n], y[2 * m, 2 * n + 2], y[2 * m + 2, 2 * n + 2], y[2 * m + 2, 2 * n]]
            counts["cells"] += 1
            masked = mask is not None and mask[m, n] == 0
            counts["masked"] += int(masked)
            st, A, P = cd.cell_status(cx, cy, ReM, M)
            status[(m, n)] = st
            a_poly[m][n] = A
            if st != "ok":
                counts[st] += 1
                continue
            if masked:
                continue
            lo, hi = padded_box([[float(c) for c in p] for p in P])
            if brute:
                cand = [q for q in range(NB * NA)
                        if all(lo[a] <= shi[q, a] and slo[q, a] <= hi[a] for a in range(3))]
            else:
                cand = np.nonzero(np.all((np.array(lo) <= shi) & (slo <= np.array(hi)), axis=1))[0].tolist()
            counts["candidates"] += len(cand)
            ncand[(m, n)] = len(cand)
            for q in cand:
                As, Q, normals = src[q]
                ax, nv = overlap(P, A, Q, normals, ReM, M)
                nvmax = max(nvmax, nv or 0)
                if ax > 0 and ax > thr * min(A, As):
                    out.append((q % NA, q // NA, n, m, ax))
    counts["kept"] = len(out)
    return out, a_poly, a_src, counts, status, src_status, nvmax, ncand


def as_arrays(lst):
    """(src (n, 2) = (I, J), ocn (n, 2) = (n, m), area) of a list of exchange_grid_curv()"""
    if not lst:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0)
    return (np.array([e[0:2] for e in lst], dtype=np.int32), np.array([e[2:4] for e in lst], dtype=np.int32),
            np.array([float(e[4]) for e in lst]))


# ---- source meshes: (sx, sy), each (NB + 1) x (NA + 1) corners in degrees ----------------------------------------------
def _vec(lon, lat):
    lam, phi = np.radians(lon), np.radians(lat)
    return np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], axis=-1)


def _lonlat(V):
    return np.degrees(np.arctan2(V[..., 1], V[..., 0])), np.degrees(np.arcsin(np.clip(V[..., 2], -1.0, 1.0)))


def _rot(axis, angle):
    """the rotation by ``angle`` radians about the unit vector ``axis`` (Rodrigues)"""
    k = np.asarray(axis, dtype=np.float64)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def _to_centre(lonc, latc):
    """the rotation that takes (1, 0, 0) to the point (lonc, latc)"""
    return _rot((0.0, 0.0, 1.0), math.radians(lonc)) @ _rot((0.0, 1.0, 0.0), -math.radians(latc))


def rotated_mesh(lonc, latc, width, height, NA, NB, angle=0.4):
    """a regular NA x NB mesh of width x height degrees about the equator of its own frame, turned by ``angle`` radians about its
    centre, the centre put at (lonc, latc)"""
    lon, lat = np.meshgrid(np.linspace(-width / 2, width / 2, NA + 1), np.linspace(-height / 2, height / 2, NB + 1))
    R = _to_centre(lonc, latc) @ _rot((1.0, 0.0, 0.0), angle)
    return _lonlat(_vec(lon, lat) @ R.T)


def polar_fan(lonc, latc, radius, NA=8, NB=2):
    """a mesh about its own pole, the pole at (lonc, latc): NA sectors, NB rings out to ``radius`` degrees; the top row of corners is
    the pole itself, one pair of numbers, so the cells of the last row are triangles with a collapsed north edge"""
    lon, lat = np.meshgrid(np.linspace(0.0, 360.0, NA + 1), 90.0 - radius * np.arange(NB, -1, -1) / NB)
    R = _to_centre(lonc, latc) @ _rot((0.0, 1.0, 0.0), math.radians(90.0))   # its pole (0, 0, 1) to (1, 0, 0), then to the centre
    sx, sy = _lonlat(_vec(lon, lat) @ R.T)
    sx[NB, :], sy[NB, :] = lonc, latc
    sx[:, NA], sy[:, NA] = sx[:, 0], sy[:, 0]   # the seam: the same bits
    return sx, sy


def global_rotated(NA=24, NB=12, lonp=40.0, latp=65.0):
    """a global NA x NB lat-lon mesh in its own frame whose north pole lies at (lonp, latp): the pole rows are one pair of numbers each
    and the seam columns the same bits, so the mesh closes exactly"""
    lon, lat = np.meshgrid(np.linspace(-180.0, 180.0, NA + 1), np.linspace(-90.0, 90.0, NB + 1))
    R = _to_centre(lonp, latp) @ _rot((0.0, 1.0, 0.0), math.radians(90.0))
    sx, sy = _lonlat(_vec(lon, lat) @ R.T)
    sx[NB, :], sy[NB, :] = lonp, latp
    sx[0, :], sy[0, :] = (lonp + 180.0) % 360.0, -latp
    sx[:, NA], sy[:, NA] = sx[:, 0], sy[:, 0]
    return sx, sy


def regular_mesh(lon0, lat0, dlon, dlat, NA, NB):
    sx, sy = np.meshgrid(lon0 + dlon * np.arange(NA + 1), lat0 + dlat * np.arange(NB + 1))
    return sx.copy(), sy.copy()


def bad_cells_mesh(lonc, latc, d):
    """5 x 2 cells of d degrees about (lonc, latc) with a NaN corner (cell (0, 0) DEGENERATE), two coincident rows over one cell (cell
    (1, 1) FLAT, its neighbours (1, 0) and (1, 2) triangles) and a last column 31 degrees away (cells (0, 4) and (1, 4) WIDE)"""
    lon, lat = regular_mesh(-2.0 * d, -d, d, d, 5, 2)
    lat[2, 1:3] = lat[1, 1:3]
    lon[:, 5] = lon[:, 4] + 31.0
    sx, sy = _lonlat(_vec(lon, lat) @ _to_centre(lonc, latc).T)
    sx[0, 0] = np.nan
    return sx, sy


def centre_and_extent(x, y):
    """(lon, lat of the mean of the finite corner vectors of a supergrid's model corners, the largest angle in degrees from it)"""
    cx, cy = np.asarray(x)[0::2, 0::2].ravel(), np.asarray(y)[0::2, 0::2].ravel()
    ok = np.isfinite(cx) & np.isfinite(cy)
    V = _vec(cx[ok], cy[ok])
    c = V.mean(axis=0)
    c = c / np.linalg.norm(c)
    lonc, latc = _lonlat(c)
    return float(lonc), float(latc), float(np.degrees(np.arccos(np.clip(V @ c, -1.0, 1.0)).max()))


def sources_for(x, y):
    """name -> (sx, sy) of the source meshes the tests lay over the target x, y"""
    lonc, latc, ext = centre_and_extent(x, y)
    size = max(2.6 * ext, 2.0)
    rot = rotated_mesh(lonc, latc, size, 0.8 * size, 12, 9)
    s = {"rotated_12x9": rot, "north_to_south": (rot[0][::-1].copy(), rot[1][::-1].copy()),
         "pole_inside": polar_fan(lonc, latc, min(max(1.5 * ext, 1.0), 20.0)),
         "bad_cells": bad_cells_mesh(lonc, latc, min(max(ext, 0.5), 4.0)),
         "one_cell": rotated_mesh(lonc, latc, min(size, 20.0), min(size, 20.0), 1, 1)}
    return s

"""The definition of the basin codes (include/ogg_hip.h, "Basin codes") in plain numpy: the box predicate in its stated rounding order,
the seed cell by the key (bits of d2, cell) over the valid cells, and the rules as sequential floods by breadth-first search, one
after the other, each on what the earlier ones left.  No passes, no classes, no union-find: what the device must reproduce bit for
bit.  A plain module (numpy only)."""
from collections import deque

import numpy as np

TOOK, SEED_LAND, SEED_OUTSIDE, SEED_CODED, SEED_OFF_GRID, SEED_INVALID = range(6)
D = 0.017453292519943295   # pi / 180, the library's SPHERE_D
SEPARATION = 1.0e-9
FIELDS = ("code", "seed_lon", "seed_lat", "lon_w", "lon_e", "lat_s", "lat_n")
RECORD = np.dtype([("seed_cell", "<i8"), ("d2_bits", "<i8"), ("status", "<i4"), ("blocking_rule", "<i4"), ("cells", "<i8")])


def in_box(lon, lat, lon_w, lon_e, lat_s, lat_n):
    """the predicate, every operation rounded on its own, in the header's order (arrays or scalars of float64)"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    W = np.float64(lon_e) - np.float64(lon_w)
    t = lon - np.float64(lon_w)
    t = t - np.float64(360.0) * np.floor(t / np.float64(360.0))
    with np.errstate(invalid="ignore"):
        return (np.float64(lat_s) <= lat) & (lat <= np.float64(lat_n)) & ((W == 360.0) | (t <= W))


def centres(x, y):
    return np.ascontiguousarray(x[1::2, 1::2]), np.ascontiguousarray(y[1::2, 1::2])


def unit(lon, lat):
    """numpy's unit vectors (the device's differ in the last bit here and there: the GPU tests hand the device's own in)"""
    lon, lat = np.asarray(lon, np.float64) * D, np.asarray(lat, np.float64) * D
    cl = np.cos(lat)
    return np.stack([cl * np.cos(lon), cl * np.sin(lon), np.sin(lat)], axis=-1)


def seed_cell(u, valid, su):
    """(cell, d2 bits) of the valid cell nearest to the unit vector su by (bits of d2, cell); (-1, bits of +inf) without a valid cell"""
    v = np.flatnonzero(valid.reshape(-1))
    if v.size == 0:
        return -1, int(np.array(np.inf).view(np.int64))
    d = u.reshape(-1, 3)[v] - np.asarray(su, np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    bits = d2.view(np.uint64)
    k = int(np.argmin(bits))   # the first of the smallest: v ascends, so the smallest cell
    return int(v[k]), int(bits[k].astype(np.int64))


def neighbours(c, ny, nx, periodic, fold):
    j, i = divmod(c, nx)
    out = []
    if i + 1 < nx:
        out.append(c + 1)
    elif periodic:
        out.append(j * nx)
    if i > 0:
        out.append(c - 1)
    elif periodic:
        out.append(j * nx + nx - 1)
    if j + 1 < ny:
        out.append(c + nx)
    elif fold:
        out.append(j * nx + nx - 1 - i)
    if j > 0:
        out.append(c - nx)
    return out


def basin_codes(x, y, wet, rules, periodic, fold, u=None, su=None, seed_max_d2=np.inf):
    """code (uint8), rule (int16), records (RECORD) of the rules (rows (code, seed_lon, seed_lat, lon_w, lon_e, lat_s, lat_n)) run in
    order on the supergrid x, y and the wet bytes.  u (cells, 3) and su (rules, 3): the unit vectors of the centres and of the seeds
    (numpy's when None)."""
    lon, lat = centres(x, y)
    ny, nx = lon.shape
    valid = np.isfinite(lon) & np.isfinite(lat)
    wet = np.asarray(wet).reshape(ny, nx) != 0
    u = unit(lon.reshape(-1), lat.reshape(-1)) if u is None else np.asarray(u, np.float64).reshape(-1, 3)
    su = unit([r[1] for r in rules], [r[2] for r in rules]) if su is None else np.asarray(su, np.float64).reshape(-1, 3)
    code = np.zeros(ny * nx, np.uint8)
    rule = np.full(ny * nx, -1, np.int16)
    rec = np.zeros(len(rules), RECORD)
    for k, r in enumerate(rules):
        sc, bits = seed_cell(u, valid, su[k])
        rec[k] = (sc, bits, TOOK, -1, 0)
        if sc < 0:
            rec[k]["status"] = SEED_INVALID
            continue
        if np.array(bits, np.int64).view(np.float64) > seed_max_d2:
            rec[k]["status"] = SEED_OFF_GRID
            continue
        box = in_box(lon, lat, *r[3:7]).reshape(-1)
        if not wet.reshape(-1)[sc]:
            rec[k]["status"] = SEED_LAND
            continue
        if not box[sc]:
            rec[k]["status"] = SEED_OUTSIDE
            continue
        if code[sc] != 0:
            rec[k]["status"], rec[k]["blocking_rule"] = SEED_CODED, rule[sc]
            continue
        E = wet.reshape(-1) & valid.reshape(-1) & (code == 0) & box
        code[sc], rule[sc] = r[0], k
        todo, n = deque([sc]), 1
        while todo:
            c = todo.popleft()
            for q in neighbours(c, ny, nx, periodic, fold):
                if E[q] and rule[q] != k:
                    code[q], rule[q] = r[0], k
                    n += 1
                    todo.append(q)
        rec[k]["cells"] = n
    return code.reshape(ny, nx), rule.reshape(ny, nx), rec


def disjoint(a, b):
    """the planner's test of two rules' boxes: latitude intervals or longitude arcs separated by more than SEPARATION degrees"""
    if a[6] + SEPARATION < b[5] or b[6] + SEPARATION < a[5]:
        return True
    WA, WB = a[4] - a[3], b[4] - b[3]
    if WA >= 360.0 or WB >= 360.0:
        return False
    d = np.fmod(b[3] - a[3], 360.0)
    if d < 0.0:
        d += 360.0
    return bool(d > WA + SEPARATION and d + WB + SEPARATION < 360.0)


def boxes_share_a_point(a, b, step=0.25):
    """whether some (lon, lat) of a fine lattice over a's box is in both boxes by the predicate itself: what a planner must never batch"""
    lon = np.arange(a[3], a[4] + 0.5 * step, step)
    lat = np.arange(a[5], a[6] + 0.5 * step, step)
    LO, LA = np.meshgrid(np.append(lon, a[4]), np.append(lat, a[6]))
    return bool(np.any(in_box(LO, LA, *a[3:7]) & in_box(LO, LA, *b[3:7])))

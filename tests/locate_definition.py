"""Point location of include/ogg_hip.h ("Point location") written out in numpy, for the tests: the canonical corner table, the cells'
normals, orientation and boxes, the key m_c(p) by brute force over every (query, cell) pair, the fractional position, and the sampling
of a model field.  Test infrastructure only.  The corner table cu and the query vectors qu are inputs, as the coast-distance
definition takes its unit vectors: they may be the device's own (the device's sin / cos need not round as the host's do).  numpy
rounds every product and sum on its own (no FMA), which is the arithmetic the header fixes."""
import numpy as np

TOL = 2.0 ** -50
PAD0 = 2.0 ** -40
FILL = 1.0e20
CELL, BILINEAR = 0, 1
D = 0.017453292519943295   # pi / 180, as csrc/ogg_sphere.h has it


def unit(lon, lat):
    """unit vectors (n, 3) as ogg_sphere.h forms them (numpy's sin / cos)"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    with np.errstate(invalid="ignore"):
        cl = np.cos(lat * D)
        return np.stack([cl * np.cos(lon * D), cl * np.sin(lon * D), np.sin(lat * D)], axis=-1)


def corner_source(ny, nx, periodic, fold):
    """(ny + 1, nx + 1) flat corner index of the canonical copy of every corner"""
    J, I = np.indices((ny + 1, nx + 1))
    I = I.copy()
    if periodic:
        I[I == nx] = 0
    if fold:
        M = nx - I[ny]
        if periodic:
            M[M == nx] = 0
        I[ny] = np.minimum(I[ny], M)
    return J * (nx + 1) + I


def corner_table(x, y, periodic, fold, unit_of=unit):
    """cu ((ny + 1)(nx + 1), 3) of a supergrid x, y with numpy's unit vectors, canonical copies included"""
    x, y = np.asarray(x), np.asarray(y)
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    u = unit_of(x[0::2, 0::2].reshape(-1), y[0::2, 0::2].reshape(-1))
    return u[corner_source(ny, nx, periodic, fold).reshape(-1)]


def is_canonical(cu, ny, nx, periodic, fold):
    """every corner of the table has the bits of its canonical copy"""
    cu = np.ascontiguousarray(cu).reshape(-1, 3)
    return cu.tobytes() == cu[corner_source(ny, nx, periodic, fold).reshape(-1)].tobytes()


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot3(p, n):
    return (p[..., 0] * n[..., 0] + p[..., 1] * n[..., 1]) + p[..., 2] * n[..., 2]


def dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def cells(cu, ny, nx):
    """dict of per-cell arrays: q (nc, 4, 3) the corners a, b, c, d; n (nc, 4, 3) the normals n_S, n_E, n_N, n_W; sigma (nc,) in
    {+1, -1, 0}; lo, hi (nc, 3) the padded box (empty where sigma = 0)"""
    cu = np.asarray(cu, np.float64).reshape(ny + 1, nx + 1, 3)
    q = np.stack([cu[:-1, :-1], cu[:-1, 1:], cu[1:, 1:], cu[1:, :-1]], axis=2).reshape(ny * nx, 4, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.stack([cross(q[:, v], q[:, (v + 1) % 4]) for v in range(4)], axis=1)
        sv = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
        sn = (n[:, 0] + n[:, 1]) + (n[:, 2] + n[:, 3])
        O = dot3(sv, sn)
        fin = np.isfinite(O)
        sigma = np.where(fin & (O > 0), 1.0, np.where(fin & (O < 0), -1.0, 0.0))
        L2 = np.zeros(ny * nx)
        for v in range(4):
            for w in range(v + 1, 4):
                L2 = np.fmax(L2, dist2(q[:, v], q[:, w]))
        pad = 0.25 * L2 + PAD0
        lo = q.min(axis=1) - pad[:, None]
        hi = q.max(axis=1) + pad[:, None]
    ok = sigma != 0
    lo[~ok] = np.inf
    hi[~ok] = -np.inf
    return dict(q=q, n=n, sigma=sigma, lo=lo, hi=hi)


def keys(g, p, c):
    """sigma S, sigma E, sigma N, sigma W and m for the pairs (p[k], cell c[k])"""
    sg = g["sigma"][c]
    T = [sg * dot3(p, g["n"][c, v]) for v in range(4)]
    m = T[0]
    for v in (1, 2, 3):
        m = np.where(T[v] < m, T[v], m)
    return T, m


def _fraction(lo, hi, lo_c, hi_c, lo_sub, hi_sub):
    hi2 = np.where(hi_c, hi_sub - lo, hi)
    lo2 = np.where(lo_c, lo_sub - hi, lo)
    den = lo2 + hi2
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.clip(lo2 / den, 0.0, 1.0)
    return np.where((lo_c & hi_c) | ~(den > 0), 0.5, v)


def position(g, p, c):
    """s, t of the points p in their cells c"""
    (S, E, N, W), _ = keys(g, p, c)
    q, n, sg = g["q"][c], g["n"][c], g["sigma"][c]
    same = lambda a, b: (a.view(np.int64) == b.view(np.int64)).all(axis=-1)   # noqa: E731
    qq = np.ascontiguousarray(q)
    cS, cE, cN, cW = same(qq[:, 0], qq[:, 1]), same(qq[:, 1], qq[:, 2]), same(qq[:, 2], qq[:, 3]), same(qq[:, 3], qq[:, 0])
    s = _fraction(W, E, cW, cE, sg * dot3(q[:, 0], n[:, 1]), sg * dot3(q[:, 1], n[:, 3]))
    t = _fraction(S, N, cS, cN, sg * dot3(q[:, 0], n[:, 2]), sg * dot3(q[:, 2], n[:, 0]))
    return s, t


def locate(cu, qu, ny, nx, g=None, tol=TOL, pairs=8_000_000):
    """cell (int32), s, t, m (fp64) of the queries qu (n, 3): the definition, over EVERY (query, cell) pair whose box holds the query.
    The pairs are enumerated without a (query x cell) matrix: the finite queries are sorted by their z, so the queries within a cell's z
    range [lo_z, hi_z] are one run of that order (two exact binary searches), and the x and y ranges and the key are tested on those
    runs.  ``tol``: the candidate threshold (inf: every cell whose box holds the query, so that m is the best key whatever its sign)."""
    g = cells(cu, ny, nx) if g is None else g
    qu = np.asarray(qu, np.float64).reshape(-1, 3)
    n = qu.shape[0]
    best_c = np.full(n, np.iinfo(np.int64).max, np.int64)
    best_m = np.full(n, -np.inf)
    s, t = np.full(n, np.nan), np.full(n, np.nan)
    kf = np.nonzero(np.isfinite(qu).all(axis=1))[0]
    order = kf[np.argsort(qu[kf, 2], kind="stable")]
    pz = qu[order, 2]
    lo, hi = g["lo"], g["hi"]
    vc = np.nonzero(g["sigma"] != 0)[0]
    a = np.searchsorted(pz, lo[vc, 2], side="left")
    cnt = np.maximum(np.searchsorted(pz, hi[vc, 2], side="right") - a, 0)
    ends = np.cumsum(cnt)
    g0 = 0
    while g0 < vc.size:
        g1 = max(g0 + 1, int(np.searchsorted(ends, (ends[g0 - 1] if g0 else 0) + pairs, side="right")))
        cg, ag, ng = vc[g0:g1], a[g0:g1], cnt[g0:g1]
        g0 = g1
        tot = int(ng.sum())
        if tot == 0:
            continue
        kc = np.repeat(cg, ng)
        kq = order[np.repeat(ag, ng) + (np.arange(tot) - np.repeat(np.cumsum(ng) - ng, ng))]
        p = qu[kq]
        inbox = ((p[:, 0] >= lo[kc, 0]) & (p[:, 0] <= hi[kc, 0]) & (p[:, 1] >= lo[kc, 1]) & (p[:, 1] <= hi[kc, 1]) &
                 (p[:, 2] >= lo[kc, 2]) & (p[:, 2] <= hi[kc, 2]))
        kq, kc = kq[inbox], kc[inbox]
        _, mm = keys(g, qu[kq], kc)
        cand = mm >= -tol
        kq, kc, mm = kq[cand], kc[cand], mm[cand]
        if kq.size == 0:
            continue
        o = np.lexsort((kc, -mm, kq))   # per query: the largest m first, ties to the smaller cell (-0.0 and 0.0 compare equal)
        kq, kc, mm = kq[o], kc[o], mm[o]
        first = np.ones(kq.size, bool)
        first[1:] = kq[1:] != kq[:-1]
        kq, kc, mm = kq[first], kc[first], mm[first]
        better = (mm > best_m[kq]) | ((mm == best_m[kq]) & (kc < best_c[kq]))
        best_m[kq[better]], best_c[kq[better]] = mm[better], kc[better]
    has = best_c < ny * nx
    cell = np.where(has, best_c, -1).astype(np.int32)
    m = np.where(has, best_m, np.nan)
    if has.any():
        s[has], t[has] = position(g, qu[has], cell[has])
    return cell, s, t, m


def locate_matrix(cu, qu, ny, nx, tol=TOL):
    """locate() by the plain (query x cell) matrix, for small inputs: the cross-check of the enumeration above"""
    g = cells(cu, ny, nx)
    qu = np.asarray(qu, np.float64).reshape(-1, 3)
    n, nc = qu.shape[0], ny * nx
    with np.errstate(invalid="ignore"):
        inbox = np.isfinite(qu).all(axis=1)[:, None] & np.ones((n, nc), bool)
        for ax in range(3):
            inbox &= (qu[:, ax, None] >= g["lo"][None, :, ax]) & (qu[:, ax, None] <= g["hi"][None, :, ax])
    cell = np.full(n, -1, np.int32)
    m = np.full(n, np.nan)
    for k in range(n):
        c = np.nonzero(inbox[k])[0]
        if c.size:
            _, mm = keys(g, np.repeat(qu[k][None], c.size, axis=0), c)
            ok = mm >= -tol
            if ok.any():
                c, mm = c[ok], mm[ok]
                j = np.lexsort((c, -mm))[0]
                cell[k], m[k] = c[j], mm[j]
    return cell, m


# ---- sampling ------------------------------------------------------------------------------------------------------
def face_neighbours(c, ny, nx, periodic, fold):
    """S, W, E, N of the cells c (-1: none, also for c = -1), as csrc/ogg_cells.h"""
    c = np.asarray(c, np.int64)
    j, i = c // nx, c % nx
    S = np.where(j > 0, c - nx, -1)
    W = np.where(i > 0, c - 1, c + nx - 1 if periodic else -1)
    E = np.where(i < nx - 1, c + 1, c - (nx - 1) if periodic else -1)
    N = np.where(j < ny - 1, c + nx, j * nx + (nx - 1 - i) if fold else -1)
    return [np.where(c >= 0, v, -1) for v in (S, W, E, N)]


def missing(v, fills):
    m = v != v
    for f in fills:
        m |= v == v.dtype.type(f)
    return m


def stencil(cell, s, t, ny, nx, periodic, fold, mode):
    """the cells (4, n) C00, C10, C01, C11 (-1: none) and their weights (4, n) (CELL: the first row alone counts)"""
    cell = np.asarray(cell, np.int64)
    n = cell.size
    idx = np.full((4, n), -1, np.int64)
    w = np.zeros((4, n))
    idx[0], w[0] = cell, 1.0
    if mode == BILINEAR:
        with np.errstate(invalid="ignore"):
            fx, fy = np.abs(s - 0.5), np.abs(t - 0.5)
            east, north = s >= 0.5, t >= 0.5
        S, W, E, N = face_neighbours(cell, ny, nx, periodic, fold)
        idx[1] = np.where(east, E, W)
        idx[2] = np.where(north, N, S)
        S1, _, _, N1 = face_neighbours(idx[1], ny, nx, periodic, fold)
        idx[3] = np.where(north, N1, S1)
        gx, gy = 1.0 - fx, 1.0 - fy
        w[0], w[1], w[2], w[3] = gx * gy, fx * gy, gx * fy, fx * fy
    return idx, w


def sample(cell, s, t, f, wet, ny, nx, periodic, fold, mode=BILINEAR, fills=()):
    """values (nrec, n) fp64 and flags (nrec, n) uint8 of the field f (nrec, ny, nx) at located points"""
    f = np.asarray(f).reshape(-1, ny * nx)
    cell = np.asarray(cell, np.int64)
    n, nrec = cell.size, f.shape[0]
    ncell = 4 if mode == BILINEAR else 1
    idx, w = stencil(cell, s, t, ny, nx, periodic, fold, mode)
    wetf = None if wet is None else (np.asarray(wet).reshape(-1) != 0)
    has = cell >= 0
    dry = has & (~wetf[np.maximum(cell, 0)] if wetf is not None else False)
    values = np.full((nrec, n), FILL)
    flags = np.zeros((nrec, n), np.uint8)
    for r in range(nrec):
        Wt, St, used = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
        for q in range(ncell):
            k = np.maximum(idx[q], 0)
            fv = f[r][k]
            ok = has & ~dry & (idx[q] >= 0) & ~missing(fv, fills)
            if wetf is not None:
                ok &= wetf[k]
            with np.errstate(invalid="ignore", over="ignore"):
                Wt = np.where(ok, Wt + w[q], Wt)
                St = np.where(ok, St + w[q] * fv.astype(np.float64), St)
            used += ok
        good = has & (used > 0) & (Wt > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            values[r] = np.where(good, St / Wt, FILL)
        flags[r] = np.where(~has, 0, np.where(~good, 3, np.where(used == ncell, 1, 2)))
    return values, flags


# ---- query sets ----------------------------------------------------------------------------------------------------
def ulp_neighbours(lon, lat):
    """the points one ulp to either side in longitude and in latitude (4 n points)"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    return (np.concatenate([np.nextafter(lon, np.inf), np.nextafter(lon, -np.inf), lon, lon]),
            np.concatenate([lat, lat, np.nextafter(lat, np.inf), np.nextafter(lat, -np.inf)]))


def mesh_queries(x, y):
    """the supergrid's own points (corners, edge midpoints, centres) and their 1-ulp neighbours: lon, lat"""
    lon, lat = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    ul, ua = ulp_neighbours(lon, lat)
    return np.concatenate([lon, ul]), np.concatenate([lat, ua])


def jittered_mesh(spacing, lat0, ny=12, nx=14, seed=0, lon0=10.0):
    """a supergrid x, y of ny x nx cells of ``spacing`` degrees from (lon0, lat0) whose interior corners are moved by up to 0.2 of
    the spacing; midpoints as means of the corners"""
    rng = np.random.default_rng(seed)
    cx, cy = np.meshgrid(lon0 + spacing * np.arange(nx + 1), lat0 + spacing * np.arange(ny + 1))
    cx[1:-1, 1:-1] += spacing * 0.2 * (2 * rng.random((ny - 1, nx - 1)) - 1)
    cy[1:-1, 1:-1] += spacing * 0.2 * (2 * rng.random((ny - 1, nx - 1)) - 1)
    x, y = np.zeros((2 * ny + 1, 2 * nx + 1)), np.zeros((2 * ny + 1, 2 * nx + 1))
    for full, c in ((x, cx), (y, cy)):
        full[0::2, 0::2] = c
        full[0::2, 1::2] = (c[:, :-1] + c[:, 1:]) / 2
        full[1::2, 0::2] = (c[:-1] + c[1:]) / 2
        full[1::2, 1::2] = (full[1::2, 0:-1:2] + full[1::2, 2::2]) / 2
    return x, y

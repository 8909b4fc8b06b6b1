"""The conservative remap of include/ogg_hip.h ("Conservative remap") written out in numpy, for the tests: the segmented sums in list
order and the fill by fronts.  Every operation is an elementwise IEEE fp64 operation on the records (a numpy array per entry, per
neighbour), so each (record, cell) value is formed by the same additions in the same order as the definition says.  Test
infrastructure only: it takes the device's exchange list as its input (that list is checked against xgrid_definition.py)."""
import numpy as np

FILL = 1.0e20
DRY, REMAPPED, FILLED, UNFILLED = 0, 1, 2, 3


def remap(atm, ocn, area, f, ny, nx, fills=(), mask=None):
    """values, flags (nrec, ny, nx) before the fill: f (nrec, NB, NA) float32 / float64, fills compared in f's type"""
    f = np.asarray(f)
    nrec, NB, NA = f.shape
    fr = f.reshape(nrec, NB * NA)
    cell = ocn[:, 1].astype(np.int64) * nx + ocn[:, 0]
    src = atm[:, 1].astype(np.int64) * NA + atm[:, 0]
    ncell = ny * nx
    start = np.zeros(ncell, np.int64)
    count = np.bincount(cell, minlength=ncell)
    first = np.r_[True, cell[1:] != cell[:-1]] if cell.size else np.zeros(0, bool)
    start[cell[first]] = np.nonzero(first)[0]
    W = np.zeros((nrec, ncell))
    S = np.zeros((nrec, ncell))
    for t in range(int(count.max()) if count.size and cell.size else 0):   # the t-th entry of every cell, left to right
        cs = np.nonzero(count > t)[0]
        e = start[cs] + t
        v = fr[:, src[e]]
        ok = ~np.isnan(v)
        for fv in fills:
            ok &= v != f.dtype.type(fv)
        a = np.broadcast_to(area[e], v.shape)
        W[:, cs] = np.where(ok, W[:, cs] + a, W[:, cs])
        S[:, cs] = np.where(ok, S[:, cs] + a * v.astype(np.float64), S[:, cs])
    wet = np.ones(ncell, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    values = np.full((nrec, ncell), FILL)
    flags = np.full((nrec, ncell), UNFILLED, np.uint8)
    rem = W > 0
    values[rem] = S[rem] / W[rem]
    flags[rem] = REMAPPED
    flags[:, ~wet] = DRY
    values[:, ~wet] = FILL
    return values.reshape(nrec, ny, nx), flags.reshape(nrec, ny, nx)


def neighbours(ny, nx, periodic, fold):
    """(4, ny * nx) cell indices of S, W, E, N, -1 for none"""
    j, i = np.divmod(np.arange(ny * nx), nx)
    c = j * nx + i
    s = np.where(j > 0, c - nx, -1)
    w = np.where(i > 0, c - 1, c + nx - 1 if periodic else -1)
    e = np.where(i < nx - 1, c + 1, c - (nx - 1) if periodic else -1)
    n = np.where(j < ny - 1, c + nx, j * nx + (nx - 1 - i) if fold else -1)
    return np.stack([s, w, e, n])


def fill(values, flags, periodic, fold, fill_max=None):
    """the fill by fronts: values, flags and the largest distance filled"""
    nrec, ny, nx = values.shape
    v, fl = values.reshape(nrec, -1).copy(), flags.reshape(nrec, -1).copy()
    nb = neighbours(ny, nx, periodic, fold)
    dist = np.where(fl == REMAPPED, 0, -1)
    k = 0
    while fill_max is None or k < fill_max:
        k += 1
        at = np.zeros(v.shape, bool)
        for d in range(4):
            ok = nb[d] >= 0
            at[:, ok] |= dist[:, nb[d][ok]] == k - 1
        front = at & (fl == UNFILLED) & (dist < 0)
        if not front.any():
            k -= 1
            break
        s = np.zeros(v.shape)
        m = np.zeros(v.shape)
        for d in range(4):   # S, W, E, N, left to right
            ok = nb[d] >= 0
            hit = np.zeros(v.shape, bool)
            hit[:, ok] = dist[:, nb[d][ok]] == k - 1
            src = np.zeros(v.shape)
            src[:, ok] = v[:, nb[d][ok]]
            s = np.where(hit, s + src, s)
            m += hit
        v[front] = s[front] / m[front]
        fl[front] = FILLED
        dist[front] = k
    return v.reshape(values.shape), fl.reshape(flags.shape), int(dist.max()) if dist.size else 0

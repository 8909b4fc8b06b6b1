"""The definition of the runoff spreading (include/ogg_hip.h, "Runoff spreading") in numpy: a loop over the mouths in ascending cell
order, the weights as int64 q, W_m their exact sum, s = q / W_m, and the per-cell sums built up mouth by mouth, so every cell's terms
arrive in ascending mouth order.  Only correctly rounded + - * / and floor: the device must give the same bits from the same unit
vectors and areas.

``prune`` looks only at the candidates whose z lies within the radius of the mouth's z (a latitude window: the chord is at least the
difference of the z components); tests/test_runoff_spread_cpu.py shows that it changes no byte."""
import math

import numpy as np

D = np.pi / 180.0
UNIFORM, BIWEIGHT = 0, 1
SHAPES = {"uniform": UNIFORM, "biweight": BIWEIGHT}
RE = 6371.0e3


def unit(lon, lat):
    lam, phi = np.asarray(lon) * D, np.asarray(lat) * D
    return np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], -1)


def radius2(km, Re=RE):
    """r2 as the package forms it"""
    half = 0.5 * (km * 1e3 / Re)
    if half >= 0.5 * math.pi:
        return 4.0
    s = math.sin(half)
    return (2 * s) * (2 * s)


def cell_area(area):
    """A_c from the supergrid area, in the mapping's order"""
    a = np.asarray(area, dtype=np.float64)
    return ((a[0::2, 0::2] + a[1::2, 1::2]) + (a[0::2, 1::2] + a[1::2, 0::2])).reshape(-1)


def centres(x, y):
    return np.asarray(x)[1::2, 1::2].reshape(-1), np.asarray(y)[1::2, 1::2].reshape(-1)


def candidates(A, wet, lon, lat):
    with np.errstate(invalid="ignore"):
        return (np.asarray(wet).reshape(-1) != 0) & np.isfinite(lon) & np.isfinite(lat) & (A > 0) & (A < np.inf)


def dist2(um, u):
    d = um - u
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def weights(At, Am, d2, r2, shape):
    """q(m, t) as int64"""
    a = np.minimum(At / Am, 256.0)
    if shape == UNIFORM:
        g = np.ones(At.size)
    else:
        h = 1.0 - d2 / r2
        g = h * h
    return np.floor((a * g) * 16777216.0).astype(np.int64)


def spread(v, A, u, cand, load, r2, shape, cls=None, prune=False):
    """v (nrec, n), A (n), u (n, 3), cand (n booleans), load (n), cls None or (n): a dict of out (nrec, n), n_mouths, mouth_cell,
    mouth_n, mouth_W and the counts the definition fixes.  A mouth that is no candidate: ValueError naming the first."""
    assert 0 < r2 <= 4
    v = np.asarray(v, dtype=np.float64)
    nrec, n = v.shape
    mouths = np.nonzero(np.asarray(load).reshape(-1) > 0)[0]
    bad = mouths[~cand[mouths]]
    if bad.size:
        raise ValueError("mouth cell %d is no candidate" % bad[0])
    ci = np.nonzero(cand)[0]
    if prune:
        order = np.argsort(u[ci, 2], kind="stable")
        zs = u[ci, 2][order]
        rr = math.sqrt(r2) * (1.0 + 1e-9) + 1e-12
    T = np.zeros((nrec, n))
    nm = np.zeros(n, np.int32)
    mouth_n, mouth_W = np.zeros(mouths.size, np.int32), np.zeros(mouths.size, np.int64)
    for k, m in enumerate(mouths):
        if prune:
            lo, hi = np.searchsorted(zs, u[m, 2] - rr, "left"), np.searchsorted(zs, u[m, 2] + rr, "right")
            sub = np.sort(ci[order[lo:hi]])
        else:
            sub = ci
        d2 = dist2(u[m], u[sub])
        keep = d2 <= r2
        if cls is not None:
            keep &= cls[sub] == cls[m]
        t, d2 = sub[keep], d2[keep]
        q = weights(A[t], A[m], d2, r2, shape)
        W = int(q.sum())
        assert W > 0 and m in t
        s = q.astype(np.float64) / np.float64(W)
        for r in range(nrec):
            F = v[r, m] * A[m]
            T[r, t] = T[r, t] + F * s
        nm[t] += 1
        mouth_n[k], mouth_W[k] = t.size, W
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(nm > 0, T / np.where(nm > 0, A, 1.0), 0.0)
    counts = dict(candidates=int(cand.sum()), mouths=int(mouths.size), pairs=int(mouth_n.sum(dtype=np.int64)),
                  max_receivers=int(mouth_n.max(initial=0)), loaded=int((nm > 0).sum()), max_mouths=int(nm.max(initial=0)))
    return dict(out=out, n_mouths=nm, mouth_cell=mouths.astype(np.int32), mouth_n=mouth_n, mouth_W=mouth_W, counts=counts)


def conservation(out, v, A, mouth_cell):
    """per record: |fsum(out A) - fsum(v A)| and fsum(|v| A), v A over the mouths"""
    res = []
    for r in range(v.shape[0]):
        f = v[r][mouth_cell] * A[mouth_cell]
        res.append((abs(math.fsum(out[r] * A) - math.fsum(f)), math.fsum(np.abs(f))))
    return res

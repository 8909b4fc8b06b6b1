"""The ocean mask of include/ogg_hip.h ("Ocean mask"), written directly in numpy: the wet rule, the face graph as explicit edge lists
(with the periodic seam and the fold), connected components by hooking and pointer jumping (the root of a component is its smallest
linear index), then the selection.  No scipy.  The tests compare the library with this bit for bit."""
import numpy as np

FILL = 1.0e20


def wet_rule(depth, fill=FILL, min_depth=0.0, mode="mask"):
    """(wet after the rule, wet before it, shallow): a cell starts wet when depth > 0 and != fill; mode mask makes the shallow ones land"""
    d = np.asarray(depth, dtype=np.float64)
    wet0 = (d > 0) & (d != fill)
    shallow = wet0 & (d < min_depth)
    wet = wet0 & ~shallow if mode == "mask" else wet0.copy()
    return wet, wet0, shallow


def edges(ny, nx, periodic, fold):
    """(a, b) linear indices of every face of the ny x nx cells"""
    idx = np.arange(ny * nx, dtype=np.int64).reshape(ny, nx)
    a = [idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    b = [idx[:, 1:].ravel(), idx[1:, :].ravel()]
    if periodic and nx > 1:
        a.append(idx[:, nx - 1])
        b.append(idx[:, 0])
    if fold:
        i = np.arange(nx // 2)
        a.append(idx[ny - 1, i])
        b.append(idx[ny - 1, nx - 1 - i])
    return np.concatenate(a), np.concatenate(b)


def roots(wet, periodic=False, fold=False):
    """root[c] (int32, -1 for land): the smallest linear index of c's component of wet cells connected through faces"""
    wet = np.asarray(wet, dtype=bool)
    ny, nx = wet.shape
    n = ny * nx
    w = wet.ravel()
    a, b = edges(ny, nx, periodic, fold)
    keep = w[a] & w[b]
    a, b = a[keep], b[keep]
    parent = np.arange(n, dtype=np.int64)
    while True:
        pa, pb = parent[a], parent[b]
        differ = pa != pb
        if not np.any(differ):
            break
        lo, hi = np.minimum(pa, pb)[differ], np.maximum(pa, pb)[differ]
        np.minimum.at(parent, hi, lo)   # hook every root under the smallest root next to it
        while True:   # pointer jumping until every cell points at a root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    out = np.where(w, parent, -1).astype(np.int32)
    return out.reshape(ny, nx)


def centres(x, y):
    """model-cell centres: supergrid points (2j+1, 2i+1)"""
    return np.asarray(x)[1::2, 1::2], np.asarray(y)[1::2, 1::2]


def unit(lon, lat):
    D = np.pi / 180.0
    lon, lat = np.asarray(lon, dtype=np.float64) * D, np.asarray(lat, dtype=np.float64) * D
    return np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)


def seed_cell(x, y, lon, lat):
    """the linear index of the model cell whose centre is nearest (squared chordal distance), ties to the smaller index"""
    cx, cy = centres(x, y)
    ux, uy, uz = unit(cx, cy)
    sx, sy, sz = unit(lon, lat)
    d2 = ((ux - sx) * (ux - sx) + (uy - sy) * (uy - sy)) + (uz - sz) * (uz - sz)
    return int(np.argmin(d2.ravel()))   # argmin takes the first of equal values


def ocean_mask(depth, x=None, y=None, min_depth=0.0, mode="mask", seeds=(), keep_min_cells=0, periodic=False, fold=False, fill=FILL):
    """dict: depth (edited), wet (uint8), root, kept_roots, seed_cells, n_components, sizes {root: cells}"""
    d = np.asarray(depth, dtype=np.float64)
    wet, wet0, shallow = wet_rule(d, fill, min_depth, mode)
    root = roots(wet, periodic, fold)
    r = root.ravel()
    labelled = r[r >= 0]
    cnt = np.bincount(labelled, minlength=d.size) if labelled.size else np.zeros(d.size, np.int64)
    comp = np.flatnonzero(cnt)
    kept, cells = set(), []
    for lon, lat in seeds:
        c = seed_cell(x, y, lon, lat)
        if r[c] < 0:
            raise ValueError("seed (%g, %g) lies on land: cell %d" % (lon, lat, c))
        cells.append(c)
        kept.add(int(r[c]))
    if not seeds and comp.size:
        big = cnt[comp].max()
        kept.add(int(comp[cnt[comp] == big].min()))
    if keep_min_cells > 0:
        kept |= set(int(c) for c in comp[cnt[comp] >= keep_min_cells])
    keep = np.isin(r, np.array(sorted(kept), dtype=np.int64)) & (r >= 0)
    out = d.ravel().copy()
    flat_wet0 = wet0.ravel()
    out[flat_wet0 & ~keep] = 0.0
    deep = keep & shallow.ravel()
    out[deep] = min_depth
    return {"depth": out.reshape(d.shape), "wet": keep.reshape(d.shape).astype(np.uint8), "root": root, "kept_roots": sorted(kept),
            "seed_cells": cells, "n_components": int(comp.size), "sizes": dict(zip(comp.tolist(), cnt[comp].tolist())),
            "masked": int(np.sum(shallow)) if mode == "mask" else 0, "deepened": int(np.sum(shallow)) if mode == "deepen" else 0,
            "removed": int(np.sum((r >= 0) & ~keep))}

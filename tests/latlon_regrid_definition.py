"""The numpy definition of the conservative regrid to a lat-lon grid (include/ogg_hip.h, "Conservative regrid to a lat-lon grid"):
the list transposed to target-cell order by its keys (k << 32) | position, then np.bincount over the transposed entries, which adds
each target cell's weights left to right from +0.0 in that order.  The products of missing values are zeroed before the sum (adding
+0.0 to a sum that starts at +0.0 changes no bit), so the sums are the definition's over the entries whose value is not missing."""
import numpy as np

FILL = 1.0e20


def keys(atm, NA):
    return atm[:, 1].astype(np.int64) * NA + atm[:, 0]


def transpose(atm, NA):
    """the permutation of the list into target-cell order, ascending list position within a cell, and the target cell of each slot"""
    k = keys(atm, NA)
    order = np.argsort((k << 32) | np.arange(k.size, dtype=np.int64), kind="stable")
    return order, k[order]


def static(atm, area, a_atm):
    """ocean_frac (NB, NA) and n_entries (NB, NA) int32"""
    NB, NA = a_atm.shape
    order, kt = transpose(atm, NA)
    W0 = np.bincount(kt, weights=area[order], minlength=NA * NB).reshape(NB, NA)
    return W0 / a_atm, np.bincount(kt, minlength=NA * NB).reshape(NB, NA).astype(np.int32)


def missing(v, fills):
    m = np.isnan(v)
    for f in fills:
        m |= v == v.dtype.type(f)
    return m


def regrid(atm, ocn, area, g, a_atm, fills=(), normalize="area"):
    """values and cover (nrec, NB, NA) of the field g (nrec, ny, nx) of float32 or float64"""
    NB, NA = a_atm.shape
    nrec, ny, nx = g.shape
    order, kt = transpose(atm, NA)
    c = (ocn[order, 1].astype(np.int64) * nx + ocn[order, 0])
    a = area[order]
    values = np.empty((nrec, NB, NA))
    cover = np.empty((nrec, NB, NA))
    for r in range(nrec):
        v = g[r].reshape(-1)[c]
        miss = missing(v, fills)
        w = np.where(miss, 0.0, a)
        p = np.where(miss, 0.0, a * v.astype(np.float64))
        W = np.bincount(kt, weights=w, minlength=NA * NB).reshape(NB, NA)
        S = np.bincount(kt, weights=p, minlength=NA * NB).reshape(NB, NA)
        with np.errstate(divide="ignore", invalid="ignore"):
            if normalize == "area":
                values[r] = np.where(W > 0, S / W, FILL)
            else:
                values[r] = np.where(W > 0, S / a_atm, 0.0)
        cover[r] = W / a_atm
    return values, cover

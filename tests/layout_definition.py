"""The definition of the processor layouts and mask tables (include/ogg_hip.h, "Processor layouts and mask tables") in numpy and
Python integers, sharing nothing with the library's approach: the extent rule restated literally with both arrays, a block's
neighbourhood built cell by cell through the index mapping (no summed-area table), the record, the ranking and the table text."""
import numpy as np

TOO_FINE, FOLD_ASYMMETRIC = 1, 2
MAX_DIV = 4096
FIELDS = ("blocks", "masked", "pes", "max_block_cells", "max_block_edge", "min_block_size", "max_wet", "masked_cells", "wet_total",
          "status")


def is_symmetric(npts, ndivs):
    if ndivs % 2 == 1 and npts % 2 == 0:
        return ndivs < npts // 2
    return ndivs % 2 == npts % 2


def extent(npts, ndivs):
    """(begin, end) lists of the rule, as the header states it"""
    assert 1 <= ndivs <= npts
    isg, ieg = 0, npts - 1
    sym = is_symmetric(npts, ndivs)
    begin, end = [None] * ndivs, [None] * ndivs
    is_, imax, ndmax = 0, ieg, ndivs
    for nd in range(ndivs):
        if nd < (ndivs - 1) // 2 + 1:
            ie = is_ + -(-(imax - is_ + 1) // (ndmax - nd)) - 1
            m = ndivs - 1 - nd
            if m > nd and sym:
                begin[m] = max(isg + ieg - ie, ie + 1)
                end[m] = max(isg + ieg - is_, ie + 1)
                imax = begin[m] - 1
                ndmax = ndmax - 1
        elif sym:
            is_, ie = begin[nd], end[nd]
        else:
            ie = is_ + -(-(imax - is_ + 1) // (ndmax - nd)) - 1
        begin[nd], end[nd] = is_, ie
        is_ = ie + 1
    return begin, end


def neighbourhood(ny, nx, periodic, fold, h, by, ey, bx, ex):
    """the set of cells (j, i) of the block's neighbourhood, cell by cell"""
    cells = set()
    for j in range(by - h, ey + h + 1):
        for i in range(bx - h, ex + h + 1):
            if i < 0 or i >= nx:
                if not periodic:
                    continue
                i = i % nx
            if j < 0:
                continue
            if j >= ny:
                k = j - ny
                if not fold or k >= ny:
                    continue
                cells.add((ny - 1 - k, nx - 1 - i))
            else:
                cells.add((j, i))
    return cells


def reached(ny, nx, periodic, fold, h, by, ey, bx, ex):
    """neighbourhood() as a boolean (ny, nx) array: the same index mapping applied to every (j, i) of the halo box at once"""
    j, i = np.broadcast_arrays(np.arange(by - h, ey + h + 1)[:, None], np.arange(bx - h, ex + h + 1)[None, :])
    outside = (i < 0) | (i >= nx)
    ok = np.ones(j.shape, bool) if periodic else ~outside
    i = np.where(outside, i % nx, i)
    ok &= j >= 0
    past = j >= ny
    k = j - ny
    ok &= ~past | (bool(fold) & (k < ny))
    jj, ii = np.where(past, ny - 1 - k, j), np.where(past, nx - 1 - i, i)
    out = np.zeros((ny, nx), bool)
    out[jj[ok], ii[ok]] = True
    return out


def blocks(wet, px, py, periodic, fold, h, xb=None, yb=None):
    """(block_wet, block_nbr), each (py, px): the wet cells of every block and of its neighbourhood; xb, yb: explicit begins"""
    ny, nx = wet.shape
    w = wet != 0
    if xb is None:
        bx, ex = extent(nx, px)
    else:
        bx, ex = list(xb), [b - 1 for b in list(xb)[1:]] + [nx - 1]
    if yb is None:
        by, ey = extent(ny, py)
    else:
        by, ey = list(yb), [b - 1 for b in list(yb)[1:]] + [ny - 1]
    own, nbr = np.zeros((py, px), np.int64), np.zeros((py, px), np.int64)
    hh = min(h, ny + nx)   # a wider halo reaches nothing more
    for b in range(py):
        for a in range(px):
            own[b, a] = int(w[by[b]:ey[b] + 1, bx[a]:ex[a] + 1].sum())
            if h == 0:
                nbr[b, a] = own[b, a]
            else:
                nbr[b, a] = int((w & reached(ny, nx, periodic, fold, hh, by[b], ey[b], bx[a], ex[a])).sum())
    return own, nbr, (bx, ex, by, ey)


def record(wet, px, py, periodic, fold, h, keep=None):
    """the record of a layout as a dict of Python ints; keep: a dict that gets block_wet and block_nbr"""
    ny, nx = wet.shape
    if px < 1 or py < 1 or px > nx or py > ny or px > MAX_DIV or py > MAX_DIV:
        return dict({f: 0 for f in FIELDS}, status=TOO_FINE)
    own, nbr, (bx, ex, by, ey) = blocks(wet, px, py, periodic, fold, h)
    if keep is not None:
        keep.update(block_wet=own, block_nbr=nbr)
    sx = [e - b + 1 for b, e in zip(bx, ex)]
    sy = [e - b + 1 for b, e in zip(by, ey)]
    masked = nbr == 0
    status = 0
    if fold and any(bx[a] + ex[px - 1 - a] != nx - 1 for a in range(px)):
        status |= FOLD_ASYMMETRIC
    return dict(blocks=px * py, masked=int(masked.sum()), pes=px * py - int(masked.sum()), max_block_cells=max(sx) * max(sy),
                max_block_edge=max(sx) + max(sy), min_block_size=min(sx + sy), max_wet=int(own.max()),
                masked_cells=int(sum(sx[a] * sy[b] for b in range(py) for a in range(px) if masked[b, a])),
                wet_total=int((wet != 0).sum()), status=status)


def masked_blocks(nbr):
    """the masked blocks (a, b) in ascending (b, a)"""
    return [(a, b) for b in range(nbr.shape[0]) for a in range(nbr.shape[1]) if nbr[b, a] == 0]


def table_text(px, py, masked):
    return "%d\n%d,%d\n" % (len(masked), px, py) + "".join("%d,%d\n" % (a + 1, b + 1) for a, b in masked)


def best(records, target):
    """records: dicts with px, py and the fields.  (winner for pes == target or None, {pes: best record} for pes <= target)"""
    key = lambda r: (r["max_block_cells"], r["max_block_edge"], r["blocks"], r["px"])   # noqa: E731
    by = {}
    for r in records:
        if r["status"] == 0 and r["pes"] <= target and (r["pes"] not in by or key(r) < key(by[r["pes"]])):
            by[r["pes"]] = r
    return by.get(target), by

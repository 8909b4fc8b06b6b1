"""The numpy definition of face topography (include/ogg_hip.h, "Face topography"), used by tests/test_topog_faces_cpu.py and
tests/test_gpu_topog_faces.py.  Built on topog_definition.cells, sample_positions and sample_values, so that no position, index or
value is restated: a face's samples are the topography's.  Slow (every sample is materialised, one face after the other), so for small
grids only."""
import numpy as np

import topog_definition as td

PERIODIC, FOLD = 1, 2                                   # OGG_MASK_PERIODIC, OGG_MASK_FOLD
F_ONE_SIDED, F_POLE, F_SEAM, F_FOLD = 1, 2, 4, 8        # OGG_FACE_*
INT_MAX, INT_MIN = int(np.iinfo(np.int32).max), int(np.iinfo(np.int32).min)
# a face record (OGG_TOPOG_FACE_WORDS int64 words), field for field at the header's byte offsets
RECORD = np.dtype([("n", "<i8"), ("n_missing", "<i8"), ("ridge_sum", "<i8"), ("n_lines", "<i4"), ("n_lines_missing", "<i4"),
                   ("n_dry_lines", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("q_min", "<i4"), ("R", "<i4"), ("n_clamped", "<i2"),
                   ("flags", "<i2")])
FIELDS = RECORD.names


def block(family, row, col, ny, nx, topology):
    """The present supergrid cells of the block of u face (jm, I) = (row, col) or v face (J, im) = (row, col), as (d, j, i, reversed):
    d the line group (dj or di), (j, i) the supergrid cell, reversed for the fold partner; and the face's flags but POLE."""
    nym, nxm = ny // 2, nx // 2
    cells, flags = [], 0
    for d in (0, 1):
        if family == "u":
            j = 2 * row + d
            west, east = 2 * col - 1, 2 * col
            if col == 0:
                west = nx - 1 if topology & PERIODIC else None
            if col == nxm:
                east = 0 if topology & PERIODIC else None
            if col in (0, nxm) and topology & PERIODIC:
                flags |= F_SEAM
            cells += [(d, j, i, False) for i in (west, east) if i is not None]
        else:
            i = 2 * col + d
            if row > 0:
                cells.append((d, 2 * row - 1, i, False))
            if row < nym:
                cells.append((d, 2 * row, i, False))
            elif topology & FOLD:
                cells.append((d, ny - 1, nx - 1 - i, True))
                flags |= F_FOLD
    if len(cells) < 4:
        flags |= F_ONE_SIDED
    return cells, flags


class Samples(object):
    """(value, valid) of the R x R samples of supergrid cells, [b, a], by the topography's definition; kept per R"""

    def __init__(self, c, q, box):
        self.c, self.flat, self.q, self.box, self.nx = c, {k: v.reshape(-1) for k, v in c.items()}, q, box, c["R"].shape[1]
        self.kept = {}

    def of(self, j, i, R):
        key = (j, i, R)
        if key not in self.kept:
            idx = np.array([j * self.nx + i])
            with np.errstate(invalid="ignore"):
                lon, lat = td.sample_positions(self.flat, R, idx)
            v, miss = td.sample_values(self.q, *self.box, lon, lat, self.flat["pole"][idx])
            self.kept[key] = (v[0].astype(np.int64), ~miss[0])
        return self.kept[key]


def face_record(family, row, col, smp, topology, wet_below):
    c = smp.c
    ny, nx = c["R"].shape
    cells, flags = block(family, row, col, ny, nx, topology)
    R = max(int(c["R"][j, i]) for _, j, i, _ in cells)
    rec = dict(n=0, n_missing=0, ridge_sum=0, n_lines=0, n_lines_missing=0, n_dry_lines=0, lo=INT_MAX, hi=INT_MIN, q_min=INT_MAX, R=R,
               n_clamped=sum(int(c["clamped"][j, i]) for _, j, i, _ in cells), flags=flags)
    if any(c["pole"][j, i] != 0 for _, j, i, _ in cells):
        rec["flags"] |= F_POLE
        return rec
    ridge = np.full((2, R), INT_MIN, dtype=np.int64)     # [d, line]
    for d, j, i, rev in cells:
        v, ok = smp.of(j, i, R)                          # [b, a]
        rec["n"] += int(ok.sum())
        rec["n_missing"] += int((~ok).sum())
        if ok.any():
            rec["q_min"] = min(rec["q_min"], int(v[ok].min()))
        w = np.where(ok, v, INT_MIN)
        line = w.max(axis=1) if family == "u" else w.max(axis=0)     # u: line b over a; v: line a over b
        if rev:
            line = line[::-1]                            # line a of the face takes the samples R - 1 - a of the partner
        ridge[d] = np.maximum(ridge[d], line)
    r = ridge.reshape(-1)
    valid = r != INT_MIN
    rec["n_lines"], rec["n_lines_missing"] = int(valid.sum()), int((~valid).sum())
    if valid.any():
        rv = r[valid]
        rec["lo"], rec["hi"], rec["ridge_sum"] = int(rv.min()), int(rv.max()), int(rv.sum())
        rec["n_dry_lines"] = int(np.count_nonzero(~(rv.astype(np.float64) < wet_below)))
    return rec


def face_records(x, y, q, lon0, dlon, lat0, dlat, topology=0, refine=None, oversample=2.0, wet_below=0.0):
    """{"u": records (nym, nxm + 1), "v": records (nym + 1, nxm)} as arrays of RECORD, of the quantised raster q"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = td.cells(x, y, dlon, dlat, refine, oversample)
    ny, nx = c["R"].shape
    assert ny % 2 == 0 and nx % 2 == 0
    nym, nxm = ny // 2, nx // 2
    smp = Samples(c, q, (lon0, dlon, lat0, dlat))
    out = {"u": np.zeros((nym, nxm + 1), dtype=RECORD), "v": np.zeros((nym + 1, nxm), dtype=RECORD)}
    for fam, arr in out.items():
        for row in range(arr.shape[0]):
            for col in range(arr.shape[1]):
                rec = face_record(fam, row, col, smp, topology, wet_below)
                arr[row, col] = tuple(rec[f] for f in FIELDS)
    return out


def records(x, y, raw, lon0, dlon, lat0, dlat, topology=0, refine=None, oversample=2.0, quantum=None, sea_level=0.0, fill=()):
    q, quantum = td.quantise(raw, quantum, fill)
    return face_records(x, y, q, lon0, dlon, lat0, dlat, topology, refine, oversample, float(sea_level) / quantum)

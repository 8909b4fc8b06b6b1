"""Inputs and truths of the face-topography tests that are not the numpy definition (tests/test_topog_faces_cpu.py holds the definition
to them, tests/test_gpu_topog_faces.py the device): planted ridges, closed forms in Python integers on small_grids' index rasters,
and the faces of the tripolar cuts that meet a seam, a fold or an edge."""
import numpy as np

import small_grids as G
import topog_faces_definition as fd

BOX = G.GLOBAL_BOX          # 0.25 degree from (-180, -90)
FLOOR, RIDGE = -1000, 50
PLANTED_R = 8               # every quarter-degree raster element gets 2 x 2 samples of a 1-degree supergrid cell
# the 4 x 4 supergrid cells (2 x 2 model cells) of 1 degree from (104, -4) the ridges are planted in
PLANTED_GRID = dict(ny=4, nx=4, lon0=104.0, lat0=-4.0)


def planted_grid():
    return G.grid(PLANTED_GRID["ny"], PLANTED_GRID["nx"], PLANTED_GRID["lon0"], PLANTED_GRID["lat0"])


ROW, COLUMN = 349, 1141     # raster row 2.75S .. 2.5S (supergrid row 1, b = 2, 3); raster column 105.25E .. 105.5E (supergrid column 1, a = 2, 3)
GAP_COLUMN = 1138           # 104.5E .. 104.75E: supergrid column 0, a = 4, 5


def planted(kind):
    """A flat raster at FLOOR with a ridge at RIDGE.  "row": raster row ROW, between the centre lines of model rows 0 and 1 (3S and
    1S) and off their face line at 2S; "row_gap": the same with raster column GAP_COLUMN left at FLOOR.  "column": raster column
    COLUMN, between the centre lines of model columns 0 and 1 (105E and 107E) and off their face line at 106E; "column_gap": the same
    with raster row ROW left at FLOOR."""
    z = np.full((720, 1440), FLOOR, dtype=np.int16)
    if kind.startswith("row"):
        z[ROW, :] = RIDGE
        if kind == "row_gap":
            z[ROW, GAP_COLUMN] = FLOOR
    else:
        z[:, COLUMN] = RIDGE
        if kind == "column_gap":
            z[ROW, COLUMN] = FLOOR
    return z


def planted_truth(kind):
    """{(family, row, col): (lo, hi, n_dry_lines, n_lines)} of faces the planted ridge decides or must leave alone, at PLANTED_R and
    sea level 0 (a ridge at +50 is dry, the floor wet); every face has 2 R = 16 lines.
    "row": the ridge lies in supergrid row 1, so in the blocks of the v faces J = 1 (rows 1, 2) and of the u faces jm = 0 (rows 0, 1).
    Every v line (along b) of J = 1 crosses it: lo = hi = RIDGE, all dry.  Of the u lines (along a, at one latitude) of jm = 0 the two
    at 2.6875S and 2.5625S (dj = 1, b = 2, 3) lie on it and the others never meet it: lo = FLOOR, hi = RIDGE, 2 dry.  "row_gap": of
    the v face (1, 0) the two lines (di = 0, a = 4, 5) pass through the gap: lo = FLOOR, 14 of 16 dry; the v face (1, 1) stays closed.
    "column": the ridge lies in supergrid column 1, so in the blocks of the u faces I = 1 (columns 1, 2): every u line crosses it;
    the v faces im = 0 (columns 0, 1) have the two lines (di = 1, a = 2, 3) on it.  "column_gap": of the u face (0, 1) the two lines
    (dj = 1, b = 2, 3) pass; the u face (1, 1) stays closed."""
    n = 2 * PLANTED_R
    closed, part, floor = (RIDGE, RIDGE, n, n), (FLOOR, RIDGE, 2, n), (FLOOR, FLOOR, 0, n)
    if kind.startswith("row"):
        t = {("v", 1, 0): closed, ("v", 1, 1): closed, ("u", 0, 0): part, ("u", 0, 1): part, ("u", 0, 2): part,
             ("u", 1, 0): floor, ("u", 1, 1): floor, ("v", 0, 0): floor, ("v", 2, 1): floor}
        if kind == "row_gap":
            t["v", 1, 0] = (FLOOR, RIDGE, n - 2, n)
        return t
    t = {("u", 0, 1): closed, ("u", 1, 1): closed, ("v", 0, 0): part, ("v", 1, 0): part, ("v", 2, 0): part,
         ("v", 1, 1): floor, ("v", 0, 1): floor, ("u", 0, 0): floor, ("u", 1, 2): floor}
    if kind == "column_gap":
        t["u", 0, 1] = (FLOOR, RIDGE, n - 2, n)
    return t


PLANTED_KINDS = ("row", "row_gap", "column", "column_gap")


def assert_planted(kind, rec):
    """rec: {"u": records, "v": records} of planted(kind) on planted_grid() at PLANTED_R"""
    for (fam, row, col), (lo, hi, dry, n) in planted_truth(kind).items():
        r = rec[fam][row, col]
        got = (int(r["lo"]), int(r["hi"]), int(r["n_dry_lines"]), int(r["n_lines"]))
        assert got == (lo, hi, dry, n), (kind, fam, row, col, got)


def mixed_grid():
    """4 x 6 supergrid cells, sheared, every column an eighth of a degree wider than the one before: by the spans the cells of one
    block get different R"""
    x, y = G.grid(4, 6, shear=True)
    x += 0.125 * np.cumsum(np.arange(7))[None, :]
    return x, y


# ---- closed forms on the index rasters -------------------------------------------------------------------------
CLOSED_GRID = dict(ny=4, nx=6, lon0=104.0, lat0=-4.0)     # 2 x 3 model cells of 2 degrees


def closed_grid():
    return G.grid(CLOSED_GRID["ny"], CLOSED_GRID["nx"], CLOSED_GRID["lon0"], CLOSED_GRID["lat0"])


def closed_form(kind, family, row, col, R):
    """(lo, hi, ridge_sum, n_lines, q_min) of a face of closed_grid() over the index raster ``kind`` ("index_js": the value is the
    raster row, "index_is": the raster column mod 251) in Python integers, R a power of two >= 2, no topology: sample a of supergrid
    column i lies (4 a + 2) // R quarter-degree columns east of the column's west edge (small_grids.index_truth), rows alike, so the
    ridge of a line is the index of its northmost (index_js) or eastmost (index_is) sample."""
    ny, nx = CLOSED_GRID["ny"], CLOSED_GRID["nx"]
    i_of = lambda i, a: (((int(CLOSED_GRID["lon0"]) + i + 180) * 4) % 1440 + (4 * a + 2) // R) % 251     # noqa: E731
    j_of = lambda j, b: (int(CLOSED_GRID["lat0"]) + j + 90) * 4 + (4 * b + 2) // R                          # noqa: E731
    cells, _ = fd.block(family, row, col, ny, nx, 0)
    ridges, lowest = [], []
    for d in (0, 1):
        mine = [(j, i) for dd, j, i, _ in cells if dd == d]
        for k in range(R):
            if family == "u":       # line (dj, b = k): one latitude, every a of the west and the east cell
                vals = [j_of(j, k) if kind == "index_js" else i_of(i, a) for j, i in mine for a in range(R)]
            else:                   # line (di, a = k): one longitude, every b of the south and the north cell
                vals = [j_of(j, b) if kind == "index_js" else i_of(i, k) for j, i in mine for b in range(R)]
            ridges.append(max(vals))
            lowest.append(min(vals))
    return min(ridges), max(ridges), sum(ridges), len(ridges), min(lowest)


def assert_closed_forms(kind, R, rec):
    for fam in ("u", "v"):
        for row in range(rec[fam].shape[0]):
            for col in range(rec[fam].shape[1]):
                r = rec[fam][row, col]
                got = (int(r["lo"]), int(r["hi"]), int(r["ridge_sum"]), int(r["n_lines"]), int(r["q_min"]))
                assert got == closed_form(kind, fam, row, col, R), (kind, R, fam, row, col, got)
                assert int(r["n_lines_missing"]) == 0 and int(r["n_missing"]) == 0


# ---- the faces of a grid that meet a seam, a fold or an edge ------------------------------------------------------
def edge_faces(ny, nx):
    """[(family, row, col)]: the u faces of the first two and last two columns of four rows, the v faces of the first and the last
    two rows of eight columns and their mirror images"""
    nym, nxm = ny // 2, nx // 2
    rows = sorted({0, nym // 2, nym - 2, nym - 1})
    base = {0, 1, 2, nxm // 2}
    cols = sorted(base | {nxm - 1 - c for c in base})
    out = [("u", r, c) for r in rows for c in (0, 1, nxm - 1, nxm)]
    out += [("v", r, c) for r in (0, nym - 1, nym) for c in cols]
    return out


def edge_records(x, y, raw, box, topology, refine):
    """{(family, row, col): record} of edge_faces by the definition"""
    q, _ = fd.td.quantise(raw)
    with np.errstate(invalid="ignore"):
        c = fd.td.cells(np.asarray(x), np.asarray(y), box[1], box[3], refine, 2.0)
    smp = fd.Samples(c, q, box)
    ny, nx = c["R"].shape
    out = {}
    for fam, row, col in edge_faces(ny, nx):
        rec = fd.face_record(fam, row, col, smp, topology, 0.0)
        out[fam, row, col] = np.array([tuple(rec[f] for f in fd.FIELDS)], dtype=fd.RECORD)[0]
    return out


def assert_edges(rec_of, ny, nx, periodic, fold):
    """rec_of(family, row, col) -> record: flags, the seam's two columns, the fold's mirror images"""
    nym, nxm = ny // 2, nx // 2
    for fam, row, col in edge_faces(ny, nx):
        r = rec_of(fam, row, col)
        flags = int(r["flags"])
        if fam == "u":
            at_edge = col in (0, nxm)
            assert bool(flags & fd.F_SEAM) == (at_edge and periodic), (fam, row, col, flags)
            assert bool(flags & fd.F_ONE_SIDED) == (at_edge and not periodic), (fam, row, col, flags)
            assert not flags & fd.F_FOLD
            if periodic and col == 0:
                assert r.tobytes() == rec_of("u", row, nxm).tobytes(), ("seam", row)
        else:
            top = row == nym
            assert bool(flags & fd.F_FOLD) == (top and fold), (fam, row, col, flags)
            assert bool(flags & fd.F_ONE_SIDED) == (row == 0 or (top and not fold)), (fam, row, col, flags)
            assert not flags & fd.F_SEAM
            if top and fold:
                assert r.tobytes() == rec_of("v", row, nxm - 1 - col).tobytes(), ("fold", col)
        if not flags & fd.F_POLE:
            assert int(r["n_lines"]) + int(r["n_lines_missing"]) == 2 * int(r["R"])
            sides = 1 if flags & fd.F_ONE_SIDED else 2
            assert int(r["n"]) + int(r["n_missing"]) == 2 * sides * int(r["R"]) ** 2

"""Atmosphere x ocean exchange grid with a gnomonic cubed-sphere atmosphere: every non-empty overlap of a cell of six tiles of N x N
cells with a MOM6 model (h) cell of a supergrid, with its area, written as FMS's first-order exchange-grid files, one per tile
(``atmos_mosaic_tile[1-6]Xocean_mosaic_tile1.nc``).  include/ogg_hip.h, "Exchange grid with a cubed-sphere atmosphere", gives the
definition; the edges of the ocean cells are great circles here (FMS's rule whenever one side is a cubed sphere), not straight in
(lon, lat) as in exchange_grid.py.  The reference has no such step.

The overlaps are found and measured on the device by libogg_hip.so (ogg_xgrid_cs_count_dev / ogg_xgrid_cs_write_dev / ogg_xgrid_cs).
The list is in one canonical order (ocean cells row-major, then tile, then atmosphere rows, then columns) and nothing is summed across
cells, so it is bit-identical whatever the split of the grid into bands or ranks.

The numbering of the tiles and the directions of (i, j) on each are THIS module's default (cubed_sphere_atm), not FMS's or any
model's: a user ties them to a model with cubed_sphere_from_corners on the model's own tile corners.

    python -m ocean_model_grid_generator_amd.exchange_grid_cs ocean_hgrid.nc --cs N [--spacing equiangular|edge_equidistant]
        [--lon_shift DEG] [--topog topog.nc | --mask ocean_mask.nc] [-o 'atmos_mosaic_tile%dXocean_mosaic_tile1.nc'] [--frac FILE]
        [--json FILE]
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import netcdf3
from .exchange_grid import DEFAULT_RE, DEFAULT_THRESHOLD, check_args, check_grid, mask_from_topog

DEFAULT_PATTERN = "atmos_mosaic_tile%dXocean_mosaic_tile1.nc"
SPACINGS = ("equiangular", "edge_equidistant")
N_MAX = 4096


# ---- the atmosphere --------------------------------------------------------------------------------------------
def table(N, spacing="equiangular"):
    """t_0 .. t_N of a face: equiangular t_k = tan(-pi/4 + k pi / (2 N)); edge_equidistant t_k = sqrt 2 tan(-alpha + 2 alpha k / N),
    alpha = asin(1 / sqrt 3) (equal arcs along a face's edge).  The ends are -1 and 1 exactly and the middle entry of an even N is 0."""
    N = int(N)
    if not 1 <= N <= N_MAX:
        raise ValueError("cubed sphere: N must be 1 .. %d (%d)" % (N_MAX, N))
    k = np.arange(N + 1, dtype=np.float64)
    if spacing == "equiangular":
        t = np.tan(-np.pi / 4 + k * np.pi / (2 * N))
    elif spacing == "edge_equidistant":
        alpha = np.arcsin(1.0 / np.sqrt(3.0))
        t = np.sqrt(2.0) * np.tan(-alpha + 2 * alpha * k / N)
    else:
        raise ValueError("cubed sphere: spacing must be one of %s (%r)" % (", ".join(SPACINGS), spacing))
    t[0], t[N] = -1.0, 1.0
    if N % 2 == 0:
        t[N // 2] = 0.0
    return t


def default_frames(lon_shift=0.0):
    """(6, 3, 3) rows e_u, e_v, e_n.  Faces 0 .. 3: normals on the equator at longitudes 0, 90, 180, 270, e_u eastward, e_v = z; face 4:
    n = +z, e_u = +y, e_v = -x; face 5: n = -z, e_u = +y, e_v = +x; the whole cube turned by lon_shift degrees about z.  This
    orientation is this module's own."""
    x, y, z = np.eye(3)
    base = np.array([[y, z, x], [-x, z, y], [-y, z, -x], [x, z, -y], [y, -x, z], [y, x, -z]])
    if lon_shift == 0.0:
        return base + 0.0   # (no -0)
    a = np.radians(float(lon_shift))
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return base @ R.T


def atm_desc(atm, t_ptr):
    """ogg_xgrid_cs_atm of a cubed sphere with its table at t_ptr (host or device memory)"""
    d = L.XgridCsAtm(t=t_ptr, N=int(atm["N"]))
    fr = np.ascontiguousarray(atm["frames"], dtype=np.float64).reshape(6, 9)
    for f in range(6):
        for k in range(9):
            d.frames[f][k] = fr[f, k]
    return d


def checked_atm(atm):
    """The cubed sphere as contiguous float64 arrays, checked by the library (OGG_EARG -> ValueError)."""
    t = L.as_f64(atm["t"]).reshape(-1)
    fr = L.as_f64(atm["frames"])
    if t.size < 2 or fr.size != 54:
        raise ValueError("cubed sphere: a table of at least two entries and six 3 x 3 frames are needed")
    out = dict(atm, t=t, frames=fr.reshape(6, 3, 3), N=t.size - 1)
    L.checked("ogg_xgrid_cs_check_atm", atm_desc(out, t.ctypes.data))
    return out


def cubed_sphere_atm(N, spacing="equiangular", frames=None, lon_shift=0.0):
    """A gnomonic cubed sphere of six tiles of N x N cells: {"t", "frames", "N", "spacing", "lon_shift"}.  ``frames``: None for
    default_frames(lon_shift), or six (e_u, e_v, e_n)."""
    fr = default_frames(lon_shift) if frames is None else np.asarray(frames, dtype=np.float64)
    return checked_atm({"t": table(N, spacing), "frames": fr, "spacing": spacing, "lon_shift": float(lon_shift)})


def _unit(lon, lat):
    lam, phi = np.radians(np.asarray(lon, dtype=np.float64)), np.radians(np.asarray(lat, dtype=np.float64))
    return np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], axis=-1)


def cubed_sphere_corners(atm):
    """(lon, lat), each (6, N + 1, N + 1) in degrees, [tile, j, i]: the corners of the cells of every tile"""
    t, fr = np.asarray(atm["t"]), np.asarray(atm["frames"]).reshape(6, 3, 3)
    xi, eta = np.meshgrid(t, t)
    P = fr[:, None, None, 2, :] + xi[None, :, :, None] * fr[:, None, None, 0, :] + eta[None, :, :, None] * fr[:, None, None, 1, :]
    P = P / np.linalg.norm(P, axis=-1, keepdims=True)
    return np.degrees(np.arctan2(P[..., 1], P[..., 0])), np.degrees(np.arcsin(np.clip(P[..., 2], -1.0, 1.0)))


def cubed_sphere_from_corners(lon, lat, tol=1.0e-9):
    """The cubed sphere of a model's own grid tiles: lon, lat (6, N + 1, N + 1) corner arrays [tile, j, i] in degrees.  The normal of
    each tile comes from its four outer corners, e_u and e_v from its i and j directions, the table from the south edge of the first
    tile.  Raises ValueError unless every corner lies within ``tol`` of its gnomonic position under them: this ties the tile numbers
    and (i, j) directions of the exchange files to the model's."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    if lon.ndim != 3 or lon.shape[0] != 6 or lon.shape[1] != lon.shape[2] or lon.shape[1] < 2 or lat.shape != lon.shape:
        raise ValueError("cubed sphere: six (N + 1) x (N + 1) corner arrays are needed (%s, %s)" % (lon.shape, lat.shape))
    N = lon.shape[1] - 1
    V = _unit(lon, lat)
    c00, c0n, cn0, cnn = V[:, 0, 0], V[:, 0, N], V[:, N, 0], V[:, N, N]
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)   # noqa: E731
    fr = np.stack([unit(c0n + cnn - c00 - cn0), unit(cn0 + cnn - c00 - c0n), unit(c00 + c0n + cn0 + cnn)], axis=1)
    t = (V[0, 0] @ fr[0, 0]) / (V[0, 0] @ fr[0, 2])
    if abs(t[0] + 1.0) > tol or abs(t[N] - 1.0) > tol:
        raise ValueError("cubed sphere: the first tile's south edge runs %.12g .. %.12g in its own frame, not -1 .. 1" % (t[0], t[N]))
    t[0], t[N] = -1.0, 1.0
    if N % 2 == 0 and abs(t[N // 2]) <= tol:
        t[N // 2] = 0.0
    atm = {"t": t, "frames": fr, "N": N, "spacing": "from_corners", "lon_shift": None}
    glon, glat = cubed_sphere_corners(atm)
    err = np.max(np.abs(_unit(glon, glat) - V), axis=(1, 2, 3))
    if not np.all(err <= tol):
        raise ValueError("cubed sphere: the corners of tile %d lie up to %.3g from their gnomonic positions (one table on both axes of "
                         "six faces of a cube): not a gnomonic cubed sphere of this kind" % (int(np.argmax(err)) + 1, float(err.max())))
    return checked_atm(atm)


# ---- results ---------------------------------------------------------------------------------------------------
def _omega2(a, b, c):
    ra, rb, rc = (np.sqrt(1.0 + p[0] * p[0] + p[1] * p[1]) for p in (a, b, c))
    d = lambda p, q, rp, rq: (p[0] * q[0] + p[1] * q[1] + 1.0) / (rp * rq)   # noqa: E731
    num = ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) / (ra * rb * rc)
    return 2.0 * np.arctan2(num, 1.0 + d(a, b, ra, rb) + d(b, c, rb, rc) + d(c, a, rc, ra))


def atm_area(t, Re):
    """A_atm of the N x N cells of a face (the same on every face), formed as the definition's keep step has it"""
    xi, eta = np.meshgrid(np.asarray(t, dtype=np.float64), np.asarray(t, dtype=np.float64))
    c00, c10 = (xi[:-1, :-1], eta[:-1, :-1]), (xi[:-1, 1:], eta[:-1, 1:])
    c11, c01 = (xi[1:, 1:], eta[1:, 1:]), (xi[1:, :-1], eta[1:, :-1])
    return (Re * Re) * (_omega2(c00, c10, c11) + _omega2(c00, c11, c01))


def ocean_frac(atm_fij, area, t, Re):
    """The fraction of every atmosphere cell (6 x N x N) covered by the list's exchange cells: their areas summed per cell with
    np.bincount in list order, over the cell's area."""
    N = t.size - 1
    a_atm = np.broadcast_to(atm_area(t, Re), (6, N, N)).copy()
    k = (atm_fij[:, 2].astype(np.int64) * N + atm_fij[:, 1]) * N + atm_fij[:, 0]
    s = np.bincount(k, weights=area, minlength=6 * N * N).reshape(6, N, N)
    return s / a_atm, a_atm


def counts_dict(c):
    return L.counts_dict(L.XGRID_CS_COUNT_FIELDS, c)


def result(atm_fij, ocn, area, a_poly, counts, atm, Re, threshold, masked=False):
    """What exchange_grid_cs() returns: the list (atm (n, 3) = (I, J, face), ocn (n, 2) = (n, m), area (n,)), A_poly per model cell,
    the ocean and land fractions and the area of every atmosphere cell (6 x N x N), the counts and a summary."""
    frac, a_atm = ocean_frac(atm_fij, area, atm["t"], Re)
    ok = np.isfinite(a_poly)
    summary = dict(counts, N=int(atm["N"]), spacing=atm.get("spacing"), lon_shift=atm.get("lon_shift"), ocean_shape=list(a_poly.shape),
                   Re=float(Re), threshold=float(threshold), masked=bool(masked), area_sum=float(np.sum(area)),
                   a_poly_sum=float(np.sum(a_poly[ok & (a_poly > 0)])), sphere=float(4.0 * np.pi * Re * Re),
                   per_tile=[int(np.sum(atm_fij[:, 2] == f)) for f in range(6)])
    return {"atm": atm_fij, "ocn": ocn, "area": area, "a_poly": a_poly, "ocean_frac": frac, "land_frac": 1.0 - frac, "a_atm": a_atm,
            "t": atm["t"], "frames": atm["frames"], "counts": counts, "summary": summary}


def host_mask(mask, shape):
    """None, or the mask as one byte per model cell (ValueError unless it has their shape)"""
    if mask is None:
        return None
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.shape != tuple(shape):
        raise ValueError("exchange grid: the mask is %s, the model cells %s" % (m.shape, tuple(shape)))
    return m


# ---- host arrays -----------------------------------------------------------------------------------------------
def exchange_grid_cs(x, y, atm, mask=None, Re=DEFAULT_RE, threshold=DEFAULT_THRESHOLD, capacity=None):
    """The exchange grid of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny even) and a cubed sphere ``atm``
    (cubed_sphere_atm, cubed_sphere_from_corners), on one GPU through the host-pointer entry.  mask: None, or one value per model
    cell; a cell where it is 0 emits nothing.  capacity: the list's first allocation (it is grown once when too small)."""
    x, y = L.as_f64(x), L.as_f64(y)
    if x.ndim != 2 or y.shape != x.shape:
        raise ValueError("exchange grid: x %s and y %s must be 2-D of one shape" % (x.shape, y.shape))
    nyp, nxp = x.shape
    check_grid(nyp, nxp)
    check_args(threshold, Re)
    atm = checked_atm(atm)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = host_mask(mask, shape)
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(Re), threshold=float(threshold))
    band.x, band.y = L.ptr(x), L.ptr(y)
    band.x_next, band.y_next = L.ptr(x[nyp - 1:]), L.ptr(y[nyp - 1:])
    band.mask = None if m is None else m.ctypes.data
    desc = atm_desc(atm, atm["t"].ctypes.data)
    a_poly = np.empty(shape, dtype=np.float64)
    counts = L.XgridCsCounts()
    cap = 4 * shape[0] * shape[1] + 4096 if capacity is None else int(capacity)
    lib = L.load()
    for _ in range(2):   # a second call only when the first capacity was too small
        fij = np.empty((cap, 3), dtype=np.int32)
        ocn = np.empty((cap, 2), dtype=np.int32)
        area = np.empty(cap, dtype=np.float64)
        rc = lib.ogg_xgrid_cs(ctypes.byref(band), ctypes.byref(desc), cap, fij.ctypes.data, ocn.ctypes.data, area.ctypes.data,
                              a_poly.ctypes.data, ctypes.byref(counts))
        if rc == L.OGG_ESHAPE and counts.kept > cap:
            cap = int(counts.kept)
            continue
        L.check(rc)
        break
    n = int(counts.kept)
    return result(fij[:n].copy(), ocn[:n].copy(), area[:n].copy(), a_poly, counts_dict(counts), atm, Re, threshold, m is not None)


# ---- device arrays ---------------------------------------------------------------------------------------------
def band_lists_dev(band, atm_desc_, stream, device, events=None):
    """Both steps on a descriptor of device pointers: (first model row, counts (int64 device tensor of 8), a_poly (rows x nx/2), atm
    (int32 (n, 3)), ocn (int32 (n, 2)), area), synchronised once between the steps (the list's length).  ``events``: a list that
    takes four torch events around the count and the write step (scripts/xgrid_cs_profile.py)."""
    import torch
    lib = L.load()
    mark = (lambda: None) if events is None else (lambda: (events.append(torch.cuda.Event(enable_timing=True)), events[-1].record()))
    m0 = int(lib.ogg_xgrid_band_first_row(ctypes.byref(band)))
    rows = int(lib.ogg_xgrid_band_out_rows(ctypes.byref(band)))
    ws_bytes = int(lib.ogg_xgrid_cs_workspace_bytes(ctypes.byref(band), ctypes.byref(atm_desc_)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    a_poly = torch.empty((rows, band.nx // 2), dtype=torch.float64, device=device)
    counts = torch.zeros(len(L.XGRID_CS_COUNT_FIELDS), dtype=torch.int64, device=device)
    mark()
    L.call("ogg_xgrid_cs_count_dev", ctypes.byref(band), ctypes.byref(atm_desc_), ws.data_ptr(), ws_bytes, a_poly.data_ptr(),
           counts.data_ptr(), stream)
    mark()
    n = int(counts[L.XGRID_CS_COUNT_FIELDS.index("kept")].item())
    fij = torch.empty((n, 3), dtype=torch.int32, device=device)
    ocn = torch.empty((n, 2), dtype=torch.int32, device=device)
    area = torch.empty(n, dtype=torch.float64, device=device)
    mark()
    if n:
        L.call("ogg_xgrid_cs_write_dev", ctypes.byref(band), ctypes.byref(atm_desc_), ws.data_ptr(), ws_bytes, fij.data_ptr(),
               ocn.data_ptr(), area.data_ptr(), stream)
    mark()
    return m0, counts, a_poly, fij, ocn, area


def assemble(pieces, shape, atm, Re, threshold, masked):
    """The result of the whole grid from [(first model row, counts, a_poly, atm, ocn, area)] as host arrays, in piece order."""
    a_poly = np.full(shape, np.nan)
    counts = {f: 0 for f in L.XGRID_CS_COUNT_FIELDS}
    for m0, c, ap, _, _, _ in pieces:
        a_poly[m0:m0 + ap.shape[0]] = ap
        for k, f in enumerate(L.XGRID_CS_COUNT_FIELDS):
            counts[f] += int(c[k])
    cat = lambda k, empty: np.concatenate([p[k] for p in pieces]) if pieces else empty   # noqa: E731
    return result(cat(3, np.zeros((0, 3), np.int32)), cat(4, np.zeros((0, 2), np.int32)), cat(5, np.zeros(0)), a_poly, counts, atm, Re,
                  threshold, masked)


# ---- files -----------------------------------------------------------------------------------------------------
def tile_paths(pattern):
    """the six file names of a pattern with one %d (the tile number 1 .. 6)"""
    try:
        paths = [pattern % (f + 1) for f in range(6)]
    except (TypeError, ValueError):
        paths = []
    if len(set(paths)) != 6:
        raise ValueError("cubed-sphere exchange grid: the file pattern needs one %%d for the tile number (%r)" % (pattern,))
    return paths


def write_xgrid_cs(pattern, res):
    """Six files in the FMS first-order exchange-grid layout of exchange_grid.write_xgrid, pattern % tile for tile = 1 .. 6: the
    entries of each face in list order (a stable partition of the list), tile1_cell = (I + 1, J + 1) on that tile, tile2_cell the
    ocean model cell.  A tile without an entry gives a file with ncells = 0 (which the classic format reads as a record dimension
    without a record).  Returns the paths."""
    paths = tile_paths(pattern)
    for f, path in enumerate(paths):
        sel = res["atm"][:, 2] == f
        n = int(sel.sum())
        ds = netcdf3.Dataset(path, [("ncells", n), ("two", 2)])
        ds.def_var("tile1_cell", netcdf3.NC_INT, ("ncells", "two"), [("standard_name", "parent_cell_indices_in_mosaic1")],
                   res["atm"][sel][:, :2].astype(np.int32) + 1)
        ds.def_var("tile2_cell", netcdf3.NC_INT, ("ncells", "two"), [("standard_name", "parent_cell_indices_in_mosaic2")],
                   res["ocn"][sel].astype(np.int32) + 1)
        ds.def_var("xgrid_area", netcdf3.NC_DOUBLE, ("ncells",), [("standard_name", "exchange_grid_area"), ("units", "m2")],
                   res["area"][sel])
        ds.write()
    return paths


def write_frac_cs(path, res):
    """ocean_frac, land_frac and area of every atmosphere cell (tile, j, i), with the table and the frames that define the tiles"""
    N = int(res["t"].size - 1)
    ds = netcdf3.Dataset(path, [("tile", 6), ("nj", N), ("ni", N), ("edge", N + 1), ("nine", 9)],
                         [("description", "ocean and land fractions of the cells of a gnomonic cubed sphere; tile numbering and (i, j) "
                                          "directions as the frames (rows e_u, e_v, e_n) give them")])
    ds.def_var("t", netcdf3.NC_DOUBLE, ("edge",), [("long_name", "gnomonic coordinate of the cell edges on both axes")], res["t"])
    ds.def_var("frames", netcdf3.NC_DOUBLE, ("tile", "nine"), [("long_name", "e_u, e_v, e_n of every tile")],
               np.asarray(res["frames"]).reshape(6, 9))
    ds.def_var("ocean_frac", netcdf3.NC_DOUBLE, ("tile", "nj", "ni"), [("units", "1")], res["ocean_frac"])
    ds.def_var("land_frac", netcdf3.NC_DOUBLE, ("tile", "nj", "ni"), [("units", "1")], res["land_frac"])
    ds.def_var("area", netcdf3.NC_DOUBLE, ("tile", "nj", "ni"), [("units", "m2")], res["a_atm"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    return ["   cubed-sphere exchange grid: %d exchange cells of 6 x %d x %d atmosphere cells and %d x %d ocean cells%s; area %.15g of "
            "4 pi Re^2, %d atmosphere cells with ocean; per tile %s"
            % (s["kept"], s["N"], s["N"], s["ocean_shape"][1], s["ocean_shape"][0], " (masked)" if s["masked"] else "",
               s["area_sum"] / s["sphere"], int(np.sum(res["ocean_frac"] > 0)), " ".join(str(v) for v in s["per_tile"])),
            "   cubed-sphere exchange grid: %d candidates on %d cell faces; %d wide, %d inverted, %d degenerate, %d masked"
            % (s["candidates"], s["face_candidates"], s["wide"], s["inverted"], s["degenerate"], s["masked"])]


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.exchange_grid_cs",
                                description="atmosphere x ocean exchange grid of a supergrid file and a gnomonic cubed-sphere atmosphere")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("--cs", type=int, required=True, metavar="N", help="six tiles of N x N cells")
    p.add_argument("--spacing", choices=SPACINGS, default="equiangular")
    p.add_argument("--lon_shift", type=float, default=0.0, help="turn the default cube by this many degrees about the polar axis")
    w = p.add_mutually_exclusive_group()
    w.add_argument("--topog", default=None, help="topog.nc: only cells with depth > 0 exchange")
    w.add_argument("--mask", default=None, help="ocean_mask.nc: only cells with mask != 0 exchange")
    p.add_argument("-o", "--output", default=DEFAULT_PATTERN, help="file pattern with %%d for the tile number")
    p.add_argument("--frac", default=None, help="write the ocean and land fractions of the atmosphere cells to this file")
    p.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD, help="area ratio below which an overlap is dropped")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    tile_paths(a.output)
    g = netcdf3.read_doubles(a.grid, names=("x", "y"))
    atm = cubed_sphere_atm(a.cs, a.spacing, lon_shift=a.lon_shift)
    from .remap import mask_from_file
    mask = mask_from_topog(a.topog) if a.topog else (mask_from_file(a.mask) if a.mask else None)
    res = exchange_grid_cs(g["x"], g["y"], atm, mask=mask, threshold=a.threshold)
    for line in summary_lines(res):
        print(line)
    write_xgrid_cs(a.output, res)
    if a.frac:
        write_frac_cs(a.frac, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

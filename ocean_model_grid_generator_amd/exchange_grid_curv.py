"""Exchange grid with a curvilinear source grid: every non-empty overlap of a cell of a logically rectangular mesh on the sphere
(another model's tripolar grid, a sea-ice or land mosaic, a regional parent grid, a rotated-pole reanalysis) with a MOM6 model (h) cell
of a supergrid, with its area, written as an FMS first-order exchange-grid file.  include/ogg_hip.h, "Exchange grid with a curvilinear
source grid", gives the definition: the edges of both meshes are great circles, a source cell with two corners more than 30 degrees
apart is skipped (WIDE), and the region of a non-convex source cell is the intersection of its four half-spaces.  The reference has no
such step.

The overlaps are found and measured on the device by libogg_hip.so (ogg_xgrid_curv_sets_dev / ogg_xgrid_curv_clip_dev /
ogg_xgrid_curv_write_dev / ogg_xgrid_curv).  The list is in one canonical order (model cells row-major, then the source cell's index
J * NA + I) and nothing is summed across pairs, so it is bit-identical whatever the split of the grid into bands or ranks and whatever
the search index.  remap.CurvilinearSource feeds it to the conservative remap.

    python -m ocean_model_grid_generator_amd.exchange_grid_curv ocean_hgrid.nc SRC_GRID.nc [--source_corners LONVAR LATVAR]
        [--topog topog.nc | --mask ocean_mask.nc] [--source_mask FILE] [-o xgrid.nc] [--json FILE]
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import netcdf3
from .exchange_grid import DEFAULT_RE, DEFAULT_THRESHOLD, check_args, check_grid, mask_from_topog, write_xgrid
from .exchange_grid_cs import host_mask

DEFAULT_FILE = "source_mosaic_tile1Xocean_mosaic_tile1.nc"
FIELDS = L.XGRID_CURV_COUNT_FIELDS
SOURCE_FIELDS = tuple(f for f in FIELDS if f.startswith("src_"))   # counted over the whole source in every band's call


# ---- the source ------------------------------------------------------------------------------------------------
def src_desc(x_ptr, y_ptr, NA, NB, ld=None, mask_ptr=None):
    """ogg_xgrid_curv_src of corners at x_ptr, y_ptr (host or device memory), checked by the library (OGG_EARG -> ValueError)"""
    d = L.XgridCurvSrc(x=x_ptr, y=y_ptr, NA=int(NA), NB=int(NB), ld=int(NA) + 1 if ld is None else int(ld), mask=mask_ptr)
    return L.checked("ogg_xgrid_curv_check", d)


def checked_source(src_lon, src_lat, src_mask=None):
    """(lon, lat, mask): the corners as contiguous float64 (NB + 1) x (NA + 1) arrays and one byte per source cell or None"""
    lon, lat = L.as_f64(src_lon), L.as_f64(src_lat)
    if lon.ndim != 2 or lat.shape != lon.shape or lon.shape[0] < 2 or lon.shape[1] < 2:
        raise ValueError("curvilinear exchange grid: the source's corner longitudes %s and latitudes %s must be 2-D of one shape, at "
                         "least 2 x 2" % (lon.shape, lat.shape))
    m = None
    if src_mask is not None:
        m = np.ascontiguousarray(np.asarray(src_mask) != 0, dtype=np.uint8)
        if m.shape != (lon.shape[0] - 1, lon.shape[1] - 1):
            raise ValueError("curvilinear exchange grid: the source mask is %s, the source cells %s"
                             % (m.shape, (lon.shape[0] - 1, lon.shape[1] - 1)))
    return lon, lat, m


def counts_dict(c):
    return L.counts_dict(FIELDS, c)


# ---- results ---------------------------------------------------------------------------------------------------
def covered(index, n, area, total):
    """the fraction of every one of n cells covered by the list's exchange cells: their areas summed per cell with np.bincount in list
    order, over the cell's area (NaN where the cell has no positive area)"""
    s = np.bincount(index, weights=area, minlength=n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total.reshape(-1) > 0, s / total.reshape(-1), np.nan).reshape(total.shape)


def result(src, ocn, area, a_poly, a_src, counts, Re, threshold, masked=False, src_masked=False):
    """What exchange_grid_curv() returns: the list (src (n, 2) = (I, J), ocn (n, 2) = (n, m), area (n,)), A_poly per model cell and
    A_src per source cell, the covered fraction of every model cell (ocn_frac) and of every source cell (src_frac), the counts and a
    summary."""
    NB, NA = a_src.shape
    ny, nx = a_poly.shape
    ocn_frac = covered(ocn[:, 1].astype(np.int64) * nx + ocn[:, 0], ny * nx, area, a_poly)
    src_frac = covered(src[:, 1].astype(np.int64) * NA + src[:, 0], NB * NA, area, a_src)
    pos = lambda a: float(np.sum(a[np.isfinite(a) & (a > 0)]))   # noqa: E731
    summary = dict(counts, source_shape=[int(NB), int(NA)], ocean_shape=[int(ny), int(nx)], Re=float(Re), threshold=float(threshold),
                   masked=bool(masked), source_masked=bool(src_masked), area_sum=float(np.sum(area)), a_poly_sum=pos(a_poly),
                   a_src_sum=pos(a_src), sphere=float(4.0 * np.pi * Re * Re),
                   ocean_cells_covered=int(np.sum(ocn_frac > 0)), source_cells_covered=int(np.sum(src_frac > 0)))
    return {"src": src, "ocn": ocn, "area": area, "a_poly": a_poly, "a_src": a_src, "ocn_frac": ocn_frac, "src_frac": src_frac,
            "counts": counts, "summary": summary}


# ---- host arrays -----------------------------------------------------------------------------------------------
def exchange_grid_curv(x, y, src_lon, src_lat, mask=None, src_mask=None, Re=DEFAULT_RE, threshold=DEFAULT_THRESHOLD, capacity=None):
    """The exchange grid of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny even) and a curvilinear source of cell
    corners src_lon, src_lat ((NB + 1) x (NA + 1), degrees), on one GPU through the host-pointer entry.  mask / src_mask: None, or one
    value per model / source cell; a cell where it is 0 emits nothing.  capacity: the list's first allocation (grown once)."""
    x, y = L.as_f64(x), L.as_f64(y)
    if x.ndim != 2 or y.shape != x.shape:
        raise ValueError("exchange grid: x %s and y %s must be 2-D of one shape" % (x.shape, y.shape))
    nyp, nxp = x.shape
    check_grid(nyp, nxp)
    check_args(threshold, Re)
    lon, lat, sm = checked_source(src_lon, src_lat, src_mask)
    NB, NA = lon.shape[0] - 1, lon.shape[1] - 1
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = host_mask(mask, shape)
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(Re), threshold=float(threshold))
    band.x, band.y = L.ptr(x), L.ptr(y)
    band.x_next, band.y_next = L.ptr(x[nyp - 1:]), L.ptr(y[nyp - 1:])
    band.mask = None if m is None else m.ctypes.data
    desc = src_desc(lon.ctypes.data, lat.ctypes.data, NA, NB, mask_ptr=None if sm is None else sm.ctypes.data)
    a_poly = np.empty(shape, dtype=np.float64)
    a_src = np.empty((NB, NA), dtype=np.float64)
    counts = L.XgridCurvCounts()
    cap = 4 * (shape[0] * shape[1] + NA * NB) + 4096 if capacity is None else int(capacity)
    lib = L.load()
    for _ in range(2):   # a second call only when the first capacity was too small
        sij = np.empty((cap, 2), dtype=np.int32)
        ocn = np.empty((cap, 2), dtype=np.int32)
        area = np.empty(cap, dtype=np.float64)
        rc = lib.ogg_xgrid_curv(ctypes.byref(band), ctypes.byref(desc), cap, sij.ctypes.data, ocn.ctypes.data, area.ctypes.data,
                                a_poly.ctypes.data, a_src.ctypes.data, ctypes.byref(counts))
        if rc == L.OGG_ESHAPE and counts.kept > cap:
            cap = int(counts.kept)
            continue
        L.check(rc)
        break
    n = int(counts.kept)
    return result(sij[:n].copy(), ocn[:n].copy(), area[:n].copy(), a_poly, a_src, counts_dict(counts), Re, threshold, m is not None,
                  sm is not None)


# ---- device arrays ---------------------------------------------------------------------------------------------
def band_lists_dev(band, desc, stream, device, events=None):
    """The three steps on descriptors of device pointers: (first model row, counts (int64 device tensor), a_poly (rows x nx/2), a_src
    (NB x NA), src (int32 (n, 2) = (I, J)), ocn (int32 (n, 2)), area), synchronised twice: the host reads the number of candidates (the
    pair workspace's size) and the list's length.  ``events``: a list that takes six torch events around the three steps
    (scripts/xgrid_curv_profile.py)."""
    import torch
    lib = L.load()
    mark = (lambda: None) if events is None else (lambda: (events.append(torch.cuda.Event(enable_timing=True)), events[-1].record()))
    m0 = int(lib.ogg_xgrid_band_first_row(ctypes.byref(band)))
    rows = int(lib.ogg_xgrid_band_out_rows(ctypes.byref(band)))
    ws_bytes = int(lib.ogg_xgrid_curv_workspace_bytes(ctypes.byref(band), ctypes.byref(desc), -1))
    if ws_bytes < 0:
        raise ValueError("curvilinear exchange grid: bad band or source")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    a_poly = torch.empty((rows, band.nx // 2), dtype=torch.float64, device=device)
    a_src = torch.empty((desc.NB, desc.NA), dtype=torch.float64, device=device)
    counts = torch.zeros(len(FIELDS), dtype=torch.int64, device=device)
    mark()
    L.call("ogg_xgrid_curv_sets_dev", ctypes.byref(band), ctypes.byref(desc), ws.data_ptr(), ws_bytes, a_poly.data_ptr(), a_src.data_ptr(),
           counts.data_ptr(), stream)
    mark()
    cand = int(counts[FIELDS.index("candidates")].item())
    pw_bytes = int(lib.ogg_xgrid_curv_workspace_bytes(ctypes.byref(band), ctypes.byref(desc), cand))
    if pw_bytes < 0:
        raise ValueError("curvilinear exchange grid: %d candidate pairs in one band: fewer than 2^31 are accepted" % cand)
    pw = torch.empty(pw_bytes, dtype=torch.uint8, device=device)
    mark()
    L.call("ogg_xgrid_curv_clip_dev", ctypes.byref(band), ctypes.byref(desc), ws.data_ptr(), ws_bytes, cand, pw.data_ptr(), pw_bytes,
           counts.data_ptr(), stream)
    mark()
    n = int(counts[FIELDS.index("kept")].item())
    sij = torch.empty((n, 2), dtype=torch.int32, device=device)
    ocn = torch.empty((n, 2), dtype=torch.int32, device=device)
    area = torch.empty(n, dtype=torch.float64, device=device)
    mark()
    if n:
        L.call("ogg_xgrid_curv_write_dev", ctypes.byref(band), ctypes.byref(desc), cand, pw.data_ptr(), pw_bytes, sij.data_ptr(),
               ocn.data_ptr(), area.data_ptr(), stream)
    mark()
    return m0, counts, a_poly, a_src, sij, ocn, area


def whole_band(x, y, mask, Re, threshold):
    """ogg_xgrid_band of a whole stitched grid on the device as one band: x, y float64 device tensors with contiguous rows, mask None or
    a uint8 device tensor"""
    nyp, nxp = x.shape
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(Re), threshold=float(threshold))
    band.x, band.y = x.data_ptr(), y.data_ptr()
    band.x_next, band.y_next = x[nyp - 1:].data_ptr(), y[nyp - 1:].data_ptr()
    band.mask = None if mask is None else mask.data_ptr()
    return band


def exchange_grid_curv_dev(x, y, src_lon, src_lat, mask=None, src_mask=None, Re=DEFAULT_RE, threshold=DEFAULT_THRESHOLD, stream=None):
    """exchange_grid_curv on device tensors: x, y ((ny + 1) x (nx + 1)) and src_lon, src_lat ((NB + 1) x (NA + 1)) float64 tensors on one
    device, the masks None or tensors of one value per cell.  The source's rows may be padded (stride(0) >= NA + 1, stride(1) == 1).
    The result holds device tensors for the list, a_poly and a_src, and host numbers for the counts."""
    import torch
    if x.dim() != 2 or y.shape != x.shape or src_lon.dim() != 2 or src_lat.shape != src_lon.shape:
        raise ValueError("curvilinear exchange grid: x, y and src_lon, src_lat must be 2-D, each pair of one shape")
    nyp, nxp = x.shape
    check_grid(nyp, nxp)
    check_args(threshold, Re)
    x, y = x.contiguous(), y.contiguous()
    if src_lon.stride(1) != 1 or src_lat.stride() != src_lon.stride():
        src_lon, src_lat = src_lon.contiguous(), src_lat.contiguous()
    NB, NA = src_lon.shape[0] - 1, src_lon.shape[1] - 1
    byte = lambda m, shape: None if m is None else (m != 0).to(torch.uint8).reshape(shape).contiguous()   # noqa: E731
    mt, st = byte(mask, ((nyp - 1) // 2, (nxp - 1) // 2)), byte(src_mask, (NB, NA))
    desc = src_desc(src_lon.data_ptr(), src_lat.data_ptr(), NA, NB, ld=src_lon.stride(0), mask_ptr=None if st is None else st.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    _, counts, a_poly, a_src, sij, ocn, area = band_lists_dev(whole_band(x, y, mt, Re, threshold), desc, stream, x.device)
    return {"src": sij, "ocn": ocn, "area": area, "a_poly": a_poly, "a_src": a_src, "counts": counts_dict(counts.cpu().numpy())}


def source_areas_dev(src_lon, src_lat, src_mask=None, Re=DEFAULT_RE, stream=None):
    """(A_src (NB x NA host array), the counts as a host array) of a source on the device alone: the sets step on a band without a
    model row"""
    import torch
    dev = src_lon.device
    NB, NA = src_lon.shape[0] - 1, src_lon.shape[1] - 1
    desc = src_desc(src_lon.data_ptr(), src_lat.data_ptr(), NA, NB, ld=src_lon.stride(0),
                    mask_ptr=None if src_mask is None else src_mask.data_ptr())
    band = L.XgridBand(nx=2, ny=2, j0=1, n_cell_rows=1, Re=float(Re), threshold=0.0)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _, counts, _, a_src, _, _, _ = band_lists_dev(band, desc, stream, dev)
    return a_src.cpu().numpy(), counts.cpu().numpy()


def assemble(pieces, shape, Re, threshold, masked=False, src_masked=False):
    """The result of the whole grid from [(first model row, counts, a_poly, a_src, src, ocn, area)] as host arrays, in piece order.  The
    source is whole in every piece: its counts and A_src are the first piece's."""
    a_poly = np.full(shape, np.nan)
    counts = {f: 0 for f in FIELDS}
    for k, (m0, c, ap, _, _, _, _) in enumerate(pieces):
        a_poly[m0:m0 + ap.shape[0]] = ap
        for i, f in enumerate(FIELDS):
            if f not in SOURCE_FIELDS or k == 0:
                counts[f] += int(c[i])
    cat = lambda k: np.concatenate([p[k] for p in pieces]) if pieces else np.zeros((0, 2), np.int32)   # noqa: E731
    area = np.concatenate([p[6] for p in pieces]) if pieces else np.zeros(0)
    a_src = np.asarray(pieces[0][3]) if pieces else np.zeros((0, 0))
    return result(cat(4), cat(5), area, a_poly, a_src, counts, Re, threshold, masked, src_masked)


# ---- files -----------------------------------------------------------------------------------------------------
def read_source_corners(path, names=None):
    """(lon, lat) of the cell corners of a source grid file: two 2-D variables ``names`` = (LONVAR, LATVAR) of a classic NetCDF file, or,
    without names, every second point of x, y of a MOM6 supergrid"""
    if names is None:
        g = netcdf3.read_doubles(path, names=("x", "y"))
        return np.ascontiguousarray(g["x"][0::2, 0::2]), np.ascontiguousarray(g["y"][0::2, 0::2])
    h = netcdf3.read_header(path)
    out = []
    for name in names:
        if name not in h.vars:
            raise KeyError("%s: no variable %s" % (path, name))
        v = h.vars[name]
        a = np.frombuffer(netcdf3.read_var_bytes(path, h, name, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)
        if a.ndim != 2:
            raise ValueError("%s: %s is %d-D, the corners must be 2-D" % (path, name, a.ndim))
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    return out[0], out[1]


def summary_lines(res):
    s = res["summary"]
    return ["   curvilinear exchange grid: %d exchange cells of %d x %d source cells and %d x %d ocean cells%s; area %.15g of the ocean "
            "cells', %.15g of the source cells'; %d ocean and %d source cells covered"
            % (s["kept"], s["source_shape"][1], s["source_shape"][0], s["ocean_shape"][1], s["ocean_shape"][0],
               " (masked)" if s["masked"] or s["source_masked"] else "", s["area_sum"] / s["a_poly_sum"] if s["a_poly_sum"] else 0.0,
               s["area_sum"] / s["a_src_sum"] if s["a_src_sum"] else 0.0, s["ocean_cells_covered"], s["source_cells_covered"]),
            "   curvilinear exchange grid: %d candidates; ocean cells skipped: %d wide, %d inverted, %d degenerate, %d masked; source cells "
            "skipped: %d wide, %d flat, %d degenerate, %d masked (%d reversed cells taken in the other order)"
            % (s["candidates"], s["wide"], s["inverted"], s["degenerate"], s["masked"], s["src_wide"], s["src_flat"], s["src_degenerate"],
               s["src_masked"], s["src_reversed"])]


def write_xgrid_curv(path, res):
    """the FMS first-order layout of exchange_grid.write_xgrid: tile1_cell is the source cell (i, j), tile2_cell the ocean model cell"""
    write_xgrid(path, dict(res, atm=res["src"]))


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.exchange_grid_curv",
                                description="exchange grid of a supergrid file and a curvilinear source grid")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("source_grid", help="the source: a MOM6 supergrid (every second point of x, y), or a file named by --source_corners")
    p.add_argument("--source_corners", nargs=2, default=None, metavar=("LONVAR", "LATVAR"), help="two 2-D variables of cell corners")
    w = p.add_mutually_exclusive_group()
    w.add_argument("--topog", default=None, help="topog.nc: only cells with depth > 0 exchange")
    w.add_argument("--mask", default=None, help="ocean_mask.nc: only cells with mask != 0 exchange")
    p.add_argument("--source_mask", default=None, help="a mask file of the source's cells: only cells with mask != 0 exchange")
    p.add_argument("-o", "--output", default=DEFAULT_FILE)
    p.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD, help="area ratio below which an overlap is dropped")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    g = netcdf3.read_doubles(a.grid, names=("x", "y"))
    lon, lat = read_source_corners(a.source_grid, a.source_corners)
    from .remap import mask_from_file
    mask = mask_from_topog(a.topog) if a.topog else (mask_from_file(a.mask) if a.mask else None)
    res = exchange_grid_curv(g["x"], g["y"], lon, lat, mask=mask, src_mask=mask_from_file(a.source_mask) if a.source_mask else None,
                             threshold=a.threshold)
    for line in summary_lines(res):
        print(line)
    write_xgrid_curv(a.output, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

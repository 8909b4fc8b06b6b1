"""Atmosphere x ocean exchange grid: every non-empty overlap of a rectilinear global atmosphere cell with a MOM6 model (h) cell of a
supergrid, with its area, written in the layout of FMS's first-order exchange-grid files (``atmos_mosaic_tile1Xocean_mosaic_tile1.nc``,
as make_coupler_mosaic writes them).  include/ogg_hip.h, "Atmosphere x ocean exchange grid", gives the definition.  The reference
has no such step.

The overlaps are found and measured on the device by libogg_hip.so (ogg_xgrid_count_dev / ogg_xgrid_write_dev / ogg_xgrid).  The list
is in one canonical order (ocean cells row-major, then atmosphere rows, then columns) and nothing is summed across cells, so it is
bit-identical whatever the split of the grid into bands or ranks.  The ocean fraction of each atmosphere cell is formed here from
the list, in list order.

    python -m ocean_model_grid_generator_amd.exchange_grid ocean_hgrid.nc --atm NLON NLAT [--topog topog.nc] -o FILE [--json FILE]
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import netcdf3

DEFAULT_THRESHOLD = 1.0e-6    # FMS's AREA_RATIO_THRESH
DEFAULT_FILE = "atmos_mosaic_tile1Xocean_mosaic_tile1.nc"
DEFAULT_RE = 6371.0e3


def regular_atm(nlon, nlat):
    """The edges of a regular global atmosphere of nlon x nlat cells."""
    nlon, nlat = int(nlon), int(nlat)
    if nlon < 1 or nlat < 1:
        raise ValueError("exchange grid: the atmosphere needs at least one cell each way (%d x %d)" % (nlon, nlat))
    return 360.0 * np.arange(nlon + 1) / nlon, -90.0 + 180.0 * np.arange(nlat + 1) / nlat


def atm_edges(lon_edges, lat_edges):
    """(lon, lat) as contiguous float64 arrays, checked by the library (OGG_EARG -> ValueError)."""
    lon, lat = L.as_f64(lon_edges).reshape(-1), L.as_f64(lat_edges).reshape(-1)
    if lon.size < 2 or lat.size < 2:
        raise ValueError("exchange grid: the atmosphere needs at least two lon and two lat edges")
    L.checked("ogg_xgrid_check_atm", L.XgridAtm(lon=lon.ctypes.data, lat=lat.ctypes.data, NA=lon.size - 1, NB=lat.size - 1))
    return lon, lat


def check_grid(nyp, nxp):
    ny, nx = nyp - 1, nxp - 1
    if ny < 2 or nx < 2 or ny % 2 or nx % 2:
        raise ValueError("exchange grid: model cells are 2 x 2 supergrid cells, but the supergrid has %d x %d cells; generate it with "
                         "--ensure_nj_even" % (ny, nx))


def check_args(threshold, Re):
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("exchange grid: threshold must be >= 0 (%r)" % (threshold,))
    if not (np.isfinite(Re) and Re > 0):
        raise ValueError("exchange grid: Re must be positive (%r)" % (Re,))


def counts_dict(c):
    return L.counts_dict(L.XGRID_COUNT_FIELDS, c)


# ---- results ---------------------------------------------------------------------------------------------------
def atm_area(lon, lat, Re):
    """A_atm of every atmosphere cell (NB x NA): Re^2 dlam (sin b_J+1 - sin b_J), formed as the definition's keep step has it.  The
    lat-lon regrid takes these bits as its cell areas, so its fractions and ocean_frac's are one number."""
    D = np.pi / 180.0
    b1, b2 = lat[:-1] * D, lat[1:] * D
    return (Re * Re) * (lon[1:] * D - lon[:-1] * D)[None, :] * (2.0 * np.cos((b1 + b2) / 2.0) * np.sin((b2 - b1) / 2.0))[:, None]


def ocean_frac(atm, area, lon, lat, Re):
    """The fraction of every atmosphere cell (NB x NA) covered by the list's exchange cells: their areas summed per atmosphere cell
    with np.bincount in list order, over the cell's area (Re^2 dlam (sin b_J+1 - sin b_J), formed as the definition has it)."""
    NA, NB = lon.size - 1, lat.size - 1
    a_atm = atm_area(lon, lat, Re)
    s = np.bincount(atm[:, 1].astype(np.int64) * NA + atm[:, 0], weights=area, minlength=NA * NB).reshape(NB, NA)
    return s / a_atm, a_atm


def result(atm, ocn, area, a_poly, counts, lon, lat, Re, threshold, masked=False):
    """What exchange_grid() returns: the list (atm (n, 2) = (I, J), ocn (n, 2) = (n, m), area (n,)), A_poly per model cell, the
    ocean fraction per atmosphere cell, the counts and a summary."""
    frac, a_atm = ocean_frac(atm, area, lon, lat, Re)
    ok = np.isfinite(a_poly)
    summary = dict(counts, n_atm_lon=int(lon.size - 1), n_atm_lat=int(lat.size - 1), ocean_shape=list(a_poly.shape), Re=float(Re),
                   threshold=float(threshold), masked=bool(masked), area_sum=float(np.sum(area)),
                   a_poly_sum=float(np.sum(a_poly[ok & (a_poly > 0)])), sphere=float(4.0 * np.pi * Re * Re))
    return {"atm": atm, "ocn": ocn, "area": area, "a_poly": a_poly, "ocean_frac": frac, "a_atm": a_atm, "lon_edges": lon,
            "lat_edges": lat, "counts": counts, "summary": summary}


# ---- host arrays -----------------------------------------------------------------------------------------------
def exchange_grid(x, y, lon_edges, lat_edges, mask=None, Re=DEFAULT_RE, threshold=DEFAULT_THRESHOLD):
    """The exchange grid of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny even) and an atmosphere of edges lon_edges
    (global: spanning 360 degrees) and lat_edges, on one GPU through the host-pointer entry.  mask: None, or one value per model cell
    ((ny / 2) x (nx / 2)); a cell where it is 0 emits nothing."""
    x, y = L.as_f64(x), L.as_f64(y)
    if x.ndim != 2 or y.shape != x.shape:
        raise ValueError("exchange grid: x %s and y %s must be 2-D of one shape" % (x.shape, y.shape))
    nyp, nxp = x.shape
    check_grid(nyp, nxp)
    check_args(threshold, Re)
    lon, lat = atm_edges(lon_edges, lat_edges)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != shape:
            raise ValueError("exchange grid: the mask is %s, the model cells %s" % (m.shape, shape))
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(Re), threshold=float(threshold))
    band.x, band.y = L.ptr(x), L.ptr(y)
    band.x_next, band.y_next = L.ptr(x[nyp - 1:]), L.ptr(y[nyp - 1:])
    band.mask = None if m is None else m.ctypes.data
    desc = L.XgridAtm(lon=lon.ctypes.data, lat=lat.ctypes.data, NA=lon.size - 1, NB=lat.size - 1)
    a_poly = np.empty(shape, dtype=np.float64)
    counts = L.XgridCounts()
    cap = 4 * shape[0] * shape[1] + 4096
    lib = L.load()
    for _ in range(2):   # a second call only when the first capacity was too small
        atm = np.empty((cap, 2), dtype=np.int32)
        ocn = np.empty((cap, 2), dtype=np.int32)
        area = np.empty(cap, dtype=np.float64)
        rc = lib.ogg_xgrid(ctypes.byref(band), ctypes.byref(desc), cap, atm.ctypes.data, ocn.ctypes.data, area.ctypes.data,
                           a_poly.ctypes.data, ctypes.byref(counts))
        if rc == L.OGG_ESHAPE and counts.kept > cap:
            cap = int(counts.kept)
            continue
        L.check(rc)
        break
    n = int(counts.kept)
    return result(atm[:n].copy(), ocn[:n].copy(), area[:n].copy(), a_poly, counts_dict(counts), lon, lat, Re, threshold, m is not None)


# ---- device arrays ---------------------------------------------------------------------------------------------
def band_lists_dev(band, atm_desc, stream, device):
    """Both steps on a descriptor of device pointers: (first model row, counts (int64 device tensor of 8), a_poly (rows x nx/2), atm,
    ocn (int32 (n, 2)), area), synchronised once between the steps (the list's length)."""
    import torch
    lib = L.load()
    m0 = int(lib.ogg_xgrid_band_first_row(ctypes.byref(band)))
    rows = int(lib.ogg_xgrid_band_out_rows(ctypes.byref(band)))
    ws_bytes = int(lib.ogg_xgrid_workspace_bytes(ctypes.byref(band), ctypes.byref(atm_desc)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    a_poly = torch.empty((rows, band.nx // 2), dtype=torch.float64, device=device)
    counts = torch.zeros(len(L.XGRID_COUNT_FIELDS), dtype=torch.int64, device=device)
    L.call("ogg_xgrid_count_dev", ctypes.byref(band), ctypes.byref(atm_desc), ws.data_ptr(), ws_bytes, a_poly.data_ptr(),
           counts.data_ptr(), stream)
    n = int(counts[L.XGRID_COUNT_FIELDS.index("kept")].item())
    atm = torch.empty((n, 2), dtype=torch.int32, device=device)
    ocn = torch.empty((n, 2), dtype=torch.int32, device=device)
    area = torch.empty(n, dtype=torch.float64, device=device)
    if n:
        L.call("ogg_xgrid_write_dev", ctypes.byref(band), ctypes.byref(atm_desc), ws.data_ptr(), ws_bytes, atm.data_ptr(),
               ocn.data_ptr(), area.data_ptr(), stream)
    return m0, counts, a_poly, atm, ocn, area


def whole_grid_lists_dev(x, y, lon, lat, mask, Re, threshold, stream, device):
    """band_lists_dev of the whole stitched grid as one band: x, y float64 device tensors ((ny + 1) x (nx + 1), contiguous rows), the
    atmosphere's edges lon, lat and the mask (None or one byte per model cell) as host arrays.  (atm, ocn, area, the mask on the
    device or None)."""
    import torch
    nyp, nxp = x.shape
    lt, bt = torch.from_numpy(lon).to(device), torch.from_numpy(lat).to(device)
    desc = L.XgridAtm(lon=lt.data_ptr(), lat=bt.data_ptr(), NA=lon.size - 1, NB=lat.size - 1)
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(Re), threshold=float(threshold))
    band.x, band.y = x.data_ptr(), y.data_ptr()
    band.x_next, band.y_next = x[nyp - 1:].data_ptr(), y[nyp - 1:].data_ptr()
    mt = None if mask is None else torch.from_numpy(mask).to(device)
    band.mask = None if mt is None else mt.data_ptr()
    _, _, _, atm, ocn, area = band_lists_dev(band, desc, stream, device)
    return atm, ocn, area, mt


def assemble(pieces, shape, lon, lat, Re, threshold, masked):
    """The result of the whole grid from [(first model row, counts, a_poly, atm, ocn, area)] as host arrays, in piece order."""
    a_poly = np.full(shape, np.nan)
    counts = {f: 0 for f in L.XGRID_COUNT_FIELDS}
    for m0, c, ap, _, _, _ in pieces:
        a_poly[m0:m0 + ap.shape[0]] = ap
        for k, f in enumerate(L.XGRID_COUNT_FIELDS):
            counts[f] += int(c[k])
    cat = lambda k, empty: np.concatenate([p[k] for p in pieces]) if pieces else empty   # noqa: E731
    atm = cat(3, np.zeros((0, 2), np.int32))
    ocn = cat(4, np.zeros((0, 2), np.int32))
    area = cat(5, np.zeros(0))
    return result(atm, ocn, area, a_poly, counts, lon, lat, Re, threshold, masked)


# ---- files -----------------------------------------------------------------------------------------------------
def write_xgrid(path, res):
    """The FMS first-order exchange-grid layout (NetCDF 64-bit offset): dims ncells, two; tile1_cell (atmosphere (i, j)) and tile2_cell
    (ocean model cell (i, j)), 1-based ints; xgrid_area in m2."""
    n = int(res["area"].size)
    ds = netcdf3.Dataset(path, [("ncells", n), ("two", 2)])
    ds.def_var("tile1_cell", netcdf3.NC_INT, ("ncells", "two"), [("standard_name", "parent_cell_indices_in_mosaic1")],
               res["atm"].astype(np.int32) + 1)
    ds.def_var("tile2_cell", netcdf3.NC_INT, ("ncells", "two"), [("standard_name", "parent_cell_indices_in_mosaic2")],
               res["ocn"].astype(np.int32) + 1)
    ds.def_var("xgrid_area", netcdf3.NC_DOUBLE, ("ncells",), [("standard_name", "exchange_grid_area"), ("units", "m2")], res["area"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    frac = res["ocean_frac"]
    return ["   exchange grid: %d exchange cells of %d x %d atmosphere cells and %d x %d ocean cells%s; area %.15g of 4 pi Re^2, "
            "%d atmosphere cells with ocean" % (s["kept"], s["n_atm_lon"], s["n_atm_lat"], s["ocean_shape"][1], s["ocean_shape"][0],
                                               " (masked)" if s["masked"] else "", s["area_sum"] / s["sphere"], int(np.sum(frac > 0))),
            "   exchange grid: %d candidates; %d cells with pole corners, %d pole-enclosing, %d inverted, %d degenerate, %d masked"
            % (s["candidates"], s["pole_cells"], s["pole_enclosing"], s["inverted"], s["degenerate"], s["masked"])]


def wet_mask(depth, fill=1.0e20):
    """depth > 0 (the convention of FMS atmosphere x ocean files: only wet cells exchange); a cell whose depth is the fill value (no
    valid sample) is dry."""
    d = np.asarray(depth)
    return ((d > 0) & (d != fill)).astype(np.uint8)


def mask_from_topog(path):
    """wet_mask of the depth of a topog.nc"""
    h = netcdf3.read_header(path)
    if "depth" not in h.vars:
        raise KeyError("%s: no variable depth" % path)
    v = h.vars["depth"]
    d = np.frombuffer(netcdf3.read_var_bytes(path, h, "depth", dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)
    fv = v.atts.get("_FillValue")
    return wet_mask(d.astype(np.float64), 1.0e20 if fv is None or isinstance(fv, str) else float(np.asarray(fv).reshape(-1)[0]))


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.exchange_grid",
                                description="atmosphere x ocean exchange grid of a supergrid file and a regular global atmosphere")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("--atm", type=int, nargs=2, required=True, metavar=("NLON", "NLAT"), help="a regular global atmosphere of NLON x NLAT cells")
    p.add_argument("--topog", default=None, help="topog.nc: only cells with depth > 0 exchange")
    p.add_argument("-o", "--output", default=DEFAULT_FILE)
    p.add_argument("--threshold", type=float, default=DEFAULT_THRESHOLD, help="area ratio below which an overlap is dropped")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    g = netcdf3.read_doubles(a.grid, names=("x", "y"))
    lon, lat = regular_atm(*a.atm)
    mask = mask_from_topog(a.topog) if a.topog else None
    res = exchange_grid(g["x"], g["y"], lon, lat, mask=mask, threshold=a.threshold)
    for line in summary_lines(res):
        print(line)
    write_xgrid(a.output, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

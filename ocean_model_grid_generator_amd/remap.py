"""Conservative remap: fields on a global lat-lon grid (temperature and salinity climatologies, monthly SST, chlorophyll, tides) put on
the model cells of a supergrid, first-order conservatively, with the wet cells the source leaves empty filled from their neighbours.
include/ogg_hip.h, "Conservative remap", gives the definition; the reference has no such step.

The weights are the exchange list of exchange_grid.py between the source's cell edges and the model cells.  The segmented, masked,
weighted sums and the fill run on the device (ogg_remap_segments_dev / ogg_remap_dev / ogg_remap_fill_dev, or the host-pointer
ogg_remap); every value is a fixed function of the list, the source and values at smaller fill distance, so the result is
bit-identical for any launch geometry and any number of ranks.

    python -m ocean_model_grid_generator_amd.remap ocean_hgrid.nc SOURCE --var V [--var V2 ...] [--topog topog.nc | --mask ocean_mask.nc]
        [--source_grid SRC_GRID.nc [--source_corners LONVAR LATVAR]] [--no_fill] [--fill_max N] -o remapped.nc [--json summary.json]

SOURCE is a NetCDF classic / 64-bit-offset file; each variable's last two dimensions are latitude and longitude (either order) on
uniform 1-D coordinates spanning 360 degrees of longitude; every dimension ahead of them is a record dimension.  With --source_grid
the source's variables are fields on the cells of that curvilinear grid (exchange_grid_curv.py gives the weights).
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _lib as L
from . import exchange_grid as X
from . import fields as F
from . import netcdf3

FILL = L.REMAP_FILL
FLAG_NAMES = ("dry", "remapped", "filled", "unfilled")
CDF2_VAR_LIMIT = F.CDF2_VAR_LIMIT
_DTYPES = F.DTYPES


# ---- sources -------------------------------------------------------------------------------------------------
class Source(F.Field):
    """A field on a global rectilinear grid: a fields.Field with data (..., NB, NA), row 0 southmost, and its cell edges lon (NA + 1,
    spanning 360 degrees) and lat (NB + 1, increasing, inside [-90, 90])."""
    _who = "remap source"

    def __init__(self, data, lon_edges, lat_edges, fill=(), name="field", lead_dims=None, coords=(), atts=(), note="", record_dim=None):
        F.Field.__init__(self, data, fill, name, lead_dims, coords, atts, note, record_dim)
        self.lon, self.lat = X.atm_edges(lon_edges, lat_edges)
        if self.data.shape[-2:] != (self.lat.size - 1, self.lon.size - 1):
            raise ValueError("remap source: data %s and %d x %d cells (lat x lon edges - 1)" % (self.data.shape, self.lat.size - 1, self.lon.size - 1))

    NA = property(lambda self: self.lon.size - 1)
    NB = property(lambda self: self.lat.size - 1)


class CurvilinearSource(F.Field):
    """A field on the cells of a curvilinear grid: a fields.Field with data (..., NB, NA) and the cells' corners corner_lon, corner_lat
    ((NB + 1) x (NA + 1), degrees), cell (J, I) between corners (J, I) and (J + 1, I + 1); rows may run north to south.  The weights are
    the list of exchange_grid_curv.py (great-circle edges; source cells wider than 30 degrees give nothing).  mask: None, or one value
    per source cell (0: the cell gives nothing)."""
    _who = "remap source"

    def __init__(self, data, corner_lon, corner_lat, fill=(), name="field", lead_dims=None, coords=(), atts=(), note="", record_dim=None,
                 mask=None):
        from . import exchange_grid_curv as XC
        F.Field.__init__(self, data, fill, name, lead_dims, coords, atts, note, record_dim)
        self.corner_lon, self.corner_lat, self.mask = XC.checked_source(corner_lon, corner_lat, mask)
        if self.data.shape[-2:] != (self.NB, self.NA):
            raise ValueError("remap source: data %s and %d x %d cells (corners - 1)" % (self.data.shape, self.NB, self.NA))
        XC.src_desc(None, None, self.NA, self.NB)

    NA = property(lambda self: self.corner_lon.shape[1] - 1)
    NB = property(lambda self: self.corner_lon.shape[0] - 1)


class _Last2(object):
    """the last two dimensions of a variable, as fields.lat_lon_dims reads them"""

    def __init__(self, v):
        self.name, self.dims = v.name, v.dims[-2:]


def read_source(path, var):
    """A Source from a NetCDF classic or 64-bit-offset file (_read_source); record (unlimited) variables are refused."""
    return _read_source(path, var)


def _read_source(path, var, records=False):
    """A Source from a NetCDF classic (CDF-1) or 64-bit-offset (CDF-2) file: the byte / short / float / double variable ``var``,
    whose last two dimensions are latitude and longitude in either order (told apart by the coordinates' units or names, as for
    topography), on uniform 1-D coordinates (cell centres or edges).  Latitude edges at centres +- half a step are clamped to +-90;
    rows are flipped when latitude decreases.  A byte or short variable is unpacked to float64 as raw * scale_factor + add_offset,
    with missing values (_FillValue, missing_value, tested on the raw values) as NaN; float and double keep their type and their fill
    values.  CDF-5 and NetCDF-4 / HDF5 files are refused.  ``records`` (opt-in): a record (unlimited) variable is read too, its
    record dimension the first leading dimension (the Source's ``record_dim``), and so is the coordinate variable of that dimension."""
    h, v = F.open_variable(path, var, "sources", records)
    lat_name, lon_name = F.lat_lon_dims(path, h, _Last2(v))
    axes = {}
    for dname in (lat_name, lon_name):
        if dname not in h.vars:
            raise ValueError("%s: no coordinate variable for dimension %s of %s" % (path, dname, var))
        cv = h.vars[dname]
        raw = netcdf3.read_var_bytes(path, h, dname, dtype=cv.nc_type)
        axes[dname] = F.uniform_axis(path, dname, np.frombuffer(raw, dtype=netcdf3.NUMPY_DTYPE[cv.nc_type]))
    data, fills, lead, coords, keep = F.read_values(path, h, v, records, keep=("units", "long_name", "standard_name"))
    if v.dims[-2] == lon_name:   # stored (..., lon, lat)
        data = np.swapaxes(data, -1, -2)
    (lat, dlat), (lon, dlon) = axes[lat_name], axes[lon_name]
    if dlon < 0:
        raise ValueError("%s: longitude %s decreases" % (path, lon_name))
    if dlat < 0:
        data, lat, dlat = data[..., ::-1, :], lat[::-1], -dlat
    NB, NA = data.shape[-2:]
    if abs(NA * dlon - 360.0) > 1e-9 * 360.0:
        raise ValueError("%s: %s covers %.10g degrees of longitude (%d x %.10g); the remap needs a global source (360 degrees)"
                         % (path, var, NA * dlon, NA, dlon))
    lon0, kind_lon = F.axis_edges(lon[0], dlon)
    if min(abs(lat[0] - 0.5 * dlat + 90.0), abs(lat[-1] + 0.5 * dlat - 90.0)) <= 1e-6 * dlat:
        lat0, kind_lat = lat[0] - 0.5 * dlat, "centres"   # centres whose half-step edges reach a pole
    else:
        lat0, kind_lat = F.axis_edges(lat[0], dlat)
    lon_edges = lon0 + dlon * np.arange(NA + 1)
    lon_edges[-1] = lon_edges[0] + 360.0
    lat_edges = np.clip(lat0 + dlat * np.arange(NB + 1), -90.0, 90.0)
    for k, pole in ((0, -90.0), (NB, 90.0)):   # an edge within rounding of a pole is the pole
        if abs(lat_edges[k] - pole) <= 1e-6 * dlat:
            lat_edges[k] = pole
    note = "%s: %s %s, %d records of %d x %d cells, longitude coordinates taken as cell %s, latitude as cell %s" % (
        path, var, tuple(v.dims), int(np.prod(v.shape[:-2], dtype=np.int64)), NB, NA, kind_lon, kind_lat)
    return Source(data, lon_edges, lat_edges, fill=fills, name=var, lead_dims=lead, coords=coords, atts=keep, note=note,
                  record_dim=v.dims[0] if v.is_record else None)


def read_curvilinear_source(path, var, grid_path, corner_names=None):
    """A CurvilinearSource from two NetCDF classic or 64-bit-offset files: the byte / short / float / double variable ``var`` of
    ``path``, whose last two dimensions are the rows and columns of the source's cells, and the cells' corners from ``grid_path``
    (exchange_grid_curv.read_source_corners: a MOM6 supergrid, of which every second point is taken, or the two 2-D variables
    ``corner_names``).  Values are unpacked and missing values found as for read_source; record variables are refused."""
    from . import exchange_grid_curv as XC
    h, v = F.open_variable(path, var, "sources", False)
    data, fills, lead, coords, keep = F.read_values(path, h, v, False, keep=("units", "long_name", "standard_name"))
    lon, lat = XC.read_source_corners(grid_path, corner_names)
    NB, NA = data.shape[-2:]
    if lon.shape != (NB + 1, NA + 1):
        raise ValueError("%s: %s has %d x %d cells, but %s gives %d x %d corners (cells + 1 each way are needed)"
                         % (path, var, NB, NA, grid_path, lon.shape[0], lon.shape[1]))
    note = "%s: %s %s, %d records of %d x %d cells on the curvilinear grid of %s" % (
        path, var, tuple(v.dims), int(np.prod(v.shape[:-2], dtype=np.int64)), NB, NA, grid_path)
    return CurvilinearSource(data, lon, lat, fill=fills, name=var, lead_dims=lead, coords=coords, atts=keep, note=note)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, source, m0=0, periodic=False, fold=False, fill_max=None):
    """an ogg_remap_params, checked by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    p = L.RemapParams(ny=int(ny), nx=int(nx), m0=int(m0), NA=source.NA, NB=source.NB, nrec=source.nrec,
                      dtype=_DTYPES[source.data.dtype], n_fill=len(source.fill), topology=M.topology_flags(periodic, fold),
                      fill_max=-1 if fill_max is None else int(fill_max))
    for k, f in enumerate(source.fill):
        p.fill[k] = float(f)
    if fill_max is not None and int(fill_max) < 0:
        raise ValueError("remap: fill_max must be >= 0 (%r)" % (fill_max,))
    return L.checked("ogg_remap_check", p)


def counts_dict(c):
    return L.counts_dict(L.REMAP_COUNT_FIELDS, c)


def result(values, flags, counts, source, periodic, fold, fill, fill_max, masked):
    """What remap() returns: values and flags (lead dims of the source, ny, nx), the counts and a summary."""
    if counts["bad_entries"]:
        raise ValueError("remap: %d list entries lie outside the cells or the source: the list belongs to other edges or rows"
                         % counts["bad_entries"])
    shape = tuple(source.data.shape[:-2]) + values.shape[-2:]
    summary = dict(counts, var=source.name, records=source.nrec, source_shape=[source.NB, source.NA],
                   shape=list(values.shape[-2:]), periodic=bool(periodic), fold=bool(fold), fill=bool(fill),
                   fill_max=None if fill_max is None else int(fill_max), masked=bool(masked))
    del summary["bad_entries"]
    return {"values": values.reshape(shape), "flags": flags.reshape(shape), "counts": counts, "summary": summary}


# ---- host arrays -----------------------------------------------------------------------------------------------
def remap(x, y, source, lon_edges=None, lat_edges=None, mask=None, fill=True, fill_max=None, fill_values=(),
          threshold=X.DEFAULT_THRESHOLD, Re=X.DEFAULT_RE):
    """The conservative remap of ``source`` onto the model cells of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny
    even), on one GPU through the host-pointer entries (ogg_xgrid, or ogg_xgrid_curv for a CurvilinearSource, for the list, ogg_remap
    for the rest).  ``source``: a Source, a CurvilinearSource, or an
    array (..., NB, NA) with lon_edges, lat_edges and fill_values.  mask: None or one value per model cell (0: dry).  fill: fill
    the wet cells the source leaves empty (up to fill_max steps, None: no limit).  A dict: values, flags (the source's leading
    dimensions, then (ny / 2, nx / 2)), counts, summary."""
    from . import ocean_mask as M
    if not isinstance(source, (Source, CurvilinearSource)):
        source = Source(source, lon_edges, lat_edges, fill=fill_values)
    x, y = L.as_f64(x), L.as_f64(y)
    if isinstance(source, CurvilinearSource):
        from . import exchange_grid_curv as XC
        lists = XC.exchange_grid_curv(x, y, source.corner_lon, source.corner_lat, mask=mask, src_mask=source.mask, Re=Re, threshold=threshold)
        lists["atm"] = lists["src"]
    else:
        lists = X.exchange_grid(x, y, source.lon, source.lat, mask=mask, Re=Re, threshold=threshold)
    shape = lists["a_poly"].shape
    m = F.cell_mask(mask, shape, "remap: the mask")
    periodic, fold = M.detect_topology(x, y, 2)
    p = params(shape[0], shape[1], source, 0, periodic, fold, fill_max)
    npair = source.nrec * shape[0] * shape[1]
    values = np.empty(npair, dtype=np.float64)
    flags = np.empty((npair + 3) // 4 * 4, dtype=np.uint8)
    counts = L.RemapCounts()
    atm, ocn, area = (np.ascontiguousarray(lists[k]) for k in ("atm", "ocn", "area"))
    L.call("ogg_remap", ctypes.byref(p), source.records.ctypes.data, atm.ctypes.data, ocn.ctypes.data, area.ctypes.data, area.size,
           None if m is None else m.ctypes.data, 1 if fill else 0, values.ctypes.data, flags.ctypes.data, ctypes.byref(counts))
    c = counts_dict(counts)
    rs = (source.nrec,) + shape
    return result(values.reshape(rs), flags[:npair].reshape(rs), c, source, periodic, fold, fill, fill_max, m is not None)


# ---- device arrays ---------------------------------------------------------------------------------------------
def flags_buffer(torch, n, device):
    """n flag bytes in an allocation rounded up to 4 bytes (the fill changes them by 32-bit compare-and-swap)"""
    return torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=device)[:n]


def piece_dev(p, f, atm, ocn, area, mask, stream, device):
    """The segment and remap steps of one piece (device tensors: f (nrec, NB, NA), the piece's list, mask None or its rows' bytes):
    values (nrec, rows, nx) float64, flags (nrec, rows, nx) uint8, counts (int64 device tensor of 8)."""
    import torch
    lib = L.load()
    wsb = int(lib.ogg_remap_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    n = int(area.numel())
    shape = (p.nrec, p.ny, p.nx)
    values = torch.empty(shape, dtype=torch.float64, device=device)
    flags = flags_buffer(torch, p.nrec * p.ny * p.nx, device).view(shape)
    counts = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=device)
    L.call("ogg_remap_segments_dev", ctypes.byref(p), ocn.data_ptr() if n else None, n, ws.data_ptr(), wsb, stream)
    L.call("ogg_remap_dev", ctypes.byref(p), f.data_ptr(), atm.data_ptr() if n else None, area.data_ptr() if n else None, n,
           None if mask is None else mask.data_ptr(), ws.data_ptr(), wsb, values.data_ptr(), flags.data_ptr(), counts.data_ptr(), stream)
    return values, flags, counts


def fill_dev(p, values, flags, counts, stream, device):
    """The fill step on the whole grid's values and flags (device tensors from piece_dev or gathered; flags in an allocation rounded
    up to 4 bytes), in place; counts (int64 device tensor of 8) gets the fill's counts."""
    import torch
    wsb = int(L.load().ogg_remap_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    L.call("ogg_remap_fill_dev", ctypes.byref(p), ws.data_ptr(), wsb, values.data_ptr(), flags.data_ptr(), counts.data_ptr(), stream)


def remap_dev(x, y, source, mask=None, fill=True, fill_max=None, threshold=X.DEFAULT_THRESHOLD, Re=X.DEFAULT_RE):
    """remap() on one GPU with the grid x, y as float64 device tensors ((ny + 1) x (nx + 1), contiguous rows) and a Source or a
    CurvilinearSource: the
    list, the segments, the remap and the fill all on the device, on its current stream.  The same dict as remap(), with host arrays."""
    import torch
    from . import ocean_mask as M
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = F.cell_mask(mask, shape, "remap: the mask")
    periodic, fold = M.topology_of_device_grid(x, y)
    p = params(shape[0], shape[1], source, 0, periodic, fold, fill_max)
    st = torch.cuda.current_stream(dev).cuda_stream
    if isinstance(source, CurvilinearSource):
        from . import exchange_grid_curv as XC
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)   # noqa: E731
        sx, sy, sm, mt = up(source.corner_lon), up(source.corner_lat), up(source.mask), up(m)
        desc = XC.src_desc(sx.data_ptr(), sy.data_ptr(), source.NA, source.NB, mask_ptr=None if sm is None else sm.data_ptr())
        _, _, _, _, atm, ocn, area = XC.band_lists_dev(XC.whole_band(x, y, mt, Re, threshold), desc, st, dev)
    else:
        atm, ocn, area, mt = X.whole_grid_lists_dev(x, y, source.lon, source.lat, m, Re, threshold, st, dev)
    f = torch.from_numpy(source.records).to(dev)
    values, flags, counts = piece_dev(p, f, atm, ocn, area, mt, st, dev)
    if fill:
        fill_dev(p, values, flags, counts, st, dev)
    return result(values.cpu().numpy(), flags.cpu().numpy(), counts_dict(counts.cpu().numpy()), source, periodic, fold, fill, fill_max,
                  m is not None)


# ---- files -----------------------------------------------------------------------------------------------------
def write_remapped(path, results, title="conservative remap onto the model cells"):
    """One float64 variable per remapped field (its source's leading dimensions, then ny, nx; _FillValue FILL) and a byte variable
    <var>_remap_flag (0 dry, 1 remapped, 2 filled, 3 unfilled), the leading coordinate variables copied from the source, as a
    NetCDF 64-bit-offset file.  ``results``: [(Source, remap() result)]."""
    dims, coords, _ = F.writer_dims("remap", [(src, [(src.name, res["values"])]) for src, res in results],
                                    "; remap fewer records at a time")
    ny, nx = results[0][1]["values"].shape[-2:]
    dims += [("ny", ny), ("nx", nx)]
    ds = netcdf3.Dataset(path, dims, global_atts=[("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells"),
                                                  ("flag_values", "0 dry, 1 remapped, 2 filled, 3 unfilled")])
    for name, nc_type, atts, vals in coords:
        ds.def_var(name, nc_type, (name,), atts, vals)
    for src, res in results:
        lead = tuple(d for d, _ in src.lead_dims)
        ds.def_var(src.name, netcdf3.NC_DOUBLE, lead + ("ny", "nx"), list(src.atts) + [("_FillValue", FILL)], res["values"])
        ds.def_var(src.name + "_remap_flag", netcdf3.NC_BYTE, lead + ("ny", "nx"),
                   [("long_name", "remap flag of " + src.name), ("flag_meanings", "dry remapped filled unfilled")],
                   res["flags"].astype(np.int8))
    ds.write()


def summary_lines(res):
    s = res["summary"]
    fill = ("%d filled (largest distance %d, %d fronts in %d launches)" % (s["filled"], s["max_distance"], s["fronts"], s["launches"])
            if s["fill"] else "no fill")
    return ["   remap: %s, %d records of %d x %d source cells onto %d x %d cells%s: %d remapped, %s, %d unfilled, %d dry"
            % (s["var"], s["records"], s["source_shape"][1], s["source_shape"][0], s["shape"][1], s["shape"][0],
               " (masked)" if s["masked"] else "", s["remapped"], fill, s["unfilled"], s["dry"])]


def mask_from_file(path):
    """the wet set of a topog.nc (depth > 0, exchange_grid.mask_from_topog) or of an ocean_mask.nc (mask != 0)"""
    h = netcdf3.read_header(path)
    if "mask" in h.vars and "depth" not in h.vars:
        return (netcdf3.read_doubles(path, names=("mask",))["mask"] != 0).astype(np.uint8)
    return X.mask_from_topog(path)


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.remap",
                                description="conservative remap of lat-lon fields onto the model cells of a supergrid file")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("source", help="the lat-lon source (NetCDF classic / 64-bit offset)")
    p.add_argument("--var", action="append", required=True, help="a variable of the source (repeatable)")
    p.add_argument("--source_grid", default=None,
                   help="the source's own curvilinear grid: a MOM6 supergrid (every second point of x, y), or a file named by "
                        "--source_corners; the source's variables are then fields on that grid's cells")
    p.add_argument("--source_corners", nargs=2, default=None, metavar=("LONVAR", "LATVAR"),
                   help="two 2-D variables of --source_grid that hold the cells' corners")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--no_fill", action="store_true", help="leave wet cells the source does not cover unfilled")
    p.add_argument("--fill_max", type=int, default=None, help="fill at most N cells away from a remapped cell")
    p.add_argument("-o", "--output", default="remapped.nc")
    p.add_argument("--json", default=None, help="write the summaries as JSON to this file")
    a = p.parse_args(argv)
    if a.source_corners and not a.source_grid:
        p.error("--source_corners needs --source_grid")
    grid = netcdf3.read_doubles(a.grid, names=("x", "y"))
    mask = mask_from_file(a.topog or a.mask) if (a.topog or a.mask) else None
    read = (lambda var: read_curvilinear_source(a.source, var, a.source_grid, a.source_corners)) if a.source_grid else \
        (lambda var: read_source(a.source, var))
    return F.run_variables(a.var, read,
                           lambda src: remap(grid["x"], grid["y"], src, mask=mask, fill=not a.no_fill, fill_max=a.fill_max),
                           summary_lines, write_remapped, a.output, a.json)


if __name__ == "__main__":
    main()
    sys.exit(0)

"""Runoff mapping: river runoff and calving on a global lat-lon grid (JRA55-do friver / licalvf, the Dai-Trenberth climatology) moved
to the nearest wet coastal cell of the model grid, conserving the mass flux, and written as a field on the model cells.
include/ogg_hip.h, "Runoff mapping", gives the definition; the reference has no such step.

Every mapped source cell (one that holds a non-missing, non-zero value in some record) goes to the target cell whose centre is
nearest by chordal distance (ties to the smaller cell); a cell's value is the sum of f * A_s over its sources in ascending source
order, over its own area.  The targets, the search, the segments and the sums run on the device (ogg_runoff_*_dev, or the host-pointer
ogg_runoff); nothing is summed across cells in a launch-dependent order, so the result is bit-identical for any launch geometry and
any number of ranks.

    python -m ocean_model_grid_generator_amd.runoff ocean_hgrid.nc SOURCE --var friver [--var licalvf ...]
        (--topog topog.nc | --mask ocean_mask.nc) [--targets coast|wet] -o runoff.nc [--json summary.json]

SOURCE is a NetCDF classic / 64-bit-offset file read as remap.py reads its sources, record (unlimited) variables included.
"""
import argparse
import ctypes
import math
import sys

import numpy as np

from . import _lib as L
from . import exchange_grid as X
from . import fields as F
from . import netcdf3
from . import remap as R

TARGETS = {"coast": L.RUNOFF_COAST, "wet": L.RUNOFF_WET}
Source = R.Source


def read_source(path, var):
    """A remap.Source of the variable ``var`` (remap._read_source), record (unlimited) variables included: its ``record_dim`` is the
    record dimension's name or None."""
    return R._read_source(path, var, records=True)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, source, targets="coast", periodic=False, fold=False, Re=X.DEFAULT_RE):
    """an ogg_runoff_params, checked by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    if targets not in TARGETS:
        raise ValueError("runoff: targets must be one of %s, not %r" % (", ".join(TARGETS), targets))
    p = L.RunoffParams(ny=int(ny), nx=int(nx), NA=source.lon.size - 1, NB=source.lat.size - 1, nrec=source.nrec,
                       dtype=R._DTYPES[source.data.dtype], n_fill=len(source.fill), topology=M.topology_flags(periodic, fold),
                       targets=TARGETS[targets], Re=float(Re))
    for k, f in enumerate(source.fill):
        p.fill[k] = float(f)
    return L.checked("ogg_runoff_check", p)


def _wet(wet, shape):
    return F.wet_mask(wet, shape, "runoff")


def cell_area(area):
    """A_c of every model cell from the supergrid area (2 ny x 2 nx), in the definition's order"""
    a = np.asarray(area, dtype=np.float64)
    return (a[0::2, 0::2] + a[1::2, 1::2]) + (a[0::2, 1::2] + a[1::2, 0::2])


def source_area(source, Re=X.DEFAULT_RE):
    """A_s (NB x NA) as the definition forms it (host sin / cos)"""
    D = np.pi / 180.0
    lon, lat = source.lon, source.lat
    b1, b2 = lat[:-1] * D, lat[1:] * D
    return (Re * Re) * (lon[1:] * D - lon[:-1] * D)[None, :] * (2.0 * np.cos((b1 + b2) / 2.0) * np.sin((b2 - b1) / 2.0))[:, None]


def _check_targets(counts, targets):
    if counts["mapped"] > 0 and counts["targets"] == 0:
        raise ValueError("runoff: no target cell (%s) while %d source cells hold runoff"
                         % ("no wet cell on a coast" if targets == "coast" else "no wet cell", counts["mapped"]))


def result(values, n_sources, src_cell, src_target, src_d2, counts, source, area, targets, periodic, fold, Re, lists=None):
    """What runoff() returns: values (lead dims of the source, ny, nx), n_sources (ny, nx), the mapped sources (cell, target, d2), the
    counts and a summary (conservation per record: sum_c value A_c against sum_s f A_s, math.fsum)."""
    ny, nx = n_sources.shape
    shape = tuple(source.data.shape[:-2]) + (ny, nx)
    Ac = cell_area(area).reshape(-1)
    As = source_area(source, Re).reshape(-1)
    recs = source.records.reshape(source.nrec, -1)
    vals = values.reshape(source.nrec, -1)
    rel = []
    for r in range(source.nrec):
        f = recs[r].astype(np.float64)
        ok = ~np.isnan(f)
        for fv in source.fill:
            ok &= recs[r] != fv
        want = math.fsum(f[ok] * As[ok])
        got = math.fsum(vals[r] * Ac)
        rel.append(0.0 if want == got else abs(got - want) / max(abs(want), abs(got)))
    summary = dict(counts, var=source.name, records=source.nrec, source_shape=[source.lat.size - 1, source.lon.size - 1],
                   shape=[ny, nx], targets_mode=targets, periodic=bool(periodic), fold=bool(fold), conservation=rel,
                   max_km=0.0, max_from=None)
    if src_d2.size:
        k = int(np.argmax(src_d2))
        J, I = divmod(int(src_cell[k]), source.lon.size - 1)
        summary["max_km"] = float(2.0 * np.arcsin(min(1.0, math.sqrt(src_d2[k]) / 2.0)) * Re / 1000.0)
        summary["max_from"] = [I, J, float(0.5 * (source.lon[I] + source.lon[I + 1])), float(0.5 * (source.lat[J] + source.lat[J + 1])),
                               int(src_target[k])]
    out = {"values": values.reshape(shape), "n_sources": n_sources, "src_cell": src_cell, "src_target": src_target, "src_d2": src_d2,
           "counts": counts, "summary": summary, "area": cell_area(area)}
    if lists is not None:
        out.update(lists)
    return out


# ---- host arrays -----------------------------------------------------------------------------------------------
def runoff(x, y, area, source, wet, targets="coast", lon_edges=None, lat_edges=None, fill_values=(), Re=X.DEFAULT_RE):
    """The runoff of ``source`` mapped onto the model cells of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny even)
    with its area (ny x nx supergrid cells), on one GPU through the host-pointer entry ogg_runoff.  ``source``: a Source, or an array
    (..., NB, NA) with lon_edges, lat_edges and fill_values.  wet: one value per model cell (0: land).  targets: "coast" or "wet".
    A dict: values (the source's leading dimensions, then (ny / 2, nx / 2)), n_sources, src_cell / src_target / src_d2 of the
    mapped sources, counts, summary, area (A_c)."""
    from . import ocean_mask as M
    if not isinstance(source, Source):
        source = Source(source, lon_edges, lat_edges, fill=fill_values)
    x, y = L.as_f64(x), L.as_f64(y)
    area = np.ascontiguousarray(area, dtype=np.float64)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    if area.shape != (nyp - 1, nxp - 1):
        raise ValueError("runoff: area %s for a supergrid of %s points" % (area.shape, x.shape))
    m = _wet(wet, shape)
    periodic, fold = M.detect_topology(x, y, 2)
    p = params(shape[0], shape[1], source, targets, periodic, fold, Re)
    ns = (source.lon.size - 1) * (source.lat.size - 1)
    values = np.empty((source.nrec,) + shape, dtype=np.float64)
    nsrc = np.empty(shape, dtype=np.int32)
    sc, st, sd = np.empty(ns, np.int32), np.empty(ns, np.int32), np.empty(ns, np.float64)
    c = L.RunoffCounts()
    lib = L.load()
    rc = lib.ogg_runoff(ctypes.byref(p), x.ctypes.data, y.ctypes.data, area.ctypes.data, m.ctypes.data, source.records.ctypes.data,
                        source.lon.ctypes.data, source.lat.ctypes.data, values.ctypes.data, nsrc.ctypes.data, sc.ctypes.data, st.ctypes.data,
                        sd.ctypes.data, ctypes.byref(c))
    counts = L.counts_dict(L.RUNOFF_COUNT_FIELDS, c)
    if rc != L.OGG_OK:
        _check_targets(counts, targets)
        raise L.OggHipError(rc, lib.ogg_last_error().decode())
    n = counts["mapped"]
    return result(values, nsrc, sc[:n], st[:n], sd[:n], counts, source, area, targets, periodic, fold, Re)


# ---- device arrays ---------------------------------------------------------------------------------------------
def runoff_dev(x, y, area, source, wet, targets="coast", Re=X.DEFAULT_RE, keep_lists=False):
    """runoff() on one GPU with the grid x, y ((ny + 1) x (nx + 1)) and area (ny x nx) as float64 device tensors and a Source: the
    five steps on the device, on its current stream, with one read of the counts between the sources and the search step.  The same
    dict as runoff(), with host arrays; with ``keep_lists`` also the target list (tgt_cell, tgt_u), the mapped list's unit vectors
    (src_u) and ds_J (ds) as the device computed them."""
    import torch
    from . import ocean_mask as M
    dev = x.device
    x, y, area = x.contiguous(), y.contiguous(), area.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    if tuple(area.shape) != (nyp - 1, nxp - 1):
        raise ValueError("runoff: area %s for a supergrid of %s points" % (tuple(area.shape), tuple(x.shape)))
    m = _wet(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, shape)
    periodic, fold = M.topology_of_device_grid(x, y)
    p = params(shape[0], shape[1], source, targets, periodic, fold, Re)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = L.load()
    wsb = int(lib.ogg_runoff_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nc, ns = shape[0] * shape[1], (source.lon.size - 1) * (source.lat.size - 1)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    wt, f, lon, lat = to(m), to(source.records), to(source.lon), to(source.lat)
    tc = torch.empty(nc, dtype=torch.int32, device=dev)
    tu = torch.empty((nc, 3), dtype=torch.float64, device=dev)
    sc = torch.empty(ns, dtype=torch.int32, device=dev)
    su = torch.empty((ns, 3), dtype=torch.float64, device=dev)
    ds = torch.empty(source.lat.size - 1, dtype=torch.float64, device=dev)
    sdst = torch.empty(ns, dtype=torch.int32, device=dev)
    sd2 = torch.empty(ns, dtype=torch.float64, device=dev)
    values = torch.empty((source.nrec,) + shape, dtype=torch.float64, device=dev)
    nsrc = torch.empty(shape, dtype=torch.int32, device=dev)
    counts = torch.zeros(len(L.RUNOFF_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_runoff_targets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), nxp, wt.data_ptr(), ws.data_ptr(), wsb, tc.data_ptr(),
           tu.data_ptr(), counts.data_ptr(), st)
    L.call("ogg_runoff_sources_dev", ctypes.byref(p), f.data_ptr(), lon.data_ptr(), lat.data_ptr(), ws.data_ptr(), wsb, sc.data_ptr(),
           su.data_ptr(), ds.data_ptr(), counts.data_ptr(), st)
    c = counts.cpu().numpy()
    nt, nm = int(c[0]), int(c[1])
    _check_targets({"targets": nt, "mapped": nm}, targets)
    L.call("ogg_runoff_search_dev", ctypes.byref(p), tc.data_ptr(), tu.data_ptr(), nt, su.data_ptr(), nm, ws.data_ptr(), wsb,
           sdst.data_ptr(), sd2.data_ptr(), counts.data_ptr(), st)
    L.call("ogg_runoff_segments_dev", ctypes.byref(p), sdst.data_ptr(), nm, ws.data_ptr(), wsb, st)
    L.call("ogg_runoff_accumulate_dev", ctypes.byref(p), f.data_ptr(), sc.data_ptr(), nm, area.data_ptr(), nxp - 1, ws.data_ptr(), wsb,
           values.data_ptr(), nsrc.data_ptr(), counts.data_ptr(), st)
    cd = L.counts_dict(L.RUNOFF_COUNT_FIELDS, counts)
    lists = None
    if keep_lists:
        lists = {"tgt_cell": tc[:nt].cpu().numpy(), "tgt_u": tu[:nt].cpu().numpy(), "src_u": su[:nm].cpu().numpy(), "ds": ds.cpu().numpy()}
    return result(values.cpu().numpy(), nsrc.cpu().numpy(), sc[:nm].cpu().numpy(), sdst[:nm].cpu().numpy(), sd2[:nm].cpu().numpy(), cd,
                  source, area.cpu().numpy(), targets, periodic, fold, Re, lists)


# ---- files -----------------------------------------------------------------------------------------------------
def write_runoff(path, results, title="runoff mapped onto the nearest coastal model cells"):
    """One float64 variable per mapped field (its source's leading dimensions, then ny, nx; units copied), the leading coordinate
    variables copied from the source (the first leading dimension written as the record dimension when the source's was), the cell
    area (m2) and n_sources (int, the number of source cells mapped to each cell), as a NetCDF 64-bit-offset file.  ``results``:
    [(Source, runoff() result)]."""
    dims, coords, record_dim = F.writer_dims("runoff", [(src, [(src.name, res["values"])]) for src, res in results], record_dims=True)
    ny, nx = results[0][1]["n_sources"].shape
    dims += [("ny", ny), ("nx", nx)]
    ds = netcdf3.Dataset(path, dims, global_atts=[("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells")],
                         record_dim=record_dim)
    for name, nc_type, atts, vals in coords:
        ds.def_var(name, nc_type, (name,), atts, vals)
    for src, res in results:
        lead = tuple(d for d, _ in src.lead_dims)
        ds.def_var(src.name, netcdf3.NC_DOUBLE, lead + ("ny", "nx"), list(src.atts), res["values"])
    ds.def_var("area", netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", "m2"), ("long_name", "model cell area")], results[0][1]["area"])
    ds.def_var("n_sources", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "source cells mapped to the cell")],
               results[0][1]["n_sources"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    out = ["   runoff: %s, %d records of %d x %d source cells onto %d x %d cells: %d %s targets; %d source cells mapped, %d skipped "
           "(zero), %d missing; %d cells receive runoff, at most %d sources in one"
           % (s["var"], s["records"], s["source_shape"][1], s["source_shape"][0], s["shape"][1], s["shape"][0], s["targets"],
              s["targets_mode"], s["mapped"], s["skipped"], s["missing"], s["cells"], s["max_sources"])]
    if s["max_from"] is not None:
        I, J, lo, la, c = s["max_from"]
        out.append("   runoff: largest move %.1f km, from source cell (%d, %d) at (%.3f, %.3f) to cell (%d, %d)"
                   % (s["max_km"], I, J, lo, la, c % s["shape"][1], c // s["shape"][1]))
    out.append("   runoff: conservation (relative difference per record): max %.3g" % max(s["conservation"] or [0.0]))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.runoff",
                                description="lat-lon runoff moved to the nearest coastal cells of a supergrid file")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("source", help="the lat-lon runoff (NetCDF classic / 64-bit offset)")
    p.add_argument("--var", action="append", required=True, help="a variable of the source (repeatable)")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--targets", choices=sorted(TARGETS), default="coast", help="coast (default): wet cells next to land; wet: every wet cell")
    p.add_argument("-o", "--output", default="runoff.nc")
    p.add_argument("--json", default=None, help="write the summaries as JSON to this file")
    a = p.parse_args(argv)
    grid = netcdf3.read_doubles(a.grid, names=("x", "y", "area"))
    wet = R.mask_from_file(a.topog or a.mask)
    return F.run_variables(a.var, lambda var: read_source(a.source, var),
                           lambda src: runoff(grid["x"], grid["y"], grid["area"], src, wet, targets=a.targets),
                           summary_lines, write_runoff, a.output, a.json)


if __name__ == "__main__":
    main()
    sys.exit(0)

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

        [--spread_km R [--spread_shape biweight|uniform] [--spread_classes basin_codes.nc [VAR]]]

SOURCE is a NetCDF classic / 64-bit-offset file read as remap.py reads its sources, record (unlimited) variables included.

Runoff spreading (include/ogg_hip.h, "Runoff spreading"): with a radius, the mapped runoff of every loaded cell is spread over the wet
cells within that distance by integer weights (a biweight of the chordal distance, or uniform, times the area ratio capped at 256),
within the cell's class when classes (basin codes) are given, and summed per receiving cell in ascending mouth order: spread() /
spread_dev() alone, or ``spread_km`` of runoff() / runoff_dev() / Supergrid.runoff().  The same bits for any index, launch and rank
count.
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


# ---- spreading -------------------------------------------------------------------------------------------------
SHAPES = {"uniform": L.SPREAD_UNIFORM, "biweight": L.SPREAD_BIWEIGHT}
DEFAULT_SPREAD_KM = 300.0


def radius2(radius_km, Re=X.DEFAULT_RE):
    """r2 of the definition, formed once: the squared chord of the radius (the whole sphere from half the circumference on)"""
    if not (isinstance(radius_km, (int, float, np.integer, np.floating)) and math.isfinite(radius_km) and radius_km > 0):
        raise ValueError("spread: the radius must be a positive number of km, not %r" % (radius_km,))
    half = 0.5 * (float(radius_km) * 1e3 / float(Re))
    if half >= 0.5 * math.pi:
        return 4.0
    s = math.sin(half)
    return (2 * s) * (2 * s)


def spread_params(ny, nx, nrec, r2, shape="biweight", classes=False):
    """an ogg_spread_params, checked by the library (OGG_EARG -> ValueError)"""
    if shape not in SHAPES:
        raise ValueError("spread: shape must be one of %s, not %r" % (", ".join(sorted(SHAPES)), shape))
    p = L.SpreadParams(ny=int(ny), nx=int(nx), nrec=int(nrec), shape=SHAPES[shape], use_classes=1 if classes else 0, r2=float(r2))
    return L.checked("ogg_spread_check", p)


def default_load(values):
    """load of spread() when none is given: 1 where some record is neither 0 nor NaN"""
    v = np.asarray(values)
    v = v.reshape((-1,) + v.shape[-2:])
    return ((v != 0) & ~np.isnan(v)).any(axis=0).astype(np.int32)


def _spread_inputs(values, shape, load, classes):
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.shape[-2:] != shape:
        raise ValueError("spread: values %s for %s model cells" % (v.shape, shape))
    ld = default_load(v) if load is None else np.ascontiguousarray(load, dtype=np.int32)
    if ld.shape != shape:
        raise ValueError("spread: load %s for %s model cells" % (ld.shape, shape))
    cl = None
    if classes is not None:
        cl = np.ascontiguousarray(classes, dtype=np.int32)
        if cl.shape != shape:
            raise ValueError("spread: classes %s for %s model cells" % (cl.shape, shape))
    return v, ld, cl


def spread_result(values_in, out, n_mouths, mouth_cell, mouth_n, mouth_W, counts, area, radius_km, shape, classes, lists=None):
    """What spread() returns: values (the shape of the input), n_mouths (ny, nx), the mouths (mouth_cell, mouth_n = |R(m)|,
    mouth_W = W_m), counts and a summary: per record the largest value before and after, and the conservation defect
    |fsum(out A) - fsum(v A)| relative to fsum(|v| A) over the mouths."""
    A = cell_area(area).reshape(-1)
    vin = values_in.reshape(-1, A.size)
    vout = out.reshape(-1, A.size)
    before, after, defect = [], [], []
    for r in range(vin.shape[0]):
        f = vin[r][mouth_cell] * A[mouth_cell]
        tot = math.fsum(np.abs(f))
        with np.errstate(invalid="ignore"):   # (a cell that is no candidate may have an area that is not finite: 0 * inf)
            d = abs(math.fsum(vout[r] * A) - math.fsum(f))
        defect.append(0.0 if d == 0.0 else (d / tot if tot > 0 and math.isfinite(d) else float("nan")))
        before.append(float(np.max(vin[r][mouth_cell], initial=0.0)))
        after.append(float(np.max(vout[r], initial=0.0)))
    summary = dict(counts, km=float(radius_km), shape=shape, classes=bool(classes), max_before=before, max_after=after, conservation=defect)
    res = {"values": out.reshape(values_in.shape), "n_mouths": n_mouths, "mouth_cell": mouth_cell, "mouth_n": mouth_n, "mouth_W": mouth_W,
           "counts": counts, "summary": summary}
    if lists is not None:
        res.update(lists)
    return res


def spread(values, x, y, area, wet, load=None, radius_km=DEFAULT_SPREAD_KM, shape="biweight", classes=None, Re=X.DEFAULT_RE):
    """``values`` (..., ny / 2, nx / 2) on the model cells of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees) with its area
    (ny x nx), spread from the cells with load > 0 (default: some record neither 0 nor NaN) over the wet cells within ``radius_km``
    (and of the same class when ``classes``, one integer per cell, is given), on one GPU through the host-pointer entry
    ogg_runoff_spread.  A dict: values, n_mouths, mouth_cell / mouth_n / mouth_W, counts, summary."""
    x, y = L.as_f64(x), L.as_f64(y)
    area = np.ascontiguousarray(area, dtype=np.float64)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    cells = ((nyp - 1) // 2, (nxp - 1) // 2)
    if area.shape != (nyp - 1, nxp - 1):
        raise ValueError("spread: area %s for a supergrid of %s points" % (area.shape, x.shape))
    v, ld, cl = _spread_inputs(values, cells, load, classes)
    m = F.wet_mask(wet, cells, "spread")
    nc = cells[0] * cells[1]
    p = spread_params(cells[0], cells[1], v.size // nc, radius2(radius_km, Re), shape, cl is not None)
    out = np.empty_like(v)
    nm = np.empty(cells, dtype=np.int32)
    mc, mn, mW = np.empty(nc, np.int32), np.empty(nc, np.int32), np.empty(nc, np.int64)
    c = L.SpreadCounts()
    L.call("ogg_runoff_spread", ctypes.byref(p), x.ctypes.data, y.ctypes.data, area.ctypes.data, m.ctypes.data,
           None if cl is None else cl.ctypes.data, ld.ctypes.data, v.ctypes.data, out.ctypes.data, nm.ctypes.data, mc.ctypes.data,
           mn.ctypes.data, mW.ctypes.data, ctypes.byref(c))
    counts = L.counts_dict(L.SPREAD_COUNT_FIELDS, c)
    n = counts["mouths"]
    return spread_result(v, out, nm, mc[:n], mn[:n], mW[:n], counts, area, radius_km, shape, cl is not None)


def spread_dev(values, x, y, area, wet, load=None, radius_km=DEFAULT_SPREAD_KM, shape="biweight", classes=None, Re=X.DEFAULT_RE,
               keep_lists=False):
    """spread() on one GPU with the grid x, y and area as float64 device tensors (``values``, ``wet``, ``load`` and ``classes``: host
    arrays or device tensors): the four steps on the device, on its current stream, with one read of the counts after the sets step
    and one after the count step.  The same dict as spread(), with host arrays; with ``keep_lists`` also u (ny nx x 3), A and the
    candidate flags (cand) as the device computed them."""
    import torch
    dev = x.device
    x, y, area = x.contiguous(), y.contiguous(), area.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    cells = ((nyp - 1) // 2, (nxp - 1) // 2)
    if tuple(area.shape) != (nyp - 1, nxp - 1):
        raise ValueError("spread: area %s for a supergrid of %s points" % (tuple(area.shape), tuple(x.shape)))
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a   # noqa: E731
    v, ld, cl = _spread_inputs(host(values), cells, None if load is None else host(load), None if classes is None else host(classes))
    m = F.wet_mask(host(wet), cells, "spread")
    nc = cells[0] * cells[1]
    p = spread_params(cells[0], cells[1], v.size // nc, radius2(radius_km, Re), shape, cl is not None)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = L.load()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    wt, lt, vt = to(m), to(ld), to(v)
    ct = None if cl is None else to(cl)
    cp = None if ct is None else ct.data_ptr()
    wsb0 = int(lib.ogg_spread_workspace_bytes(ctypes.byref(p), 0))
    ws0 = torch.empty(wsb0, dtype=torch.uint8, device=dev)
    u = torch.empty((nc, 3), dtype=torch.float64, device=dev)
    A = torch.empty(nc, dtype=torch.float64, device=dev)
    cand = torch.empty(nc, dtype=torch.uint8, device=dev)
    mc = torch.empty(nc, dtype=torch.int32, device=dev)
    counts = torch.zeros(len(L.SPREAD_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_spread_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), nxp, area.data_ptr(), nxp - 1, wt.data_ptr(), lt.data_ptr(),
           ws0.data_ptr(), wsb0, u.data_ptr(), A.data_ptr(), cand.data_ptr(), mc.data_ptr(), counts.data_ptr(), st)
    n = int(counts.cpu().numpy()[1])
    mn = torch.empty(n, dtype=torch.int32, device=dev)
    mW = torch.empty(n, dtype=torch.int64, device=dev)
    L.call("ogg_spread_count_dev", ctypes.byref(p), u.data_ptr(), A.data_ptr(), cp, mc.data_ptr(), n, ws0.data_ptr(), wsb0, mn.data_ptr(),
           mW.data_ptr(), counts.data_ptr(), st)
    P = int(counts.cpu().numpy()[2])
    wsb = int(lib.ogg_spread_workspace_bytes(ctypes.byref(p), P))   # refused before the keys are allocated
    if wsb < 0:
        raise L.OggHipError(L.OGG_EARG, "libogg_hip: %s" % lib.ogg_last_error().decode())
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ws[:wsb0].copy_(ws0)   # the smaller workspace is a prefix of the larger
    del ws0
    out = torch.empty(v.shape, dtype=torch.float64, device=dev)
    nm = torch.empty(cells, dtype=torch.int32, device=dev)
    L.call("ogg_spread_pairs_dev", ctypes.byref(p), u.data_ptr(), cp, mc.data_ptr(), mn.data_ptr(), n, P, ws.data_ptr(), wsb, st)
    L.call("ogg_spread_apply_dev", ctypes.byref(p), vt.data_ptr(), u.data_ptr(), A.data_ptr(), mc.data_ptr(), mW.data_ptr(), n, P,
           ws.data_ptr(), wsb, out.data_ptr(), nm.data_ptr(), counts.data_ptr(), st)
    cd = L.counts_dict(L.SPREAD_COUNT_FIELDS, counts)
    lists = None
    if keep_lists:
        lists = {"u": u.cpu().numpy(), "A": A.cpu().numpy(), "cand": cand.cpu().numpy()}
    return spread_result(v, out.cpu().numpy(), nm.cpu().numpy(), mc[:n].cpu().numpy(), mn.cpu().numpy(), mW.cpu().numpy(), cd,
                         area.cpu().numpy(), radius_km, shape, cl is not None, lists)


def with_spread(res, sp, keep_lists=True):
    """a runoff() result with the spreading ``sp`` of its values put in: values the spread ones, values_mapped those before, n_mouths,
    spread_counts, the summary's "spread" and, with ``keep_lists``, the mouths"""
    res["values_mapped"] = res["values"]
    res["values"] = sp["values"]
    res["n_mouths"] = sp["n_mouths"]
    res["spread_counts"] = sp["counts"]
    res["summary"]["spread"] = sp["summary"]
    if keep_lists:
        for k in ("mouth_cell", "mouth_n", "mouth_W"):
            res[k] = sp[k]
    return res


# ---- host arrays -----------------------------------------------------------------------------------------------
def runoff(x, y, area, source, wet, targets="coast", lon_edges=None, lat_edges=None, fill_values=(), Re=X.DEFAULT_RE, spread_km=None,
           spread_shape="biweight", spread_classes=None):
    """The runoff of ``source`` mapped onto the model cells of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; nx, ny even)
    with its area (ny x nx supergrid cells), on one GPU through the host-pointer entry ogg_runoff.  ``source``: a Source, or an array
    (..., NB, NA) with lon_edges, lat_edges and fill_values.  wet: one value per model cell (0: land).  targets: "coast" or "wet".
    A dict: values (the source's leading dimensions, then (ny / 2, nx / 2)), n_sources, src_cell / src_target / src_d2 of the
    mapped sources, counts, summary, area (A_c).  With ``spread_km`` the mapped values are spread (spread(), load = n_sources): values
    are the spread ones, values_mapped those before, and n_mouths, spread_counts, mouth_cell / mouth_n / mouth_W are added."""
    from . import ocean_mask as M
    if spread_km is not None:
        radius2(spread_km, Re)   # refused before any device work
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
    res = result(values, nsrc, sc[:n], st[:n], sd[:n], counts, source, area, targets, periodic, fold, Re)
    if spread_km is None:
        return res
    return with_spread(res, spread(res["values"], x, y, area, m, load=nsrc, radius_km=spread_km, shape=spread_shape,
                                   classes=spread_classes, Re=Re))


# ---- device arrays ---------------------------------------------------------------------------------------------
def runoff_dev(x, y, area, source, wet, targets="coast", Re=X.DEFAULT_RE, keep_lists=False, spread_km=None, spread_shape="biweight",
               spread_classes=None):
    """runoff() on one GPU with the grid x, y ((ny + 1) x (nx + 1)) and area (ny x nx) as float64 device tensors and a Source: the
    five steps on the device, on its current stream, with one read of the counts between the sources and the search step.  The same
    dict as runoff(), with host arrays; with ``keep_lists`` also the target list (tgt_cell, tgt_u), the mapped list's unit vectors
    (src_u) and ds_J (ds) as the device computed them.  ``spread_km``: as for runoff(), through spread_dev(); the mouths with
    ``keep_lists``."""
    import torch
    from . import ocean_mask as M
    if spread_km is not None:
        radius2(spread_km, Re)   # refused before any device work
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
    res = result(values.cpu().numpy(), nsrc.cpu().numpy(), sc[:nm].cpu().numpy(), sdst[:nm].cpu().numpy(), sd2[:nm].cpu().numpy(), cd,
                 source, area.cpu().numpy(), targets, periodic, fold, Re, lists)
    if spread_km is None:
        return res
    return with_spread(res, spread_dev(res["values"], x, y, area, m, load=res["n_sources"], radius_km=spread_km, shape=spread_shape,
                                       classes=spread_classes, Re=Re), keep_lists)


# ---- files -----------------------------------------------------------------------------------------------------
def write_runoff(path, results, title="runoff mapped onto the nearest coastal model cells", spread_classes="none"):
    """One float64 variable per mapped field (its source's leading dimensions, then ny, nx; units copied), the leading coordinate
    variables copied from the source (the first leading dimension written as the record dimension when the source's was), the cell
    area (m2) and n_sources (int, the number of source cells mapped to each cell), as a NetCDF 64-bit-offset file.  ``results``:
    [(Source, runoff() result)].  Results with spread values: those are written, with n_mouths (int, the mouths that reach each cell; of
    the first result, like n_sources) and the global attributes spread_km, spread_shape and spread_classes (``spread_classes``: the
    name of the class variable, "none" without classes)."""
    dims, coords, record_dim = F.writer_dims("runoff", [(src, [(src.name, res["values"])]) for src, res in results], record_dims=True)
    ny, nx = results[0][1]["n_sources"].shape
    dims += [("ny", ny), ("nx", nx)]
    gatts = [("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells")]
    sp = results[0][1].get("summary", {}).get("spread") if "n_mouths" in results[0][1] else None
    if sp is not None:
        gatts += [("spread_km", float(sp["km"])), ("spread_shape", sp["shape"]), ("spread_classes", str(spread_classes) if sp["classes"] else "none")]
    ds = netcdf3.Dataset(path, dims, global_atts=gatts, record_dim=record_dim)
    for name, nc_type, atts, vals in coords:
        ds.def_var(name, nc_type, (name,), atts, vals)
    for src, res in results:
        lead = tuple(d for d, _ in src.lead_dims)
        ds.def_var(src.name, netcdf3.NC_DOUBLE, lead + ("ny", "nx"), list(src.atts), res["values"])
    ds.def_var("area", netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", "m2"), ("long_name", "model cell area")], results[0][1]["area"])
    ds.def_var("n_sources", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "source cells mapped to the cell")],
               results[0][1]["n_sources"])
    if sp is not None:
        ds.def_var("n_mouths", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "mouth cells whose spread runoff reaches the cell")],
                   results[0][1]["n_mouths"])
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
    sp = s.get("spread")
    if sp is not None:
        out.append("   runoff: %s spread over %g km (%s%s): %d mouths, %d mouth-receiver pairs, at most %d receivers of one mouth; %d cells "
                   "receive, at most %d mouths in one" % (s["var"], sp["km"], sp["shape"], ", within classes" if sp["classes"] else "",
                                                          sp["mouths"], sp["pairs"], sp["max_receivers"], sp["loaded"], sp["max_mouths"]))
        out.append("   runoff: largest flux per area %.6g before, %.6g after spreading; conservation defect relative to sum |v| A: max %.3g"
                   % (max(sp["max_before"] or [0.0]), max(sp["max_after"] or [0.0]), max(sp["conservation"] or [0.0])))
    return out


def check_spread_flags(km, shape, classes, km_flag, shape_flag, classes_flag):
    """the refusals of the spread flags of either command line, before anything is read"""
    if km is None:
        if shape is not None or classes:
            raise ValueError("%s and %s need %s" % (shape_flag, classes_flag, km_flag))
        return
    if not (math.isfinite(km) and km > 0):
        raise ValueError("%s must be a positive number of km, not %r" % (km_flag, km))
    if shape is not None and shape not in SHAPES:
        raise ValueError("%s must be biweight or uniform, not %r" % (shape_flag, shape))
    if classes is not None and not isinstance(classes, bool) and not 1 <= len(classes) <= 2:
        raise ValueError("%s takes a file and at most one variable name" % classes_flag)


def read_classes(path, var="basin"):
    """the integer variable ``var`` (ny, nx) of a NetCDF classic / 64-bit-offset file (basin_codes.nc) as int32 classes"""
    h = netcdf3.read_header(path)
    if var not in h.vars:
        raise ValueError("%s: no variable %r" % (path, var))
    v = h.vars[var]
    if v.nc_type not in (netcdf3.NC_BYTE, netcdf3.NC_SHORT, netcdf3.NC_INT) or len(v.shape) != 2:
        raise ValueError("%s: %r must be an integer variable on (ny, nx)" % (path, var))
    dt = {netcdf3.NC_BYTE: ">i1", netcdf3.NC_SHORT: ">i2", netcdf3.NC_INT: ">i4"}[v.nc_type]
    return np.frombuffer(netcdf3.read_var_bytes(path, h, var, dtype=v.nc_type), dtype=dt).astype(np.int32).reshape(v.shape)


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
    p.add_argument("--spread_km", type=float, default=None, help="spread the mapped runoff over the wet cells within this many km")
    p.add_argument("--spread_shape", choices=sorted(SHAPES), default=None, help="biweight (default) or uniform weights")
    p.add_argument("--spread_classes", nargs="+", default=None, metavar=("FILE", "VAR"),
                   help="basin_codes.nc [VAR, default basin]: the runoff stays within the class of its mouth")
    p.add_argument("-o", "--output", default="runoff.nc")
    p.add_argument("--json", default=None, help="write the summaries as JSON to this file")
    a = p.parse_args(argv)
    check_spread_flags(a.spread_km, a.spread_shape, a.spread_classes, "--spread_km", "--spread_shape", "--spread_classes")
    grid = netcdf3.read_doubles(a.grid, names=("x", "y", "area"))
    wet = R.mask_from_file(a.topog or a.mask)
    classes, cname = None, "none"
    if a.spread_classes:
        cname = a.spread_classes[1] if len(a.spread_classes) > 1 else "basin"
        classes = read_classes(a.spread_classes[0], cname)
    return F.run_variables(a.var, lambda var: read_source(a.source, var),
                           lambda src: runoff(grid["x"], grid["y"], grid["area"], src, wet, targets=a.targets, spread_km=a.spread_km,
                                              spread_shape=a.spread_shape or "biweight", spread_classes=classes),
                           summary_lines, lambda path, out: write_runoff(path, out, spread_classes=cname), a.output, a.json)


if __name__ == "__main__":
    main()
    sys.exit(0)

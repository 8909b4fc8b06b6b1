"""Point location and sampling: for a list of (longitude, latitude) points the model cell that holds each, where in the cell it lies
(s, t in 0 .. 1) and the value of model fields there, for moorings, tide gauges, profiles, section end points, mask and basin seeds and
river mouths.  include/ogg_hip.h, "Point location", gives the definition; the reference has no such step.

A cell's edges are great circles between its corners' unit vectors; the cell of a point is the one with the largest key m = the
smallest of the four signed edge measures, among the cells whose padded box holds the point and whose m >= -2^-50.  There is no walk
over the grid: the device registers every cell in a grid of cubes and tests, for each query, every cell of its cube (ogg_locate_sets_dev,
ogg_locate_index_dev, ogg_locate_search_dev, or the host-pointer ogg_locate), which is the brute-force answer on any mesh.  Sampling
(ogg_locate_sample_dev / ogg_locate_sample) takes the cell's value or an index-space bilinear mean of the four nearest centres.

    python -m ocean_model_grid_generator_amd.locate ocean_hgrid.nc POINTS [--fields F.nc --var V]... [--topog topog.nc | --mask
        ocean_mask.nc] [--mode bilinear|cell] -o points.nc [--json summary.json]

POINTS: a text file, ``lon lat [name]`` per line (``#`` starts a comment), or a NetCDF classic / 64-bit-offset file with 1-D lon and lat.
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import exchange_grid as X
from . import fields as F
from . import netcdf3

MODES = L.LOCATE_MODES
FILL = L.REMAP_FILL
Field = F.Field   # a field on the model cells: data (..., ny, nx)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, n, periodic=False, fold=False, mode="bilinear", nrec=0, dtype=np.float64, fill_values=()):
    """an ogg_locate_params, checked by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    if mode not in MODES:
        raise ValueError("locate: mode must be one of %s, not %r" % (", ".join(sorted(MODES)), mode))
    if np.dtype(dtype) not in F.DTYPES:
        raise ValueError("locate: a float32 or float64 field is needed, not %s" % np.dtype(dtype))
    fills = [float(f) for f in fill_values]
    if len(fills) > L.REMAP_MAX_FILLS:
        raise ValueError("locate: at most %d fill values" % L.REMAP_MAX_FILLS)
    p = L.LocateParams(ny=int(ny), nx=int(nx), n=int(n), nrec=int(nrec), topology=M.topology_flags(periodic, fold), mode=MODES[mode],
                       dtype=F.DTYPES[np.dtype(dtype)], n_fill=len(fills))
    for k, f in enumerate(fills):
        p.fill[k] = f
    return L.checked("ogg_locate_check", p)


def _points(lon, lat):
    lon, lat = L.as_f64(lon).reshape(-1), L.as_f64(lat).reshape(-1)
    if lon.shape != lat.shape:
        raise ValueError("locate: %d longitudes and %d latitudes" % (lon.size, lat.size))
    return lon, lat


def result(cell, s, t, m, counts, lon, lat, shape, periodic, fold, names=None, cu=None, qu=None):
    """What locate() returns, per point: cell (int32, -1 where none), cell_j, cell_i, s, t, margin (the key m), lon, lat; the counts
    and a summary"""
    nx = shape[1]
    has = cell >= 0
    out = {"lon": lon, "lat": lat, "cell": cell, "cell_j": np.where(has, cell // nx, -1).astype(np.int32),
           "cell_i": np.where(has, cell % nx, -1).astype(np.int32), "s": s, "t": t, "margin": m, "counts": counts, "shape": tuple(shape),
           "periodic": bool(periodic), "fold": bool(fold), "names": list(names) if names is not None else None, "samples": []}
    out["summary"] = dict(counts, shape=list(shape), points=int(cell.size), periodic=bool(periodic), fold=bool(fold),
                          tests_per_query=(counts["tests"] / cell.size) if cell.size else 0.0)
    if cu is not None:
        out["cu"], out["qu"] = cu, qu
    return out


# ---- host arrays -----------------------------------------------------------------------------------------------
def locate(x, y, lon, lat, periodic=None, fold=None, names=None, keep_vectors=False):
    """The model cells of a stitched supergrid x, y ((2 ny + 1) x (2 nx + 1), degrees) that hold the points lon, lat (degrees), on one
    GPU through the host-pointer entry ogg_locate.  periodic, fold: None to read them from the grid (ocean_mask.detect_topology).  A
    dict: see result(); with ``keep_vectors`` also the corner table cu and the query vectors qu as the device formed them."""
    from . import ocean_mask as M
    x, y = L.as_f64(x), L.as_f64(y)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    lon, lat = _points(lon, lat)
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.detect_topology(x, y, 2))
    n = lon.size
    p = params(shape[0], shape[1], n, periodic, fold)
    cell = np.empty(n, np.int32)
    s, t, m = (np.empty(n, np.float64) for _ in range(3))
    cu = np.empty(((shape[0] + 1) * (shape[1] + 1), 3)) if keep_vectors else None
    qu = np.empty((n, 3)) if keep_vectors else None
    c = L.LocateCounts()
    L.call("ogg_locate", ctypes.byref(p), x.ctypes.data, y.ctypes.data, lon.ctypes.data, lat.ctypes.data, cell.ctypes.data, s.ctypes.data,
           t.ctypes.data, m.ctypes.data, L.ptr(cu), L.ptr(qu), ctypes.byref(c))
    return result(cell, s, t, m, L.counts_dict(L.LOCATE_COUNT_FIELDS, c), lon, lat, shape, periodic, fold, names, cu, qu)


def _field(field, shape, fill_values):
    fld = field if isinstance(field, F.Field) else F.Field(field, fill=fill_values)
    if tuple(fld.data.shape[-2:]) != tuple(shape):
        raise ValueError("locate: the field ends in %s, the grid has %d x %d model cells (ny, nx)" % (tuple(fld.data.shape[-2:]), shape[0], shape[1]))
    return fld


def sample_located(res, field, wet=None, mode="bilinear", fill_values=()):
    """The field (a Field, or an array (..., ny, nx) with ``fill_values``) at the points of a locate() result, through the host-pointer
    entry ogg_locate_sample: {"name", "values" (lead dims..., point) fp64, "flags" the same shape uint8, "counts", "field"}, which is
    also appended to res["samples"]."""
    shape = res["shape"]
    fld = _field(field, shape, fill_values)
    m = F.cell_mask(wet, shape, "locate: the wet mask")
    n = res["cell"].size
    p = params(shape[0], shape[1], n, res["periodic"], res["fold"], mode, fld.nrec, fld.data.dtype, fld.fill)
    values = np.empty((fld.nrec, n), np.float64)
    flags = np.empty((fld.nrec, n), np.uint8)
    c = L.LocateCounts()
    L.call("ogg_locate_sample", ctypes.byref(p), res["cell"].ctypes.data, res["s"].ctypes.data, res["t"].ctypes.data, fld.data.ctypes.data,
           L.ptr(m), values.ctypes.data, flags.ctypes.data, ctypes.byref(c))
    lead = fld.data.shape[:-2]
    out = {"name": fld.name, "values": values.reshape(lead + (n,)), "flags": flags.reshape(lead + (n,)), "mode": mode, "field": fld,
           "counts": {k: v for k, v in L.counts_dict(L.LOCATE_COUNT_FIELDS, c).items() if k.startswith("flag")}}
    res["samples"].append(out)
    return out


def sample(x, y, lon, lat, field, wet=None, mode="bilinear", fill_values=(), periodic=None, fold=None):
    """locate() and sample_located() in one: the locate() dict with the sampled field in res["samples"][0]"""
    res = locate(x, y, lon, lat, periodic, fold)
    sample_located(res, field, wet, mode, fill_values)
    return res


def depth_field(depth):
    """the depth of a topography (ny, nx) as the Field that main() and the file command sample"""
    return F.Field(np.ascontiguousarray(depth, dtype=np.float64), name="depth", atts=[("units", "m")])


def set_wet(res, wet):
    """res["wet"]: the wet byte of the cell that holds each point (-1 where none); nothing without a wet set"""
    if wet is not None:
        w = F.cell_mask(wet, res["shape"], "locate: the wet mask").reshape(-1)
        res["wet"] = np.where(res["cell"] >= 0, w[np.maximum(res["cell"], 0)], -1).astype(np.int8)
    return res


# ---- device arrays ---------------------------------------------------------------------------------------------
def locate_dev(x, y, lon, lat, periodic=None, fold=None, names=None, keep_vectors=False, field=None, wet=None, mode="bilinear",
               fill_values=()):
    """locate() on one GPU with the grid x, y ((2 ny + 1) x (2 nx + 1)) as float64 device tensors and the points as numpy arrays or
    device tensors: the sets, index and search steps on the device's current stream, and with ``field`` (a Field, an array or a device
    tensor (..., ny, nx)) the sample step.  The same dict as locate(), with host arrays."""
    import torch
    from . import ocean_mask as M
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.topology_of_device_grid(x, y))
    if hasattr(lon, "device") and hasattr(lon, "data_ptr"):
        dlon, dlat = lon.to(torch.float64).reshape(-1).contiguous(), lat.to(torch.float64).reshape(-1).contiguous()
        lon, lat = dlon.cpu().numpy(), dlat.cpu().numpy()
    else:
        lon, lat = _points(lon, lat)
        dlon, dlat = torch.from_numpy(lon).to(dev), torch.from_numpy(lat).to(dev)
    n = int(dlon.numel())
    p = params(shape[0], shape[1], n, periodic, fold)
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_locate_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    cu = torch.empty(((shape[0] + 1) * (shape[1] + 1), 3), dtype=torch.float64, device=dev)
    qu = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cell = torch.empty(n, dtype=torch.int32, device=dev)
    s, t, m = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    counts = torch.zeros(len(L.LOCATE_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_locate_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), nxp, ws.data_ptr(), wsb, cu.data_ptr(), counts.data_ptr(), st)
    L.call("ogg_locate_index_dev", ctypes.byref(p), ws.data_ptr(), wsb, counts.data_ptr(), st)
    L.call("ogg_locate_search_dev", ctypes.byref(p), cu.data_ptr(), dlon.data_ptr(), dlat.data_ptr(), ws.data_ptr(), wsb, qu.data_ptr(),
           cell.data_ptr(), s.data_ptr(), t.data_ptr(), m.data_ptr(), counts.data_ptr(), st)
    sampled = None
    if field is not None:
        if hasattr(field, "data_ptr"):
            df = field.contiguous()
            fld = F.Field(np.empty(tuple(df.shape), np.float32 if df.dtype == torch.float32 else np.float64), fill=fill_values)
        else:
            fld = _field(field, shape, fill_values)
            df = torch.from_numpy(fld.data).to(dev)
        if tuple(df.shape[-2:]) != tuple(shape):
            raise ValueError("locate: the field ends in %s, the grid has %d x %d model cells (ny, nx)" % (tuple(df.shape[-2:]), shape[0], shape[1]))
        wm = F.cell_mask(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, shape, "locate: the wet mask")
        dw = torch.from_numpy(wm).to(dev) if wm is not None else None
        ps = params(shape[0], shape[1], n, periodic, fold, mode, fld.nrec, fld.data.dtype, fld.fill)
        values = torch.empty((fld.nrec, n), dtype=torch.float64, device=dev)
        flags = torch.empty((fld.nrec, n), dtype=torch.uint8, device=dev)
        L.call("ogg_locate_sample_dev", ctypes.byref(ps), cell.data_ptr(), s.data_ptr(), t.data_ptr(), df.data_ptr(),
               dw.data_ptr() if dw is not None else None, values.data_ptr(), flags.data_ptr(), counts.data_ptr(), st)
        lead = tuple(df.shape[:-2])
        sampled = {"name": fld.name, "values": values.cpu().numpy().reshape(lead + (n,)), "flags": flags.cpu().numpy().reshape(lead + (n,)),
                   "mode": mode, "field": fld}
    cd = L.counts_dict(L.LOCATE_COUNT_FIELDS, counts)
    res = result(cell.cpu().numpy(), s.cpu().numpy(), t.cpu().numpy(), m.cpu().numpy(), cd, lon, lat, shape, periodic, fold, names,
                 cu.cpu().numpy() if keep_vectors else None, qu.cpu().numpy() if keep_vectors else None)
    if sampled is not None:
        sampled["counts"] = {k: v for k, v in cd.items() if k.startswith("flag")}
        res["samples"].append(sampled)
    return res


# ---- files -----------------------------------------------------------------------------------------------------
def read_points(path):
    """(lon, lat, names or None) of a points file: a NetCDF classic / 64-bit-offset file with 1-D ``lon`` and ``lat``, or a text file
    with ``lon lat [name]`` per line, where ``#`` starts a comment (a file in which some points are named and others are not gives
    the unnamed ones an empty name)"""
    with open(path, "rb") as fh:
        magic = fh.read(4)
    if magic[:3] == b"CDF" or magic[1:4] == b"HDF":
        h = netcdf3.read_header(path)
        g = {}
        for name in ("lon", "lat"):
            v = h.vars.get(name)
            if v is None or len(v.shape) != 1 or v.is_record or v.nc_type not in (netcdf3.NC_FLOAT, netcdf3.NC_DOUBLE):
                raise ValueError("%s: 1-D fixed-size float or double variables lon and lat are needed (variables: %s)"
                                 % (path, ", ".join(sorted(h.vars))))
            g[name] = np.frombuffer(netcdf3.read_var_bytes(path, h, name, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type])
        lon, lat = _points(g["lon"], g["lat"])
        return lon, lat, None
    lon, lat, names = [], [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if len(w) not in (2, 3):
                raise ValueError("%s:%d: %d values: lon lat [name]" % (path, no, len(w)))
            try:
                a, b = float(w[0]), float(w[1])
            except ValueError:
                raise ValueError("%s:%d: two numbers are needed: %s" % (path, no, " ".join(w)))
            lon.append(a)
            lat.append(b)
            names.append(w[2] if len(w) == 3 else "")
    if not lon:
        raise ValueError("%s: no points" % path)
    return np.array(lon), np.array(lat), (names if any(names) else None)


def write_locate(path, res, title="model cells and sampled fields at points"):
    """lon, lat, s, t, margin (double), cell_j and cell_i (int, -1 where none), an optional name (char), with a wet set the byte wet
    of the cell that holds the point, and per sampled field a double
    <V> (the field's leading dimensions, then point; _FillValue 1e20) and a byte <V>_locate_flag, dim ``point``, as a NetCDF
    64-bit-offset file"""
    n = res["cell"].size
    names = res.get("names")
    dims = [("point", n)]
    entries = [(smp["field"], [(smp["name"], smp["values"])]) for smp in res["samples"]]
    lead, coords, _ = F.writer_dims("locate", entries)
    width = max([len(s.encode()) for s in names] + [1]) if names is not None else 0
    if names is not None:
        dims.append(("name_len", width))
    ds = netcdf3.Dataset(path, lead + dims, global_atts=[
        ("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells, great-circle edges"), ("ny", int(res["shape"][0])),
        ("nx", int(res["shape"][1])), ("periodic", int(res["periodic"])), ("fold", int(res["fold"]))])
    for d, nc_type, atts, vals in coords:
        ds.def_var(d, nc_type, (d,), atts, vals)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("point",), [("units", "degrees_east")], res["lon"])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("point",), [("units", "degrees_north")], res["lat"])
    ds.def_var("cell_j", netcdf3.NC_INT, ("point",), [("long_name", "row of the model cell that holds the point, -1 where none")], res["cell_j"])
    ds.def_var("cell_i", netcdf3.NC_INT, ("point",), [("long_name", "column of the model cell that holds the point, -1 where none")],
               res["cell_i"])
    ds.def_var("s", netcdf3.NC_DOUBLE, ("point",), [("long_name", "fractional position from the cell's west (0) to its east (1) edge")], res["s"])
    ds.def_var("t", netcdf3.NC_DOUBLE, ("point",), [("long_name", "fractional position from the cell's south (0) to its north (1) edge")],
               res["t"])
    ds.def_var("margin", netcdf3.NC_DOUBLE, ("point",), [("long_name", "the smallest signed great-circle edge measure of the point in its cell")],
               res["margin"])
    if names is not None:
        chars = np.zeros((n, width), "S1")
        for k, s in enumerate(names):
            b = s.encode()
            chars[k, :len(b)] = np.frombuffer(b, "S1")
        ds.def_var("name", netcdf3.NC_CHAR, ("point", "name_len"), [], chars)
    if res.get("wet") is not None:
        ds.def_var("wet", netcdf3.NC_BYTE, ("point",), [("long_name", "1 the cell that holds the point is wet, 0 land, -1 no cell")], res["wet"])
    for smp in res["samples"]:
        fld = smp["field"]
        vd = tuple(d for d, _ in fld.lead_dims) + ("point",)
        ds.def_var(smp["name"], netcdf3.NC_DOUBLE, vd, list(fld.atts) + [("_FillValue", FILL), ("locate_mode", smp["mode"])], smp["values"])
        ds.def_var(smp["name"] + "_locate_flag", netcdf3.NC_BYTE, vd,
                   [("long_name", "0 no cell, 1 all cells of the stencil used, 2 fewer used, 3 none (dry or missing)")], smp["flags"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    topo = ", ".join([t for t, f in (("periodic", s["periodic"]), ("folded", s["fold"])) if f]) or "neither periodic nor folded"
    out = ["   locate: %d points on %d x %d cells (%s): %d located, %d outside the grid, %d not finite; %.1f cell tests per point (%s, %d "
           "large cells)" % (s["points"], s["shape"][1], s["shape"][0], topo, s["located"], s["outside"], s["invalid"], s["tests_per_query"],
                             "%d cubes per axis" % s["cubes"] if s["cubes"] else "brute force", s["large_cells"])]
    names = res.get("names")
    for k in np.nonzero(res["cell"] < 0)[0][:20]:
        out.append("   locate: point %d%s at lon %.6f, lat %.6f is in no cell" % (k, " (%s)" % names[k] if names and names[k] else "",
                                                                                res["lon"][k], res["lat"][k]))
    if int((res["cell"] < 0).sum()) > 20:
        out.append("   locate: ... and %d more" % (int((res["cell"] < 0).sum()) - 20))
    for smp in res["samples"]:
        c = smp["counts"]
        out.append("   locate: %s (%s): %d values from a full stencil, %d from part of it, %d dry or missing, %d without a cell"
                   % (smp["name"], smp["mode"], c["flag1"], c["flag2"], c["flag3"], c["flag0"]))
    return out


def read_field(path, var, shape):
    """a Field on the model cells from a NetCDF classic / 64-bit-offset file (record and packed variables as elsewhere)"""
    from . import latlon_regrid as G
    return G.read_field(path, var, shape)


def main(argv=None):
    from . import remap as R
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.locate",
                                description="the model cells that hold a list of points, and model fields sampled there")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("points", help="text file of `lon lat [name]` lines, or a NetCDF file with 1-D lon and lat")
    p.add_argument("--fields", action="append", default=[], help="a file of fields on the model cells (repeat with --var)")
    p.add_argument("--var", action="append", default=[], help="the variable of the --fields file at the same position")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--mode", choices=sorted(MODES), default="bilinear", help="how fields are sampled (default bilinear)")
    p.add_argument("-o", "--output", default="points.nc")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    if len(a.fields) != len(a.var):
        raise ValueError("locate: %d --fields and %d --var: one --var for every --fields" % (len(a.fields), len(a.var)))
    grid = netcdf3.read_doubles(a.grid, names=("x", "y"))
    lon, lat, names = read_points(a.points)
    res = locate(grid["x"], grid["y"], lon, lat, names=names)
    wet = R.mask_from_file(a.topog or a.mask) if (a.topog or a.mask) else None
    set_wet(res, wet)
    if a.topog:   # the depth too, as main() samples it
        sample_located(res, depth_field(netcdf3.read_doubles(a.topog, names=("depth",))["depth"]), wet, a.mode)
    for path, var in zip(a.fields, a.var):
        fld = read_field(path, var, res["shape"])
        print(fld.note)
        sample_located(res, fld, wet, a.mode)
    for line in summary_lines(res):
        print(line)
    write_locate(a.output, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(res["summary"], samples=[dict(s["counts"], name=s["name"], mode=s["mode"]) for s in res["samples"]]), fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

"""Distance to the coast: for every wet model cell the nearest coastal land cell and its distance, and for every land cell the
nearest coastal wet cell, as MOM6 set-ups need it to taper salinity restoring near land, to spread runoff, to build sponges and to
spot enclosed waters.  include/ogg_hip.h, "Distance to the coast", gives the definition; the reference has no such step.

Cell centres are unit vectors and nearness is the chordal distance of the runoff mapping (ties to the smaller cell); a cell is
coastal when a face neighbour (the ocean mask's topology; the grid's edge is no coast) has the other wetness.  The sets and the
search run on the device (ogg_coast_sets_dev and ogg_coast_search_dev, or the host-pointer ogg_coast_distance): one workgroup per
tile of cells prunes an index of the coastal cells for all of its cells at once.  The device returns the nearest cell and the squared
chordal distance d2; the distance in metres is formed here with numpy from d2, so every path, knob and rank count writes the same
bytes.

    python -m ocean_model_grid_generator_amd.coast_distance ocean_hgrid.nc (--topog topog.nc | --mask ocean_mask.nc)
        [--sides wet|land|both] -o coast_distance.nc [--json summary.json]
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

SIDES = {"wet": L.COAST_WET, "land": L.COAST_LAND, "both": L.COAST_WET | L.COAST_LAND}
FILL = 1.0e20          # distance where there is no answer


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, sides="both", periodic=False, fold=False):
    """an ogg_coast_params, checked by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    if sides not in SIDES:
        raise ValueError("coast distance: sides must be one of %s, not %r" % (", ".join(sorted(SIDES)), sides))
    return L.checked("ogg_coast_check", L.CoastParams(ny=int(ny), nx=int(nx), topology=M.topology_flags(periodic, fold), sides=SIDES[sides]))


def _wet(wet, shape):
    return F.wet_mask(wet, shape, "coast distance")


def distance_of(d2, nearest, Re=X.DEFAULT_RE):
    """metres from the device's d2: Re * (2 * arcsin(minimum(1, 0.5 * sqrt(d2)))), FILL where there is no answer"""
    d = Re * (2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.sqrt(d2))))
    return np.where(nearest < 0, FILL, d)


def result(nearest, d2, flags, counts, x, y, sides, periodic, fold, Re, lists=None):
    """What coast_distance() returns, per cell in (ny, nx): distance (metres, FILL without an answer), nearest_j and nearest_i (-1
    where none), nearest and d2 as the device gave them, wet and coast (uint8, from the flag bytes), flags; the counts and a summary.
    x, y: the supergrid points, numpy arrays or device tensors (only the farthest cell's centre is read)."""
    ny, nx = nearest.shape
    has = nearest >= 0
    wet = (flags & L.COAST_F_WET).astype(np.uint8)
    summary = dict(counts, shape=[ny, nx], sides=sides, periodic=bool(periodic), fold=bool(fold), Re=float(Re),
                   tests_per_query=(counts["tests"] / counts["queries"]) if counts["queries"] else 0.0, farthest=None)
    sel = has & (wet != 0)
    if sel.any():   # the grid's own "point Nemo": the wet cell farthest from land
        k = int(np.argmax(np.where(sel, d2, -1.0)))
        j, i = divmod(k, nx)
        t = int(nearest.flat[k])
        summary["farthest"] = {"km": float(distance_of(d2.flat[k], nearest.flat[k], Re)) / 1000.0, "j": j, "i": i,
                               "lon": float(x[2 * j + 1, 2 * i + 1]), "lat": float(y[2 * j + 1, 2 * i + 1]), "nearest_j": t // nx,
                               "nearest_i": t % nx}
    out = {"distance": distance_of(d2, nearest, Re), "nearest_j": np.where(has, nearest // nx, -1).astype(np.int32),
           "nearest_i": np.where(has, nearest % nx, -1).astype(np.int32), "nearest": nearest, "d2": d2, "wet": wet,
           "coast": ((flags & L.COAST_F_COAST) != 0).astype(np.uint8), "flags": flags, "counts": counts, "summary": summary}
    if lists is not None:
        out.update(lists)
    return out


# ---- host arrays -----------------------------------------------------------------------------------------------
def coast_distance(x, y, wet, sides="both", periodic=None, fold=None, Re=X.DEFAULT_RE):
    """The distance to the coast of the model cells of a stitched supergrid x, y ((2 ny + 1) x (2 nx + 1), degrees) with the wet set
    ``wet`` (one value per model cell, 0: land), on one GPU through the host-pointer entry ogg_coast_distance.  sides: "wet", "land"
    or "both", the cells that are queried.  periodic, fold: None to read them from the grid (ocean_mask.detect_topology).  A dict:
    see result()."""
    from . import ocean_mask as M
    x, y = L.as_f64(x), L.as_f64(y)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = _wet(wet, shape)
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.detect_topology(x, y, 2))
    p = params(shape[0], shape[1], sides, periodic, fold)
    nearest = np.empty(shape, np.int32)
    d2 = np.empty(shape, np.float64)
    flags = np.empty(shape, np.uint8)
    c = L.CoastCounts()
    L.call("ogg_coast_distance", ctypes.byref(p), x.ctypes.data, y.ctypes.data, m.ctypes.data, nearest.ctypes.data, d2.ctypes.data,
           flags.ctypes.data, ctypes.byref(c))
    counts = L.counts_dict(L.COAST_COUNT_FIELDS, c)
    return result(nearest, d2, flags, counts, x, y, sides, periodic, fold, Re)


# ---- device arrays ---------------------------------------------------------------------------------------------
def coast_distance_dev(x, y, wet, sides="both", periodic=None, fold=None, Re=X.DEFAULT_RE, keep_lists=False):
    """coast_distance() on one GPU with the grid x, y ((2 ny + 1) x (2 nx + 1)) as float64 device tensors: the two steps on the
    device, on its current stream, with one read of the counts between them.  The same dict as coast_distance(), with host arrays;
    with ``keep_lists`` also the unit vectors of every cell (u) and the coastal lists (land_cell, land_u, wet_cell, wet_u) as the
    device computed them."""
    import torch
    from . import ocean_mask as M
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = _wet(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, shape)
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.topology_of_device_grid(x, y))
    p = params(shape[0], shape[1], sides, periodic, fold)
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_coast_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nc = shape[0] * shape[1]
    wt = torch.from_numpy(m).to(dev)
    flags = torch.empty(shape, dtype=torch.uint8, device=dev)
    u = torch.empty((nc, 3), dtype=torch.float64, device=dev)
    lc, wc = (torch.empty(nc, dtype=torch.int32, device=dev) for _ in range(2))
    lu, wu = (torch.empty((nc, 3), dtype=torch.float64, device=dev) for _ in range(2))
    nearest = torch.empty(shape, dtype=torch.int32, device=dev)
    d2 = torch.empty(shape, dtype=torch.float64, device=dev)
    counts = torch.zeros(len(L.COAST_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_coast_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), nxp, wt.data_ptr(), ws.data_ptr(), wsb, flags.data_ptr(),
           u.data_ptr(), lc.data_ptr(), lu.data_ptr(), wc.data_ptr(), wu.data_ptr(), counts.data_ptr(), st)
    c = counts.cpu().numpy()
    nw, nl = int(c[0]), int(c[1])
    L.call("ogg_coast_search_dev", ctypes.byref(p), flags.data_ptr(), u.data_ptr(), lc.data_ptr(), lu.data_ptr(), nl, wc.data_ptr(),
           wu.data_ptr(), nw, ws.data_ptr(), wsb, nearest.data_ptr(), d2.data_ptr(), counts.data_ptr(), st)
    cd = L.counts_dict(L.COAST_COUNT_FIELDS, counts)
    lists = None
    if keep_lists:
        lists = {"u": u.cpu().numpy(), "land_cell": lc[:nl].cpu().numpy(), "land_u": lu[:nl].cpu().numpy(),
                 "wet_cell": wc[:nw].cpu().numpy(), "wet_u": wu[:nw].cpu().numpy()}
    return result(nearest.cpu().numpy(), d2.cpu().numpy(), flags.cpu().numpy(), cd, x, y, sides, periodic, fold, Re, lists)


# ---- files -----------------------------------------------------------------------------------------------------
def write_coast_distance(path, res, title="distance to the coast of the model cells"):
    """distance (double, metres, _FillValue 1e20), nearest_j and nearest_i (int, -1 where none), wet and coast (byte), dims (ny, nx),
    as a NetCDF 64-bit-offset file"""
    ny, nx = res["nearest"].shape
    s = res["summary"]
    ds = netcdf3.Dataset(path, [("ny", ny), ("nx", nx)], global_atts=[
        ("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells"), ("sides", s["sides"]), ("Re", float(s["Re"])),
        ("periodic", int(s["periodic"])), ("fold", int(s["fold"]))])
    ds.def_var("distance", netcdf3.NC_DOUBLE, ("ny", "nx"),
               [("units", "m"), ("long_name", "great-circle distance to the nearest cell across the coast"), ("_FillValue", FILL)],
               res["distance"])
    ds.def_var("nearest_j", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "row of the nearest cell across the coast, -1 where none")],
               res["nearest_j"])
    ds.def_var("nearest_i", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "column of the nearest cell across the coast, -1 where none")],
               res["nearest_i"])
    ds.def_var("wet", netcdf3.NC_BYTE, ("ny", "nx"), [("long_name", "1 wet, 0 land")], res["wet"])
    ds.def_var("coast", netcdf3.NC_BYTE, ("ny", "nx"), [("long_name", "1 where a face neighbour has the other wetness")], res["coast"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    topo = ", ".join([t for t, f in (("periodic", s["periodic"]), ("folded", s["fold"])) if f]) or "neither periodic nor folded"
    out = ["   coast distance: %d x %d cells (%s): %d coastal wet and %d coastal land cells; %d of %d queries (%s) answered, %.1f "
           "distance tests per query (%d tiles, %s)"
           % (s["shape"][1], s["shape"][0], topo, s["coast_wet"], s["coast_land"], s["answered"], s["queries"], s["sides"],
              s["tests_per_query"], s["tiles"], "%d cubes per axis" % s["cubes"] if s["cubes"] else "brute force")]
    f = s["farthest"]
    if f is not None:
        out.append("   coast distance: the wet cell farthest from land is (j=%d, i=%d) at lon %.4f, lat %.4f: %.1f km from cell (j=%d, i=%d)"
                   % (f["j"], f["i"], f["lon"], f["lat"], f["km"], f["nearest_j"], f["nearest_i"]))
    return out


def main(argv=None):
    from . import remap as R
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.coast_distance",
                                description="distance to the coast of the model cells of a supergrid file")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--sides", choices=sorted(SIDES), default="both", help="the cells that get a distance (default both)")
    p.add_argument("-o", "--output", default="coast_distance.nc")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    grid = netcdf3.read_doubles(a.grid, names=("x", "y"))
    res = coast_distance(grid["x"], grid["y"], R.mask_from_file(a.topog or a.mask), sides=a.sides)
    for line in summary_lines(res):
        print(line)
    write_coast_distance(a.output, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

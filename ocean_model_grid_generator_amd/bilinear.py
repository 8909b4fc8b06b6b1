"""Bilinear interpolation: scalar and vector fields on a global lat-lon grid (initial temperature and salinity, SST restoring,
atmospheric state, winds, wind stress, currents) interpolated between the source's cell centres at the h, u or v points of a
supergrid, and vectors turned from (east, north) to the grid's own x and y directions with angle_dx.  include/ogg_hip.h, "Bilinear
interpolation", gives the definition; the reference has no such step.

The locate, the masked weighted sums and the rotation run on the device (ogg_bilinear_dev / ogg_bilinear_rotate_dev, or the
host-pointer ogg_bilinear); at the h points the wet points the source leaves empty are filled by the remap's own fill
(ogg_remap_fill_dev).  Every value is a fixed function of one point, so the result is bit-identical for any launch geometry and
any number of ranks.  At u, v and c points there is no mask and no fill: a point with no valid corner stays unfilled (flag 3).

    python -m ocean_model_grid_generator_amd.bilinear ocean_hgrid.nc SOURCE [--var V]... [--vector U V]... [--points h|u|v|c]
        [--topog topog.nc | --mask ocean_mask.nc] [--no_fill] [--fill_max N] [--no_rotate] -o interp.nc [--json summary.json]

SOURCE is read as for the remap (remap.read_source).  --points c (vectors only) gives the first component at the u points and the
second at the v points.  angle_dx comes from the grid file.
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _lib as L
from . import exchange_grid as X
from . import fields as F
from . import netcdf3
from . import remap as R

FILL = L.REMAP_FILL
FLAG_NAMES = ("dry", "interpolated", "filled", "unfilled")
POINTS = L.BILINEAR_POINTS
_DIMS = {"h": ("ny", "nx"), "u": ("ny", "nxq"), "v": ("nyq", "nx")}


def point_shape(ny, nx, kind):
    """rows and columns of the h, u or v points of ny x nx model cells"""
    return {"h": (ny, nx), "u": (ny, nx + 1), "v": (ny + 1, nx)}[kind]


def _kinds(points, vector):
    """the point kinds of the first and of the second component"""
    return ("u", "v") if points == "c" else (points, points) if vector else (points,)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, source, points="h", ncomp=1, m0=0, periodic=False, fold=False, fill_max=None, has_mask=False):
    """an ogg_bilinear_params, checked by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    if points not in POINTS:
        raise ValueError("bilinear: points must be one of h, u, v, c, not %r" % (points,))
    if fill_max is not None and int(fill_max) < 0:
        raise ValueError("bilinear: fill_max must be >= 0 (%r)" % (fill_max,))
    p = L.BilinearParams(ny=int(ny), nx=int(nx), m0=int(m0), NA=source.lon.size - 1, NB=source.lat.size - 1, nrec=source.nrec,
                         dtype=R._DTYPES[source.data.dtype], n_fill=len(source.fill), points=POINTS[points], ncomp=int(ncomp),
                         topology=M.topology_flags(periodic, fold), fill_max=-1 if fill_max is None else int(fill_max))
    for k, f in enumerate(source.fill):
        p.fill[k] = float(f)
    check(p, has_mask)
    return p


def check(p, has_mask=False):
    """ogg_bilinear_check: the reason of a refusal as a ValueError (no device is needed)"""
    L.checked("ogg_bilinear_check", p, 1 if has_mask else 0)


def _pair(source, source2):
    """the second component must lie on the first's grid, in its type and with its fill values"""
    if source2 is None:
        return
    if not (np.array_equal(source.lon, source2.lon) and np.array_equal(source.lat, source2.lat)):
        raise ValueError("bilinear: the two components %s and %s are on different grids" % (source.name, source2.name))
    if source.data.shape != source2.data.shape or source.data.dtype != source2.data.dtype:
        raise ValueError("bilinear: the two components are %s %s and %s %s" % (source.data.dtype, source.data.shape, source2.data.dtype,
                                                                                 source2.data.shape))
    if tuple(source.fill) != tuple(source2.fill):
        raise ValueError("bilinear: the two components have different fill values (%s, %s)" % (source.fill, source2.fill))


def result(arrays, source, source2, points, periodic, fold, fill, fill_max, masked, rotated):
    """What bilinear() returns: values and flags (the source's leading dimensions, then the points' rows and columns); for a vector
    also values2 and flags2, and rot_cos / rot_sin (rot_cos2 / rot_sin2 at c points: the v points') when there was an angle; the counts
    of the first component's flags and a summary."""
    lead = tuple(source.data.shape[:-2])
    out = {}
    for k in ("values", "flags", "values2", "flags2"):
        if arrays.get(k) is not None:
            out[k] = arrays[k].reshape(lead + arrays[k].shape[-2:])
    for k in ("rot_cos", "rot_sin", "rot_cos2", "rot_sin2"):
        if arrays.get(k) is not None:
            out[k] = arrays[k]
    n = np.bincount(out["flags"].reshape(-1), minlength=4)
    counts = {"dry": int(n[0]), "interpolated": int(n[1]), "filled": int(n[2]), "unfilled": int(n[3])}
    names = [source.name] + ([source2.name] if source2 is not None else [])
    summary = dict(counts, var=names, records=source.nrec, source_shape=[source.lat.size - 1, source.lon.size - 1], points=points,
                   shape=list(out["values"].shape[-2:]), periodic=bool(periodic), fold=bool(fold), fill=bool(fill),
                   fill_max=None if fill_max is None else int(fill_max), masked=bool(masked), vector=source2 is not None,
                   grid_relative=bool(rotated))
    out.update(counts=counts, summary=summary)
    return out


# ---- host arrays -----------------------------------------------------------------------------------------------
def bilinear(x, y, source, source2=None, angle_dx=None, points="h", mask=None, fill=True, fill_max=None, rotate=True):
    """The bilinear interpolation of ``source`` (a remap.Source; with ``source2`` the eastward and northward components of a vector)
    at the ``points`` ("h", "u", "v", or "c" for a vector) of a stitched supergrid x, y ((2 ny + 1) x (2 nx + 1), degrees), on one GPU
    through the host-pointer entry ogg_bilinear.  mask (h points only): None or one value per model cell (0: dry).  fill (h points
    only; elsewhere nothing is filled): fill the wet points the source leaves empty, up to fill_max steps.  A vector is turned to the
    grid's directions with ``angle_dx`` (the supergrid's, degrees) unless rotate is False; without angle_dx it cannot be turned.  A
    dict: see result()."""
    from . import ocean_mask as M
    _pair(source, source2)
    x, y = L.as_f64(x), L.as_f64(y)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    ny, nx = (nyp - 1) // 2, (nxp - 1) // 2
    vector = source2 is not None
    m = F.cell_mask(mask, (ny, nx), "bilinear: the mask")
    fill = bool(fill) and points == "h"
    periodic, fold = M.detect_topology(x, y, 2) if fill else (False, False)
    p = params(ny, nx, source, points, 2 if vector else 1, 0, periodic, fold, fill_max, m is not None)
    ang = _angle(angle_dx, x.shape, vector, rotate)
    kinds = _kinds(points, vector)
    nrec = source.nrec
    arr = {}
    for sfx, kind in zip(("", "2"), kinds):
        shape = point_shape(ny, nx, kind)
        npair = nrec * shape[0] * shape[1]
        arr["values" + sfx] = np.empty((nrec,) + shape, dtype=np.float64)
        arr["_flags" + sfx] = np.empty((npair + 3) // 4 * 4, dtype=np.uint8)
    if ang is not None:
        for sfx, kind in zip(("", "2"), kinds if points == "c" else kinds[:1]):
            arr["rot_cos" + sfx] = np.empty(point_shape(ny, nx, kind), dtype=np.float64)
            arr["rot_sin" + sfx] = np.empty(point_shape(ny, nx, kind), dtype=np.float64)
    at = lambda k: None if arr.get(k) is None else arr[k].ctypes.data   # noqa: E731
    L.call("ogg_bilinear", ctypes.byref(p), x.ctypes.data, y.ctypes.data, None if ang is None else ang.ctypes.data,
           source.lon.ctypes.data, source.lat.ctypes.data, source.records.ctypes.data,
           source2.records.ctypes.data if vector else None, None if m is None else m.ctypes.data, 1 if fill else 0,
           1 if rotate else 0, at("values"), at("_flags"), at("values2"), at("_flags2"), at("rot_cos"), at("rot_sin"), at("rot_cos2"),
           at("rot_sin2"))
    for sfx in ("", "2")[:len(kinds)]:
        v = arr["values" + sfx]
        arr["flags" + sfx] = arr.pop("_flags" + sfx)[:v.size].reshape(v.shape)
    return result(arr, source, source2, points, periodic, fold, fill, fill_max, m is not None, vector and rotate and ang is not None)


def _angle(angle_dx, shape, vector, rotate):
    if not vector:
        return None
    if angle_dx is None:
        if rotate:
            raise ValueError("bilinear: a vector is turned to the grid's directions with angle_dx; pass it, or rotate=False")
        return None
    a = L.as_f64(angle_dx)
    if a.shape != shape:
        raise ValueError("bilinear: angle_dx is %s, the supergrid %s" % (a.shape, shape))
    return a


# ---- device arrays ---------------------------------------------------------------------------------------------
def bilinear_dev(x, y, source, source2=None, angle_dx=None, points="h", mask=None, fill=True, fill_max=None, rotate=True):
    """bilinear() on one GPU with the grid x, y (and angle_dx) as float64 device tensors ((2 ny + 1) x (2 nx + 1), contiguous rows)
    and remap.Source fields: the locate, the sums, the fill and the rotation all on the device, on its current stream.  The same
    dict as bilinear(), with host arrays."""
    import torch
    from . import ocean_mask as M
    _pair(source, source2)
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    ny, nx = (nyp - 1) // 2, (nxp - 1) // 2
    vector = source2 is not None
    m = F.cell_mask(mask, (ny, nx), "bilinear: the mask")
    fill = bool(fill) and points == "h"
    periodic, fold = False, False
    if fill:
        periodic, fold = M.topology_of_device_grid(x, y)
    p = params(ny, nx, source, points, 2 if vector else 1, 0, periodic, fold, fill_max, m is not None)
    if vector and angle_dx is None and rotate:
        raise ValueError("bilinear: a vector is turned to the grid's directions with angle_dx; pass it, or rotate=False")
    ang = None
    if vector and angle_dx is not None:
        ang = angle_dx.contiguous()
        if tuple(ang.shape) != (nyp, nxp):
            raise ValueError("bilinear: angle_dx is %s, the supergrid %s" % (tuple(ang.shape), (nyp, nxp)))
    st = torch.cuda.current_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    lon, lat, f = to(source.lon), to(source.lat), to(source.records)
    f2 = to(source2.records) if vector else None
    mt = None if m is None else to(m)
    kinds = _kinds(points, vector)
    nrec = source.nrec
    t = {}
    for sfx, kind in zip(("", "2"), kinds):
        shape = (nrec,) + point_shape(ny, nx, kind)
        t["values" + sfx] = torch.empty(shape, dtype=torch.float64, device=dev)
        t["flags" + sfx] = R.flags_buffer(torch, nrec * shape[1] * shape[2], dev).view(shape)
    turn = ang is not None and rotate
    if points == "c" and turn:
        t["cross"], t["cross2"] = torch.empty_like(t["values"]), torch.empty_like(t["values2"])
    dp = lambda k: None if t.get(k) is None else t[k].data_ptr()   # noqa: E731
    L.call("ogg_bilinear_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), nxp, lon.data_ptr(), lat.data_ptr(), f.data_ptr(),
           None if f2 is None else f2.data_ptr(), None if mt is None else mt.data_ptr(), dp("values"), dp("flags"), dp("values2"),
           dp("flags2"), dp("cross"), dp("cross2"), st)
    if fill:   # each component from its own copy of the flags, still eastward and northward
        q = R.params(ny, nx, source, 0, periodic, fold, fill_max)
        for sfx in ("", "2")[:len(kinds)]:
            counts = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
            R.fill_dev(q, t["values" + sfx], t["flags" + sfx], counts, st, dev)
    if ang is not None:
        for sfx, kind in zip(("", "2"), kinds if points == "c" else kinds[:1]):
            for k in ("rot_cos", "rot_sin"):
                t[k + sfx] = torch.empty(point_shape(ny, nx, kind), dtype=torch.float64, device=dev)
        L.call("ogg_bilinear_rotate_dev", ctypes.byref(p), ang.data_ptr(), nxp, dp("values"), dp("flags"), dp("values2"), dp("flags2"),
               dp("cross"), dp("cross2"), dp("rot_cos"), dp("rot_sin"), dp("rot_cos2"), dp("rot_sin2"), 1 if rotate else 0, st)
    arr = {k: v.cpu().numpy() for k, v in t.items() if not k.startswith("cross")}
    return result(arr, source, source2, points, periodic, fold, fill, fill_max, m is not None, turn)


# ---- files -----------------------------------------------------------------------------------------------------
def write_bilinear(path, results, title="bilinear interpolation at the grid's points"):
    """One float64 variable per interpolated field (its source's leading dimensions, then the points' rows and columns: ny, nx at
    the h points, ny, nxq at the u points, nyq, nx at the v points; _FillValue FILL) and a byte variable <var>_interp_flag (0 dry, 1
    interpolated, 2 filled, 3 unfilled), the leading coordinate variables copied from the source, as a NetCDF 64-bit-offset file.  A
    vector's components carry the attributes vector_component, vector_partner and grid_relative ("true": along the grid's x and y;
    "false": eastward and northward).  ``results``: [((Source,) or (Source, Source), bilinear() result)]."""
    names = [s.name for srcs, _ in results for s in srcs]
    for n in names:
        if names.count(n) > 1:
            raise ValueError("bilinear: the variable %s is asked for twice" % n)
    dims, coords, _ = F.writer_dims("bilinear", [(srcs[0], [(s.name, res[key]) for s, key in zip(srcs, ("values", "values2"))])
                                                 for srcs, res in results], "; interpolate fewer records at a time")
    kinds = [k for _, res in results for k in _kinds(res["summary"]["points"], res["summary"]["vector"])]
    s0 = results[0][1]["summary"]
    ny, nx = s0["shape"][0] - (s0["points"] == "v"), s0["shape"][1] - (s0["points"] in ("u", "c"))
    dims += [("ny", ny), ("nx", nx)] + ([("nyq", ny + 1)] if "v" in kinds else []) + ([("nxq", nx + 1)] if "u" in kinds else [])
    ds = netcdf3.Dataset(path, dims, global_atts=[("title", title), ("points", "MOM6 h (ny, nx), u (ny, nxq) and v (nyq, nx) points"),
                                                  ("flag_values", "0 dry, 1 interpolated, 2 filled, 3 unfilled")])
    for name, nc_type, atts, vals in coords:
        ds.def_var(name, nc_type, (name,), atts, vals)
    for srcs, res in results:
        s = res["summary"]
        lead = tuple(d for d, _ in srcs[0].lead_dims)
        for k, (src, kind) in enumerate(zip(srcs, _kinds(s["points"], s["vector"]))):
            sfx = "2" if k else ""
            atts = list(src.atts) + [("_FillValue", FILL), ("points", kind)]
            if s["vector"]:
                atts += [("vector_component", "y" if k else "x"), ("vector_partner", srcs[1 - k].name),
                         ("grid_relative", "true" if s["grid_relative"] else "false")]
            ds.def_var(src.name, netcdf3.NC_DOUBLE, lead + _DIMS[kind], atts, res["values" + sfx])
            ds.def_var(src.name + "_interp_flag", netcdf3.NC_BYTE, lead + _DIMS[kind],
                       [("long_name", "interpolation flag of " + src.name), ("flag_meanings", "dry interpolated filled unfilled")],
                       res["flags" + sfx].astype(np.int8))
    ds.write()


def summary_lines(res):
    s = res["summary"]
    fill = "%d filled" % s["filled"] if s["fill"] else "no fill"
    what = "vector (%s, %s), %s" % (s["var"][0], s["var"][1], "grid-relative" if s["grid_relative"] else "east / north") if s["vector"] \
        else s["var"][0]
    return ["   bilinear: %s, %d records of %d x %d source cells at the %s points (%d x %d)%s: %d interpolated, %s, %d unfilled, %d dry"
            % (what, s["records"], s["source_shape"][1], s["source_shape"][0], s["points"], s["shape"][1], s["shape"][0],
               " (masked)" if s["masked"] else "", s["interpolated"], fill, s["unfilled"], s["dry"])]


def requests(variables, vectors, points):
    """[(name,) or (name, name)] of --var and --vector, checked against --points before anything is read"""
    out = [(v,) for v in (variables or ())] + [tuple(v) for v in (vectors or ())]
    if not out:
        raise ValueError("bilinear: nothing to interpolate: give --var V or --vector U V")
    if points not in POINTS:
        raise ValueError("bilinear: points must be one of h, u, v, c, not %r" % (points,))
    if points == "c" and variables:
        raise ValueError("bilinear: c points are for vectors (the first component at u, the second at v); a scalar needs h, u or v")
    return out


def run_requests(reqs, read, interpolate):
    """[(sources, result)] of every request: ``read(name)`` gives a Source, ``interpolate(source, source2)`` the result"""
    out = []
    for names in reqs:
        srcs = tuple(read(n) for n in names)
        res = interpolate(srcs[0], srcs[1] if len(srcs) > 1 else None)
        if res is not None:
            for line in summary_lines(res):
                print(line)
        out.append((srcs, res))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.bilinear",
                                description="bilinear interpolation of lat-lon fields at the points of a supergrid file")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("source", help="the lat-lon source (NetCDF classic / 64-bit offset)")
    p.add_argument("--var", action="append", default=None, help="a scalar variable of the source (repeatable)")
    p.add_argument("--vector", nargs=2, action="append", default=None, metavar=("U", "V"),
                   help="the eastward and northward components of a vector (repeatable)")
    p.add_argument("--points", choices=sorted(POINTS), default="h", help="h (default), u, v, or c: a vector's components at u and v")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet (h points)")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet (h points)")
    p.add_argument("--no_fill", action="store_true", help="leave wet h points the source does not cover unfilled")
    p.add_argument("--fill_max", type=int, default=None, help="fill at most N cells away from an interpolated point")
    p.add_argument("--no_rotate", action="store_true", help="leave vectors as eastward and northward components")
    p.add_argument("-o", "--output", default="interp.nc")
    p.add_argument("--json", default=None, help="write the summaries as JSON to this file")
    a = p.parse_args(argv)
    reqs = requests(a.var, a.vector, a.points)
    need_angle = bool(a.vector) and not a.no_rotate
    grid = netcdf3.read_doubles(a.grid, names=("x", "y") + (("angle_dx",) if need_angle else ()))
    mask = R.mask_from_file(a.topog or a.mask) if (a.topog or a.mask) else None

    def read(name):
        src = R.read_source(a.source, name)
        print(src.note)
        return src
    out = run_requests(reqs, read, lambda s, s2: bilinear(grid["x"], grid["y"], s, s2, angle_dx=grid.get("angle_dx") if s2 is not None else None,
                                                          points=a.points, mask=mask, fill=not a.no_fill, fill_max=a.fill_max,
                                                          rotate=not a.no_rotate))
    write_bilinear(a.output, out)
    F.dump_summaries(a.json, out)
    return out


if __name__ == "__main__":
    main()
    sys.exit(0)

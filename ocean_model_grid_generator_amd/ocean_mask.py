"""Ocean mask: minimum depth and connected basins.  A cell of a topography result is wet when its depth is > 0 (and not the fill
value); cells shallower than a minimum depth become land (or are deepened to it), and then only the connected bodies of water that
hold a seed in the open ocean (or, without seeds, the largest one) stay wet.  Inland depressions below sea level, seas cut off by a
sill and one-cell ponds become land.  GFDL's preprocessing calls this step "ice9".  include/ogg_hip.h, "Ocean mask", gives the
definition; the reference has no such step.

Cells connect through shared faces only, across the periodic seam and across the tripolar fold when the grid has them
(detect_topology reads both from the grid's corner points).  The components are found on the device by union-find
(ogg_mask_label_dev: a tile-local labelling in LDS, a merge across tile edges, seam and fold, a flatten), the cells kept are written by
ogg_mask_apply_dev; only the seeds' roots and the choice of kept roots are looked at on the host.  Every output is an integer or a
copy, so the result is bit-identical on every run.

    python -m ocean_model_grid_generator_amd.ocean_mask topog.nc --grid ocean_hgrid.nc [--min_depth D] [--deepen]
        [--seed LON LAT]... [--keep_min_cells N] -o topog_edited.nc [--mask ocean_mask.nc] [--json s.json]
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import netcdf3

FILL = 1.0e20          # topography.FILL
CHORD_TOL = 1.0e-9     # two points are one point on the sphere when the chord between their unit vectors is at most this
N_LISTED = 10          # removed basins listed in the summary (largest first)
MODES = {"mask": L.MASK_MASK, "deepen": L.MASK_DEEPEN}


# ---- topology ------------------------------------------------------------------------------------------------
def _unit(lon, lat):
    D = np.pi / 180.0
    lon, lat = np.asarray(lon, dtype=np.float64) * D, np.asarray(lat, dtype=np.float64) * D
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def _chord(u, v):
    return np.sqrt(np.sum((u - v) ** 2, axis=-1))


def detect_topology(x, y, stride=2):
    """(periodic, fold) of the cells of a supergrid x, y ((NY + 1) x (NX + 1) points, degrees) at ``stride`` (2: model cells, 1:
    supergrid cells), from the corner points P[j][i] = (x, y)[stride j][stride i]: periodic when in every point row the first and last
    points are one point on the sphere; folded when the top point row maps onto itself reversed (P[top][i] = P[top][NX - i]) and is
    not a single point (a row at 90 degrees is a pole, not a fold).  Unit vectors are compared, chord <= CHORD_TOL."""
    x, y = np.asarray(x), np.asarray(y)
    px, py = x[::stride, ::stride], y[::stride, ::stride]
    return topology_of_edges((px[:, 0], py[:, 0]), (px[:, -1], py[:, -1]), (px[-1], py[-1]))


def topology_of_edges(first, last, top):
    """detect_topology from the corner points it reads: the first and last point columns and the top point row, each (lon, lat)"""
    if np.asarray(top[0]).size < 2:
        return False, False
    periodic = bool(np.all(_chord(_unit(*first), _unit(*last)) <= CHORD_TOL))
    t = _unit(*top)
    fold = bool(np.all(_chord(t, t[::-1]) <= CHORD_TOL) and np.any(_chord(t, t[0]) > CHORD_TOL))
    return periodic, fold


def topology_of_device_grid(x, y, stride=2):
    """detect_topology of a supergrid held as device tensors: only the corner columns and the top row are copied to the host"""
    xs, ys = x[::stride, ::stride], y[::stride, ::stride]
    return topology_of_edges(*[(xs[sl].cpu().numpy(), ys[sl].cpu().numpy())
                               for sl in ((slice(None), 0), (slice(None), -1), (-1, slice(None)))])


def topology_flags(periodic, fold):
    return (L.MASK_PERIODIC if periodic else 0) | (L.MASK_FOLD if fold else 0)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, periodic, fold, min_depth=0.0, mode="mask", keep_min_cells=0, fill=FILL):
    """an ogg_mask_params, checked by the library (OGG_EARG -> ValueError)"""
    if mode not in MODES:
        raise ValueError("ocean mask: mode must be 'mask' or 'deepen', not %r" % (mode,))
    p = L.MaskParams(ny=int(ny), nx=int(nx), topology=topology_flags(periodic, fold), mode=MODES[mode], fill=float(fill),
                     min_depth=float(min_depth), keep_min_cells=int(keep_min_cells))
    return L.checked("ogg_mask_check", p)


def _seeds(seeds):
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.float64).reshape(-1, 2)) if len(seeds) else np.zeros((0, 2))
    if s.shape[0] > L.MASK_MAX_SEEDS:
        raise ValueError("ocean mask: %d seeds (at most %d)" % (s.shape[0], L.MASK_MAX_SEEDS))
    return s


def _stride(shape, xshape):
    ny, nx = shape
    if xshape == (2 * ny + 1, 2 * nx + 1):
        return 2
    if xshape == (ny + 1, nx + 1):
        return 1
    raise ValueError("ocean mask: %d x %d cells are neither the model cells nor the supergrid cells of a grid of %d x %d points"
                     % (ny, nx, xshape[0], xshape[1]))


def _cell_point(stride, c, nx):
    """the point of cell c that stands for it: the centre of a model cell (supergrid point (2j+1, 2i+1)), the south-west corner of a
    supergrid cell"""
    j, i = divmod(int(c), nx)
    return (2 * j + 1, 2 * i + 1) if stride == 2 else (j, i)


def result(depth, wet, root, counts, comps, kept, seed_cells, seeds, x, y, stride, periodic, fold, min_depth, mode, keep_min_cells):
    """What ocean_mask() returns: the edited depth, the final wet mask, the roots, and the summary.  x, y: the supergrid points, numpy
    arrays or device tensors (only the listed basins' points are read)."""
    ny, nx = root.shape
    kept_set = set(int(r) for r in kept)
    roots_of = (np.iinfo(np.int32).max - (comps & 0xFFFFFFFF)).astype(np.int64)
    cells_of = (comps >> 32).astype(np.int64)
    gone = [(int(n), int(r)) for n, r in zip(cells_of, roots_of) if int(r) not in kept_set and not (keep_min_cells > 0 and n >= keep_min_cells)]
    removed = []
    for n, r in gone[:N_LISTED]:
        k = _cell_point(stride, r, nx)
        lon, lat = float(x[k]), float(y[k])
        removed.append({"cells": n, "root": r, "j": r // nx, "i": r % nx, "lon": lon, "lat": lat})
    largest = int(counts["largest"])
    summary = dict(counts, largest_cells=largest >> 32, largest_root=int(np.iinfo(np.int32).max - (largest & 0xFFFFFFFF)) if largest else -1,
                   shape=[ny, nx], cells="model" if stride == 2 else "supergrid", periodic=bool(periodic), fold=bool(fold),
                   min_depth=float(min_depth), mode=mode, keep_min_cells=int(keep_min_cells), removed_components=len(gone),
                   removed_largest=removed,
                   seeds=[{"lon": float(s[0]), "lat": float(s[1]), "cell": int(c), "j": int(c) // nx, "i": int(c) % nx,
                           "root": int(root.flat[int(c)])} for s, c in zip(seeds, seed_cells)])
    del summary["largest"]
    return {"depth": depth, "wet": wet, "root": root, "summary": summary}


# ---- host arrays -----------------------------------------------------------------------------------------------
def ocean_mask(depth, x, y, min_depth=0.0, mode="mask", seeds=(), keep_min_cells=0, fill=FILL):
    """The ocean mask of ``depth`` (ny x nx cells of a topography result) on the supergrid x, y ((2 ny + 1) x (2 nx + 1) points for
    model cells, (ny + 1) x (nx + 1) for supergrid cells), on one GPU through the host-pointer entry.  seeds: (lon, lat) pairs (model
    cells only).  A dict: depth (edited), wet (uint8), root (int32, before the selection, -1 for land), summary."""
    d = L.as_f64(depth)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if d.ndim != 2 or x.ndim != 2 or y.shape != x.shape:
        raise ValueError("ocean mask: depth %s, x %s and y %s must be 2-D (x and y of one shape)" % (d.shape, x.shape, y.shape))
    ny, nx = d.shape
    stride = _stride(d.shape, x.shape)
    s = _seeds(seeds)
    if s.shape[0] and stride != 2:
        raise ValueError("ocean mask: seeds need model cells (a seed picks the cell whose centre, supergrid point (2j+1, 2i+1), is nearest)")
    periodic, fold = detect_topology(x, y, stride)
    p = params(ny, nx, periodic, fold, min_depth, mode, keep_min_cells, fill)
    xc, yc = (np.ascontiguousarray(x), np.ascontiguousarray(y)) if s.shape[0] else (None, None)
    out = np.empty_like(d)
    wet = np.empty(d.shape, dtype=np.uint8)
    root = np.empty(d.shape, dtype=np.int32)
    cells = np.zeros(max(s.shape[0], 1), dtype=np.int64)
    cap = d.size
    comps = np.zeros(cap, dtype=np.int64)
    counts = L.MaskCounts()
    L.call("ogg_ocean_mask", ctypes.byref(p), d.ctypes.data, L.ptr(xc), L.ptr(yc), int(s.shape[0]), s.ctypes.data if s.shape[0] else None,
           out.ctypes.data, wet.ctypes.data, root.ctypes.data, cells.ctypes.data, comps.ctypes.data, cap, ctypes.byref(counts))
    cdict = L.counts_dict(L.MASK_COUNT_FIELDS, counts)
    comps = comps[:cdict["components"]]
    kept = _kept_roots(root, cells[:s.shape[0]], cdict, s.shape[0])
    return result(out, wet, root, cdict, comps, kept, cells[:s.shape[0]], s, x, y, stride, periodic, fold, min_depth, mode, keep_min_cells)


def _kept_roots(root, seed_cells, counts, n_seeds):
    """the roots kept by the seeds, or without seeds the largest component's root (the choice ogg_ocean_mask makes too)"""
    if n_seeds:
        return sorted(set(int(root.flat[int(c)]) for c in seed_cells))
    if counts["components"]:
        return [int(np.iinfo(np.int32).max - (counts["largest"] & 0xFFFFFFFF))]
    return []


# ---- device arrays ---------------------------------------------------------------------------------------------
def ocean_mask_dev(depth, x, y, min_depth=0.0, mode="mask", seeds=(), keep_min_cells=0, fill=FILL):
    """ocean_mask() on device tensors: depth (ny x nx float64) and the supergrid x, y (float64, contiguous rows) on one GPU.  The
    label step, the seed lookup and the apply step run on the device; the host reads the counts, the seeds' cells and roots, and the
    component list, and chooses the kept roots.  The kernels run on the device's current stream.  The same dict as ocean_mask(), with
    host arrays."""
    import torch
    dev = depth.device
    depth = depth.contiguous()
    x, y = x.contiguous(), y.contiguous()
    ny, nx = depth.shape
    stride = _stride(tuple(depth.shape), tuple(x.shape))
    s = _seeds(seeds)
    if s.shape[0] and stride != 2:
        raise ValueError("ocean mask: seeds need model cells (a seed picks the cell whose centre, supergrid point (2j+1, 2i+1), is nearest)")
    periodic, fold = topology_of_device_grid(x, y, stride)
    p = params(ny, nx, periodic, fold, min_depth, mode, keep_min_cells, fill)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = L.load()
    wsb = int(lib.ogg_mask_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    root = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    comps = torch.empty(ny * nx, dtype=torch.int64, device=dev)
    counts = torch.zeros(len(L.MASK_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_mask_label_dev", ctypes.byref(p), depth.data_ptr(), ws.data_ptr(), wsb, root.data_ptr(), comps.data_ptr(),
           counts.data_ptr(), st)
    cells = np.zeros(0, dtype=np.int64)
    if s.shape[0]:
        ll = torch.from_numpy(s).to(dev)
        so = torch.empty(2 * s.shape[0], dtype=torch.int64, device=dev)
        L.call("ogg_mask_seed_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), x.shape[1], int(s.shape[0]), ll.data_ptr(), so.data_ptr(), st)
        cells = so.cpu().numpy()[1::2].copy()
    cdict = L.counts_dict(L.MASK_COUNT_FIELDS, counts)
    seed_roots = root.view(-1)[torch.from_numpy(cells).to(dev)].cpu().numpy() if cells.size else np.zeros(0, np.int32)
    for k in range(cells.size):
        if seed_roots[k] < 0:
            j, i = divmod(int(cells[k]), nx)
            raise ValueError("ocean mask: seed %d (%g, %g) lies on land: cell (j, i) = (%d, %d) has depth %.17g"
                             % (k, s[k, 0], s[k, 1], j, i, float(depth[j, i])))
    kept = sorted(set(int(r) for r in seed_roots)) if cells.size else _kept_roots(None, (), cdict, 0)
    kt = torch.tensor(kept if kept else [0], dtype=torch.int32, device=dev)
    out = torch.empty_like(depth)
    wet = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
    L.call("ogg_mask_apply_dev", ctypes.byref(p), depth.data_ptr(), root.data_ptr(), ws.data_ptr(), wsb, kt.data_ptr(), len(kept),
           out.data_ptr(), wet.data_ptr(), counts.data_ptr(), st)
    cdict = L.counts_dict(L.MASK_COUNT_FIELDS, counts)
    comp = np.sort(comps[:cdict["components"]].cpu().numpy())[::-1]
    return result(out.cpu().numpy(), wet.cpu().numpy(), root.cpu().numpy(), cdict, comp, kept, cells, s, x, y, stride, periodic, fold,
                  min_depth, mode, keep_min_cells)


# ---- topog.nc --------------------------------------------------------------------------------------------------
def edit_topog(topo, res):
    """the topography result with the edited depth, and the depth as sampled in depth_sampled (written after the other variables)"""
    out = dict(topo)
    out["depth_sampled"] = topo["depth"]
    out["depth"] = res["depth"]
    return out


def read_topog(path):
    """A topography result from a topog.nc that topography.write_topog wrote: its variables and the summary entries write_topog needs."""
    h = netcdf3.read_header(path)
    out = {}
    for name, v in h.vars.items():
        a = np.frombuffer(netcdf3.read_var_bytes(path, h, name, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type])
        out[name] = a.astype(a.dtype.newbyteorder("=")).reshape(v.shape)
    if "depth" not in out:
        raise KeyError("%s: no variable depth" % path)
    g = h.gatts
    num = lambda k, d: float(np.asarray(g[k]).reshape(-1)[0]) if k in g and not isinstance(g[k], str) else d   # noqa: E731
    cells = "model" if str(g.get("cells", "MOM6 model")).startswith("MOM6 model") else "supergrid"
    out["summary"] = {"cells": cells, "quantum": num("quantum", 1.0), "sea_level": num("sea_level", 0.0),
                      "oversample": num("oversample", 2.0), "refine": int(num("refine", 0)) or None}
    fv = h.vars["depth"].atts.get("_FillValue")
    out["fill"] = FILL if fv is None or isinstance(fv, str) else float(np.asarray(fv).reshape(-1)[0])
    return out


def write_mask(path, res):
    """the final wet mask (NetCDF 64-bit offset): dims (ny, nx), variable mask, double, 1 wet and 0 land"""
    ny, nx = res["wet"].shape
    s = res["summary"]
    ds = netcdf3.Dataset(path, [("ny", ny), ("nx", nx)], global_atts=[
        ("title", "ocean mask: minimum depth and connected basins"),
        ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells" if s["cells"] == "model" else "supergrid cells"),
        ("min_depth", float(s["min_depth"])), ("mode", s["mode"]), ("keep_min_cells", int(s["keep_min_cells"])),
        ("periodic", int(s["periodic"])), ("fold", int(s["fold"]))])
    ds.def_var("mask", netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", "1"), ("long_name", "ocean mask: 1 wet, 0 land")],
               res["wet"].astype(np.float64))
    ds.write()


def summary_lines(res):
    s = res["summary"]
    topo = ", ".join([t for t, f in (("periodic", s["periodic"]), ("folded", s["fold"])) if f]) or "neither periodic nor folded"
    rule = ("%d cells shallower than %g m made land" % (s["masked"], s["min_depth"]) if s["mode"] == "mask"
            else "%d cells deepened to %g m" % (s["deepened"], s["min_depth"]))
    lines = ["   ocean mask: %d wet cells (%s); %s; %d connected basins, %d kept (%s); %d cells in %d basins removed; %d wet cells remain"
             % (s["wet_in"], topo, rule, s["components"], s["kept"], "%d seeds" % len(s["seeds"]) if s["seeds"] else "the largest",
                s["removed"], s["removed_components"], s["wet_out"])]
    for b in s["removed_largest"]:
        lines.append("   ocean mask: removed a basin of %d cells at lon %.4f, lat %.4f (cell j=%d, i=%d)" % (b["cells"], b["lon"], b["lat"],
                                                                                                         b["j"], b["i"]))
    return lines


def main(argv=None):
    from . import topography as T
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.ocean_mask",
                                description="minimum depth and connected basins of a topog.nc on its supergrid")
    p.add_argument("topog", help="topog.nc (as the topography step writes it)")
    p.add_argument("--grid", required=True, help="ocean_hgrid.nc the topography was sampled on")
    p.add_argument("--min_depth", type=float, default=0.0, help="wet cells shallower than this become land (or are deepened)")
    p.add_argument("--deepen", action="store_true", help="deepen cells shallower than --min_depth instead of making them land")
    p.add_argument("--seed", type=float, nargs=2, action="append", default=[], metavar=("LON", "LAT"),
                   help="a point in the open ocean: every basin holding a seed is kept (default: the largest basin)")
    p.add_argument("--keep_min_cells", type=int, default=0, help="also keep every basin of at least N cells")
    p.add_argument("-o", "--output", default="topog_edited.nc")
    p.add_argument("--mask", default=None, help="also write the mask (1 wet, 0 land) to this file")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    topo = read_topog(a.topog)
    g = netcdf3.read_doubles(a.grid, names=("x", "y"))
    res = ocean_mask(topo["depth"], g["x"], g["y"], min_depth=a.min_depth, mode="deepen" if a.deepen else "mask",
                     seeds=[tuple(s) for s in a.seed], keep_min_cells=a.keep_min_cells, fill=topo["fill"])
    for line in summary_lines(res):
        print(line)
    T.write_topog(a.output, edit_topog(topo, res))
    if a.mask:
        write_mask(a.mask, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

"""Sill depths: at what depth every wet model cell is connected to a seed (the open ocean), in which region of equal sill depth it
lies, and which face is the gate of each region.  include/ogg_hip.h, "Sill depths", gives the definition; the reference has no such
step.  It answers in one field what otherwise takes one ocean mask per candidate depth: at what depth is the Mediterranean connected
to the Atlantic on THIS grid, and where does the cell-mean topography close a strait that the raster has open?

The search runs on the device (ogg_sill_depth_dev, or the host-pointer ogg_sill_depth) over integer face weights, bit by bit on the
ocean mask's union-find; every output is an integer, so every path, knob and rank count writes the same bytes.  Two ways to weigh a
face: ``cells``, the smaller depth of its two cells (what a model without porous barriers sees), and ``faces``, the sill of the face
topography (what the raster says is there; a cell's sill can then exceed its own mean depth).  Connections go through faces only; a
channel one cell wide counts as open; the result is relative to the chosen seeds.

    python -m ocean_model_grid_generator_amd.sill_depth ocean_hgrid.nc (--topog topog.nc | --mask ocean_mask.nc --topog topog.nc)
        [--faces topog_faces.nc] [--weights cells|faces] [--seed LON LAT]... [--quantum Q] [--min_cells N] -o sill_depth.nc
        [--report basins.json]
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

FILL = 1.0e20
Q_MAX = (1 << 30) - 1
WEIGHTS = ("cells", "faces")
MIN_CELLS = 16         # regions smaller than this are not basins (on a plain slope every cell is its own region)
N_LISTED = 10          # basins printed by summary_lines (largest first)
N_GATES = 8            # gates listed per basin
REACH_LAND, REACH_CONNECTED, REACH_SEED, REACH_CUT_OFF = 0, 1, 2, 3


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, periodic, fold, bits, n_seeds, tile_rows=0):
    """the six scalars every ogg_sill_* entry takes first (ny, nx, topology, bits, n_seeds, tile_rows), checked by the library
    (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    p = (int(ny), int(nx), M.topology_flags(periodic, fold), int(bits), int(n_seeds), int(tile_rows))
    lib = L.load()
    if lib.ogg_sill_check(*p) != L.OGG_OK:
        raise ValueError(lib.ogg_last_error().decode())
    return p


def bits_for(top):
    """the smallest bits (1 .. 30) that holds the weight ``top``"""
    return min(max(int(top).bit_length(), 1), L.SILL_MAX_BITS)


def _face_shapes(wu, wv):
    if wu.ndim != 2 or wv.ndim != 2 or wu.shape[1] < 2 or wv.shape != (wu.shape[0] + 1, wu.shape[1] - 1):
        raise ValueError("sill depth: wu %s and wv %s must be (ny, nx + 1) and (ny + 1, nx)" % (tuple(wu.shape), tuple(wv.shape)))
    return wu.shape[0], wu.shape[1] - 1


def _seed_cells(seeds):
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
    if s.size < 1:
        raise ValueError("sill depth: at least one seed cell is needed")
    return s


# ---- integer weights and seed cells ------------------------------------------------------------------------------
def sill_depth_faces(wu, wv, seeds, periodic, fold, bits=None):
    """The sill depths of ny x nx cells from integer face weights wu (ny, nx + 1) and wv (ny + 1, nx) (numpy integer arrays, quanta,
    positive down) and seed cell indices, on one GPU through the host-pointer entry.  bits: None takes the smallest value that holds
    the largest weight.  A dict: b, region (int32), gate_u, gate_v (uint8), counts, bits."""
    wu, wv = np.asarray(wu), np.asarray(wv)
    if wu.dtype.kind not in "iu" or wv.dtype.kind not in "iu":
        raise ValueError("sill depth: the face weights must be integer arrays (%s, %s)" % (wu.dtype, wv.dtype))
    ny, nx = _face_shapes(wu, wv)
    if bits is None:
        bits = bits_for(max(int(np.max(wu, initial=0)), int(np.max(wv, initial=0))))
    s = _seed_cells(seeds)
    p = params(ny, nx, periodic, fold, bits, s.size)
    # (a weight outside int32 is clamped either way: -1 and 2^30 stand for every such value and are counted as it would be)
    u32, v32 = (np.ascontiguousarray(np.clip(w, -1, 1 << 30), dtype=np.int32) for w in (wu, wv))
    b = np.empty((ny, nx), np.int32)
    region = np.empty((ny, nx), np.int32)
    gu = np.empty((ny, nx + 1), np.uint8)
    gv = np.empty((ny + 1, nx), np.uint8)
    c = np.zeros(len(L.SILL_COUNT_FIELDS), dtype=np.int64)
    L.call("ogg_sill_depth", *p, u32.ctypes.data, v32.ctypes.data, s.ctypes.data, b.ctypes.data, region.ctypes.data, gu.ctypes.data,
           gv.ctypes.data, c.ctypes.data)
    return {"b": b, "region": region, "gate_u": gu, "gate_v": gv, "counts": L.counts_dict(L.SILL_COUNT_FIELDS, c), "bits": int(bits)}


def sill_depth_faces_dev(wu, wv, seeds, periodic, fold, bits=None):
    """sill_depth_faces() on device tensors: wu, wv integer tensors and seeds an int64 tensor (or a sequence) of cell indices, on the
    device's current stream.  The same dict with device tensors (the counts are read back)."""
    import torch
    dev = wu.device
    if wu.dtype.is_floating_point or wv.dtype.is_floating_point:
        raise ValueError("sill depth: the face weights must be integer tensors (%s, %s)" % (wu.dtype, wv.dtype))
    ny, nx = _face_shapes(wu, wv)
    if bits is None:
        bits = bits_for(max(int(wu.max()), int(wv.max()), 0))
    s = seeds.to(torch.int64).reshape(-1).contiguous() if hasattr(seeds, "data_ptr") else torch.from_numpy(_seed_cells(seeds)).to(dev)
    if s.numel() < 1:
        raise ValueError("sill depth: at least one seed cell is needed")
    p = params(ny, nx, periodic, fold, bits, s.numel())
    u32, v32 = (w.clamp(-1, 1 << 30).to(torch.int32).contiguous() for w in (wu, wv))
    wsb = int(L.load().ogg_sill_workspace_bytes(ny, nx))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    b = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    region = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    gu = torch.empty((ny, nx + 1), dtype=torch.uint8, device=dev)
    gv = torch.empty((ny + 1, nx), dtype=torch.uint8, device=dev)
    counts = torch.empty(len(L.SILL_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_sill_depth_dev", *p, u32.data_ptr(), v32.data_ptr(), s.data_ptr(), ws.data_ptr(), wsb, b.data_ptr(),
           region.data_ptr(), gu.data_ptr(), gv.data_ptr(), counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return {"b": b, "region": region, "gate_u": gu, "gate_v": gv, "counts": L.counts_dict(L.SILL_COUNT_FIELDS, counts), "bits": int(bits)}


# ---- weights from depths -----------------------------------------------------------------------------------------
def quantise(d, quantum):
    """q(d) = clip(rint(d / quantum), 0, 2^30 - 1) as int64, 0 for a non-finite d or the 1e20 fill (numpy arrays or device tensors)"""
    if hasattr(d, "data_ptr"):
        import torch
        ok = torch.isfinite(d) & (d != FILL)
        q = torch.clamp(torch.round(torch.where(ok, d, torch.zeros_like(d)) / quantum), 0, Q_MAX)
        return torch.where(ok, q, torch.zeros_like(q)).to(torch.int64)
    d = np.asarray(d, dtype=np.float64)
    ok = np.isfinite(d) & (d != FILL)
    with np.errstate(over="ignore"):
        q = np.clip(np.rint(np.where(ok, d, 0.0) / quantum), 0, Q_MAX)
    return np.where(ok, q, 0).astype(np.int64)


def _zeros(like, shape):
    if hasattr(like, "data_ptr"):
        import torch
        return torch.zeros(shape, dtype=torch.int64, device=like.device)
    return np.zeros(shape, dtype=np.int64)


def _minimum(a, b):
    if hasattr(a, "data_ptr"):
        import torch
        return torch.minimum(a, b)
    return np.minimum(a, b)


def _flip(a):
    return a.flip(-1) if hasattr(a, "data_ptr") else a[..., ::-1]


def cell_face_weights(q, periodic, fold):
    """``cells``: the weight of a face is the smaller q of its two cells (q: int64, 0 where not wet); the seam's and the fold's faces
    take the cell across; a face with one side only holds 0"""
    ny, nx = q.shape
    wu, wv = _zeros(q, (ny, nx + 1)), _zeros(q, (ny + 1, nx))
    wu[:, 1:nx] = _minimum(q[:, :-1], q[:, 1:])
    wv[1:ny] = _minimum(q[:-1], q[1:])
    if periodic:
        wu[:, 0] = _minimum(q[:, -1], q[:, 0])
        wu[:, nx] = wu[:, 0]
    if fold:
        wv[ny] = _minimum(q[-1], _flip(q[-1]))
    return wu, wv


def raster_face_weights(fu, fv, wetq, periodic, fold, quantum):
    """``faces``: q(depth_max) of the face topography (fu (ny, nx + 1), fv (ny + 1, nx); 1e20 where the face has no line), 0 next to
    a cell that is not wet (wetq: int64, non-zero where wet)"""
    one = (wetq != 0).to(wetq.dtype) if hasattr(wetq, "data_ptr") else (wetq != 0).astype(np.int64)
    ou, ov = cell_face_weights(one, periodic, fold)
    return quantise(fu, quantum) * ou, quantise(fv, quantum) * ov


def _lookup_seeds(x, y, seeds, ny, nx, periodic, fold):
    """the cells of (lon, lat) seeds by the ocean mask's seed lookup (ogg_mask_seed_dev); x, y numpy arrays or device tensors"""
    import torch
    from . import ocean_mask as M
    s = M._seeds(seeds)
    if not hasattr(x, "data_ptr"):
        dev = torch.device("cuda", torch.cuda.current_device())
        x, y = torch.from_numpy(L.as_f64(x)).to(dev), torch.from_numpy(L.as_f64(y)).to(dev)
    x, y = x.contiguous(), y.contiguous()
    p = M.params(ny, nx, periodic, fold)
    ll = torch.from_numpy(s).to(x.device)
    so = torch.empty(2 * s.shape[0], dtype=torch.int64, device=x.device)
    L.call("ogg_mask_seed_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), x.shape[1], int(s.shape[0]), ll.data_ptr(), so.data_ptr(),
           torch.cuda.current_stream(x.device).cuda_stream)
    return s, so.cpu().numpy()[1::2].copy()


def default_seed(q):
    """the wet cell with the largest q (q: int64 numpy, 0 where not wet), the smallest index among ties"""
    flat = q.reshape(-1)
    if flat.size == 0 or int(flat.max()) <= 0:
        raise ValueError("sill depth: no wet cell with a positive depth to seed from")
    return int(np.argmax(flat))   # the first of the largest


def _check(depth_shape, x_shape, weights, faces, quantum, min_cells):
    if weights not in WEIGHTS:
        raise ValueError("sill depth: weights must be 'cells' or 'faces', not %r" % (weights,))
    if weights == "faces" and faces is None:
        raise ValueError("sill depth: weights='faces' needs the face topography (faces=)")
    if not (np.isfinite(quantum) and quantum > 0.0):
        raise ValueError("sill depth: quantum must be > 0 (%r)" % (quantum,))
    if int(min_cells) < 1:
        raise ValueError("sill depth: min_cells must be >= 1 (%r)" % (min_cells,))
    if len(depth_shape) != 2 or tuple(x_shape) != (2 * depth_shape[0] + 1, 2 * depth_shape[1] + 1):
        raise ValueError("sill depth: depth %s needs a supergrid of %s points, not %s"
                         % (tuple(depth_shape), (2 * depth_shape[0] + 1, 2 * depth_shape[1] + 1) if len(depth_shape) == 2 else "?",
                            tuple(x_shape)))


def _face_fields(faces, shape, to):
    ny, nx = shape
    fu, fv = faces["u"]["depth_max"], faces["v"]["depth_max"]
    if tuple(fu.shape) != (ny, nx + 1) or tuple(fv.shape) != (ny + 1, nx):
        raise ValueError("sill depth: the face topography (%s, %s) does not belong to %d x %d cells" % (tuple(fu.shape), tuple(fv.shape), ny, nx))
    return to(fu), to(fv)


# ---- the result ------------------------------------------------------------------------------------------------
def _gates(region, gu, gv, periodic, fold):
    """every gate once: arrays kind (0 u, 1 v), j, i, the enclosed cell and the cell on the far side"""
    ny, nx = region.shape
    out = []
    j, i = np.nonzero(gu[:, :nx])                    # column nx repeats column 0
    a = j * nx + np.where(i > 0, i - 1, nx - 1)
    b = j * nx + i
    out.append((np.zeros(j.size, np.int64), j, i, gu[j, i], a, b))
    j, i = np.nonzero(gv)
    keep = (j < ny) | (i < nx - 1 - i)               # the fold's faces i > nx - 1 - i repeat their partners
    j, i = j[keep], i[keep]
    a = np.where(j < ny, (j - 1) * nx + i, (ny - 1) * nx + i)
    b = np.where(j < ny, j * nx + i, (ny - 1) * nx + nx - 1 - i)
    out.append((np.ones(j.size, np.int64), j, i, gv[j, i], a, b))
    kind, j, i, code, a, b = (np.concatenate(c) for c in zip(*out))
    inside = np.where(code == 1, a, b)
    return kind, j, i, inside, np.where(code == 1, b, a)


def basin_list(b, region, gu, gv, q, quantum, x, y, periodic, fold, area=None, min_cells=MIN_CELLS):
    """The regions with 0 < b < SEED of at least min_cells cells, sorted by cells (largest first, then by region): sill depth, cells,
    area, deepest cell, gates (at most N_GATES listed, n_gates in all) and the region behind each gate."""
    ny, nx = b.shape
    bf, rf = b.reshape(-1), region.reshape(-1)
    sel = (bf > 0) & (bf < L.SILL_SEED)
    ids, cells = np.unique(rf[sel], return_counts=True)
    big = cells >= int(min_cells)
    ids, cells = ids[big], cells[big]
    order = np.lexsort((ids, -cells))
    ids, cells = ids[order], cells[order]
    kind, gj, gi, inside, far = _gates(region, gu, gv, periodic, fold)
    greg = rf[inside]
    qf = q.reshape(-1)
    af = None if area is None else np.asarray(area, dtype=np.float64).reshape(-1)
    out = []
    for r, n in zip(ids, cells):
        members = np.nonzero(rf == r)[0]
        deep = int(members[np.argmax(qf[members])])
        gates = []
        mine = np.nonzero(greg == r)[0]
        for g in mine[:N_GATES]:
            k = (2 * int(gj[g]) + 1, 2 * int(gi[g])) if kind[g] == 0 else (2 * int(gj[g]), 2 * int(gi[g]) + 1)
            lon, lat = float(x[k]), float(y[k])
            gates.append({"face": "uv"[int(kind[g])], "j": int(gj[g]), "i": int(gi[g]), "lon": lon if np.isfinite(lon) else None,
                          "lat": lat if np.isfinite(lat) else None, "behind_region": int(rf[far[g]]),
                          "behind_sill_depth": None if bf[far[g]] == L.SILL_SEED else float(bf[far[g]] * quantum)})
        out.append({"region": int(r), "sill_depth": float(int(bf[r]) * quantum), "cells": int(n),
                    "area_m2": None if af is None else float(np.sum(af[members])),
                    "deepest_cell": {"j": deep // nx, "i": deep % nx, "depth": float(int(qf[deep]) * quantum)},
                    "n_gates": int(mine.size), "gates": gates})
    return out


def result(raw, q, wet, seed_cells, seeds, x, y, periodic, fold, quantum, weights, area=None, min_cells=MIN_CELLS):
    """What sill_depth() returns: sill_depth (double, b * quantum; 1e20 where b = 0; the cell's own depth at a seed), reach (uint8: 0
    not wet, 1 connected, 2 seed, 3 wet but cut off), region, gate_u, gate_v, b, counts, basins and a summary.  q: int64 q(depth) of
    the wet cells, 0 elsewhere.  x, y: the supergrid points, numpy arrays or device tensors (only the gates' points are read)."""
    b, region = raw["b"], raw["region"]
    ny, nx = b.shape
    sd = np.where(b == 0, FILL, b.astype(np.float64) * quantum)
    sd = np.where(b == L.SILL_SEED, q.astype(np.float64) * quantum, sd)
    reach = np.where(b == L.SILL_SEED, REACH_SEED, np.where(b > 0, REACH_CONNECTED, np.where(wet != 0, REACH_CUT_OFF, REACH_LAND)))
    basins = basin_list(b, region, raw["gate_u"], raw["gate_v"], q, quantum, x, y, periodic, fold, area, min_cells)
    summary = dict(raw["counts"], shape=[ny, nx], periodic=bool(periodic), fold=bool(fold), quantum=float(quantum), weights=weights,
                   bits=int(raw["bits"]), min_cells=int(min_cells), n_basins=len(basins),
                   seeds=[{"lon": None if s is None else float(s[0]), "lat": None if s is None else float(s[1]), "cell": int(c),
                           "j": int(c) // nx, "i": int(c) % nx} for s, c in zip(seeds, seed_cells)])
    return {"sill_depth": sd, "reach": reach.astype(np.uint8), "region": region, "gate_u": raw["gate_u"], "gate_v": raw["gate_v"], "b": b,
            "counts": raw["counts"], "basins": basins, "summary": summary}


def _resolve_seeds(seeds, x, y, q_host, ny, nx, periodic, fold):
    if len(seeds) == 0:
        return [None], np.array([default_seed(q_host)], dtype=np.int64)
    s, cells = _lookup_seeds(x, y, seeds, ny, nx, periodic, fold)
    for k, c in enumerate(cells):
        if not 0 <= c < ny * nx:
            raise ValueError("sill depth: seed %d (%g, %g) found no cell centre" % (k, s[k, 0], s[k, 1]))
        if q_host.reshape(-1)[c] <= 0:
            raise ValueError("sill depth: seed %d (%g, %g) lies on land: cell (j, i) = (%d, %d)" % (k, s[k, 0], s[k, 1], c // nx, c % nx))
    return list(s), cells


# ---- host arrays -----------------------------------------------------------------------------------------------
def sill_depth(depth, x, y, wet=None, faces=None, seeds=(), quantum=0.01, weights="cells", area=None, min_cells=MIN_CELLS):
    """The sill depths of the model cells of a stitched supergrid x, y ((2 ny + 1) x (2 nx + 1), degrees) with cell depths ``depth``
    (ny, nx; metres, positive down), on one GPU.  wet: one value per model cell (0: land), None: the cells with q(depth) > 0.  faces:
    a face_topography() result, needed by weights='faces'.  seeds: (lon, lat) pairs, resolved with the ocean mask's seed lookup;
    without one, the wet cell with the largest q(depth).  area: None or the model-cell areas, for the basins' areas.  A dict: see
    result()."""
    from . import ocean_mask as M
    d = L.as_f64(depth)
    x, y = L.as_f64(x), L.as_f64(y)
    _check(d.shape, x.shape, weights, faces, quantum, min_cells)
    ny, nx = d.shape
    q = quantise(d, quantum)
    m = (q > 0).astype(np.uint8) if wet is None else F.wet_mask(wet, d.shape, "sill depth")
    q = np.where(m != 0, q, 0)
    periodic, fold = M.detect_topology(x, y, 2)
    if weights == "cells":
        wu, wv = cell_face_weights(q, periodic, fold)
    else:
        fu, fv = _face_fields(faces, d.shape, L.as_f64)
        wu, wv = raster_face_weights(fu, fv, q, periodic, fold, quantum)
    named, cells = _resolve_seeds(seeds, x, y, q, ny, nx, periodic, fold)
    raw = sill_depth_faces(wu, wv, cells, periodic, fold, bits_for(max(int(wu.max(initial=0)), int(wv.max(initial=0)))))
    return result(raw, q, m, cells, named, x, y, periodic, fold, quantum, weights, area, min_cells)


# ---- device arrays ---------------------------------------------------------------------------------------------
def sill_depth_dev(depth, x, y, wet=None, faces=None, seeds=(), quantum=0.01, weights="cells", area=None, min_cells=MIN_CELLS):
    """sill_depth() with depth (ny x nx float64) and the supergrid x, y as device tensors: the weights are formed, and the search
    runs, on the device's current stream.  faces: a face_topography result (host arrays or device tensors).  The same dict as
    sill_depth(), with host arrays."""
    import torch
    from . import ocean_mask as M
    dev = depth.device
    d = depth.to(torch.float64).contiguous()
    _check(tuple(d.shape), tuple(x.shape), weights, faces, quantum, min_cells)
    ny, nx = d.shape
    q = quantise(d, quantum)
    if wet is None:
        m = (q > 0).to(torch.uint8)
    else:
        m = torch.from_numpy(F.wet_mask(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, (ny, nx), "sill depth")).to(dev)
    q = torch.where(m != 0, q, torch.zeros_like(q))
    periodic, fold = M.topology_of_device_grid(x, y)
    if weights == "cells":
        wu, wv = cell_face_weights(q, periodic, fold)
    else:
        to = lambda a: (a if hasattr(a, "data_ptr") else torch.from_numpy(L.as_f64(a))).to(dev, torch.float64)   # noqa: E731
        fu, fv = _face_fields(faces, (ny, nx), to)
        wu, wv = raster_face_weights(fu, fv, q, periodic, fold, quantum)
    qh = q.cpu().numpy()
    named, cells = _resolve_seeds(seeds, x, y, qh, ny, nx, periodic, fold)
    raw = sill_depth_faces_dev(wu, wv, cells, periodic, fold, bits_for(max(int(wu.max()), int(wv.max()), 0)))
    raw = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in raw.items()}
    if area is not None and hasattr(area, "cpu"):
        area = area.cpu().numpy()
    return result(raw, qh, m.cpu().numpy(), cells, named, x, y, periodic, fold, quantum, weights, area, min_cells)


# ---- files -----------------------------------------------------------------------------------------------------
def write_sill_depth(path, res, title="sill depths of the model cells"):
    """sill_depth (double, 1e20 where no connection), reach (byte), region and b (int), dims (ny, nx); gate_u (ny, nxp) and gate_v
    (nyp, nx) (byte), as a NetCDF 64-bit-offset file; quantum, weights, seeds and bits as global attributes"""
    ny, nx = res["b"].shape
    s = res["summary"]
    seeds = " ".join("%d" % k["cell"] if k["lon"] is None else "%r,%r" % (k["lon"], k["lat"]) for k in s["seeds"])
    ds = netcdf3.Dataset(path, [("ny", ny), ("nx", nx), ("nyp", ny + 1), ("nxp", nx + 1)], global_atts=[
        ("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells"), ("periodic", int(s["periodic"])),
        ("fold", int(s["fold"])), ("quantum", float(s["quantum"])), ("weights", s["weights"]), ("seeds", seeds), ("bits", int(s["bits"])),
        ("seed_cells", np.array([k["cell"] for k in s["seeds"]], dtype=np.int32))])
    ds.def_var("sill_depth", netcdf3.NC_DOUBLE, ("ny", "nx"),
               [("units", "m"), ("long_name", "deepest connection of the cell to a seed; its own depth at a seed"), ("_FillValue", FILL)],
               res["sill_depth"])
    ds.def_var("reach", netcdf3.NC_BYTE, ("ny", "nx"), [("long_name", "0 not wet, 1 connected, 2 seed, 3 wet but cut off")],
               res["reach"].astype(np.int8))
    ds.def_var("region", netcdf3.NC_INT, ("ny", "nx"),
               [("long_name", "smallest cell index of the cell's region of equal sill depth, -1 where there is no connection")], res["region"])
    ds.def_var("b", netcdf3.NC_INT, ("ny", "nx"), [("long_name", "sill depth in quanta; 2^30 at a seed")], res["b"])
    ds.def_var("gate_u", netcdf3.NC_BYTE, ("ny", "nxp"),
               [("long_name", "gate code of the u face: 1 the west cell is enclosed, 2 the east cell, 0 no gate")], res["gate_u"].astype(np.int8))
    ds.def_var("gate_v", netcdf3.NC_BYTE, ("nyp", "nx"),
               [("long_name", "gate code of the v face: 1 the south cell is enclosed, 2 the north cell, 0 no gate")], res["gate_v"].astype(np.int8))
    ds.write()


def summary_lines(res):
    s = res["summary"]
    topo = ", ".join([t for t, f in (("periodic", s["periodic"]), ("folded", s["fold"])) if f]) or "neither periodic nor folded"
    out = ["   sill depth: %d x %d cells (%s), %s weights of %g m in %d bits: %d seeds, %d cells connected, %d cut off, %d regions, "
           "%d gate faces, %d basins of at least %d cells"
           % (s["shape"][1], s["shape"][0], topo, s["weights"], s["quantum"], s["bits"], len(s["seeds"]), s["n_connected"], s["n_cut_off"],
              s["n_regions"], s["n_gate_faces"], s["n_basins"], s["min_cells"])]
    for k in res["basins"][:N_LISTED]:
        line = "   sill depth: sill %.2f m, %d cells" % (k["sill_depth"], k["cells"])
        for g in k["gates"][:1]:
            place = "an invalid point" if g["lon"] is None or g["lat"] is None else "%.4f, %.4f" % (g["lon"], g["lat"])
            line += ", gate %s(%d, %d) at %s, behind region %d" % (g["face"], g["j"], g["i"], place, g["behind_region"])
        if k["n_gates"] > 1:
            line += " (%d gates)" % k["n_gates"]
        out.append(line)
    return out


def write_report(path, res):
    with open(path, "w") as fh:
        json.dump({"summary": res["summary"], "basins": res["basins"]}, fh, indent=1)


def read_faces(path):
    """the sills of a topog_faces.nc as face_topography.write_topog_faces wrote it: {"u": {"depth_max"}, "v": {"depth_max"}}"""
    g = netcdf3.read_doubles(path, names=("depthu_max", "depthv_max"))
    return {"u": {"depth_max": g["depthu_max"]}, "v": {"depth_max": g["depthv_max"]}}


def main(argv=None):
    from . import ocean_mask as M
    from . import remap as R
    from . import runoff as RO
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.sill_depth",
                                description="sill depths of the model cells of a supergrid file: the deepest connection to a seed")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("--topog", required=True, help="topog.nc: the cell depths; without --mask, cells with depth > 0 are wet")
    p.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--faces", default=None, help="topog_faces.nc of the face topography (needed by --weights faces)")
    p.add_argument("--weights", choices=WEIGHTS, default="cells")
    p.add_argument("--seed", type=float, nargs=2, action="append", default=[], metavar=("LON", "LAT"),
                   help="a point in the open ocean (default: the deepest wet cell)")
    p.add_argument("--quantum", type=float, default=0.01, help="metres per quantum of depth")
    p.add_argument("--min_cells", type=int, default=MIN_CELLS, help="regions smaller than this are not listed as basins")
    p.add_argument("-o", "--output", default="sill_depth.nc")
    p.add_argument("--report", default=None, help="write the summary and the basin list as JSON to this file")
    a = p.parse_args(argv)
    if a.weights == "faces" and not a.faces:
        p.error("--weights faces needs --faces")
    h = netcdf3.read_header(a.grid)
    grid = netcdf3.read_doubles(a.grid, names=("x", "y") + (("area",) if "area" in h.vars else ()))
    topo = M.read_topog(a.topog)
    res = sill_depth(topo["depth"], grid["x"], grid["y"], wet=R.mask_from_file(a.mask or a.topog), faces=read_faces(a.faces) if a.faces else None,
                     seeds=[tuple(s) for s in a.seed], quantum=a.quantum, weights=a.weights,
                     area=RO.cell_area(grid["area"]) if "area" in grid else None, min_cells=a.min_cells)
    for line in summary_lines(res):
        print(line)
    write_sill_depth(a.output, res)
    if a.report:
        write_report(a.report, res)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)

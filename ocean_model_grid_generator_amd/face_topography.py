"""Face topography: what lies between two neighbouring model cells, for MOM6's sub-grid topography at velocity points (include/ogg_hip.h,
"Face topography", gives the definition).  The reference has no such step.

Every u and v face of the model grid gets one integer record from the device (ogg_topog_faces_dev / ogg_topog_faces): the block of
supergrid cells on either side of the face is sampled as the topography samples them, every line of samples that crosses the face
along the grid's own coordinate keeps its highest point (its ridge), and the record holds the lowest ridge (the sill: the deepest way
through the face), the highest, their sum and how many lines are dry.  The floating outputs are a fixed function of those integers.

It is not Adcroft's thin-wall coarsening: the lines follow the grid, and a passage that runs diagonally through the block is not found.
One lat-lon source only; the faces are not edited by the ocean mask.
"""
import ctypes

import numpy as np

from . import _lib as L
from . import netcdf3
from . import topography as T

NO_FACES = ("face topography (--topog_faces_file, --faces) follows lines of samples in one lat-lon raster: it is not made from a list of "
            "sources or from a projected source")
FILL = T.FILL
INT_MAX, INT_MIN = int(np.iinfo(np.int32).max), int(np.iinfo(np.int32).min)
FAMILIES = ("u", "v")


def single_source(source, **kw):
    """the one lat-lon Source the faces are sampled from; a list or a projected source is refused"""
    src = T.as_sources(source, **kw)
    if isinstance(src, T.SourceList):
        raise ValueError(NO_FACES)
    return src


def topology_flags(topology):
    """OGG_MASK_PERIODIC | OGG_MASK_FOLD of ``topology``: the flags themselves, or a (periodic, fold) pair"""
    if isinstance(topology, (tuple, list)):
        from . import ocean_mask as M
        return M.topology_flags(*topology)
    return int(topology)


class FaceParams(object):
    """The leading arguments of the ogg_topog_faces* entries: the whole stitched grid as one TopogBand of model cells (``grid``), the row
    stride ``ld``, the topology flags and the two output row ranges.  points() sets the pointers of x and y; args() gives the arguments."""

    def __init__(self, ny, nx, ld, topology, refine, oversample, u_rows, v_rows):
        self.ny, self.nx, self.ld, self.topology = int(ny), int(nx), int(ld), int(topology)
        (self.ju0, self.ju1), (self.jv0, self.jv1) = (int(v) for v in u_rows), (int(v) for v in v_rows)
        self.grid = L.TopogBand(nx=self.nx, j0=0, n_cell_rows=self.ny, cells=L.TOPOG_MODEL_CELLS, refine=int(refine or 0),
                                oversample=float(oversample))

    def points(self, x_ptr, y_ptr):
        self.grid.x, self.grid.y = x_ptr, y_ptr
        return self

    def args(self):
        return (ctypes.byref(self.grid), self.ld, self.topology, self.ju0, self.ju1, self.jv0, self.jv1)


def params(ny, nx, topology, refine=None, oversample=2.0, ld=None, u_rows=None, v_rows=None, desc=None, device=False):
    """FaceParams of ny x nx supergrid cells after the library's check took them (a refusal as a ValueError, before any device work);
    ``u_rows``, ``v_rows``: the (first, one past the last) output rows, default all; ``desc``: the source's descriptor."""
    nym = ny // 2
    if refine is not None and not 1 <= int(refine) <= L.TOPOG_MAX_REFINE:
        raise ValueError("face topography: refine must be 1 .. %d (%r)" % (L.TOPOG_MAX_REFINE, refine))
    p = FaceParams(ny, nx, nx + 1 if ld is None else ld, topology_flags(topology), refine, oversample,
                   (0, nym) if u_rows is None else u_rows, (0, nym + 1) if v_rows is None else v_rows)
    if desc is None:   # the grid's own refusals: any good source stands in
        desc = L.TopogSource(data=8, dtype=L.TOPOG_INT16, Nx=1, Ny=1, dlon=360.0, dlat=180.0, lon0=-180.0, lat0=-90.0, quantum=1.0)
    if L.load().ogg_topog_faces_check(*p.args(), ctypes.byref(desc), 1 if device else 0) != L.OGG_OK:
        raise ValueError(L.load().ogg_last_error().decode())
    return p


def empty_records(shape):
    return np.zeros(shape, dtype=L.TOPOG_FACE_RECORD)


# ---- the floating outputs ----------------------------------------------------------------------------------------
def fields_from_records(rec, quantum):
    """depth_max (the sill), depth_min, depth_ave, open_fraction as float64 with FILL where the face has no line, and n_lines, R, flag"""
    nl = rec["n_lines"].astype(np.int64)
    ok = nl > 0
    den = np.where(ok, nl, 1).astype(np.float64)
    q = float(quantum)
    out = {"depth_max": np.where(ok, -rec["lo"].astype(np.float64) * q, FILL),
           "depth_min": np.where(ok, -rec["hi"].astype(np.float64) * q, FILL),
           "depth_ave": np.where(ok, -(rec["ridge_sum"].astype(np.float64) / den) * q, FILL),
           "open_fraction": np.where(ok, 1.0 - rec["n_dry_lines"].astype(np.float64) / den, FILL),
           "n_lines": nl.astype(np.int32), "R": rec["R"].astype(np.int32), "flag": rec["flags"].astype(np.int8)}
    return out


def summary_of(rec):
    nl, dry = rec["n_lines"], rec["n_dry_lines"]
    return {"n_faces": int(rec.size), "n_one_sided": int(np.count_nonzero(rec["flags"] & L.FACE_ONE_SIDED)),
            "n_pole": int(np.count_nonzero(rec["flags"] & L.FACE_POLE)), "n_no_line": int(np.count_nonzero(nl == 0)),
            "n_closed": int(np.count_nonzero((nl > 0) & (dry == nl))), "n_partly_open": int(np.count_nonzero((dry > 0) & (dry < nl))),
            "n_samples": int(rec["n"].sum()) + int(rec["n_missing"].sum()), "n_valid_samples": int(rec["n"].sum()),
            "R_max": int(rec["R"].max()) if rec.size else 0, "n_clamped_cells": int(rec["n_clamped"].sum())}


def result(rec_u, rec_v, source, sea_level, refine, oversample, topology):
    """What face_topography() returns: {"u": fields and records, "v": the same, "summary"}"""
    out = {}
    for fam, rec in zip(FAMILIES, (rec_u, rec_v)):
        out[fam] = dict(fields_from_records(rec, source.quantum), records=rec)
    out["summary"] = {"u": summary_of(rec_u), "v": summary_of(rec_v), "quantum": float(source.quantum), "sea_level": float(sea_level),
                      "refine": None if refine is None else int(refine), "oversample": float(oversample),
                      "topology": int(topology_flags(topology)), "source": source.describe()}
    return out


def _check_grid(shape_x, shape_y):
    if len(shape_x) != 2 or tuple(shape_y) != tuple(shape_x):
        raise ValueError("face topography: x %s and y %s must be 2-D of one shape" % (tuple(shape_x), tuple(shape_y)))
    return shape_x[0] - 1, shape_x[1] - 1


# ---- host arrays -------------------------------------------------------------------------------------------------
def face_topography(x, y, source, lon0=None, dlon=None, lat0=None, dlat=None, refine=None, oversample=2.0, quantum=None, sea_level=0.0,
                    topology=None, fill=()):
    """Face topography of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees; ny and nx even) from one lat-lon raster (a Source,
    or an int16 / float32 / float64 array with its box), on one GPU (ogg_topog_faces).  ``topology``: OGG_MASK_PERIODIC | OGG_MASK_FOLD
    or a (periodic, fold) pair; None: detected as the ocean mask detects it.  {"u": {...}, "v": {...}, "summary": {...}}: per family
    depth_max (the sill), depth_min, depth_ave, open_fraction, n_lines, R, flag and the integer records; u on (nym, nxm + 1), v on
    (nym + 1, nxm)."""
    src = single_source(source, lon0=lon0, dlon=dlon, lat0=lat0, dlat=dlat, quantum=quantum, fill=fill)
    x, y = L.as_f64(x), L.as_f64(y)
    ny, nx = _check_grid(x.shape, y.shape)
    if topology is None:
        from . import ocean_mask as M
        topology = M.detect_topology(x, y)
    desc = src.descriptor(sea_level)
    p = params(ny, nx, topology, refine, oversample, desc=desc)
    p.points(L.ptr(x), L.ptr(y))
    rec_u, rec_v = empty_records((ny // 2, nx // 2 + 1)), empty_records((ny // 2 + 1, nx // 2))
    L.call("ogg_topog_faces", *p.args(), ctypes.byref(desc), rec_u.ctypes.data, rec_v.ctypes.data)
    return result(rec_u, rec_v, src, sea_level, refine, oversample, topology)


# ---- device arrays -----------------------------------------------------------------------------------------------
def records_dev(p, desc, stream, device):
    """ogg_topog_faces_dev on parameters and a source descriptor of device pointers: (u records, v records, workspace) as int64
    device tensors rows x faces x 7, not synchronised; only the rows of the parameters' ranges"""
    import torch
    words = L.TOPOG_FACE_WORDS
    nxm = p.nx // 2
    out_u = torch.empty((p.ju1 - p.ju0, nxm + 1, words), dtype=torch.int64, device=device)
    out_v = torch.empty((p.jv1 - p.jv0, nxm, words), dtype=torch.int64, device=device)
    ws_bytes = int(L.load().ogg_topog_workspace_bytes())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    L.call("ogg_topog_faces_dev", *p.args(), ctypes.byref(desc), ws.data_ptr(), ws_bytes, out_u.data_ptr(), out_v.data_ptr(), stream)
    return out_u, out_v, ws


def records_to_host(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(L.TOPOG_FACE_RECORD).reshape(t.shape[0], t.shape[1])


def face_topography_dev(x, y, source, refine=None, oversample=2.0, sea_level=None, topology=None, u_rows=None, v_rows=None):
    """face_topography() of device tensors x, y (float64, one shape; rows may be strided) and a topography.DeviceSource (or a Source,
    uploaded here): the same result.  ``sea_level``: None takes the DeviceSource's (0 for a Source).  ``u_rows``, ``v_rows``: only these
    output rows (the records and fields then hold those rows)."""
    import torch
    if isinstance(source, T.DeviceSourceList):
        raise ValueError(NO_FACES)
    dev = source if isinstance(source, T.DeviceSource) else T.DeviceSource(single_source(source), x.device, sea_level or 0.0)
    sea_level = dev.sea_level if sea_level is None else float(sea_level)
    if isinstance(dev.source, T.SourceList) or dev.source.projection is not None:
        raise ValueError(NO_FACES)
    ny, nx = _check_grid(tuple(x.shape), tuple(y.shape))
    if x.dtype != torch.float64 or y.dtype != torch.float64 or x.stride(1) != 1 or y.stride(1) != 1 or x.stride(0) != y.stride(0):
        x, y = x.to(torch.float64).contiguous(), y.to(torch.float64).contiguous()
    if topology is None:
        from . import ocean_mask as M
        topology = M.topology_of_device_grid(x, y)
    desc = L.TopogSource.from_buffer_copy(dev.desc)   # the uploaded raster with this call's sea level
    desc.wet_below = sea_level / dev.source.quantum
    p = params(ny, nx, topology, refine, oversample, ld=x.stride(0), u_rows=u_rows, v_rows=v_rows, desc=desc, device=True)
    p.points(x.data_ptr(), y.data_ptr())
    st = torch.cuda.current_stream(x.device).cuda_stream
    out_u, out_v, ws = records_dev(p, desc, st, x.device)
    torch.cuda.synchronize(x.device)
    return result(records_to_host(out_u), records_to_host(out_v), dev.source, sea_level, refine, oversample, topology)


# ---- files -------------------------------------------------------------------------------------------------------
_D = netcdf3.NC_DOUBLE
# file name pattern (%s: the family), key of the result, type, unit, long name (%s: the family)
_VARS = (("depth%s_max", "depth_max", _D, "m", "depth of the SILL of the %s face: the deepest of the grid-following lines across the face, "
          "each taken at its highest point (positive down, not clamped at zero)"),
         ("depth%s_min", "depth_min", _D, "m", "depth of the shallowest grid-following line across the %s face, taken at its highest point"),
         ("depth%s_ave", "depth_ave", _D, "m", "mean over the grid-following lines across the %s face of the depth at each line's highest "
          "point"),
         ("open_fraction_%s", "open_fraction", _D, "1", "fraction of the lines across the %s face whose highest point is below sea level"),
         ("n_lines_%s", "n_lines", netcdf3.NC_INT, "1", "number of lines across the %s face that have a sample with a value"),
         ("flag_%s", "flag", netcdf3.NC_BYTE, "1", "%s face: 1 one-sided, 2 a cell of the block encloses a pole (no lines), 4 periodic "
          "partner used, 8 fold partner used"))


def write_topog_faces(path, res):
    """topog_faces.nc (NetCDF 64-bit offset): dims ny, nx (model cells), nyq = ny + 1, nxq = nx + 1; the u set on (ny, nxq), the v set on
    (nyq, nx); depths as doubles with _FillValue where a face has no line.  The names are this file's own: MOM6's names for its
    velocity-point topography are parameters, and mapping them is left to the user."""
    nym, nxq = res["u"]["depth_max"].shape
    s = res["summary"]
    ds = netcdf3.Dataset(path, [("ny", nym), ("nx", nxq - 1), ("nyq", nym + 1), ("nxq", nxq)], global_atts=[
        ("title", "face topography: sill, shallowest and mean ridge depth of the grid-following lines across every u and v face"),
        ("caveat", "not a thin-wall coarsening: lines follow the grid, diagonal passages are not found; not edited by an ocean mask"),
        ("quantum", float(s["quantum"])), ("sea_level", float(s["sea_level"])), ("oversample", float(s["oversample"])),
        ("refine", int(s["refine"] or 0)), ("topology", int(s["topology"])), ("source", str(s["source"]))])
    for fam, dims in (("u", ("ny", "nxq")), ("v", ("nyq", "nx"))):
        for pattern, key, nctype, unit, long_name in _VARS:
            atts = [("units", unit), ("long_name", long_name % fam)] + ([("_FillValue", FILL)] if nctype == _D else [])
            ds.def_var(pattern % fam, nctype, dims, atts, res[fam][key])
    ds.write()


def summary_lines(res):
    lines = []
    for fam in FAMILIES:
        s, f = res["summary"][fam], res[fam]
        lines.append("   face topography: %d %s faces, %d samples (%d valid), R up to %d; %d one-sided, %d pole, %d without a line; "
                     "%d closed, %d partly open" % (s["n_faces"], fam, s["n_samples"], s["n_valid_samples"], s["R_max"], s["n_one_sided"],
                                                    s["n_pole"], s["n_no_line"], s["n_closed"], s["n_partly_open"]))
        ok = f["n_lines"] > 0
        if np.any(ok):
            gap = np.where(ok, f["depth_max"] - f["depth_ave"], -np.inf)
            j, i = np.unravel_index(int(np.argmax(gap)), gap.shape)
            lines.append("   face topography: largest sill-to-mean gap of the %s faces %.6g at j=%d, i=%d (sill %.6g, mean %.6g)"
                         % (fam, float(gap[j, i]), j, i, float(f["depth_max"][j, i]), float(f["depth_ave"][j, i])))
    return lines

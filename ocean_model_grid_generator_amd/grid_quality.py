"""Grid-quality report of a stitched supergrid: cell sizes, aspect ratio, corner non-orthogonality, smoothness and sub-grid seams
(include/ogg_hip.h, "Grid-quality report", gives the definitions).  The reference has no such check.

Every number comes from libogg_hip.so (ogg_grid_quality_band_dev / ogg_grid_quality): one record per band of the stitched grid, merged
here by (value, j, i) and integer sums -- no floating-point sum anywhere, so a report is bit-identical whatever the split into bands.

    python -m ocean_model_grid_generator_amd.grid_quality FILE [--json OUT] [--radius R]

checks an existing ocean_hgrid.nc (NetCDF classic CDF-1 or 64-bit-offset CDF-2, as the reference writes it) on one GPU.  A file
carries no sub-grid boundaries, so its report has the whole-grid section only.
"""
import argparse
import ctypes
import json
import math
import sys

import numpy as np

from . import _lib as L

DEFAULT_RE = 6371.0e3   # the reference's default radius (ocean_grid_generator._default_Re)


# ---- records -------------------------------------------------------------------------------------------------
def record_from_bytes(buf):
    """An ogg_grid_quality_result (bytes, or an int64 array of its bytes) as ([extremum tuple or None] * 12, [count] * 15); an
    extremum tuple is (value, j, i, lon, lat)."""
    r = L.QualityResult.from_buffer_copy(bytes(np.asarray(buf).tobytes()) if not isinstance(buf, (bytes, bytearray)) else buf)
    ext = [None if e.j < 0 else (e.value, int(e.j), int(e.i), e.lon, e.lat) for e in r.ext]
    return ext, [int(c) for c in r.count]


def _better(is_min, a, b):
    """Extremum a beats b: the larger (smaller) value, ties to the smallest (j, i)."""
    if a is None:
        return False
    if b is None:
        return True
    if a[0] != b[0]:
        return a[0] < b[0] if is_min else a[0] > b[0]
    return (a[1], a[2]) < (b[1], b[2])


_IS_MIN = [name.endswith("_min") for name in L.QUALITY_EXTREMA]


def merge(records):
    """Merge records: exact whatever their order."""
    ext, cnt = [None] * L.QUALITY_N_EXTREMA, [0] * L.QUALITY_N_COUNTS
    for e, c in records:
        for k in range(L.QUALITY_N_EXTREMA):
            if _better(_IS_MIN[k], e[k], ext[k]):
                ext[k] = e[k]
        cnt = [a + b for a, b in zip(cnt, c)]
    return ext, cnt


def _ext(t):
    return None if t is None else {"value": float(t[0]), "j": int(t[1]), "i": int(t[2]), "lon": float(t[3]), "lat": float(t[4])}


def section(rec, metrics):
    """The report of one section from its merged record."""
    e, c = rec
    X = {n: k for k, n in enumerate(L.QUALITY_EXTREMA)}
    C = {n: k for k, n in enumerate(L.QUALITY_COUNTS)}
    out = {
        "dx": {"min": _ext(e[X["dx_min"]]), "max": _ext(e[X["dx_max"]]), "n": c[C["n_dx"]], "n_degenerate": c[C["n_dx_degenerate"]]},
        "dy": {"min": _ext(e[X["dy_min"]]), "max": _ext(e[X["dy_max"]]), "n": c[C["n_dy"]], "n_degenerate": c[C["n_dy_degenerate"]]},
        "area": {"min": _ext(e[X["area_min"]]), "max": _ext(e[X["area_max"]]), "n": c[C["n_area"]], "n_zero": c[C["n_area_zero"]]},
        "aspect_ratio_max": _ext(e[X["aspect_max"]]),
        "rx_max": _ext(e[X["rx_max"]]),
        "ry_max": _ext(e[X["ry_max"]]),
    }
    if not metrics:   # --skip_metrics: dx, dy, area were never computed
        out = {k: None for k in out}
    dm = e[X["delta_max"]]   # the record holds tan(delta)
    if dm is not None:
        dm = (math.degrees(math.atan(dm[0])),) + tuple(dm[1:])
    out["corner"] = {"delta_max_deg": _ext(dm), "n": c[C["n_corners"]], "n_degenerate": c[C["n_corner_degenerate"]],
                     "histogram": c[C["hist0"]:C["hist0"] + L.QUALITY_N_BINS]}
    return out


def report(pieces, Re, nyp, nx, metrics):
    """The report from the records of all pieces of the stitched grid, in stitched order: pieces = [(section name or None, first
    stitched row, record)].
    A piece ends a section when the next piece has another name; its seam and dy-ratio-across-the-row-above are that joint's."""
    out = {"Re": float(Re), "nyp": int(nyp), "nxp": int(nx) + 1, "metrics": bool(metrics), "degenerate_m": L.QUALITY_DEGENERATE_M,
           "corner_bin_edges_deg": list(L.QUALITY_BIN_EDGES_DEG)}
    out["grid"] = section(merge(r for _, _, r in pieces), metrics)
    names = []
    for name, _, _ in pieces:
        if name is not None and name not in names:
            names.append(name)
    for name in names:
        out[name] = section(merge(r for n, _, r in pieces if n == name), metrics)
    joints = []
    for k in range(len(pieces) - 1):
        (lo, _, (e, _)), (up, j_up, _) = pieces[k], pieces[k + 1]
        if lo is not None and up != lo:
            seam = e[L.QUALITY_EXTREMA.index("seam_max")]
            ry = e[L.QUALITY_EXTREMA.index("ry_next_max")]
            joints.append({"lower": lo, "upper": up, "j": int(j_up), "seam_m": _ext(seam),
                           "ry": _ext(ry) if metrics else None})
    if names:
        out["joints"] = joints
    return out


def summary_lines(rep):
    """A few lines for stdout."""
    g = rep["grid"]

    def at(e, unit=""):
        return "n/a" if e is None else "%.6g%s at (j, i) = (%d, %d), (lon, lat) = (%.4f, %.4f)" % (e["value"], unit, e["j"], e["i"], e["lon"], e["lat"])

    lines = []
    if g["dx"] is not None:
        lines.append("   grid quality: min dx %s" % at(g["dx"]["min"], " m"))
        lines.append("   grid quality: min dy %s" % at(g["dy"]["min"], " m"))
        lines.append("   grid quality: max aspect ratio %s" % at(g["aspect_ratio_max"]))
        lines.append("   grid quality: max dx ratio along i %s" % at(g["rx_max"]))
        lines.append("   grid quality: max dy ratio along j %s" % at(g["ry_max"]))
    c = g["corner"]
    lines.append("   grid quality: max corner non-orthogonality %s; %d corners, %d degenerate, histogram %s over bins with edges %s deg"
                 % (at(c["delta_max_deg"], " deg"), c["n"], c["n_degenerate"], c["histogram"], rep["corner_bin_edges_deg"]))
    for jt in rep.get("joints", []):
        s, r = jt["seam_m"], jt["ry"]
        lines.append("   grid quality: joint %s/%s at j=%s: seam %s m, dy ratio %s" % (
            jt["lower"], jt["upper"], jt["j"], "n/a" if s is None else "%.3g" % s["value"], "n/a" if r is None else "%.6g" % r["value"]))
    return lines


# ---- host arrays ---------------------------------------------------------------------------------------------
def grid_quality(x, y, dx=None, dy=None, area=None, Re=DEFAULT_RE, sections=None, seams=None):
    """Report of a stitched supergrid given as host arrays (x, y: nyp x nxp; dx: nyp x nx; dy: ny x nxp; area: ny x nx, all in
    metres and degrees); dx, dy, area None: the items that need them are null (as with --skip_metrics).  ``sections``: [(sub-grid
    name, first stitched point row)] south -> north, to report per sub-grid and per joint; ``seams``: for every joint, the lower
    sub-grid's own last point row (x, y) that stitching dropped, or None."""
    x, y = L.as_f64(x), L.as_f64(y)
    nyp, nxp = x.shape
    nx = nxp - 1
    metrics = dx is not None
    if metrics:
        dx, dy, area = L.as_f64(dx), L.as_f64(dy), L.as_f64(area)
        if dx.shape != (nyp, nx) or dy.shape != (nyp - 1, nxp) or area.shape != (nyp - 1, nx):
            raise ValueError("grid_quality: shapes x %s dx %s dy %s area %s" % (x.shape, dx.shape, dy.shape, area.shape))
    if y.shape != x.shape or nyp < 2 or nx < 1:
        raise ValueError("grid_quality: x %s, y %s" % (x.shape, y.shape))
    secs = list(sections) if sections else [(None, 0)]
    starts = [int(j) for _, j in secs] + [nyp]
    pieces = []
    for k, (name, j0) in enumerate(secs):
        j1, last = starts[k + 1], k == len(secs) - 1
        if not 0 <= j0 < j1 <= nyp:
            raise ValueError("grid_quality: sections %s of %d rows" % (secs, nyp))
        b = L.QualityBand(nx=nx, j0=j0, n_pt_rows=j1 - j0, n_cell_rows=j1 - j0 - (1 if last else 0), Re=float(Re), metrics=int(metrics))
        keep = [x[j0:j1], y[j0:j1]]
        b.x, b.y = L.ptr(keep[0]), L.ptr(keep[1])
        if metrics:
            keep += [dx[j0:j1], dy[j0:j1 - (1 if last else 0)], area[j0:j1 - (1 if last else 0)]]
            b.dx, b.dy, b.area = L.ptr(keep[2]), L.ptr(keep[3]), L.ptr(keep[4])
        if not last:
            b.x_next, b.y_next = L.ptr(x[j1]), L.ptr(y[j1])
            if metrics:
                b.dx_next = L.ptr(dx[j1])
                b.dy_next = L.ptr(dy[j1]) if j1 < nyp - 1 else None
            if seams is not None and seams[k] is not None:
                sx, sy = L.as_f64(seams[k][0]).reshape(-1), L.as_f64(seams[k][1]).reshape(-1)
                assert sx.shape == (nxp,) and sy.shape == (nxp,)
                keep += [sx, sy]
                b.x_seam, b.y_seam = L.ptr(sx), L.ptr(sy)
        res = L.QualityResult()
        L.call("ogg_grid_quality", ctypes.byref(b), ctypes.byref(res))
        pieces.append((name, j0, record_from_bytes(bytes(res))))
    return report(pieces, Re, nyp, nx, metrics)


# ---- device arrays -------------------------------------------------------------------------------------------
def band_record_dev(band, stream, device):
    """Run ogg_grid_quality_band_dev on a descriptor of device pointers; the record as an int64 device tensor (not synchronised)."""
    import torch
    ws_bytes = int(L.load().ogg_grid_quality_workspace_bytes(band.nx, band.n_pt_rows))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=device)
    out = torch.zeros(ctypes.sizeof(L.QualityResult) // 8, dtype=torch.int64, device=device)
    L.call("ogg_grid_quality_band_dev", ctypes.byref(band), ws.data_ptr(), ws_bytes, out.data_ptr(), stream)
    return out, ws


def grid_quality_dev(x, y, dx=None, dy=None, area=None, Re=DEFAULT_RE):
    """Report of a whole stitched grid held in device tensors (one band, no sub-grid sections)."""
    import torch
    nyp, nxp = x.shape
    metrics = dx is not None
    b = L.QualityBand(nx=nxp - 1, j0=0, n_pt_rows=nyp, n_cell_rows=nyp - 1, Re=float(Re), metrics=int(metrics))
    b.x, b.y = x.data_ptr(), y.data_ptr()
    if metrics:
        b.dx, b.dy, b.area = dx.data_ptr(), dy.data_ptr(), area.data_ptr()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    rec, ws = band_record_dev(b, stream, x.device)
    host = rec.cpu().numpy()
    del ws
    return report([(None, 0, record_from_bytes(host))], Re, nyp, nxp - 1, metrics)


# ---- files ---------------------------------------------------------------------------------------------------
def check_file(path, Re=DEFAULT_RE, device="cuda:0"):
    """Report of the supergrid in a NetCDF classic file (x, y, dx, dy, area), on one GPU: the big-endian bytes go to the device as
    they are and are swapped there (ogg_bswap64_dev)."""
    import torch

    from . import netcdf3
    f = netcdf3.read_header(path)
    dev = torch.device(device)
    st = torch.cuda.current_stream(dev).cuda_stream
    fields = {}
    for name in ("x", "y", "dx", "dy", "area"):
        raw = netcdf3.read_var_bytes(path, f, name, dtype=netcdf3.NC_DOUBLE)
        shape = f.vars[name].shape
        src = torch.from_numpy(np.frombuffer(raw, dtype=np.int64).reshape(shape)).to(dev)
        dst = torch.empty(shape, dtype=torch.float64, device=dev)
        L.call("ogg_bswap64_dev", dst.numel(), src.data_ptr(), dst.data_ptr(), st)
        fields[name] = dst
        del src
    nyp, nxp = fields["x"].shape
    want = {"y": (nyp, nxp), "dx": (nyp, nxp - 1), "dy": (nyp - 1, nxp), "area": (nyp - 1, nxp - 1)}
    for k, shp in want.items():
        if tuple(fields[k].shape) != shp:
            raise ValueError("%s: %s has shape %s, expected %s for x of %s" % (path, k, tuple(fields[k].shape), shp, (nyp, nxp)))
    return grid_quality_dev(fields["x"], fields["y"], fields["dx"], fields["dy"], fields["area"], Re=Re)


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.grid_quality",
                                description="grid-quality report of a supergrid file (NetCDF classic / 64-bit offset)")
    p.add_argument("file")
    p.add_argument("--json", default=None, help="write the report as JSON to this file")
    p.add_argument("--radius", type=float, default=DEFAULT_RE, help="radius of the sphere in metres (default %(default)s)")
    a = p.parse_args(argv)
    rep = check_file(a.file, Re=a.radius)
    rep["file"] = a.file
    for line in summary_lines(rep):
        print(line)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rep, fh, indent=1)
    return rep


if __name__ == "__main__":
    main()
    sys.exit(0)

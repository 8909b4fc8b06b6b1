"""Stereographic regional supergrids: the oblique stereographic lattice about a centre, for pan-Arctic and circum-Antarctic domains
and every shelf domain that reaches a pole.  The domain may hold a geographic pole: as the centre point (lat_c = +-90 exactly), as a
cell corner next to it, or inside a cell.  include/ogg_hip.h, "Stereographic regional grids", gives the definition; the reference
makes the global tripolar grid only.

The domain centre (lon_c, lat_c) is the plane's origin and the grid's x axis there is turned by ``tilt`` degrees counter-clockwise from
east.  The supergrid has nx by ny cells, both even, of ``delta`` degrees AT THE CENTRE, where the scale is true; cells are isotropic
everywhere and shrink with 1 / (1 + rho^2/4) away from the centre.  The metrics are analytic and exact on the sphere.  Two kernels
(ogg_regional_stereo_tables_dev, ogg_regional_stereo_band_dev), as for the other regional kinds; no band split changes a bit.  x has
its jump of 360 degrees on the meridian opposite lon_c beyond a pole of the domain.  The file has the layout of the tripolar main().

    python -m ocean_model_grid_generator_amd.regional_stereo --lon_c LON --lat_c LAT [--tilt DEG] -r INV_RES
        (--cells NI NJ | --extent_km LX LY) [-f ocean_hgrid.nc] [--no_changing_meta] [--skip_metrics] [--quality_report q.json]
        [--bands N]
"""
import argparse
import collections
import math
import sys

import numpy as np

from . import _lib as L
from . import regional as R

DEFAULT_RE = R.DEFAULT_RE
FIELDS = R.FIELDS
KIND = "stereographic"
PROJECTION = ("p' = (1 - rho2/4, X, Y) / (1 + rho2/4), rho2 = X^2 + Y^2, X = (i - nx/2) delta pi/180, Y = (j - ny/2) delta pi/180: "
              "oblique stereographic, true scale at the centre; x jumps by 360 on the meridian opposite lon_c beyond a pole")

# the eight scalars every ogg_regional_stereo_* entry takes first, in the header's order: list(p) spreads them into a call
Params = collections.namedtuple("Params", "nx ny lon_c lat_c tilt delta Re metrics")
shapes = R.shapes
band_rows = R.band_rows


def params(lon_c, lat_c, nx, ny, delta, tilt=0.0, Re=DEFAULT_RE, metrics=True):
    """the parameters of a grid as the entries take them, checked by the library (OGG_EARG -> ValueError, no device is needed)"""
    p = Params(int(nx), int(ny), float(lon_c), float(lat_c), float(tilt), float(delta), float(Re), int(bool(metrics)))
    lib = L.load()
    if lib.ogg_regional_stereo_check(*p) != L.OGG_OK:
        raise ValueError(lib.ogg_last_error().decode())
    return p


def cells_for_extent(lx_km, ly_km, delta, Re=DEFAULT_RE):
    """(nx, ny): the smallest even numbers of supergrid cells of ``delta`` degrees at the centre that span lx_km along the grid's x
    centre line and ly_km along its y centre line: a half-length L/2 on the sphere is the plane half-width 2 tan(L / (4 Re))"""
    dl = math.radians(delta)
    n = []
    for length in (lx_km, ly_km):
        quarter = 0.25 * length * 1000.0 / Re
        if quarter >= 0.25 * math.pi:
            raise ValueError("regional stereo: an extent of %g km reaches beyond the hemisphere about the centre" % length)
        n.append(2.0 * (2.0 * math.tan(quarter)) / dl)
    even = lambda v: max(2, 2 * int(math.ceil(0.5 * v - 1e-9)))   # noqa: E731
    return even(n[0]), even(n[1])


# ---- host arrays ---------------------------------------------------------------------------------------------
def stereo_grid(lon_c, lat_c, nx, ny, delta, tilt=0.0, Re=DEFAULT_RE, metrics=True):
    """The supergrid as numpy arrays, on one GPU through the host-pointer entry ogg_regional_stereo_grid: a dict with x, y (degrees,
    (ny+1) x (nx+1)) and, with ``metrics``, dx ((ny+1) x nx), dy (ny x (nx+1)), area (ny x nx) in metres and angle_dx (degrees)."""
    p = params(lon_c, lat_c, nx, ny, delta, tilt, Re, metrics)
    names = FIELDS if metrics else FIELDS[:2]
    out = {f: np.empty(shapes(p.nx, p.ny)[f], np.float64) for f in names}
    L.call("ogg_regional_stereo_grid", *(list(p) + [out[f].ctypes.data if f in out else None for f in FIELDS]))
    return out


# ---- device arrays ---------------------------------------------------------------------------------------------
def stereo_grid_dev(lon_c, lat_c, nx, ny, delta, tilt=0.0, Re=DEFAULT_RE, metrics=True, bands=1, device="cuda:0"):
    """stereo_grid() with the fields as float64 device tensors: the table launch and one launch per band of point rows on the
    device's current stream, no host synchronisation.  ``bands`` changes no bit."""
    import torch
    p = params(lon_c, lat_c, nx, ny, delta, tilt, Re, metrics)
    dev = torch.device(device)
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_regional_stereo_workspace_bytes(*p))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    names = FIELDS if metrics else FIELDS[:2]
    out = {f: torch.empty(shapes(p.nx, p.ny)[f], dtype=torch.float64, device=dev) for f in names}
    L.call("ogg_regional_stereo_tables_dev", *(list(p) + [ws.data_ptr(), wsb, st]))
    for j0, n in band_rows(p.ny, bands):
        ptrs = [(out[f][j0:].data_ptr() if j0 < out[f].shape[0] else None) if f in out else None for f in FIELDS]
        L.call("ogg_regional_stereo_band_dev", *(list(p) + [j0, n, ws.data_ptr(), wsb] + ptrs + [st]))
    return out


# ---- files and the summary ---------------------------------------------------------------------------------------
def atts(p):
    return R.rotation_atts(p, KIND) + [("regional_projection", PROJECTION)]


def closed_form_area(p):
    """8 Re^2 [(B/a) atan(A/a) + (A/b) atan(B/b)] of the whole domain, A and B its plane half-widths"""
    A, B = 0.5 * p.nx * math.radians(p.delta), 0.5 * p.ny * math.radians(p.delta)
    a, b = math.sqrt(4.0 + B * B), math.sqrt(4.0 + A * A)
    return 8.0 * p.Re ** 2 * ((B / a) * math.atan(A / a) + (A / b) * math.atan(B / b))


def poles(p):
    """{"north" / "south": {"point": [j, i]} or {"cell": [j, i]}} for each geographic pole inside the domain: the supergrid point it
    sits on (the centre of a grid with lat_c = +-90 only) or the supergrid cell that holds it"""
    out = {}
    if abs(p.lat_c) == 90.0:
        return {"north" if p.lat_c > 0 else "south": {"point": [p.ny // 2, p.nx // 2]}}
    cl, sl = math.cos(math.radians(p.lat_c)), math.sin(math.radians(p.lat_c))
    ct, st = math.cos(math.radians(p.tilt)), math.sin(math.radians(p.tilt))
    d = math.radians(p.delta)
    for name, s in (("north", 1.0), ("south", -1.0)):
        den = 1.0 + s * sl
        if den < 0.25:
            continue
        fi, fj = s * 2.0 * cl * st / den / d + p.nx // 2, s * 2.0 * cl * ct / den / d + p.ny // 2
        if 0.0 <= fi <= p.nx and 0.0 <= fj <= p.ny:
            out[name] = {"cell": [min(int(fj), p.ny - 1), min(int(fi), p.nx - 1)]}
    return out


def summary(grid, p):
    """corners, extreme dx and dy, the angle_dx range, the area against its closed form (the last four only with metrics) and the
    poles of the domain"""
    x, y = grid["x"], grid["y"]
    s = {"kind": KIND, "nx": int(p.nx), "ny": int(p.ny), "lon_c": float(p.lon_c), "lat_c": float(p.lat_c), "tilt": float(p.tilt),
         "delta": float(p.delta), "Re": float(p.Re),
         "corners": {n: [float(x[j, i]), float(y[j, i])] for n, (j, i) in (("SW", (0, 0)), ("SE", (0, -1)), ("NW", (-1, 0)), ("NE", (-1, -1)))},
         "poles": poles(p)}
    if "dx" in grid:
        area, exact = float(np.sum(grid["area"])), closed_form_area(p)
        s.update(dx_min=float(grid["dx"].min()), dx_max=float(grid["dx"].max()), dy_min=float(grid["dy"].min()), dy_max=float(grid["dy"].max()),
                 angle_dx_min=float(grid["angle_dx"].min()), angle_dx_max=float(grid["angle_dx"].max()), area=area, area_closed_form=exact,
                 area_relative_error=(area - exact) / exact)
    return s


def summary_lines(s):
    out = R.summary_lines(s)
    for name, where in sorted(s["poles"].items()):
        kind, (j, i) = next(iter(where.items()))
        out.append("   regional: the %s pole %s (j, i) = (%d, %d)" % (name, "is the supergrid point" if kind == "point" else "lies in the supergrid cell", j, i))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.regional_stereo",
                                 description="a stereographic regional supergrid, which may hold a pole, in the file layout of the tripolar grid")
    ap.add_argument("--lon_c", type=float, required=True, help="longitude of the domain centre, degrees")
    ap.add_argument("--lat_c", type=float, required=True, help="latitude of the domain centre, degrees (90 or -90: the centre point is the pole)")
    ap.add_argument("--tilt", type=float, default=0.0, help="the grid's x axis at the centre, degrees counter-clockwise from east (default 0)")
    ap.add_argument("-r", "--inverse_resolution", type=float, required=True,
                    help="model cells per degree at the centre, where the scale is true (the supergrid step is half a model cell)")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--cells", type=int, nargs=2, metavar=("NI", "NJ"), help="model cells along x and y")
    g.add_argument("--extent_km", type=float, nargs=2, metavar=("LX", "LY"),
                   help="extent along the grid's two centre lines, rounded up to whole model cells")
    ap.add_argument("-f", "--gridfilename", default="ocean_hgrid.nc")
    ap.add_argument("--no_changing_meta", action="store_true", help="do not write meta data that might change from run to run")
    ap.add_argument("--skip_metrics", action="store_true", help="x and y only: dx, dy, area are written as -1 and angle_dx as 0")
    ap.add_argument("--quality_report", default=None, help="write the grid-quality report (grid_quality) as JSON to this file")
    ap.add_argument("--bands", type=int, default=1, help="launches the rows are split over (changes no byte)")
    ap.add_argument("--Re", type=float, default=DEFAULT_RE, help="sphere radius in metres")
    a = ap.parse_args(argv)
    if not a.inverse_resolution > 0.0:
        raise ValueError("regional stereo: -r %g: the inverse resolution must be positive" % a.inverse_resolution)
    delta = 0.5 / a.inverse_resolution
    if a.cells:
        nx, ny = 2 * a.cells[0], 2 * a.cells[1]
    else:
        nx, ny = cells_for_extent(a.extent_km[0], a.extent_km[1], delta, a.Re)
    p = params(a.lon_c, a.lat_c, nx, ny, delta, a.tilt, a.Re, not a.skip_metrics)
    dev = stereo_grid_dev(a.lon_c, a.lat_c, nx, ny, delta, a.tilt, a.Re, not a.skip_metrics, bands=a.bands)
    grid = {f: t.cpu().numpy() for f, t in dev.items()}
    s = summary(grid, p)
    for line in summary_lines(s):
        print(line)
    history = None
    if not a.no_changing_meta:
        import datetime
        history = "This grid file was generated via command " + " ".join(sys.argv) + " on " + str(datetime.date.today())
    R.write_regional(a.gridfilename, grid, atts(p), history)
    if a.quality_report:
        from . import ocean_grid_generator as O
        rep = O.grid_quality(grid["x"], grid["y"], grid.get("dx"), grid.get("dy"), grid.get("area"), Re=a.Re)
        O._write_quality_report(rep, a.quality_report)
    return s


if __name__ == "__main__":
    main()
    sys.exit(0)

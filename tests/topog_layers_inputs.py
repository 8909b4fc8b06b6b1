"""The named inputs of the layered-topography tests (tests/test_topog_layers_cpu.py, tests/test_gpu_topog_layers.py): small lat-lon
patches and strips near the poles, and polar-stereographic rasters placed RELATIVE to a patch -- the raster's origin is the projection
of the patch's centre less an offset in elements, so "inside", "across the left edge" and so on need no inverse projection.  The offsets
are irrational multiples of an element (.37, .61, ...), so that patch and raster are not commensurate and next to no sample falls on
an element's edge."""
import numpy as np

import topog_layers_definition as TL

A_WGS84, E_WGS84 = 6378137.0, 0.0818191908426215
PROJECTIONS = {
    "south_wgs84": dict(h=-1, lat_ts=-71.0, lon0=0.0, a=A_WGS84, e=E_WGS84),         # BedMachine Antarctica, IBCSO's plane
    "north_wgs84": dict(h=1, lat_ts=70.0, lon0=-45.0, a=A_WGS84, e=E_WGS84),          # BedMachine Greenland
    "south_sphere": dict(h=-1, lat_ts=-65.0, lon0=170.0, a=6371000.0, e=0.0),
    "north_sphere": dict(h=1, lat_ts=90.0, lon0=0.0, a=6371000.0, e=0.0),
}


def stereo(name, lat_gate=40.0):
    return TL.Stereo(lat_gate=lat_gate, **PROJECTIONS[name])


def patch(lon_c, lat_c, ny=16, nx=16, dlon=0.31, dlat=0.043, shear=0.07):
    """x, y ((ny + 1) x (nx + 1)) of a sheared lat-lon patch around (lon_c, lat_c)"""
    j, i = np.meshgrid(np.arange(ny + 1) - ny / 2.0, np.arange(nx + 1) - nx / 2.0, indexing="ij")
    return lon_c + dlon * (i + shear * j), lat_c + dlat * (j - 0.5 * shear * i)


def strip(n, lon_c, lat_c, **kw):
    return patch(lon_c, lat_c, ny=1, nx=n, **kw)


def index_values(Ny, Nx):
    """(I + 3 J) mod 1000 as int16"""
    J, I = np.meshgrid(np.arange(Ny), np.arange(Nx), indexing="ij")
    return ((I + 3 * J) % 1000).astype(np.int16)


def smooth_values(Ny, Nx, amplitude=3000.0):
    """a smooth float32 field of the element indices"""
    J, I = np.meshgrid(np.arange(Ny), np.arange(Nx), indexing="ij")
    return (amplitude * np.sin(0.045 * I + 0.3) * np.cos(0.031 * J - 0.2) - 500.0).astype(np.float32)


def raster_at(proj, lon_c, lat_c, N, d, off_x, off_y, values="index"):
    """(data, box): an N x N raster of d metre elements whose element (off_x, off_y) (fractional) lies at the projection of
    (lon_c, lat_c)"""
    open_gate = TL.Stereo(proj.h, proj.lat_ts, proj.lon0, proj.a, proj.e, lat_gate=-80.0)   # wherever the layer's own gate is
    X, Y, ok = TL.project(open_gate, lon_c, lat_c)
    assert bool(ok)
    box = (float(X) - off_x * d, d, float(Y) - off_y * d, d)
    return (index_values(N, N) if values == "index" else smooth_values(N, N)), box


# name -> (projection, patch centre, raster size, element size, the patch centre's place in the raster in elements, gate, values)
# a 16 x 16 patch of 0.31 x 0.043 degree cells is about 5 degrees by 0.7 degrees: near 84 degrees about 55 km by 80 km
_PLACED = {
    "inside_south": ("south_wgs84", (37.3, -84.1), 200, 1000.0, (100.37, 99.61), 40.0, "index"),
    "inside_north": ("north_wgs84", (-61.7, 83.6), 200, 1000.0, (99.61, 100.37), 40.0, "smooth"),
    "inside_sphere_south": ("south_sphere", (-140.2, -82.9), 128, 2000.0, (64.37, 63.61), 40.0, "index"),
    "inside_sphere_north": ("north_sphere", (12.9, 85.2), 64, 5000.0, (32.37, 31.61), 40.0, "smooth"),
    "fine_elements": ("south_wgs84", (101.3, -86.0), 200, 500.0, (100.37, 99.61), 40.0, "index"),
    "left_edge": ("south_wgs84", (37.3, -84.1), 100, 1000.0, (0.37, 50.61), 40.0, "index"),
    "right_edge": ("south_wgs84", (37.3, -84.1), 100, 1000.0, (99.63, 50.61), 40.0, "index"),
    "bottom_edge": ("north_wgs84", (-61.7, 83.6), 100, 1000.0, (50.37, 0.61), 40.0, "index"),
    "top_edge": ("north_wgs84", (-61.7, 83.6), 100, 1000.0, (50.37, 99.39), 40.0, "index"),
    "gate_south": ("south_wgs84", (37.3, -84.1), 200, 1000.0, (100.37, 99.61), 84.1037, "index"),
    "gate_north": ("north_sphere", (12.9, 85.2), 64, 5000.0, (32.37, 31.61), 85.2037, "smooth"),
    "wrong_hemisphere": ("south_wgs84", (37.3, 84.1), 64, 5000.0, (32.37, 31.61), -80.0, "index"),
}


def placed(name):
    """(x, y, layer) of a placement: the patch and the one projected layer of tests/topog_layers_definition.py"""
    pname, (lon_c, lat_c), N, d, (ox, oy), gate, values = _PLACED[name]
    proj = stereo(pname, gate)
    if name == "wrong_hemisphere":   # the raster sits where the patch's mirror image is
        data, box = raster_at(proj, lon_c, -lat_c, N, d, ox, oy, values)
    else:
        data, box = raster_at(proj, lon_c, lat_c, N, d, ox, oy, values)
    x, y = patch(lon_c, lat_c)
    return x, y, TL.layer(data, box, proj)


def pole_corner(sign):
    """a patch whose first (south) or last (north) point row is the pole itself, and a raster around the pole"""
    proj = stereo("south_wgs84" if sign < 0 else "north_wgs84")
    x, y = patch(23.7, 0.0, ny=8, nx=16, dlon=7.3, dlat=0.11, shear=0.0)
    y = sign * (90.0 - 0.11 * (np.arange(9) if sign < 0 else np.arange(8, -1, -1)))[:, None] + 0.0 * x
    data, box = raster_at(proj, 0.0, 90.0 * sign, 200, 1000.0, 100.37, 99.61)
    return x, y, TL.layer(data, box, proj)


def pole_enclosing(sign, name=None):
    """one cell around the pole (corners at 89.5 degrees, a quarter turn apart) and a raster around the pole"""
    proj = stereo(name or ("south_wgs84" if sign < 0 else "north_sphere"))
    x = np.array([[-135.0, -45.0], [135.0, 45.0]]) + 11.3
    y = np.full((2, 2), sign * 89.5)
    data, box = raster_at(proj, 0.0, 90.0 * proj.h, 64, 5000.0, 32.37, 31.61, "smooth" if sign > 0 else "index")   # around its own pole
    return x, y, TL.layer(data, box, proj)


def nonfinite(value):
    """the inside_south placement with one interior point's longitude, and another's latitude, not finite"""
    x, y, ly = placed("inside_south")
    x, y = x.copy(), y.copy()
    x[5, 6] = value
    y[9, 11] = value
    return x, y, ly


NAMED = tuple(_PLACED) + ("pole_corner_south", "pole_corner_north", "pole_enclosing_south", "pole_enclosing_north", "nan", "pinf", "minf")
REFINES = (1, 7, 8, 9, 63, 64, 65)


def named(name):
    if name in _PLACED:
        return placed(name)
    if name.startswith("pole_corner"):
        return pole_corner(-1 if name.endswith("south") else 1)
    if name.startswith("pole_enclosing"):
        return pole_enclosing(-1 if name.endswith("south") else 1)
    return nonfinite({"nan": np.nan, "pinf": np.inf, "minf": -np.inf}[name])


def strips():
    """1 x n strips across the left edge of the inside_south raster's neighbourhood, n = 1 .. 129 at the sizes that matter to the
    walk (a wavefront takes four cells at a time)"""
    _, _, ly = placed("left_edge")
    return [(n,) + strip(n, 37.3, -84.1, dlon=0.04) + (ly,) for n in (1, 2, 3, 4, 5, 63, 64, 65, 129)]


# ---- lists -------------------------------------------------------------------------------------------------------------
def global_int16():
    """a global 0.5 degree int16 raster in metres"""
    lon = -180.0 + 0.5 * (np.arange(720) + 0.5)
    lat = -90.0 + 0.5 * (np.arange(360) + 0.5)
    z = 3000.0 * np.sin(np.radians(3 * lon))[None, :] * np.cos(np.radians(2 * lat))[:, None] - 1200.0
    return z.astype(np.int16), (-180.0, 0.5, -90.0, 0.5)


def two_layers():
    """a projected float32 raster (quantum 0.01) with planted fill holes over the global int16 raster (q_mul = 100), on a patch that
    straddles the projected raster's right edge"""
    x, y, top = placed("right_edge")
    data = smooth_values(100, 100, amplitude=900.0)
    data[10:40, 60:95] = -9999.0
    data[::7, ::5] = np.nan
    top = TL.layer(data, top["box"], top["proj"], quantum=0.01, fill=(-9999.0,))
    g, gbox = global_int16()
    return x, y, [top, TL.layer(g, gbox, q_mul=100, quantum=1.0)]


def three_layers():
    """a fine projected raster over a coarser one of another plane (different lat_ts and element size) over lat-lon"""
    x, y, top = placed("left_edge")
    p2 = stereo("south_sphere")
    d2, box2 = raster_at(p2, 37.3, -84.1, 64, 2000.0, 40.37, 31.61)
    d2 = d2.copy()
    d2[20:30, :] = -32768
    g, gbox = global_int16()
    return x, y, [top, TL.layer(d2, box2, p2, fill=(-32768,)), TL.layer(g, gbox)]


def four_layers():
    """three_layers under a small projected raster with holes: four layers, every one of which gives some samples"""
    x, y, rest = three_layers()
    p0 = stereo("south_wgs84")
    d0, box0 = raster_at(p0, 37.3, -84.1, 64, 500.0, 32.37, 31.61)
    d0 = d0.copy()
    d0[::3, ::4] = -1
    return x, y, [TL.layer(d0, box0, p0, fill=(-1,))] + rest

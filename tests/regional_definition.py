"""The definition of the regional grids (include/ogg_hip.h, "Regional grids") restated in numpy, statement by statement, and the
cases the truth table (scripts/regional_truth.py -> tests/golden/regional_truth.npz) and the tests share.

regional(..., M=NP) evaluates the definition in fp64; with another math module M (the truth script's 50-digit one, on numpy object
arrays) the same statements give the truth.  The metrics are the header's literal forms: dy = Re (phi'_{j+1} - phi'_j) and area =
Re^2 dlam' (sin phi'_{j+1} - sin phi'_j), differences of neighbouring rows and all; their cancellation is part of this definition's
own error, the yardstick the device is held to.
"""
import numpy as np

RE = 6371.0e3
FIELDS = ("x", "y", "dx", "dy", "area", "angle_dx")
RELATIVE = ("dx", "dy", "area")          # errors of these are relative to the truth, the others absolute in degrees


class NP:
    """fp64"""
    D = np.pi / 180.0
    num = staticmethod(lambda v: np.asarray(v, dtype=np.float64))
    cos, sin, sqrt, arctan2, arctan, sinh, cosh, tanh = np.cos, np.sin, np.sqrt, np.arctan2, np.arctan, np.sinh, np.cosh, np.tanh


def rotation(lat_c, tilt, M=NP):
    """q1, q2, q3: the columns of Ry(-lat_c) Rx(tilt)"""
    cl, sl = M.cos(M.num(lat_c) * M.D), M.sin(M.num(lat_c) * M.D)
    ct, st = M.cos(M.num(tilt) * M.D), M.sin(M.num(tilt) * M.D)
    zero = M.num(0.0)
    return (cl, zero, sl), (-sl * st, ct, cl * st), (-sl * ct, -st, cl * ct)


def row_scalars(jc, delta, kind, M=NP):
    """cos phi', sin phi', phi' of the rows with centred indices jc = j - ny/2"""
    u = (jc * delta) * M.D
    if kind == "mercator":
        return 1.0 / M.cosh(u), M.tanh(u), M.arctan(M.sinh(u))
    return M.cos(u), M.sin(u), u


def regional(lon_c, lat_c, nx, ny, delta, kind="mercator", tilt=0.0, Re=RE, M=NP):
    """{x, y, dx, dy, area, angle_dx} of the whole grid"""
    assert nx % 2 == 0 and ny % 2 == 0 and kind in ("latlon", "mercator")
    delta, Re, lon_c = M.num(delta), M.num(Re), M.num(lon_c)
    q1, q2, q3 = rotation(lat_c, tilt, M)
    lam = (M.num(np.arange(nx + 1) - nx // 2) * delta) * M.D
    c, s = M.cos(lam), M.sin(lam)
    a = [c * q1[k] + s * q2[k] for k in range(3)]
    ez = -s * q1[2] + c * q2[2]
    jc = M.num(np.arange(ny + 1) - ny // 2)
    cp, sp, phi = row_scalars(jc, delta, kind, M)
    dl = delta * M.D
    px, py, pz = (cp[:, None] * a[k][None, :] + sp[:, None] * q3[k] for k in range(3))
    x = lon_c + M.arctan2(py, px) / M.D
    y = M.arctan2(pz, M.sqrt(px * px + py * py)) / M.D
    angle = M.arctan2(np.broadcast_to(ez[None, :], px.shape), cp[:, None] * q3[2] - sp[:, None] * a[2][None, :]) / M.D
    dx = np.repeat(((Re * cp) * dl)[:, None], nx, axis=1)
    dy = np.repeat((Re * (phi[1:] - phi[:-1]))[:, None], nx + 1, axis=1)
    area = np.repeat((((Re * Re) * dl) * (sp[1:] - sp[:-1]))[:, None], nx, axis=1)
    return {"x": x, "y": y, "dx": dx, "dy": dy, "area": area, "angle_dx": angle}


def closed_form_area(nx, ny, delta, kind, Re=RE):
    """Re^2 dlam' (sin phi'_top - sin phi'_bottom)"""
    top = 0.5 * ny * delta * NP.D
    return Re ** 2 * (nx * delta * NP.D) * 2.0 * (np.tanh(top) if kind == "mercator" else np.sin(top))


def error(field, value, hi, lo):
    """|value - truth| with the truth as hi + lo (hi = fp64(truth), lo = fp64(truth - hi)): value - hi is exact for neighbouring
    doubles.  Degrees for x, y, angle_dx; relative to the truth for dx, dy, area.  angle_dx is a direction: with tilt = -180 every
    point sits on the cut of atan2, where -180 and 180 are the same answer (the truth's sin(-pi) is 0, fp64's is -1.2e-16), so its
    distance is taken modulo 360."""
    e = np.abs((value - hi) - lo)
    if field == "angle_dx":
        e = np.minimum(e, np.abs(360.0 - e))
    return e / np.abs(hi) if field in RELATIVE else e


# (name, lon_c, lat_c, tilt, kind, delta, nx, ny): every lat_c of {0, 45, -60, 89 with a 0.5 degree domain}, every lon_c of {0, 179.9,
# -300}, every tilt of {0, 37.3, 90, -180}, both kinds, delta from 1 to 1/16 degree, on the shapes of the device tests: 2 x 2 cells,
# 130 x 2 and 2 x 130, point rows of 63, 65 and 129 (an even nx has no row of 64 points: nx = 64 gives the dx and area rows of 64),
# the 8 x 8 cells of the polar domain, and 258 columns: more than one workgroup across a row, more rows than a workgroup walks
CASES = [
    ("2x2_origin", 0.0, 0.0, 0.0, "latlon", 1.0, 2, 2),
    ("2x2_tilted", 179.9, 45.0, 37.3, "mercator", 0.5, 2, 2),
    ("2x2_polar", -300.0, 89.0, 90.0, "mercator", 0.25, 2, 2),
    ("8x8_polar_latlon", 0.0, 89.0, -180.0, "latlon", 0.0625, 8, 8),
    ("8x8_polar_mercator", 179.9, 89.0, 37.3, "mercator", 0.0625, 8, 8),
    ("130x2_equator", -300.0, 0.0, 0.0, "mercator", 1.0, 130, 2),
    ("130x2_tilted", 0.0, 45.0, 37.3, "latlon", 0.25, 130, 2),
    ("2x130_turned", 179.9, 0.0, 90.0, "latlon", 1.0, 2, 130),
    ("2x130_south", 0.0, -60.0, -180.0, "mercator", 0.125, 2, 130),
    ("62x4_south", -300.0, -60.0, 37.3, "mercator", 0.0625, 62, 4),
    ("64x6_turned", 179.9, 45.0, 90.0, "latlon", 0.5, 64, 6),
    ("128x4_flipped", 0.0, 0.0, -180.0, "mercator", 1.0, 128, 4),
    ("62x4_plain", 179.9, 0.0, 0.0, "latlon", 0.0625, 62, 4),
    ("64x4_north", -300.0, 45.0, 0.0, "mercator", 0.25, 64, 4),
    ("128x2_south", 0.0, -60.0, 90.0, "latlon", 0.125, 128, 2),
    ("258x10_tilted", 0.0, 45.0, 37.3, "mercator", 0.0625, 258, 10),
]
POLAR = tuple(c[0] for c in CASES if abs(c[2]) == 89.0)   # x and angle_dx are ill-conditioned there: a group of their own


def case_args(case):
    name, lon_c, lat_c, tilt, kind, delta, nx, ny = case
    return dict(lon_c=lon_c, lat_c=lat_c, nx=nx, ny=ny, delta=delta, kind=kind, tilt=tilt, Re=RE)

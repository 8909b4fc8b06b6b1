"""The definition of the stereographic regional grids (include/ogg_hip.h, "Stereographic regional grids") restated in numpy, statement
by statement, and the cases the truth table (scripts/regional_stereo_truth.py -> tests/golden/regional_stereo_truth.npz) and the tests
share.

stereo(..., M=NP) evaluates the definition in fp64; with another math module M (the truth script's 50-digit one, on numpy object
arrays) the same statements give the truth.  The area is the header's literal form, a difference of neighbouring edge terms; its
cancellation, about eps |Y| / d, is part of this definition's own error, the yardstick the device is held to.
"""
import numpy as np

from regional_definition import NP, RE, rotation

FIELDS = ("x", "y", "dx", "dy", "area", "angle_dx")
RELATIVE = ("dx", "dy", "area")          # errors of these are relative to the truth, the others absolute in degrees


def stereo(lon_c, lat_c, nx, ny, delta, tilt=0.0, Re=RE, M=NP):
    """{x, y, dx, dy, area, angle_dx} of the whole grid"""
    assert nx % 2 == 0 and ny % 2 == 0
    delta, Re, lon = M.num(delta), M.num(Re), M.num(lon_c)
    q1, q2, q3 = rotation(lat_c, tilt, M)
    d = delta * M.D
    X = M.num(np.arange(nx + 2) - nx // 2) * d          # one line beyond the grid: X_{i+1} of the last column
    Y = M.num(np.arange(ny + 2) - ny // 2) * d
    Xp, Yp = X[None, :nx + 1], Y[:ny + 1, None]
    rho2 = Xp * Xp + Yp * Yp
    m = 1 + rho2 / 4
    p = [(Xp * q2[k] + Yp * q3[k] + (1 - rho2 / 4) * q1[k]) / m for k in range(3)]
    x = lon + M.arctan2(p[1], p[0]) / M.D
    y = M.arctan2(p[2], M.sqrt(p[0] * p[0] + p[1] * p[1])) / M.D
    t = [q2[k] - (Xp / 2) * (q1[k] + p[k]) for k in range(3)]
    angle = M.arctan2(t[2], p[0] * t[1] - p[1] * t[0]) / M.D
    a = M.sqrt(4 + Y[:ny + 1] * Y[:ny + 1])
    dxh = (4 / a)[:, None] * M.arctan(a[:, None] * d / ((a * a)[:, None] + (X[:nx] * X[1:nx + 1])[None, :]))
    b = M.sqrt(4 + X[:nx + 1] * X[:nx + 1])
    dyh = (4 / b)[None, :] * M.arctan(b[None, :] * d / ((b * b)[None, :] + (Y[:ny] * Y[1:ny + 1])[:, None]))
    area = Re * Re * ((Y[1:ny + 1, None] * dxh[1:] - Y[:ny, None] * dxh[:-1]) + (X[None, 1:nx + 1] * dyh[:, 1:] - X[None, :nx] * dyh[:, :-1])) / 2
    if abs(lat_c) == 90.0:      # the centre IS the pole: p_x = p_y = 0, and the three values are defined (the limit along lon_c)
        x[ny // 2, nx // 2], y[ny // 2, nx // 2], angle[ny // 2, nx // 2] = lon, M.num(lat_c), M.num(tilt)
    return {"x": x, "y": y, "dx": Re * dxh, "dy": Re * dyh, "area": area, "angle_dx": angle}


def closed_form_area(nx, ny, delta, Re=RE):
    """8 Re^2 [(B/a) atan(A/a) + (A/b) atan(B/b)]"""
    A, B = 0.5 * nx * delta * NP.D, 0.5 * ny * delta * NP.D
    a, b = np.sqrt(4.0 + B * B), np.sqrt(4.0 + A * A)
    return 8.0 * Re ** 2 * ((B / a) * np.arctan(A / a) + (A / b) * np.arctan(B / b))


def error(field, value, hi, lo):
    """|value - truth| with the truth as hi + lo (hi = fp64(truth), lo = fp64(truth - hi)).  Degrees for x, y, angle_dx; relative to
    the truth for dx, dy, area.  x and angle_dx are directions: on the cut of atan2 (the meridian opposite lon_c beyond a pole, every
    point with tilt = -180) -180 and 180 are the same answer, so their distance is taken modulo 360."""
    e = np.abs((value - hi) - lo)
    if field in ("x", "angle_dx"):
        e = np.minimum(e, np.abs(360.0 - e))
    return e / np.abs(hi) if field in RELATIVE else e


# (name, lon_c, lat_c, tilt, delta, nx, ny): every lat_c of {0, 45, -60, 90, -90}, every lon_c of {0, 179.9, -300}, every tilt of {0,
# 37.3, 90, -180}, delta from 1 to 1/16 degree, on the shapes of the device tests: 2 x 2 cells, 130 x 2 and 2 x 130, point rows of 63,
# 65 and 129 about a wavefront's 63 owned columns and 64 lanes, and 258 x 10: more than one workgroup across a row, more rows than a
# workgroup walks; and one grid of 4 degree steps, beyond the step up to which the device takes the area's small arctangent by its series.
# The POLAR cases: a pole as the centre point -- a model corner (8 x 8: the centre has even indices), a face point
# (10 x 8) and a model centre (10 x 10) -- and a pole inside a cell (lat_c = 89.97: 0.03 degrees from the centre point, in the cell
# north-east of it).
CASES = [
    ("2x2_origin", 0.0, 0.0, 0.0, 1.0, 2, 2),
    ("2x2_tilted", 179.9, 45.0, 37.3, 0.5, 2, 2),
    ("130x2_equator", -300.0, 0.0, 0.0, 1.0, 130, 2),
    ("130x2_tilted", 0.0, 45.0, 37.3, 0.25, 130, 2),
    ("2x130_turned", 179.9, 0.0, 90.0, 1.0, 2, 130),
    ("2x130_south", 0.0, -60.0, -180.0, 0.125, 2, 130),
    ("62x4_south", -300.0, -60.0, 37.3, 0.0625, 62, 4),
    ("64x6_turned", 179.9, 45.0, 90.0, 0.5, 64, 6),
    ("128x4_flipped", 0.0, 0.0, -180.0, 1.0, 128, 4),
    ("258x10_tilted", 0.0, 45.0, 37.3, 0.0625, 258, 10),
    ("10x8_coarse", 179.9, -60.0, 90.0, 4.0, 10, 8),
    ("8x8_north", 0.0, 90.0, 0.0, 0.5, 8, 8),
    ("10x8_south", 179.9, -90.0, 37.3, 0.25, 10, 8),
    ("10x10_north", -300.0, 90.0, -180.0, 0.0625, 10, 10),
    ("6x6_inside", 0.0, 89.97, 37.3, 0.125, 6, 6),
]
POLAR = tuple(c[0] for c in CASES if abs(c[2]) > 89.0)   # x and angle_dx are ill-conditioned there: a group of their own


def case_args(case):
    name, lon_c, lat_c, tilt, delta, nx, ny = case
    return dict(lon_c=lon_c, lat_c=lat_c, nx=nx, ny=ny, delta=delta, tilt=tilt, Re=RE)

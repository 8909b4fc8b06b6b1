"""A conditioned bound for angle_dx at EVERY point of a mesh (plain numpy, no fixtures; used by the GPU parity tests and by
tests/test_angle_bounds_cpu.py).

angle_x (OGG:719-729) is atan2(N, D) of the stencil

    N = y[i+1] - y[i-1]                                   (one-sided at the two row ends: y[1] - y[0], y[-1] - y[-2])
    D = (x[i+1] - x[i-1]) * cos(y[i] * PI_180)

so when every coordinate of the mesh moves by at most eps_x, eps_y degrees, N moves by at most 2 eps_y, D by at most
2 eps_x |cos phi| (plus the change of cos phi itself, |x[i+1] - x[i-1]| sin(phi) PI_180 eps_y: under 1 % of 2 eps wherever the stencil is
narrower than a degree, 8 % measured where it is widest -- 90 degrees, on the bipolar cap's top row next to a pole point -- and left to
the factor 1.5 below), and to first order the angle by

    sensitivity = hypot(2 eps_y, 2 eps_x |cos phi|) / hypot(N, D)        [radians]

Two implementations whose meshes agree to eps therefore agree in the angle to `angle_bound_deg`: 1.5 x that (the second-order term is at
most 5 % where sensitivity < 0.05, the limit of the `regular` class; a uniform perturbation of the oracle's own mesh stays within 1.08 x the
first-order term, tests/test_angle_bounds_cpu.py) plus 8 ulp of 180 degrees for the rounding of atan2, cos and the division by PI_180.
Where the sensitivity is 0.05 rad or more the first-order model does not hold and the field is noise in the reference itself: such points
(`singular`) are COUNTED, from the reference mesh alone, and nothing is asserted about their value.  Rows of a lat-lon sub-grid (N == 0 in
every column, angle 0) are `flat`: there the angle is atan2(0, +) == 0 in any arithmetic and must be equal, not close.
"""
import numpy as np

PI_180 = np.pi / 180.0
SINGULAR_SENSITIVITY = 0.05            # radians: where the first-order model stops holding
SECOND_ORDER = 1.5
ULP_180 = float(np.spacing(180.0))
MAX_SINGULAR_WITH_CAP = 3              # the top row of the bipolar cap at supergrid columns Ni/4, Ni/2, 3Ni/4


def stencil(x, y):
    """N, D of angle_x and |cos phi|, every point of the mesh (degrees in, degrees out)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 2 and x.shape[1] >= 2, (x.shape, y.shape)
    N, dxs = np.empty_like(y), np.empty_like(x)
    N[:, 1:-1], dxs[:, 1:-1] = y[:, 2:] - y[:, :-2], x[:, 2:] - x[:, :-2]
    N[:, 0], dxs[:, 0] = y[:, 1] - y[:, 0], x[:, 1] - x[:, 0]
    N[:, -1], dxs[:, -1] = y[:, -1] - y[:, -2], x[:, -1] - x[:, -2]
    c = np.cos(y * PI_180)
    return N, dxs * c, np.abs(c)


def shape(x, y):
    """Radians of angle per degree of stencil noise: 1 / hypot(N, D); inf where the stencil vanishes."""
    N, D, _ = stencil(x, y)
    with np.errstate(divide="ignore"):
        return 1.0 / np.hypot(N, D)


def sensitivity(x, y, eps_x, eps_y):
    """First-order change (radians) of atan2(N, D) when every x moves by at most eps_x and every y by at most eps_y degrees; eps_x,
    eps_y scalars or arrays that broadcast against the mesh.  inf where the stencil vanishes."""
    N, D, c = stencil(x, y)
    num = np.hypot(2.0 * np.asarray(eps_y, dtype=np.float64), 2.0 * np.asarray(eps_x, dtype=np.float64) * c)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = num / np.hypot(N, D)
    return np.where(np.isnan(s), np.inf, s)        # 0 / 0: no perturbation allowed AND no stencil -- singular all the same


def angle_bound_deg(x, y, eps_x, eps_y):
    return np.degrees(SECOND_ORDER * sensitivity(x, y, eps_x, eps_y)) + 8.0 * ULP_180


def classify(x, y, angle, eps_x=1e-12, eps_y=1e-12):
    """(flat, singular, regular): three boolean masks of the mesh's shape, each point in exactly one."""
    N, _, _ = stencil(x, y)
    flat_rows = np.all(N == 0, axis=1) & np.all(np.asarray(angle) == 0, axis=1)
    flat = np.broadcast_to(flat_rows[:, None], N.shape).copy()
    singular = ~flat & ~(sensitivity(x, y, eps_x, eps_y) < SINGULAR_SENSITIVITY)
    return flat, singular, ~flat & ~singular


def adiff(a, b):
    """|a - b| modulo 360 degrees."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.minimum(d, np.abs(d - 360.0))


def check_angle(got_angle, want_x, want_y, want_angle, eps_x, eps_y, max_singular, name=""):
    """Hold `got_angle` to the reference at every point: equal on flat rows, within angle_bound_deg at regular points; singular points are
    counted on the REFERENCE (mesh and angle of `want` alone, so the code under test has no say in it) and may not number more than
    `max_singular`.  Returns {"worst_ratio": max d / bound over the regular points, "n_singular", "n_regular", "n_flat"}."""
    got_angle, want_angle = np.asarray(got_angle), np.asarray(want_angle)
    assert got_angle.shape == want_angle.shape == np.shape(want_x), (name, got_angle.shape, want_angle.shape, np.shape(want_x))
    flat, singular, regular = classify(want_x, want_y, want_angle, eps_x, eps_y)
    n_sing = int(singular.sum())
    assert n_sing <= max_singular, "%s: angle_dx: %d singular points in the reference mesh, at most %d expected: %s" % (
        name, n_sing, max_singular, np.argwhere(singular)[:8].tolist())
    bad = flat & (got_angle != want_angle)
    assert not bad.any(), "%s: angle_dx differs on flat (lat-lon) rows at %d points, first (j, i, got, want): %s" % (
        name, int(bad.sum()), [(int(j), int(i), float(got_angle[j, i]), float(want_angle[j, i])) for j, i in np.argwhere(bad)[:5]])
    d = adiff(got_angle, want_angle)
    bound = angle_bound_deg(want_x, want_y, eps_x, eps_y)
    ratio = np.where(regular, d / np.where(regular, bound, 1.0), 0.0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)              # a NaN in the field is a failure, not a pass
    rep = {"worst_ratio": float(ratio.max(initial=0.0)), "n_singular": n_sing, "n_regular": int(regular.sum()), "n_flat": int(flat.sum())}
    if rep["worst_ratio"] > 1.0:
        order = np.argsort(ratio, axis=None)[::-1][:5]
        worst = [(int(j), int(i), float(d[j, i]), float(bound[j, i])) for j, i in zip(*np.unravel_index(order, ratio.shape)) if ratio[j, i] > 1.0]
        raise AssertionError("%s: angle_dx beyond its conditioned bound at %d regular points; five worst (j, i, d, bound): %s" % (
            name, int((ratio > 1.0).sum()), worst))
    return rep

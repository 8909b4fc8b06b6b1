"""EVERY dx, dy, area and angle of the generic stencil (OGG:687-729) against the 50-digit truth, element by element, with a bound that follows
the conditioning of the reference's own formula (plain numpy; used by tests/test_stencil_bounds_cpu.py, tests/test_gpu_stencil_truth.py, the
stencil tests of tests/test_gpu_parity.py and tests/test_gpu_random_shapes.py, and -- for the scale -- by scripts/truth_table.py --groups
stencil).

The fixtures tests/golden/truth_stencil_*.npz hold, for the four meshes of tests/stencil_meshes.py and nine windows of them, the mesh itself
(fp64, the INPUT) and the value of the reference's lines as coded on that input without rounding, at every element of dx (nj1, ni), dy (nj, ni1),
area with latlon_areafix on (`area`) and off (`area_nofix`) (nj, ni) and angle_x (nj1, ni1), as hi + lo pairs (hi = fp64(truth), lo = the rest as
fp32: 2^-77 of the value, the bound is never below 2^-53 of it), and per field the oracle's own distance from that truth in units of the scale
below (`R` = max, `Rmed` = median).

The scale `s` of an element: first-order propagation of ONE rounding (u = 2^-53, relative) per operation of the reference's formula, inputs
exact.  e(v) is the bound on the absolute error of the computed v, in units of u:

  an edge between the points a and b (dx: b = (j, i), a = (j, i+1); dy: a = (j+1, i))
    d   = x_a - x_b                                e(d)   = |d|
    m   = mdist(x_a, x_b)                          e(m)   = e(d)            fmod is exact, and of mod(d, 360), mod(-d, 360) the smaller one
                                                                            is the one that needed no + 360: |x_a - x_b| counts, not m
    dxi = m PI_180                                 e(dxi) = e(m) PI_180 + |dxi|
    lv  = (0.5 (y_a + y_b)) PI_180                 e(lv)  = 0.5 |y_a + y_b| PI_180 + |lv|   (= 2 |lv|)
    c   = cos(lv),  sn = sin(lv)                   e(c)   = |sn| e(lv) + |c|,   e(sn) = |c| e(lv) + |sn|
    a   = (y_a - y_b) PI_180                       e(a)   = 2 |a|
    t   = dxi c                                    e(t)   = |c| e(dxi) + |dxi| e(c) + |t|       <- |dxi| |sn| 2 |lv| = |t| 2 |lv tan(lv)|: the
                                                                                                  term that owns the rows next to a pole
    q   = a a + t t                                e(q)   = 2 |a| e(a) + a^2 + 2 |t| e(t) + t^2 + q
    r   = sqrt(q),  L = Re r                       e(r)   = e(q) / (2 r) + r,   e(L) = Re e(r) + L          s(dx) = s(dy) = u e(L)
  area, latlon_areafix (OGG:711-713), between the edge rows j and j+1
    M   = 0.5 (dxi_up + dxi)                       e(M)   = 0.5 (e(dxi_up) + e(dxi)) + |M|
    S   = sn_up - sn                               e(S)   = e(sn_up) + e(sn) + |S|              <- (|sn_up| + |sn|) against |S|: the cancellation
    A   = Re^2 (M S)                               e(A)   = Re^2 (|S| e(M) + |M| e(S) + |M S|) + |A|
  area without it (OGG:715)
    A   = 0.25 ((dx_up + dx) (dy_right + dy))      e(A)   = 0.25 (|Y| (e(dx_up) + e(dx) + |X|) + |X| (e(dy_right) + e(dy) + |Y|) + |X Y|)
  angle (OGG:725-728), N = y_r - y_l, X = x_r - x_l (one-sided at the two row ends), arg = y_c PI_180
    e(N) = |N|,  e(X) = |X|,  e(arg) = |arg|,  cc = cos(arg): e(cc) = |sin(arg)| |arg| + |cc|,  D = X cc: e(D) = |cc| e(X) + |X| e(cc) + |D|
    th  = atan2(N, D)                              e(th)  = (|D| e(N) + |N| e(D)) / (N^2 + D^2) + |th|     (|N D| / (N^2 + D^2) times the two
                                                                                                            relative roundings, and atan2's own)
    ang = th / PI_180                              e(ang) = e(th) / PI_180 + |ang|

An element passes if |value - truth| <= K_REF * max(R, 1) * s, with K_REF = 1.5 (tests/test_gpu_truth.py) and R the oracle's largest
|error| / s of the element's class, read from the fixture; the floor of one s keeps a class in which the oracle happens to be exact from
demanding exactness.  ONE class per field: s adds the absolute values of every term, so it is a worst case, and the oracle's largest
|error| / s is 0.25 to 0.95 on every fixture and field -- the pole rows, the whole turns and the fold row included -- with medians of 0.04 to
0.28 (the table scripts/truth_table.py --groups stencil prints): nothing forces a split, and the floor of one s is what
every element is held to, 1.5 s.  Where the truth is exactly zero the value
must be exactly +0.0 -- for the angle, the zero numpy's arctan2 gives: -0.0 where N is -0.0, which the library promises.  Angles are compared
modulo 360 degrees.

Left out, of the angle alone: the points where hypot(e(N), e(D)) u / hypot(N, D), the first-order turn of (N, D) under its own roundings, reaches
angle_bounds.SINGULAR_SENSITIVITY (0.05 rad).  These are the points at +-90 degrees whose N vanishes: cos(fl(90 PI_180)) = 6e-17 carries the
rounding of its argument, 1.7e-16, so the SIGN of D -- an angle of 0 or 180 degrees -- is the arithmetic's.  (N = D = 0 with e(N) = e(D) = 0,
the displaced pole's own row, is not among them: the angle there is exactly 0 in any arithmetic.)  They are counted on the fixture's mesh
alone, the count is stored in the fixture, and check() requires the two to agree.  Nothing else is left out of any field.

A mesh WITHOUT a truth (the random and ragged meshes of the parity tests) is held against the oracle: |device - oracle| <= (K_REF + 1) * R * s
with R = max(the largest R of that field over the fixtures, 1): the triangle inequality over |device - truth| <= K_REF R s and |oracle - truth|
<= R s.
"""
import os

import numpy as np

import angle_bounds
from test_gpu_truth import K_REF

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI_180 = np.pi / 180.0
RE = 6371.0e3
U = 2.0 ** -53
FIELDS = ("dx", "dy", "area", "area_nofix", "angle")
FILES = {"bipolar": "truth_stencil_bipolar.npz", "dpole": "truth_stencil_dpole.npz", "turns": "truth_stencil_turns.npz", "edge": "truth_stencil_edge.npz",
         "windows": "truth_stencil_windows.npz"}
MAX_FILE_BYTES = 1 << 20


def scalar(a):
    return np.asarray(a).reshape(-1)[0]


def mdist(a, b):
    return np.minimum(np.mod(a - b, 360.0), np.mod(b - a, 360.0))


def _edge(xa, ya, xb, yb, Re):
    """The quantities of the edge b -> a and their error bounds in units of u: {"L", "eL", "dxi", "edxi", "sn", "esn"}."""
    d = xa - xb
    dxi = mdist(xa, xb) * PI_180
    edxi = np.abs(d) * PI_180 + np.abs(dxi)
    lv = (0.5 * (ya + yb)) * PI_180
    elv = 0.5 * np.abs(ya + yb) * PI_180 + np.abs(lv)
    c, sn = np.cos(lv), np.sin(lv)
    ec, esn = np.abs(sn) * elv + np.abs(c), np.abs(c) * elv + np.abs(sn)
    a = (ya - yb) * PI_180
    ea = 2.0 * np.abs(a)
    t = dxi * c
    et = np.abs(c) * edxi + np.abs(dxi) * ec + np.abs(t)
    q = a * a + t * t
    eq = 2.0 * np.abs(a) * ea + a * a + 2.0 * np.abs(t) * et + t * t + q
    r = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        er = np.where(r > 0, eq / (2.0 * r), 0.0) + r
    return {"L": Re * r, "eL": Re * er + Re * r, "dxi": dxi, "edxi": edxi, "sn": sn, "esn": esn}


def angle_terms(x, y):
    """N, D of angle_x and e(N), e(D) in units of u, every point of the mesh."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, X = np.empty_like(y), np.empty_like(x)
    N[:, 1:-1], X[:, 1:-1] = y[:, 2:] - y[:, :-2], x[:, 2:] - x[:, :-2]
    N[:, 0], X[:, 0] = y[:, 1] - y[:, 0], x[:, 1] - x[:, 0]
    N[:, -1], X[:, -1] = y[:, -1] - y[:, -2], x[:, -1] - x[:, -2]
    arg = y * PI_180
    cc = np.cos(arg)
    ecc = np.abs(np.sin(arg)) * np.abs(arg) + np.abs(cc)
    D = X * cc
    eD = np.abs(cc) * np.abs(X) + np.abs(X) * ecc + np.abs(D)
    return N, D, np.abs(N), eD


def angle_singular(x, y):
    """The points left out of the angle: the first-order model of atan2(N, D) under the roundings of N and D does not hold (from the mesh alone)."""
    N, D, eN, eD = angle_terms(x, y)
    num, hyp = np.hypot(eN, eD) * U, np.hypot(N, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        sens = np.where(hyp > 0, num / hyp, np.where(num > 0, np.inf, 0.0))
    return ~(sens < angle_bounds.SINGULAR_SENSITIVITY)


def scales(x, y, Re=RE):
    """{field: s}, every element of every field, in the field's own unit (metres, square metres, degrees)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ei = _edge(x[:, 1:], y[:, 1:], x[:, :-1], y[:, :-1], Re)
        ej = _edge(x[1:, :], y[1:, :], x[:-1, :], y[:-1, :], Re)
        M = 0.5 * (ei["dxi"][1:] + ei["dxi"][:-1])
        eM = 0.5 * (ei["edxi"][1:] + ei["edxi"][:-1]) + np.abs(M)
        S = ei["sn"][1:] - ei["sn"][:-1]
        eS = ei["esn"][1:] + ei["esn"][:-1] + np.abs(S)
        Re2 = Re ** 2
        eA = Re2 * (np.abs(S) * eM + np.abs(M) * eS + np.abs(M * S)) + np.abs(Re2 * (M * S))
        X, Y = ei["L"][1:] + ei["L"][:-1], ej["L"][:, 1:] + ej["L"][:, :-1]
        eX, eY = ei["eL"][1:] + ei["eL"][:-1] + X, ej["eL"][:, 1:] + ej["eL"][:, :-1] + Y
        eA2 = 0.25 * (Y * eX + X * eY + X * Y)
        N, D, eN, eD = angle_terms(x, y)
        th = np.arctan2(N, D)
        h2 = N * N + D * D
        with np.errstate(divide="ignore"):
            eth = np.where(h2 > 0, (np.abs(D) * eN + np.abs(N) * eD) / np.where(h2 > 0, h2, 1.0), 0.0) + np.abs(th)
        eang = eth / PI_180 + np.abs(th / PI_180)
    return {"dx": U * ei["eL"], "dy": U * ej["eL"], "area": U * eA, "area_nofix": U * eA2, "angle": U * eang}


def oracle(x, y, Re=RE):
    """The oracle's five fields of a mesh (one row of points: empty dy and areas, like numpy's slices)."""
    from oracle import ogg_oracle as orc
    dx, dy, area = orc.generate_grid_metrics_MIDAS(x, y, Re)
    return {"dx": dx, "dy": dy, "area": area, "area_nofix": orc.generate_grid_metrics_MIDAS(x, y, Re, latlon_areafix=False)[2], "angle": orc.angle_x(x, y)}


def shapes(nj1, ni1):
    return {"dx": (nj1, ni1 - 1), "dy": (nj1 - 1, ni1), "area": (nj1 - 1, ni1 - 1), "area_nofix": (nj1 - 1, ni1 - 1), "angle": (nj1, ni1)}


def distance(v, hi, lo, field):
    """|v - truth|, truth = hi + lo; modulo 360 degrees for the angle; inf where v is not finite."""
    d = np.abs((np.asarray(v, dtype=np.float64) - hi) - lo.astype(np.float64))
    if field == "angle":
        d = np.minimum(d, np.abs(d - 360.0))
    return np.where(np.isfinite(d), d, np.inf)


_CACHE = {}


def names():
    """The fixtures: the four meshes, then the nine windows."""
    import stencil_meshes as sm
    return list(sm.MESHES) + list(sm.WINDOWS)


def load(name):
    """One fixture: {"x", "y", "truth": {field: (hi, lo)}, "R": {field: max}, "Rmed": {field: median}, "n_singular"}; read-only arrays."""
    import stencil_meshes as sm
    if name in _CACHE:
        return _CACHE[name]
    fname = FILES[name] if name in sm.MESHES else FILES["windows"]
    z = np.load(os.path.join(GOLD, fname))
    if name in sm.MESHES:
        x, y = z[name + "_x"], z[name + "_y"]
    else:
        m = sm.WINDOWS[name][0]
        base = load(m)
        x, y = sm.window({m: (base["x"], base["y"])}, name)
    s = {"x": x, "y": y, "truth": {}, "R": {}, "Rmed": {}, "n_singular": int(scalar(z[name + "_angle_nsing"]))}
    shp = shapes(*x.shape)
    for f in FIELDS:
        hi, lo = z["%s_%s_hi" % (name, f)], z["%s_%s_lo" % (name, f)]
        assert hi.shape == lo.shape == shp[f] and hi.dtype == np.float64 and lo.dtype == np.float32, (name, f, hi.shape, shp[f])
        s["truth"][f] = (hi, lo)
        s["R"][f], s["Rmed"][f] = float(scalar(z["%s_%s_R" % (name, f)])), float(scalar(z["%s_%s_Rmed" % (name, f)]))
    for a in (x, y):
        a.setflags(write=False)
    _CACHE[name] = s
    return s


def r_max(field):
    """max(the largest R of `field` over the fixtures, 1)."""
    return max([load(n)["R"][field] for n in names()] + [1.0])


class StencilBoundError(AssertionError):
    """check() failed; `.worst` = the worst elements as (field, j, i, distance, bound), worst first."""

    def __init__(self, msg, worst):
        super().__init__(msg)
        self.worst = worst


def _judge(name, f, d, bound, s, left_out, zero, zero_bad, rep_extra):
    """Report line of one field and its failures (ratio > 1 or a wrong zero).  "median_over_s" is over the held elements that are not exact
    zeros (`zero`), the fixture's definition of Rmed."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
        over_s = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0))
    ratio = np.where(left_out, 0.0, ratio)
    ratio = np.where(zero_bad, np.inf, ratio)
    over_s = np.where(left_out, 0.0, over_s)
    held = ~left_out
    rep = {"worst_over_bound": float(ratio.max(initial=0.0)), "worst_over_s": float(over_s.max(initial=0.0)),
           "median_over_s": float(np.median(over_s[held & ~zero])) if (held & ~zero).any() else 0.0, "n": int(held.sum())}
    rep.update(rep_extra)
    bad = []
    for k in np.argsort(ratio, axis=None)[::-1][:5]:
        j, i = np.unravel_index(k, ratio.shape)
        if ratio[j, i] > 1.0:
            bad.append((float(ratio[j, i]), f, int(j), int(i), float(d[j, i]), float(bound[j, i])))
    return rep, bad


def _raise_or_return(name, what, rep, bad):
    if bad:
        bad.sort(reverse=True)
        worst = [b[1:] for b in bad[:5]]
        raise StencilBoundError("%s: beyond %s; worst (field, j, i, distance, bound): %s" % (name, what, worst), worst)
    return rep


def check(name, got, tag=""):
    """Hold `got` = {field: array} (any of FIELDS; the fixture's shapes) to the truth of the fixture `name` at every element.  Returns
    {field: {"worst_over_bound", "worst_over_s", "median_over_s", "n", "R", "n_zero", "n_singular"}}; raises StencilBoundError naming the five
    worst elements if any is beyond its bound, not finite, or a wrong zero."""
    fx = load(name)
    x, y = fx["x"], fx["y"]
    s_all = scales(x, y)
    sing = angle_singular(x, y)
    assert int(sing.sum()) == fx["n_singular"], "%s: %d points left out of the angle on this host, %d in the fixture" % (name, int(sing.sum()), fx["n_singular"])
    rep, bad = {}, []
    for f in FIELDS:
        if f not in got:
            continue
        v = np.asarray(got[f])
        hi, lo = fx["truth"][f]
        assert v.shape == hi.shape, (name, tag, f, v.shape, hi.shape)
        if v.size == 0:
            continue
        s = s_all[f]
        d = distance(v, hi, lo, f)
        bound = K_REF * max(fx["R"][f], 1.0) * s
        left_out = sing if f == "angle" else np.zeros(v.shape, bool)
        zero = (hi == 0) & (lo == 0) & ~left_out
        if f == "angle":
            N, D, _, _ = angle_terms(x, y)
            want0 = np.arctan2(N, D) / PI_180                 # +-0.0 where the truth is exactly zero: numpy's zero, by the sign of N
        else:
            want0 = np.zeros(v.shape)
        zero_bad = zero & ~((v == 0) & (np.signbit(v) == np.signbit(want0)))
        r, b = _judge(name, f, d, bound, s, left_out, zero, zero_bad, {"R": fx["R"][f], "n_zero": int(zero.sum()), "n_singular": int(left_out.sum())})
        rep[f] = r
        bad += b
    return _raise_or_return("%s %s" % (name, tag), "the bound against the truth", rep, bad)


def check_against_oracle(x, y, got, Re=RE, name=""):
    """A mesh without a truth: |got - oracle| <= (K_REF + 1) * R * s at every element (R = r_max(field)); the angle modulo 360 degrees and not
    at the points angle_singular leaves out.  Returns {field: {"worst_over_bound", "worst_over_s", "median_over_s", "n", "n_singular"}}."""
    want = oracle(np.asarray(x), np.asarray(y), Re)
    s_all = scales(x, y, Re)
    sing = angle_singular(x, y)
    rep, bad = {}, []
    for f in FIELDS:
        if f not in got:
            continue
        v, w = np.asarray(got[f]), want[f]
        assert v.shape == w.shape, (name, f, v.shape, w.shape)
        if v.size == 0:
            continue
        d = distance(v, w, np.zeros(w.shape, np.float32), f)
        left_out = sing if f == "angle" else np.zeros(v.shape, bool)
        r, b = _judge(name, f, d, (K_REF + 1.0) * r_max(f) * s_all[f], s_all[f], left_out, s_all[f] == 0, np.zeros(v.shape, bool), {"n_singular": int(left_out.sum())})
        rep[f] = r
        bad += b
    return _raise_or_return(name, "the bound against the oracle", rep, bad)

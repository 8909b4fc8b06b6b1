"""CPU tests of the every-point check of angle_dx (tests/angle_bounds.py, applied by test_gpu_parity._check_supergrid and
test_gpu_pipeline._same_as_function_level), with the oracle alone:

  * no false alarm: angle_x of the oracle's mesh perturbed within +- eps stays within the bound of that eps at every regular point;
  * census: every flag set a GPU caller of _check_supergrid uses has, in the ORACLE's mesh, the three singular points of the bipolar cap's
    top row (supergrid columns Ni/4, Ni/2, 3Ni/4) and no other, none without a cap;
  * planted defects: local errors of the kind the fused pass invites -- one point, one column with the one-sided stencil, one mirror-image
    column with the wrong sign, one zero -- pass the 99.9 % quantile that was the only check of this field, and fail the new one.
"""
import json
import os

import numpy as np
import pytest

import angle_bounds as ab
from oracle import ogg_oracle as orc
from test_gpu_parity import _bipolar_rows, _check_supergrid, _row_tolerances
from test_gpu_random_shapes import _random_flags

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EPS = 1e-12
SMALL = {"r0.25": dict(inverse_resolution=0.25, ensure_nj_even=True),
         "r0.5_dp": dict(inverse_resolution=0.5, r_dp=0.2, ensure_nj_even=True)}
_CACHE = {}


def _oracle(flags):
    """make_supergrid without the metrics (the angle does not depend on them), computed once per flag set and never modified."""
    key = json.dumps(flags, sort_keys=True)
    if key not in _CACHE:
        f = dict(flags)
        r = f.pop("inverse_resolution")
        f["skip_metrics"] = True
        w = orc.make_supergrid(r, skip_doughnut_rows=True, **f)
        for k in ("x", "y", "angle_dx"):
            w[k].setflags(write=False)
        _CACHE[key] = w
    return _CACHE[key]


def _eps_arrays(w):
    return _row_tolerances(w, "x")[0], _row_tolerances(w, "y")[0]


def _old_quantile_line_passes(got_angle, want_angle):
    d = np.abs(got_angle - want_angle)
    d = np.minimum(d, np.abs(d - 360.0))
    return float(np.quantile(d, 0.999)) < 1e-9


# ---------------------------------------------------------------------------------------------------------------
# no false alarm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_perturbed_mesh_stays_within_the_bound(name):
    w = _oracle(SMALL[name])
    x, y = w["x"], w["y"]
    flat, singular, regular = ab.classify(x, y, w["angle_dx"], EPS, EPS)
    assert int(singular.sum()) == 3 and regular.any() and flat.any()
    bound = ab.angle_bound_deg(x, y, EPS, EPS)
    first = np.degrees(ab.sensitivity(x, y, EPS, EPS))
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(5):
        xp = x + rng.uniform(-EPS, EPS, x.shape)
        yp = y + rng.uniform(-EPS, EPS, y.shape)
        d = ab.adiff(orc.angle_x(xp, yp), w["angle_dx"])
        assert np.all(d[regular] <= bound[regular]), float((d[regular] / bound[regular]).max())
        worst = max(worst, float(((d[regular] - 8 * ab.ULP_180) / first[regular]).max()))
        # the same through the check itself, on the cap's rows above the joint (a perturbed lat-lon row is not flat any more)
        cap = slice(_bipolar_rows(w)[0] + 1, _bipolar_rows(w)[1])
        ab.check_angle(orc.angle_x(xp, yp)[cap], x[cap], y[cap], w["angle_dx"][cap], EPS, EPS, 3, name)
    # the first-order term alone covers every point but the top row's neighbours of a pole point, where the stencil spans 90 degrees of
    # longitude and the change of cos(phi) with y, which the model leaves out, adds 8 %: well inside the factor 1.5
    assert worst <= 1.1, worst


@pytest.mark.parametrize("name", sorted(SMALL))
def test_oracle_against_itself_passes_with_zero_differences(name):
    w = _oracle(SMALL[name])
    ex, ey = _eps_arrays(w)
    rep = ab.check_angle(w["angle_dx"].copy(), w["x"], w["y"], w["angle_dx"], ex, ey, 3, name)
    assert rep["worst_ratio"] == 0.0 and rep["n_singular"] == 3
    assert rep["n_flat"] + rep["n_regular"] + rep["n_singular"] == w["x"].size
    _check_supergrid({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}, w, "cpu_self_" + name)


def test_bound_figures_of_the_small_grids():
    """The size of the bound at eps = 1e-12 (the figures the design of the check was based on): of the order of 1e-10 degrees over the
    cap at 2 degree spacing, growing towards the two pole points, where the stencil shrinks."""
    w = _oracle(SMALL["r0.25"])
    _, _, regular = ab.classify(w["x"], w["y"], w["angle_dx"], EPS, EPS)
    b = ab.angle_bound_deg(w["x"], w["y"], EPS, EPS)[regular]
    assert 5e-11 < np.quantile(b, 0.999) < 5e-10 and 1e-10 < b.max() < 7e-8, (float(np.quantile(b, 0.999)), float(b.max()))


# ---------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------
def _census_sets():
    out = []
    for name, cfg in sorted(json.load(open(os.path.join(GOLD, "ref_hashes.json")))["configs"].items()):
        out.append(("golden:" + name, dict(cfg["flags"])))
    for seed in range(6):                                      # test_gpu_random_shapes.test_tripolar_pass_random_plans: the same draws
        rng = np.random.default_rng(5000 + seed)
        r = float(rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 3.0]))
        out.append(("random_plan:%d" % seed, dict(inverse_resolution=r, ensure_nj_even=bool(rng.integers(0, 2)))))
    for seed in range(40):                                     # test_main_random_flags_*: drawn with their seeds
        out.append(("random_flags:%d" % seed, _random_flags(seed)))
    return out


# flag sets whose ORACLE mesh has more singular points than the cap's three would be named here with their own count and the pole each
# point touches: {name: count}.  None does.
CENSUS_EXCEPTIONS = {}


@pytest.mark.parametrize("name,flags", _census_sets(), ids=[n for n, _ in _census_sets()])
def test_census_of_singular_points(name, flags):
    try:
        w = _oracle(flags)
    except BaseException:                                      # the oracle rejects this set (its guards, or a cut that needs an absent cap)
        return
    lo, hi = _bipolar_rows(w)
    ex, ey = _eps_arrays(w)
    x, y, a = w["x"], w["y"], w["angle_dx"]
    if flags["inverse_resolution"] >= 4:                       # the caps only: the lat-lon rows in between are flat by construction
        sc = w["sub"].get("SC")
        n_sc = sc[0].shape[0] - 1 if sc is not None and np.ptp(sc[0], axis=0).max() > 0 else 0
        keep = np.r_[0:n_sc, lo:hi]
        x, y, a, ex, ey = x[keep], y[keep], a[keep], ex[keep], ey[keep]
    flat, singular, regular = ab.classify(x, y, a, ex, ey)
    cap = ab.MAX_SINGULAR_WITH_CAP if hi > lo else 0
    assert int(singular.sum()) <= CENSUS_EXCEPTIONS.get(name, cap), (name, np.argwhere(singular).tolist())
    if hi > lo:                                                # ... and they are the three points of the cap's top row
        Ni = x.shape[1] - 1
        assert np.argwhere(singular).tolist() == [[x.shape[0] - 1, c] for c in (Ni // 4, Ni // 2, 3 * Ni // 4)], name
    assert not np.any(singular & (ex == 0)) and np.all(flat | singular | regular)


# ---------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------
def _one_sided_column(w, rows, col):
    """angle_x of `rows` at column `col` with the stencil of a row END (OGG:726: forward difference)."""
    x, y = w["x"], w["y"]
    return np.arctan2(y[rows, col + 1] - y[rows, col], (x[rows, col + 1] - x[rows, col]) * np.cos(y[rows, col] * orc.PI_180)) / orc.PI_180


def _defects(w):
    lo, hi = _bipolar_rows(w)
    Ni = w["x"].shape[1] - 1
    mid = (lo + hi) // 2
    a = w["angle_dx"]
    out = {}
    d = a.copy()
    d[mid, Ni // 8 + 3] += 1e-6
    out["one mid-cap point off by 1e-6 degrees"] = d
    d = a.copy()
    rows = np.arange(lo + 10, lo + 40)
    d[rows, 64] = _one_sided_column(w, rows, 64)
    out["supergrid column 64 of 30 cap rows from the one-sided stencil"] = d
    d = a.copy()
    d[lo:hi - 1, Ni // 4 + 7] *= -1.0                          # a mirror image (angle = -a of its source column) with the sign dropped
    out["one image column with the sign flipped"] = d
    d = a.copy()
    d[mid + 5, 3 * Ni // 8] = 0.0
    out["one value set to 0"] = d
    return out


DEFECTS = ["one mid-cap point off by 1e-6 degrees", "supergrid column 64 of 30 cap rows from the one-sided stencil",
           "one image column with the sign flipped", "one value set to 0"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_passes_the_quantile_and_fails_the_every_point_check(defect):
    w = _oracle(SMALL["r0.5_dp"])
    assert w["x"].shape == (277, 361) and _bipolar_rows(w) == (216, 277)
    bad = _defects(w)[defect]
    n_changed = int((bad != w["angle_dx"]).sum())
    assert 1 <= n_changed <= 60
    # the gap: the line that was the suite's only check of this field at small sizes lets every one of them through
    assert _old_quantile_line_passes(bad, w["angle_dx"]), defect
    got = {k: v for k, v in w.items()}
    got["angle_dx"] = bad
    with pytest.raises(AssertionError, match="angle_dx beyond its conditioned bound at %d regular points" % n_changed):
        _check_supergrid(got, w, "planted")
    # the same between the two paths of main() (test_gpu_pipeline._same_as_function_level: eps = TOL_COORD on the cap's rows)
    lo, hi = _bipolar_rows(w)
    with pytest.raises(AssertionError, match="beyond its conditioned bound"):
        ab.check_angle(bad[lo:hi], w["x"][lo:hi], w["y"][lo:hi], w["angle_dx"][lo:hi], EPS, EPS, 3, "planted")


def test_planted_defect_on_a_flat_row_and_a_nan_fail():
    w = _oracle(SMALL["r0.25"])
    ex, ey = _eps_arrays(w)
    bad = w["angle_dx"].copy()
    bad[40, 17] = 1e-300                                       # a lat-lon row: equal, not close
    with pytest.raises(AssertionError, match="flat"):
        ab.check_angle(bad, w["x"], w["y"], w["angle_dx"], ex, ey, 3)
    bad = w["angle_dx"].copy()
    bad[-5, 20] = np.nan
    with pytest.raises(AssertionError, match="beyond its conditioned bound"):
        ab.check_angle(bad, w["x"], w["y"], w["angle_dx"], ex, ey, 3)
    with pytest.raises(AssertionError, match="singular points in the reference mesh"):
        ab.check_angle(w["angle_dx"], w["x"], w["y"], w["angle_dx"], ex, ey, 0)

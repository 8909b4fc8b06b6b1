"""GPU parity tests: every hot-path function of SURVEY 8(a), called through the C ABI (ctypes), against the oracle on
the same inputs and against the committed golden fixtures (generated from the reference itself).

Tolerances (fp64; BASELINE.json's north_star asks for max-abs coordinate diff < 1e-12 deg and area diff < 1e-6 m^2):
the kernels follow the oracle's operation order with FMA contraction off, so the only differences are last-ulp
differences between the device libm (ocml) and the host's (numpy: glibc / SVML).  What that noise floor does to each
field was measured (DESIGN.md "Parity"); the bounds below are those measurements with margin:

  coordinates x, y (all sub-grids)      1e-12 deg   (north_star bound; measured <= 2e-13)
  bipolar x next to the symmetry        2e-11 deg   acos/asin are ill-conditioned there (App. C: 6e-12 at 1/8 deg)
    meridian, y at the two pole points
  MIDAS dx, dy                          rel 2e-15 + abs 1e-10 m
  MIDAS area                            rel 5e-12   (cancellation in sin(phi[j+1])-sin(phi[j]): 1 ulp of sin moves the
                                                    area by 3e-5 m^2 at 1/8 deg -- the 1e-6 m^2 target is below 1 ulp)
  bipolar quadrature dx, dy, area       rel 5e-14
  displaced-pole quadrature dx, dy,     rel 2e-12 * Ni  (10x the measured difference, which grows with the resolution: finite
                     area                             differences of an arc of 2e-3 * 360/Ni degrees; see dp_quad_rel_tol)
  angle_dx                              EVERY point: equal on lat-lon rows; elsewhere within the first-order change of atan2(N, D) under
                                        the coordinate bounds above, x 1.5 (tests/angle_bounds.py); nothing at the three points of the
                                        bipolar cap's top row where the stencil vanishes (columns Ni/4, Ni/2, 3Ni/4), whose number is
                                        counted on the oracle's mesh; and 99.9 % of a grid within 1e-9 deg
"""
import json
import os

import numpy as np
import pytest

import angle_bounds
import stencil_bounds
import stencil_plans
from oracle import ogg_oracle as orc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL_COORD = 1e-12
TOL_COORD_ILL = 2e-11
BP_POLE_POINT_TOL_Y = 1e-6
REPORT = {}


@pytest.fixture(scope="module")
def ogg(hip):
    import ocean_model_grid_generator_amd.ocean_grid_generator as m
    return m


def maxabs(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def maxrel(a, b, floor=0.0):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor + 1e-300))) if a.size else 0.0


def record(name, **vals):
    REPORT[name] = vals
    out = os.environ.get("OGG_PARITY_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def fvec():
    return np.load(os.path.join(GOLD, "ref_functions.npz"))


# ---------------------------------------------------------------------------------------------------------------
# a1-a3: Mercator and lat-lon builders
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ni", [180, 1440, 5760, 11520])
def test_mercator_axis(ogg, fvec, Ni):
    phi = np.array([-66.85954725 * orc.PI_180, 64.05895973 * orc.PI_180])
    ys = ogg.y_mercator_rounded(Ni, phi)
    assert np.array_equal(ys, orc.y_mercator_rounded(Ni, phi))          # integers: exact
    yf = ogg.y_mercator(Ni, phi)
    assert maxrel(yf, orc.y_mercator(Ni, phi)) < 5e-16
    got = ogg.phi_mercator(Ni, np.arange(ys[0], ys[1] + 1))
    want = orc.phi_mercator(Ni, np.arange(ys[0], ys[1] + 1))
    assert maxabs(got, want) < 5e-14
    if "phiM_%d" % Ni in fvec:
        assert np.array_equal(ys, fvec["ymr_%d" % Ni])
        assert maxabs(got, fvec["phiM_%d" % Ni]) < 5e-14
    record("phi_mercator_%d" % Ni, maxabs=maxabs(got, want))


@pytest.mark.parametrize("even", [True, False])
def test_generate_mercator_grid(ogg, even):
    x, y = ogg.generate_mercator_grid(720, -66.85954725, 64.05895973, -300.0, 360, 1.0, True, even)
    ox, oy = orc.generate_mercator_grid(720, -66.85954725, 64.05895973, -300.0, 360, 1.0, True, even)
    assert np.array_equal(x, ox)                                         # i*360/Ni: exact arithmetic
    assert maxabs(y, oy) < 5e-14


def test_mercator_enhanced_equator(ogg):
    x, y = ogg.generate_mercator_grid(1440, -68.0, 65.0, -300.0, 360, 2.0, True, False, enhanced_equatorial=4)
    ox, oy = orc.generate_mercator_grid(1440, -68.0, 65.0, -300.0, 360, 2.0, True, False, enhanced_equatorial=4)
    assert x.shape == ox.shape and maxabs(y, oy) < 1e-13 and np.array_equal(x, ox)


def test_generate_latlon_grid(ogg, fvec):
    x, y = ogg.generate_latlon_grid(24, 5, -300.0, 360, -78.0, 11.3, ensure_nj_even=True)
    assert np.array_equal(x, fvec["ll_x"]) and np.array_equal(y, fvec["ll_y"])   # +,*,/ only: bit-exact
    x, y = ogg.generate_latlon_grid(1440, 110, -300.0, 360, -78.0, 11.11590341532381, ensure_nj_even=False)
    ox, oy = orc.generate_latlon_grid(1440, 110, -300.0, 360, -78.0, 11.11590341532381, ensure_nj_even=False)
    assert np.array_equal(x, ox) and np.array_equal(y, oy)


# ---------------------------------------------------------------------------------------------------------------
# a4, a16, a17: mdist, MIDAS metrics, angle
# ---------------------------------------------------------------------------------------------------------------
def test_mdist_exact(ogg, fvec):
    assert np.array_equal(ogg.mdist(fvec["mdist_a"], fvec["mdist_b"]), fvec["mdist_out"])   # fmod is exact
    assert np.array_equal(ogg.mdist(fvec["mdist_a"], -300.0), orc.mdist(fvec["mdist_a"], -300.0))


def test_midas_golden_distorted_mesh(ogg, fvec):
    x, y = fvec["md_x"], fvec["md_y"]
    dx, dy, area = ogg.generate_grid_metrics_MIDAS(x, y)
    assert maxrel(dx, fvec["md_dx"]) < 2e-15 and maxrel(dy, fvec["md_dy"]) < 2e-15
    assert maxrel(area, fvec["md_area"]) < 5e-12
    _, _, area2 = ogg.generate_grid_metrics_MIDAS(x, y, latlon_areafix=False)
    assert maxrel(area2, fvec["md_area_nofix"]) < 5e-15
    ang = ogg.angle_x(x, y)
    assert maxabs(ang, fvec["md_angle"]) < 1e-12
    # ... and every element within its conditioned bound of the oracle (tests/stencil_bounds.py)
    stencil_bounds.check_against_oracle(x, y, {"dx": dx, "dy": dy, "area": area, "area_nofix": area2, "angle": ang}, name="golden distorted mesh")


@pytest.mark.parametrize("shape", [(1, 2), (1, 300), (2, 2), (40, 2), (3, 65), (17, 64), (33, 257), (200, 1000)])
def test_midas_ragged_shapes(ogg, shape):
    """Lat-lon meshes with 0.05 degrees of noise to +-80 degrees and to +-89.99 degrees (the noise carries points of the outer rows past the
    pole).  The relative lines stay on both ranges: at +-80 degrees the conditioned bound of dx and dy, 2.5 s, is 1.4e-15 to 6e-15 of the value,
    not always under their 2e-15 (tests/test_stencil_bounds_cpu.py::test_check_against_oracle); the conditioned check is added to them."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    nj, ni = shape
    for lat_max in (80.0, 89.99):
        x = np.tile(-300 + np.arange(ni) * 360.0 / max(ni - 1, 1), (nj, 1)) + rng.normal(0, 0.05, shape)
        y = np.tile(np.linspace(-lat_max, lat_max, nj).reshape(nj, 1), (1, ni)) + rng.normal(0, 0.05, shape)
        dx, dy, area = ogg.generate_grid_metrics_MIDAS(x, y)
        odx, ody, oar = orc.generate_grid_metrics_MIDAS(x, y)
        assert dx.shape == odx.shape and dy.shape == ody.shape and area.shape == oar.shape     # a single row: dy and area are empty, like numpy's
        # against the ORACLE the relative lines hold next to the pole as well: the device does the oracle's operations on the oracle's bits,
        # so lv is the same double and the two cos(lv) differ by an ulp of a well-conditioned call.  (Against the truth they would not
        # hold there: the rounding of lv itself is what the conditioned bound allows for.)  A failure here is an arithmetic difference.
        assert maxrel(dx, odx) < 2e-15 and maxrel(dy, ody) < 2e-15
        assert maxabs(area, oar) <= 5e-12 * (np.abs(oar).max() if oar.size else 1.0)
        ang = ogg.angle_x(x, y)
        assert maxabs(ang, orc.angle_x(x, y)) < 1e-11
        rep = stencil_bounds.check_against_oracle(x, y, {"dx": dx, "dy": dy, "area": area, "angle": ang,
                                                         "area_nofix": ogg.generate_grid_metrics_MIDAS(x, y, latlon_areafix=False)[2]},
                                                  name="ragged %s to %g degrees" % (shape, lat_max))
        record("midas_ragged_%dx%d_lat%g" % (nj, ni, lat_max), **{f: r["worst_over_bound"] for f, r in rep.items()})


@pytest.mark.parametrize("shape", [(2, 2), (5, 63), (7, 258), (31, 513), (200, 1000), (64, 5761)])
def test_midas_tile_heights_and_streaming_kernel_agree_bitwise(hip, ogg, shape, monkeypatch):
    """Two implementations of the generic stencil kernel -- the LDS-staged tile walk (mdist from one reduction, non-temporal stores)
    at every tile height, and the streaming walk of rounds 1-3 (OGG_MIDAS_TILE_ROWS=0: rows straight from global memory, wave shuffles,
    mdist from two reductions) -- must give the same BITS on a distorted mesh whose longitudes wrap around, for both area forms and for
    the angle-only call.  At the default target of 2048 workgroups every one of these shapes plans two rows per tile whatever the setting, so
    the settings are run again with OGG_MIDAS_TARGET_WG=1, one workgroup per column tile, where each plans the height its name says (as
    far as the mesh has rows: at most 12, 16 for the streaming kernel); the plan is asserted through the library's query."""
    rng = np.random.default_rng(shape[0] * 7919 + shape[1])
    nj, ni = shape
    x = np.tile(-300 + np.arange(ni) * 720.0 / max(ni - 1, 1), (nj, 1)) + rng.normal(0, 0.05, shape)     # twice around: mod 360 at work
    y = np.tile(np.linspace(-89.5, 89.5, nj).reshape(nj, 1), (1, ni)) + rng.normal(0, 0.05, shape)
    x[0, 0], x[-1, -1] = x[0, 1], x[-1, -2] + 1e-20                                                       # a zero and a tiny difference
    ref = None
    gx = (ni + 255) // 256
    for target, rows in [(t, r) for t in (None, "1") for r in ("0", "1", "2", "4", "6", "8", "12", "99")]:
        monkeypatch.setenv("OGG_MIDAS_TILE_ROWS", rows)
        if target is None:
            monkeypatch.delenv("OGG_MIDAS_TARGET_WG", raising=False)
            want = (4, min(2, nj)) if rows != "0" else (0, 4)
        else:
            monkeypatch.setenv("OGG_MIDAS_TARGET_WG", target)
            h = min(int(rows), 12, nj)
            want = (4 if h <= 4 else 6 if h <= 6 else 8 if h <= 8 else 12, h) if rows != "0" else (0, min(max(nj * gx, 4), 16))
        assert stencil_plans.planned(hip, ni, nj, True) == want, (target, rows)
        got = ogg.generate_grid_metrics_MIDAS(x, y) + ogg.generate_grid_metrics_MIDAS(x, y, latlon_areafix=False)[2:] + (ogg.angle_x(x, y),)
        if ref is None:
            ref = got
            odx, ody, oar = orc.generate_grid_metrics_MIDAS(x, y)
            assert maxrel(got[0], odx) < 2e-15 and maxrel(got[1], ody) < 2e-15 and maxabs(got[2], oar) <= 5e-12 * np.abs(oar).max()
            continue
        for k, (a, b) in enumerate(zip(ref, got)):
            assert np.array_equal(a, b), (target, rows, k, float(np.abs(a - b).max()))


def test_midas_mercator_r8_band(ogg):
    """The HBM-bound kernel at 1/8 degree width (5761 columns), 400 rows."""
    xo, yo = orc.generate_mercator_grid(5760, -66.85954725, 64.05895973, -300.0, 360, 8.0, True, False)
    xo, yo = np.ascontiguousarray(xo[1000:1400]), np.ascontiguousarray(yo[1000:1400])
    dx, dy, area = ogg.generate_grid_metrics_MIDAS(xo, yo)
    odx, ody, oar = orc.generate_grid_metrics_MIDAS(xo, yo)
    record("midas_r8_band", dx=maxabs(dx, odx), dy=maxabs(dy, ody), area=maxabs(area, oar), area_rel=maxrel(area, oar))
    assert maxrel(dx, odx) < 2e-15 and maxrel(dy, ody) < 2e-15 and maxrel(area, oar) < 5e-12
    ang = ogg.angle_x(xo, yo)
    assert np.array_equal(ang, orc.angle_x(xo, yo))     # atan2(0, +) == 0 on a lat-lon mesh
    rep = stencil_bounds.check_against_oracle(xo, yo, {"dx": dx, "dy": dy, "area": area, "angle": ang}, name="Mercator 1/8 degree band")
    record("midas_r8_band_conditioned", **{f: r["worst_over_bound"] for f, r in rep.items()})


def test_midas_mercator_r16_band(ogg):
    """The same at 1/16 degree width (11521 columns, BASELINE config 5), 200 rows of the Mercator sub-grid either side of 50 S."""
    phi = orc.phi_mercator(11520, np.arange(-2909, 2691 + 1))
    j0 = int(np.searchsorted(phi, -50.0)) - 100
    lam = -300.0 + np.arange(11521) * 360 / float(11520)
    xo = np.ascontiguousarray(np.tile(lam, (201, 1)))
    yo = np.ascontiguousarray(np.tile(phi[j0:j0 + 201].reshape(-1, 1), (1, 11521)))
    dx, dy, area = ogg.generate_grid_metrics_MIDAS(xo, yo)
    odx, ody, oar = orc.generate_grid_metrics_MIDAS(xo, yo)
    record("midas_r16_band", dx=maxabs(dx, odx), dy=maxabs(dy, ody), area=maxabs(area, oar), area_rel=maxrel(area, oar))
    assert maxrel(dx, odx) < 2e-15 and maxrel(dy, ody) < 2e-15 and maxrel(area, oar) < 5e-12
    assert np.array_equal(ogg.angle_x(xo, yo), orc.angle_x(xo, yo))


def test_angle_shape_error(ogg):
    with pytest.raises(Exception, match="same shape"):
        ogg.angle_x(np.zeros((3, 4)), np.zeros((3, 5)))


# ---------------------------------------------------------------------------------------------------------------
# a5-a9: bipolar cap
# ---------------------------------------------------------------------------------------------------------------
def test_bipolar_projection_golden_special_points(ogg, fvec):
    lams, phis, hi, hj = ogg.bipolar_projection(fvec["bp_lamg"], fvec["bp_phig"], float(fvec["bp_lon_bp"]), float(fvec["bp_rp"]))
    lamg, phig = fvec["bp_lamg"], fvec["bp_phig"]
    pole = phig == 90.0
    # exact special values the reference guarantees: symmetry meridians and the pole row
    dl = lamg - float(fvec["bp_lon_bp"])
    assert np.all(lams[dl == 90] == float(fvec["bp_lon_bp"]) + 90) and np.all(lams[dl == 270] == float(fvec["bp_lon_bp"]) + 270)
    assert maxabs(lams[~pole], fvec["bp_lams"][~pole]) < TOL_COORD_ILL and maxabs(phis, fvec["bp_phis"]) < TOL_COORD_ILL
    assert maxrel(hi, fvec["bp_hi"]) < 1e-12 and maxrel(hj, fvec["bp_hj"]) < 1e-12
    hi2, hj2 = ogg.bipolar_projection(lamg, phig, float(fvec["bp_lon_bp"]), float(fvec["bp_rp"]), metrics_only=True)
    assert np.array_equal(hi2, hi) and np.array_equal(hj2, hj)


@pytest.mark.parametrize("Ni,Nj,lat0", [(48, 10, 64.05895973), (1440, 238, 64.97316302279852), (5760, 960, 64.03160594077568),
                                        (11520, 1920, 64.04528618884338)])
def test_bipolar_cap_mesh(ogg, fvec, Ni, Nj, lat0):
    lams, phis, hi, hj = ogg.generate_bipolar_cap_mesh(Ni, Nj, lat0, -300.0, ensure_nj_even=False)
    ol, op, ohi, ohj = orc.generate_bipolar_cap_mesh(Ni, Nj, lat0, -300.0, False)
    # known answers
    assert phis[-1, Ni // 4] == 90.0 and phis[-1, 3 * Ni // 4] == 90.0
    assert np.all(lams[:, Ni // 4] == -300.0 + 90)
    assert abs(phis[-1, 0] - lat0) < 1e-12 and abs(phis[-1, Ni // 2] - lat0) < 1e-12
    d = np.abs(lams - ol)
    ill = np.zeros(lams.shape, bool)
    for c in (Ni // 4, 3 * Ni // 4):
        ill[:, max(c - 2, 0):c + 3] = True                   # cells adjacent to the symmetry meridians
    ill[-1, :] = True                                         # the fold row through the two poles
    record("bp_mesh_%d" % Ni, x_all=float(d.max()), x_regular=float(d[~ill].max()), y=maxabs(phis, op),
           frac_x_gt_1e12=float((d > 1e-12).mean()))
    # north_star's 1e-12 degrees at EVERY point, the symmetry meridians and the two pole points included (measured: x <= 8.8e-13 at 1/16
    # degree, y <= 2.8e-14; rounds 1-2 needed 2e-11 / 1e-6 at those points, before asin / acos were restated from the library)
    assert d.max() < TOL_COORD
    dy_ = np.abs(phis - op)
    assert dy_.max() < TOL_COORD
    assert maxrel(hi, ohi) < 1e-11 and maxrel(hj, ohj) < 1e-11
    if Ni == 48:
        assert maxabs(lams, fvec["bpm_lams"]) < TOL_COORD_ILL and maxabs(phis, fvec["bpm_phis"]) < TOL_COORD_ILL


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_bipolar_quad_golden_small(ogg, fvec, order):
    Ni, Nj, lat0 = int(fvec["bpm_Ni"]), int(fvec["bpm_Nj"]), float(fvec["bpm_lat0"])
    dxq, dyq, daq = ogg.bipolar_cap_metrics_quad_fast(order, Ni, Nj, lat0, float(fvec["bp_lon_bp"]), float(fvec["bp_rp"]))
    for a, k in ((dxq, "dx"), (dyq, "dy"), (daq, "da")):
        assert maxrel(a, fvec["bpq%d_%s" % (order, k)]) < 5e-14, k


def test_bipolar_quad_uncoded_order(ogg):
    with pytest.raises(Exception, match="Uncoded order"):
        ogg.bipolar_cap_metrics_quad_fast(6, 48, 10, 64.0, -300.0, 0.23)


@pytest.mark.parametrize("Ni,Nj,lat0", [(1440, 238, 64.97316302279852), (333, 7, 70.0)])
def test_bipolar_quad_vs_oracle(ogg, Ni, Nj, lat0):
    rp = np.tan(0.5 * (90 - lat0) * orc.PI_180)
    got = ogg.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
    want = orc.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
    record("bp_quad_%d" % Ni, dx=maxrel(got[0], want[0]), dy=maxrel(got[1], want[1]), area=maxrel(got[2], want[2]),
           area_abs=maxabs(got[2], want[2]))
    for g, w in zip(got, want):
        assert maxrel(g, w) < 5e-14
    # analytic self-check of the reference (OGG:732-770): % errors of sum(area), meridian arc, parallel arc, fold
    err = orc.metrics_error(got[0], got[1], got[2], Ni, lat0, 90.0, bipolar=True)
    oerr = orc.metrics_error(want[0], want[1], want[2], Ni, lat0, 90.0, bipolar=True)
    assert max(abs(a - b) for a, b in zip(err, oerr)) < 1e-11
    if Ni == 1440:
        assert max(abs(e) for e in err) < 1e-9


def _libm_check(which, x, y=None):
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    n_diff = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    L.call("ogg_libm_check_dev", which, x.numel(), x.data_ptr(), y.data_ptr() if y is not None else None, n_diff.data_ptr(),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(n_diff.item())


def test_asin_unit_equals_library_asin(hip):
    """The mesh takes asin from a restatement of the device library's own algorithm (coefficients as scalar operands): every bit must
    agree with asin(), on 4e7 arguments of [0, 1] incl. the ends, the neighbours of 0.5 and of 1, and tiny values."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(11)
    n = 40_000_000
    x = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g)
    x[: n // 8] = x[: n // 8] ** 8                          # small arguments
    x[n // 8: n // 4] = 1.0 - x[n // 8: n // 4] ** 6        # next to 1
    special = torch.tensor([0.0, 1.0, 0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1), np.nextafter(1.0, 0), 5e-324, 1e-300, 2.0 ** -27,
                            2.0 ** -540], dtype=torch.float64, device="cuda:0")
    x[-special.numel():] = special
    assert _libm_check(0, x) == 0


def test_atan_atan2_restatements_equal_the_library(hip):
    """atan_lib / atan2_lib (ogg_math.h) against the device library's atan / atan2: every bit, 4e7 arguments each over 600 binades,
    both signs, signed zeros, equal magnitudes, arguments next to 1."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(12)
    n = 40_000_000

    def spread(k):
        m = torch.rand(k, dtype=torch.float64, device="cuda:0", generator=g) + 1.0
        e = torch.randint(-300, 300, (k,), device="cuda:0", generator=g).to(torch.float64)
        sgn = torch.randint(0, 2, (k,), device="cuda:0", generator=g).to(torch.float64) * 2 - 1
        return sgn * m * torch.exp2(e)

    x = spread(n)
    x[: n // 4] = (torch.rand(n // 4, dtype=torch.float64, device="cuda:0", generator=g) * 4 - 2)       # around +-1
    sp = torch.tensor([0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0), 5e-324, -5e-324, 1.7e308, -1.7e308,
                       float("inf"), float("-inf")], dtype=torch.float64, device="cuda:0")
    x[-sp.numel():] = sp
    assert _libm_check(1, x) == 0
    y = spread(n)
    x = spread(n)
    q = n // 4
    x[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 2 - 1                     # comparable magnitudes
    y[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 2 - 1
    y[q: q + 1000] = x[q: q + 1000]                                                                      # |y| == |x|
    fy = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 3.0, 5e-324], dtype=torch.float64, device="cuda:0")
    fx = torch.tensor([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 2.0, -2.0, -5e-324, 1.7e308], dtype=torch.float64, device="cuda:0")
    y[-fy.numel():] = fy
    x[-fx.numel():] = fx
    assert _libm_check(2, x, y) == 0


def test_rcp_and_sqrt_without_scaling_equal_the_ieee_operations(hip):
    """rcp_ieee_normal / sqrt_ieee_normal (ogg_math.h: the compiler's own fma sequences without the scaling and special-case steps) against
    1.0 / x and sqrt(x): every bit, 4e7 operands over 2^-700 .. 2^700 incl. powers of two and their neighbours."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(13)
    n = 40_000_000
    m = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g) + 1.0
    m[: n // 16] = 1.0 + torch.randint(0, 64, (n // 16,), device="cuda:0", generator=g).to(torch.float64) * 2.0 ** -52      # just above 2^k
    m[n // 16: n // 8] = 2.0 - (1 + torch.randint(0, 64, (n // 16,), device="cuda:0", generator=g).to(torch.float64)) * 2.0 ** -52
    e = torch.randint(-700, 700, (n,), device="cuda:0", generator=g).to(torch.float64)
    x = torch.ldexp(m, e.to(torch.int32))
    x[n // 2:] = 1.0 + torch.rand(n - n // 2, dtype=torch.float64, device="cuda:0", generator=g) * 1e6      # the mesh's 1 + a b
    x[-4:] = torch.tensor([1.0, 2.0 ** -700, 2.0 ** 700, 4.0], dtype=torch.float64, device="cuda:0")
    assert _libm_check(3, x) == 0
    x[n // 2:] = 1.0 / x[n // 2:]                                                                          # the mesh's rden
    assert _libm_check(4, x) == 0


def test_division_without_scaling_and_vector_register_arctangents_equal_the_library(hip):
    """The forms the literal displaced-pole quadrature takes (ogg_math.h): y / x without v_div_scale / v_div_fmas / v_div_fixup for
    operands within 2^-300 .. 2^300 (or y = +-0); atan / atan2 with their coefficients in vector registers and the fma chain as one asm
    statement.  Every bit against the device library, 2e7 arguments each."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(14)
    n = 20_000_000

    def spread(k, emax):
        m = torch.rand(k, dtype=torch.float64, device="cuda:0", generator=g) + 1.0
        e = torch.randint(-emax, emax, (k,), device="cuda:0", generator=g).to(torch.float64)
        sgn = torch.randint(0, 2, (k,), device="cuda:0", generator=g).to(torch.float64) * 2 - 1
        return sgn * m * torch.exp2(e)

    x, y = spread(n, 300), spread(n, 300)
    q = n // 4
    x[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 4 - 2        # the quadrature's own range: O(1) operands
    y[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 4 - 2
    y[q: q + 1000] = x[q: q + 1000]
    y[q + 1000: q + 2000] = 0.0
    y[q + 2000: q + 3000] = -0.0
    assert _libm_check(5, x, y) == 0
    x2, y2 = spread(n, 300), spread(n, 300)
    x2[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 4 - 2
    y2[:q] = torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) * 4 - 2
    fy = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 3.0, 5e-324], dtype=torch.float64, device="cuda:0")
    fx = torch.tensor([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 2.0, -2.0, -5e-324, 1.7e308], dtype=torch.float64, device="cuda:0")
    y2[-fy.numel():] = fy
    x2[-fx.numel():] = fx
    assert _libm_check(7, x2, y2) == 0
    sp = torch.tensor([0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0), 5e-324, -5e-324, 1.7e308, -1.7e308,
                       float("inf"), float("-inf")], dtype=torch.float64, device="cuda:0")
    x2[-sp.numel():] = sp
    assert _libm_check(6, x2) == 0
    x3 = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g) * 2 - 1           # |x| <= 1 everywhere: the wave-uniform short path
    assert _libm_check(6, x3) == 0
    # the generic stencil kernel takes a caller's arrays: infinities and NaNs must come out as the library's atan2 gives them
    inf, nan = float("inf"), float("nan")
    sy = torch.tensor([inf, inf, -inf, -inf, inf, -inf, 1.0, -1.0, 1.0, -1.0, nan, 1.0, nan, inf, 0.0, -0.0], dtype=torch.float64, device="cuda:0")
    sx = torch.tensor([inf, -inf, inf, -inf, 2.0, -3.0, inf, inf, -inf, -inf, 1.0, nan, nan, nan, inf, -inf], dtype=torch.float64, device="cuda:0")
    y2[: sy.numel()] = sy
    x2[: sx.numel()] = sx
    assert _libm_check(9, x2, y2) == 0


def test_mdist_restatements_equal_numpy_mod(hip, ogg):
    """mdist (OGG:682-684) from two fma reductions (ogg_math.h mdist) and from ONE (mdist_one: the generic stencil kernel's) against
    numpy.mod's own definition -- fmod, + 360 where negative -- evaluated on the device: every bit, 4e7 pairs: longitudes of a grid, differences
    within an ulp of multiples of 360, TINY differences of either sign (-2.8e-14 < d < 0: the exact d + 360 rounds to 360.0 -- numpy's answer,
    which the retry of round 1-3's pymod360 turned into a negative number), huge ones, infinities and NaNs."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(21)
    n = 40_000_000
    q = n // 5
    x = (torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g) - 0.5) * 1440.0
    y = (torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g) - 0.5) * 1440.0
    k = torch.randint(-6, 7, (q,), device="cuda:0", generator=g).to(torch.float64)
    ulps = torch.randint(-2, 3, (q,), device="cuda:0", generator=g).to(torch.float64)
    y[:q] = x[:q] + 360.0 * k + ulps * 2.0 ** -43                                   # within a few ulp of a multiple of 360 apart
    e = torch.randint(-1070, -40, (q,), device="cuda:0", generator=g).to(torch.int32)
    sgn = torch.randint(0, 2, (q,), device="cuda:0", generator=g).to(torch.float64) * 2 - 1
    tiny = sgn * torch.ldexp(torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) + 1.0, e)
    x[q:2 * q] = tiny                                                               # tiny differences of either sign (y = 0)
    y[q:2 * q] = 0.0
    big = torch.ldexp(torch.rand(q, dtype=torch.float64, device="cuda:0", generator=g) + 1.0, torch.randint(30, 200, (q,), device="cuda:0", generator=g).to(torch.int32))
    x[2 * q:3 * q] = big * sgn                                                      # up to 2^200 (beyond 1e12: the fmod path)
    sp = torch.tensor([0.0, -0.0, 360.0, -360.0, 720.0, 1e-20, -1e-20, 2.8e-14, -2.8e-14, -2.9e-14, float("inf"), float("-inf"), float("nan"), 1e12, -1e12],
                      dtype=torch.float64, device="cuda:0")
    x[-sp.numel():] = sp
    y[-sp.numel():] = 0.0
    for which in (13, 14):
        assert _libm_check(which, x, y) == 0, which
    # the host-pointer entry, tiny operands: numpy's values bit for bit
    a = np.array([1e-20, -1e-20, -2e-14, 2e-14, -3e-14, 5e-324, -5e-324, 359.99999999999994, -359.99999999999994])
    assert np.array_equal(ogg.mdist(a, 0.0), orc.mdist(a, 0.0)) and np.array_equal(ogg.mdist(0.0, a), orc.mdist(0.0, a))


def test_bipolar_mesh_does_not_depend_on_rows_per_workgroup(ogg, monkeypatch):
    got = []
    for rows in ("8", "1", "5", "32"):
        monkeypatch.setenv("OGG_MESH_ROWS", rows)
        got.append(ogg.generate_bipolar_cap_mesh(720, 61, 64.05895973, -300.0))
    for g in got[1:]:
        for a, b in zip(got[0][:2], g[:2]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_bipolar_quad_does_not_depend_on_chunking(ogg, order, monkeypatch):
    """A wave walks a chunk of cell rows; where the chunks end depends on the size of the band (OGG_QUAD_TARGET_WAVES, band sharding).
    The value of a cell must not: every chunk length gives the same bits (1 row per chunk ... the whole cap in one chunk)."""
    Ni, Nj, lat0 = 1440, 96, 64.05895973
    rp = np.tan(0.5 * (90 - lat0) * orc.PI_180)
    got = []
    for target in ("1000000", "700", "97", "1"):
        monkeypatch.setenv("OGG_QUAD_TARGET_WAVES", target)
        got.append(ogg.bipolar_cap_metrics_quad_fast(order, Ni, Nj, lat0, -300.0, rp))
    for g in got[1:]:
        for a, b in zip(got[0], g):
            assert np.array_equal(a, b)


def test_bipolar_quad_full_size_r8_by_zone(ogg):
    """BASELINE config 2's cap (5760 x 960 cells) against the oracle, in bands from the joint to the pole: the algebraic
    per-point form, the guarded rows and the cells re-evaluated by the literal fix-up must all stay at the same level."""
    Ni, Nj, lat0 = 5760, 960, 64.03160594077568
    rp = np.tan(0.5 * (90 - lat0) * orc.PI_180)
    got = ogg.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
    worst = {}
    for a, b in ((0, 24), (470, 494), (860, 890), (890, 930), (930, 960)):
        want = orc.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp, rows_per_chunk=8, j_first=a, j_last=b)
        for g, w, name in zip(got, want, ("dx", "dy", "area")):
            gg, ww = g[a:b], w[a:b]
            m = ww != 0
            assert np.array_equal(gg[~m], ww[~m])                      # dy == 0 on the meridians alpha2 == 1
            worst[(name, a)] = float((np.abs(gg - ww)[m] / np.abs(ww[m])).max())
        assert maxabs(got[2][a:b], want[2][a:b]) < 1e-6                # north_star: area diff < 1e-6 m^2
    record("bp_quad_r8_zones", **{"%s_%d" % k: v for k, v in worst.items()})
    assert max(worst.values()) < 5e-14


def test_bipolar_quad_full_size_r16_by_zone(ogg):
    """BASELINE config 5's cap (11520 x 1920 cells, 1/16 degree) against the oracle by zones -- the joint, mid-cap, 88 degrees (where the
    guarded rows begin), 89 degrees, the pole rows -- at the bounds of the 1/8 degree test: pole-adjacent cells are half the size here and
    the literal sequence of OGG:69-79 loses more digits there, which the guard (K = 4000) and the literal fix-up must absorb."""
    Ni, Nj, lat0 = 11520, 1920, 64.04528618884338
    rp = np.tan(0.5 * (90 - lat0) * orc.PI_180)
    got = ogg.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
    worst, worst_area = {}, 0.0
    for a, b in ((0, 16), (950, 966), (1764, 1780), (1838, 1854), (1888, 1920)):
        want = orc.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp, rows_per_chunk=4, j_first=a, j_last=b)
        for g, w, name in zip(got, want, ("dx", "dy", "area")):
            gg, ww = g[a:b], w[a:b]
            m = ww != 0
            assert np.array_equal(gg[~m], ww[~m])                      # dy == 0 on the meridians alpha2 == 1
            worst[(name, a)] = float((np.abs(gg - ww)[m] / np.abs(ww[m])).max())
        worst_area = max(worst_area, maxabs(got[2][a:b], want[2][a:b]))
        del want
    record("bp_quad_r16_zones", area_max_abs=worst_area, **{"%s_%d" % k: v for k, v in worst.items()})
    assert worst_area < 1e-6                                            # north_star: area diff < 1e-6 m^2 (measured 7.2e-8)
    # the cells that touch the two pole points (last zone): 6.0e-14 relative in area WITH EVERY CELL LITERAL (OGG_BP_GUARD_K=0,
    # scripts/guard_k_probe.py r16: ocml against the host libm through the reference's own acos -> tan -> atan -> cos round trip); the
    # guard (K = 4000) adds nothing to it (dx 1.6e-14, dy 1.9e-14, area 6.0e-14 with and without)
    pole_area = worst.pop(("area", 1888))
    assert pole_area < 2e-13 and max(worst.values()) < 5e-14, (pole_area, worst)


def test_bipolar_cap_ij_array(ogg):
    rng = np.random.default_rng(5)
    i, j = np.sort(rng.uniform(0, 48, 33)), np.sort(rng.uniform(0, 9.9, 7))
    hi, hj = ogg.bipolar_cap_ij_array(i, j, 48, 10, 64.05895973, -300.0, 0.2313)
    ohi, ohj = orc.bipolar_cap_ij_array(i, j, 48, 10, 64.05895973, -300.0, 0.2313)
    assert maxrel(hi, ohi) < 1e-13 and maxrel(hj, ohj) < 1e-13


# ---------------------------------------------------------------------------------------------------------------
# a10-a15: displaced-pole cap
# ---------------------------------------------------------------------------------------------------------------
def _dp(fvec):
    return [int(fvec["dp_Ni"]), int(fvec["dp_Nj"]), float(fvec["dp_lon0"]), float(fvec["dp_lat0"]), float(fvec["dp_lon_dp"]),
            float(fvec["dp_r_dp"])]


def test_displaced_pole_grid_golden(ogg, fvec):
    x, y, londp, latdp = ogg.generate_displaced_pole_grid(*_dp(fvec))
    assert maxabs(x, fvec["dp_x"]) < TOL_COORD and maxabs(y, fvec["dp_y"]) < TOL_COORD
    assert abs(londp - fvec["dp_pole"][0]) < TOL_COORD and abs(latdp - fvec["dp_pole"][1]) < TOL_COORD
    assert np.all(np.abs(x[0, :] - (80.0 - 360)) < TOL_COORD)                    # pole row is (lon_dp-360, lat_dp)


def test_displaced_pole_mesh_fractional_golden(ogg, fvec):
    lam, phi, _, _ = ogg.displacedPoleCap_mesh(fvec["dpf_i"], fvec["dpf_j"], *_dp(fvec))
    assert maxabs(lam, fvec["dpf_lam"]) < TOL_COORD and maxabs(phi, fvec["dpf_phi"]) < TOL_COORD
    gad = ogg.great_arc_distance(fvec["dpf_j"], fvec["dpf_i"] + 1e-3, fvec["dpf_j"], fvec["dpf_i"] - 1e-3, *_dp(fvec))
    assert maxrel(gad, fvec["dp_gad"]) < dp_quad_rel_tol(_dp(fvec)[0])


@pytest.mark.parametrize("Ni,Nj,r_dp", [(1440, 140, 0.2), (720, 70, 0.34135899793333113), (5760, 560, 0.2)])
def test_displaced_pole_grid_unwrap(ogg, Ni, Nj, r_dp):
    """x must follow the sequential unwrap exactly: any wrong state would show as a 360 degree error."""
    x, y, _, _ = ogg.generate_displaced_pole_grid(Ni, Nj, -300.0, -78.0, 80.0, r_dp)
    ox, oy, _, _ = orc.generate_displaced_pole_grid(Ni, Nj, -300.0, -78.0, 80.0, r_dp)
    record("dp_mesh_%d" % Ni, x=maxabs(x, ox), y=maxabs(y, oy))
    assert maxabs(x, ox) < TOL_COORD and maxabs(y, oy) < TOL_COORD


def test_monotonic_bounding_and_projection(ogg):
    rng = np.random.default_rng(11)
    v = rng.uniform(-180, 180, (9, 700))
    v[:, 300:] = np.sort(v[:, 300:], axis=1)
    want = orc.monotonic_bounding(v.copy(), -300.0)
    got = ogg.monotonic_bounding(v.copy(), -300.0)
    assert np.array_equal(got, want)                                              # comparisons and -360 only: bit-exact
    lon = np.tile(-300 + np.arange(600) * 0.6, (5, 1))
    lat = np.tile(np.linspace(-90, -78, 5).reshape(5, 1), (1, 600))
    z0 = 0.2 * (np.cos(80 * orc.PI_180) + 1j * np.sin(80 * orc.PI_180))
    rj = np.tan((90 - 78.0) * orc.PI_180)
    lam, phi = ogg.displacedPoleCap_projection(lon, lat, z0, rj)
    olam, ophi = orc.displacedPoleCap_projection(lon, lat, z0, rj)
    assert maxabs(lam, olam) < TOL_COORD and maxabs(phi, ophi) < TOL_COORD
    u, v2, du, dv = ogg.displacedPoleCap_baseGrid(np.arange(5.0), np.arange(4.0), 72, 14, -300.0, -78.0)
    assert np.array_equal(u, -300.0 + np.arange(5.0) * 360.0 / 72.0) and np.array_equal(v2, -90.0 + np.arange(4.0) * 12.0 / 14.0)


@pytest.mark.parametrize("arc_form", [None, "literal", "chord"])
@pytest.mark.parametrize("order", [2, 4])
def test_displaced_pole_quad_golden_small(ogg, fvec, order, arc_form):
    """Against the vectors of the reference itself; arc_form None = the default (the chord form, OGG_DP_ARC)."""
    got = ogg.displacedPoleCap_metrics_quad(order, *_dp(fvec), arc_form=arc_form)
    if arc_form is None:
        for a, b in zip(got, ogg.displacedPoleCap_metrics_quad(order, *_dp(fvec), arc_form="chord")):
            assert np.array_equal(a, b)
    for a, k in zip(got, ("dx", "dy", "da")):
        want = fvec["dpq%d_%s" % (order, k)]
        # row 0 is the pole itself (h -> 0): compare relative to the field's scale
        assert maxabs(a, want) <= dp_quad_rel_tol(_dp(fvec)[0]) * np.abs(want).max(), (k, maxabs(a, want))


def test_c_entry_points_without_arc_form_run_the_default_form(hip, ogg):
    """ogg_displaced_pole_metrics_quad (no arc_form argument) is the chord form since round 4, like the Python host's default: one
    default on every layer; the literal form through the *_form entry points."""
    from ocean_model_grid_generator_amd import _lib as L
    nx, ny = 360, 40
    a = [np.empty((ny + 1, nx)), np.empty((ny, nx + 1)), np.empty((ny, nx))]
    L.call("ogg_displaced_pole_metrics_quad", 4, nx, ny, -300.0, -78.0, 80.0, 0.2, 6371.0e3, L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]))
    chord = ogg.displacedPoleCap_metrics_quad(4, nx, ny, -300.0, -78.0, 80.0, 0.2, arc_form="chord")
    lit = ogg.displacedPoleCap_metrics_quad(4, nx, ny, -300.0, -78.0, 80.0, 0.2, arc_form="literal")
    for x, c, l in zip(a, chord, lit):
        assert np.array_equal(x, c) and not np.array_equal(x, l)


def test_displaced_pole_quad_order_not_coded(ogg):
    for order in (3, 5):
        with pytest.raises(Exception, match="order not coded"):
            ogg.displacedPoleCap_metrics_quad(order, 72, 14, -300.0, -78.0, 80.0, 0.2)
    with pytest.raises(Exception, match="order not coded"):
        ogg.numerical_hi(np.arange(3.0), np.arange(3.0), 72, 14, -300.0, -78.0, 80.0, 0.2, 1e-3, order=3)


@pytest.mark.parametrize("arc_form", ["literal", "chord"])
@pytest.mark.parametrize("Ni,Nj,r_dp,order", [(1440, 140, 0.2, 4), (720, 70, 0.34135899793333113, 4), (360, 70, 0.2, 2), (100, 9, 0.5, 4)])
def test_displaced_pole_quad_vs_oracle(ogg, Ni, Nj, r_dp, order, arc_form):
    """Whole cap, the rows around r = r_pole (where the longitude swings by 180 degrees between two columns) included; both arc
    forms are held to the same bound: at every size they are equally far from the oracle (see dp_quad_rel_tol)."""
    got = ogg.displacedPoleCap_metrics_quad(order, Ni, Nj, -300.0, -78.0, 80.0, r_dp, arc_form=arc_form)
    want = orc.displacedPoleCap_metrics_quad(order, Ni, Nj, -300.0, -78.0, 80.0, r_dp)
    jm = int(np.ceil(0.49 * Nj))
    rel = [float(np.max(np.abs(g[jm:] - w[jm:]) / np.abs(w[jm:]))) for g, w in zip(got, want)]
    record("dp_quad_%s_%d_o%d" % (arc_form, Ni, order), dx_rel=rel[0], dy_rel=rel[1], area_rel=rel[2], area_abs=maxabs(got[2][jm:], want[2][jm:]))
    assert max(rel) < dp_quad_rel_tol(Ni)
    for g, w in zip(got, want):                       # doughnut rows incl. the pole: relative to the field scale
        assert maxabs(g, w) <= dp_quad_rel_tol(Ni) * np.abs(w).max()


@pytest.mark.parametrize("Ni,Nj,kw,order", [(72, 14, dict(r_dp=0.2), 4), (72, 14, dict(r_dp=0.2), 2), (100, 9, dict(r_dp=0.35), 4),
                                            (720, 70, dict(r_dp=0.2), 4), (1440, 140, dict(r_dp=0.34135899793333113), 4),
                                            (2880, 40, dict(r_dp=0.05), 4)])
def test_literal_quad_walks_agree_bitwise(ogg, monkeypatch, Ni, Nj, kw, order):
    """Two independently written walks of the literal displaced-pole quadrature must give the same BITS: the LDS-pipelined one (pending
    rows in an LDS ring, batched look-back, restated arctangents with their coefficients in vector registers) and the register-pipelined
    one (OGG_DQ_WALK=regs: block-by-block look-back, the device library's own atan2 / atan).  A wrong unwrap state -- both probes of a pair
    lowered by 360 degrees or neither -- changes dx, dy, area by 1e-10 relative only, below what a comparison with the CPU oracle at its
    libm-noise tolerance can see; bit-identity of two implementations sees it (this test failed on a maps bug that every tolerance test
    passed)."""
    monkeypatch.delenv("OGG_DQ_WALK", raising=False)
    a = ogg.displacedPoleCap_metrics_quad(order, Ni, Nj, -300.0, -78.0, 80.0, kw["r_dp"], arc_form="literal")
    monkeypatch.setenv("OGG_DQ_WALK", "regs")
    b = ogg.displacedPoleCap_metrics_quad(order, Ni, Nj, -300.0, -78.0, 80.0, kw["r_dp"], arc_form="literal")
    for x, y, f in zip(a, b, ("dx", "dy", "area")):
        assert np.array_equal(x, y), (f, float(np.abs(x - y).max()), int((x != y).sum()))


def test_displaced_pole_quad_bands_are_bit_identical(hip):
    """Band form: any split of the cap's rows gives the bits of the whole cap (both arc forms), and the literal form's look-back
    raises no error flag."""
    import ctypes
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    Ni, Nj, order = 300, 41, 4
    st = torch.cuda.current_stream().cuda_stream

    def run(form, j0, n_dx, n_cell):
        wsb = int(lib.ogg_displaced_pole_quad_workspace_bytes(order, Ni, n_cell))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
        out = [torch.full(shp, float("nan"), dtype=torch.float64, device="cuda:0") for shp in ((n_dx, Ni), (n_cell, Ni + 1), (n_cell, Ni))]
        L.call("ogg_displaced_pole_metrics_quad_form_sym_ws_dev", form, L.SYM_DEFAULT, order, Ni, Nj, -300.0, -78.0, 80.0, 0.3, 6371.0e3, j0, n_dx, n_cell,
               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), wsb, st)
        flag = ctypes.c_int(-1)
        L.call("ogg_workspace_error_flag_dev", ws.data_ptr(), ctypes.byref(flag), st)
        assert flag.value == 0
        return [t.cpu().numpy() for t in out]

    for form in (L.DP_ARC_LITERAL, L.DP_ARC_CHORD):
        whole = run(form, 0, Nj + 1, Nj)
        assert not any(np.isnan(w).any() for w in whole)
        for cuts in ((0, 13, Nj), (0, 1, 2, 40, Nj), (0, Nj)):
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                parts.append(run(form, lo, hi - lo + (1 if hi == Nj else 0), hi - lo))
            for k in range(3):
                assert np.array_equal(np.concatenate([q[k] for q in parts]), whole[k]), (form, cuts, k)
        top = run(form, Nj, 1, 0)                      # a band that owns only the j = ny row of dxq
        assert np.array_equal(top[0][0], whole[0][Nj])


@pytest.mark.parametrize("fd", [2, 4, 6])
def test_numerical_h(ogg, fvec, fd):
    dp = _dp(fvec)
    hi = ogg.numerical_hi(fvec["dpf_j"], fvec["dpf_i"], *dp, eps=1e-3, order=fd)
    hj = ogg.numerical_hj(fvec["dpf_j"], fvec["dpf_i"], *dp, eps=1e-3, order=fd)
    ohi = orc.numerical_hi(fvec["dpf_j"], fvec["dpf_i"], *dp, eps=1e-3, order=fd)
    ohj = orc.numerical_hj(fvec["dpf_j"], fvec["dpf_i"], *dp, eps=1e-3, order=fd)
    tol = dp_quad_rel_tol(_dp(fvec)[0])
    assert maxabs(hi, ohi) <= tol * np.abs(ohi).max() and maxabs(hj, ohj) <= tol * np.abs(ohj).max()
    if fd == 6:
        assert maxabs(hi, fvec["dp_hi6"]) <= tol * np.abs(ohi).max()


# ---------------------------------------------------------------------------------------------------------------
# whole supergrid through main(): golden fixtures of the reference's own test configurations
# ---------------------------------------------------------------------------------------------------------------
def dp_quad_rel_tol(Ni):
    """Relative bound for the displaced-pole quadrature against the oracle: 10x the measured difference.  The reference
    differentiates a great-arc distance numerically with eps = 1e-3 index units (OGG:535-562): the two probes of a pair are
    2e-3 * 360/Ni degrees apart, one ulp of atan2 in either longitude moves their distance by ~2e-16 / (3.5e-5 * 360/Ni), and
    the measured difference between ocml and the host libm grows accordingly with Ni -- 7e-12 (Ni = 72), 7.5e-11 (360),
    2.4e-10 (1440), 1.3e-9 (5760, 1/8 degree); both arc forms, see DESIGN.md section 2."""
    return 2.0e-12 * Ni


# (abs, rel) per field and kind of sub-grid.  lat-lon sub-grids (Mercator, Southern Ocean, regular southern cap): x, y are
# +,-,*,/ only (bit-identical) except the Mercator atan(sinh); dx, dy, area one or two libm calls from them.  Bipolar cap: x next
# to the symmetry meridians and y at the two pole points are ill-conditioned in the reference itself.
SUB_TOL = {
    "latlon": {"x": (1e-13, 0.0), "y": (1e-13, 0.0), "dx": (1e-10, 5e-14), "dy": (2e-8, 5e-14), "area": (1e-6, 1.2e-11)},   # area: 10 x the measured 1.2e-12
    # (area: 6.5e-14 in the four cells that touch the pole points at 1/2 degree, <= 1e-14 elsewhere)
    # (x, y: the bound of the REGULAR points of the cap; the ill-conditioned ones keep TOL_COORD_ILL / 1e-6 by the masks of _row_tolerances)
    "bipolar": {"x": (TOL_COORD, 0.0), "y": (TOL_COORD, 0.0), "dx": (1e-9, 5e-14), "dy": (1e-9, 5e-14), "area": (1e-6, 2e-13)},
    # displaced-pole cap: metrics purely RELATIVE, dp_quad_rel_tol(Ni) (None below) -- at 1/8 degree that is 1.15e-8 of a 7 km cell: the
    # measured differences from the oracle are 1.3e-6 m (dx), 1.8e-6 m (dy) and 2e-3 m^2 (area), i.e. north_star's 1e-6 m^2 is NOT met
    # here, and cannot be: the fp64 reference itself is 1.2e-9 relative = 3e-3 m^2 away from the exact value of its own formula
    # (tests/test_gpu_truth.py, profiles/r04_truth_table.json)
    # (the 1e-9 m of dx only matters where a test keeps the cap's own pole row, exfracdp = 0: dx -> 0 there)
    "dpole": {"x": (TOL_COORD, 0.0), "y": (TOL_COORD, 0.0), "dx": (1e-9, None), "dy": (0.0, None), "area": (0.0, None)},
}
FIELD_TOL = SUB_TOL  # (old name, imported elsewhere)


def _piece(sub, name, k):
    v = sub[name]
    return v[("x", "y", "dx", "dy", "area", "angle_dx")[k]] if isinstance(v, dict) else v[k]


def _bipolar_rows(got):
    """(lo, hi): the stitched point rows that come from the bipolar cap (it is the northernmost piece and keeps all its rows); (n, n) without one."""
    n = got["x"].shape[0]
    return (n - _piece(got["sub"], "BP", 0).shape[0], n) if "BP" in got["sub"] else (n, n)


def _row_tolerances(got, field):
    """Per-POINT (abs, rel) arrays of a stitched field from the sub-grids `got` was stitched from, rows counted from the NORTH end (south
    cuts remove rows at the south end only): x, y, dx, angle_dx drop the southern piece's last row at every joint, dy and area do not.
    The bipolar cap's coordinates are held to TOL_COORD at every point but the ill-conditioned ones, by masks: x keeps TOL_COORD_ILL on the
    top (fold) row and within 2 columns of the two symmetry meridians Ni/4, 3Ni/4 (the `ill` mask of test_bipolar_cap_mesh); y keeps 1e-6 at
    the three points of the top row where the stencil of the angle vanishes (columns Ni/4, Ni/2, 3Ni/4), nowhere else."""
    k = ("x", "y", "dx", "dy", "area").index(field)
    n, ncol = got[field].shape
    a, r = np.zeros((n, ncol)), np.zeros((n, ncol))
    hi = n
    Ni = got["x"].shape[1] - 1
    names = [s for s in ("BP", "Merc", "SO", "SC") if s in got["sub"]]
    for pos, name in enumerate(names):
        rows = _piece(got["sub"], name, k).shape[0]
        if field in ("x", "y", "dx") and pos > 0 and rows > 0:
            rows -= 1     # its last row was replaced by the first row of the piece above (a piece cut away altogether has none)
        kind = "bipolar" if name == "BP" else "latlon"
        if name == "SC" and np.ptp(_piece(got["sub"], "SC", 0), axis=0).max() > 0:   # longitudes vary along j: displaced pole
            kind = "dpole"
        ta, tr = SUB_TOL[kind][field]
        lo = max(hi - rows, 0)
        a[lo:hi], r[lo:hi] = ta, (dp_quad_rel_tol(Ni) if tr is None else tr)
        if kind == "bipolar" and field == "x" and hi > lo:
            for c in (Ni // 4, 3 * Ni // 4):
                a[lo:hi, max(c - 2, 0):c + 3] = TOL_COORD_ILL
            a[hi - 1, :] = TOL_COORD_ILL
        if kind == "bipolar" and field == "y" and hi > lo:
            a[hi - 1, [Ni // 4, Ni // 2, 3 * Ni // 4]] = BP_POLE_POINT_TOL_Y
        hi = lo
    assert hi == 0, (field, hi)
    return a, r


def _check_supergrid(got, want, name):
    """Every element of every stitched field against the oracle / the golden arrays, each point held to the bound of the sub-grid it
    came from (SUB_TOL); angle_dx to the bound that follows from the coordinate bounds enforced here (tests/angle_bounds.py)."""
    rep = {}
    for f in ("x", "y", "dx", "dy", "area"):
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        d = np.abs(got[f] - want[f])
        rep[f] = float(d.max())
        a, r = _row_tolerances(got, f)
        bad = d > a + r * np.abs(want[f])
        assert not bad.any(), (name, f, rep[f], np.argwhere(bad)[:5].tolist())
    # angle_dx is noise at singular points (the two bipolar pole points, the displaced pole): compare where the
    # argument of atan2 is well-conditioned, i.e. everywhere except a few points; demand 99.9 % within 1e-9 deg
    d = np.abs(got["angle_dx"] - want["angle_dx"])
    d = np.minimum(d, np.abs(d - 360.0))
    rep["angle_dx_p999"] = float(np.quantile(d, 0.999))
    assert rep["angle_dx_p999"] < 1e-9, (name, rep)
    # ... and EVERY point: equal on the lat-lon rows, within the conditioned bound at every regular point, and no more singular points in
    # the reference mesh than the bipolar cap's three
    lo, hi = _bipolar_rows(got)
    ang = angle_bounds.check_angle(got["angle_dx"], want["x"], want["y"], want["angle_dx"], _row_tolerances(got, "x")[0],
                                   _row_tolerances(got, "y")[0], angle_bounds.MAX_SINGULAR_WITH_CAP if hi > lo else 0, name)
    rep["angle_dx_worst_d_over_bound"], rep["angle_dx_singular_points"] = ang["worst_ratio"], ang["n_singular"]
    record("supergrid_" + name, **rep)


@pytest.mark.parametrize("name", ["r0.25_even", "r0.5_dp"])
def test_main_vs_reference_golden(ogg, name, tmp_path):
    flags = json.load(open(os.path.join(GOLD, "ref_hashes.json")))["configs"][name]["flags"]
    want = np.load(os.path.join(GOLD, "ref_small_%s.npz" % name))
    out = tmp_path / "g.nc"
    got = ogg.main(gridfilename=str(out), no_changing_meta=True, return_arrays=True, **flags)
    _check_supergrid(got, want, name)
    # the file holds the same arrays, in the reference's layout (OGG:795-821)
    from scipy.io import netcdf_file
    nc = netcdf_file(str(out), "r", mmap=False)
    assert list(nc.dimensions.keys()) == ["nyp", "nxp", "ny", "nx", "string"]
    assert list(nc.variables.keys()) == ["tile", "y", "x", "dy", "dx", "area", "angle_dx"]
    assert nc.version_byte == 2 and nc.variables["area"].units == b"m2" and nc.variables["dx"].units == b"meters"
    assert b"".join(nc.variables["tile"][:5]) == b"tile1"
    for f in ("x", "y", "dx", "dy", "area", "angle_dx"):
        assert np.array_equal(nc.variables[f][:], got[f])
    nc.close()


@pytest.mark.parametrize("name", ["r1_cut2", "r2", "r2_equenh4", "r2_skip_metrics", "r0.5_latdp", "r1_dp_cutang", "r1_matchdy", "r4_om4",
                                  "r4_om5proto"])
def test_main_vs_oracle(ogg, name):
    cfg = json.load(open(os.path.join(GOLD, "ref_hashes.json")))["configs"][name]
    flags = dict(cfg["flags"])
    got = ogg.main(gridfilename=None, no_changing_meta=True, return_arrays=True, **flags)
    for f, shp in cfg["shapes"].items():
        assert list(got[f].shape) == shp, (f, got[f].shape, shp)          # shapes pinned by the reference run
    r = flags.pop("inverse_resolution")
    want = orc.make_supergrid(r, **flags)
    _check_supergrid(got, want, name)


@pytest.mark.parametrize("name", ["r0.5_latdp", "r1_dp_cutang", "r4_om4"])
def test_main_vs_oracle_literal_arc_form(ogg, name, monkeypatch):
    """The same through the literal arc form of the displaced-pole quadrature (the reference's operation sequence; opt-in since round 4):
    once by argument, once by OGG_DP_ARC -- the same bits either way, and different bits from the default chord form in the cap's metrics."""
    cfg = json.load(open(os.path.join(GOLD, "ref_hashes.json")))["configs"][name]
    flags = dict(cfg["flags"])
    got = ogg.main(gridfilename=None, no_changing_meta=True, return_arrays=True, dp_arc="literal", **flags)
    monkeypatch.setenv("OGG_DP_ARC", "literal")
    env = ogg.main(gridfilename=None, no_changing_meta=True, return_arrays=True, **flags)
    monkeypatch.delenv("OGG_DP_ARC")
    chord = ogg.main(gridfilename=None, no_changing_meta=True, return_arrays=True, **flags)
    for f in ("x", "y", "dx", "dy", "area", "angle_dx"):
        assert np.array_equal(got[f], env[f]), f
    assert not np.array_equal(got["area"], chord["area"]) and np.array_equal(got["x"], chord["x"])
    r = flags.pop("inverse_resolution")
    _check_supergrid(got, orc.make_supergrid(r, **flags), name + "_literal")


def test_cli_end_to_end(hip, tmp_path):
    """`python -m ocean_model_grid_generator_amd` with the reference's flag spelling writes the reference's file layout."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ocean_hgrid_res4.0.nc"
    p = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd", "-f", str(out), "-r", "0.25", "--ensure_nj_even",
                        "--no_changing_meta", "--write_subgrid_files"], cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Wrote the whole grid to file" in p.stdout and "runtime(secs)" in p.stdout
    from scipy.io import netcdf_file
    nc = netcdf_file(str(out), "r", mmap=False)
    want = np.load(os.path.join(GOLD, "ref_small_r0.25_even.npz"))
    assert nc.variables["x"].shape == (135, 181) and nc.variables["area"].shape == (134, 180)
    assert maxabs(nc.variables["y"][:].copy(), want["y"]) < 1e-6 and np.array_equal(nc.variables["x"][:, 0].copy(), want["x"][:, 0])
    nc.close()
    for tag in ("Merc", "BP", "SO", "SC"):
        assert os.path.exists(str(out) + tag + ".nc"), tag


@pytest.mark.parametrize("name,argv,shape", [
    ("C1", ["-r", "2", "--skip_metrics"], (1117, 1441)),
    ("C2", ["-r", "4", "--r_dp", "0.2", "--south_cutoff_row", "83"], (2161, 2881)),
    ("C4", ["-r", "8", "--lon_dp", "80", "--lat_dp", "-85.85", "--grids", "so", "sc", "bipolar", "mercator"], (4485, 5761)),
])
def test_cli_baseline_command_lines(hip, tmp_path, name, argv, shape):
    """BASELINE.json's configurations as COMMAND LINES of the drop-in (`python -m ocean_model_grid_generator_amd`, the reference's flag
    spelling; config 4 in the spelling the reference accepts): the file has the reference's layout and the shapes of the
    reference's own run, Sum(area) closes on the sphere's area south of the cut, and the metadata-free header is
    reproducible (two runs, identical bytes)."""
    import subprocess
    import sys
    from scipy.io import netcdf_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for k in range(2 if name == "C1" else 1):
        out = tmp_path / ("g%d.nc" % k)
        p = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd", "-f", str(out), "--no_changing_meta"] + argv, cwd=root,
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "Wrote the whole grid to file" in p.stdout
        outs.append(out)
    nc = netcdf_file(str(outs[0]), "r", mmap=True)
    assert nc.version_byte == 2 and list(nc.variables.keys()) == ["tile", "y", "x", "dy", "dx", "area", "angle_dx"]
    assert nc.variables["x"].shape == shape and nc.variables["area"].shape == (shape[0] - 1, shape[1] - 1)
    y = nc.variables["y"][:, (shape[1] - 1) // 4].copy()             # the symmetry meridian: from the southern edge to the north pole
    assert np.all(np.diff(y) > 0) and y[-1] == 90.0
    if "--skip_metrics" in argv:
        assert float(nc.variables["area"][:].max()) == -1.0 and float(nc.variables["dx"][:].min()) == -1.0      # OGG:1009-1011
    else:
        area = float(np.sum(nc.variables["area"][:], dtype=np.float64))
        assert 0.8 * 4 * np.pi * 6371.0e3 ** 2 < area <= 4 * np.pi * 6371.0e3 ** 2 * (1 + 1e-9)
    del y
    nc.close()
    if len(outs) == 2:
        assert open(str(outs[0]), "rb").read() == open(str(outs[1]), "rb").read()


def test_cli_refuses_the_literal_config_4_string_like_the_reference(hip, tmp_path):
    """BASELINE.json spells config 4 `--grids so sc bp merc`; `bp` and `merc` are not tokens of the reference (OGG:1003, 1035), which then
    dereferences the never-assigned phiMerc (OGG:1083: UnboundLocalError).  The drop-in refuses the same command line, with a message."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd", "-f", str(tmp_path / "g.nc"), "--no_changing_meta", "-r", "2",
                        "--lon_dp", "80", "--lat_dp", "-85.85", "--grids", "so", "sc", "bp", "merc"], cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "add mercator to --grids" in (p.stderr + p.stdout)
    assert not os.path.exists(str(tmp_path / "g.nc"))


def test_main_rejects_bad_flags(ogg):
    with pytest.raises(SystemExit):
        ogg.main(1.0, gridfilename=None, r_dp=0.2, lat_dp=-85.0)
    with pytest.raises(SystemExit):
        ogg.main(1.0, gridfilename=None, match_dy=["sc"])


# ---------------------------------------------------------------------------------------------------------------
# the literal kernels behind the default fast forms (selected by environment variables read at first use, hence a
# fresh process): they must agree with the oracle at the same level, and with the default forms within their bounds
# ---------------------------------------------------------------------------------------------------------------
_LITERAL_SCRIPT = r"""
import sys, json
sys.path.insert(0, %(root)r)
import numpy as np
import ocean_model_grid_generator_amd.ocean_grid_generator as ogg
from oracle import ogg_oracle as orc
out = {}
Ni, Nj, lat0 = 720, 120, 64.05895973
rp = np.tan(0.5 * (90 - lat0) * orc.PI_180)
got = ogg.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
want = orc.bipolar_cap_metrics_quad_fast(5, Ni, Nj, lat0, -300.0, rp)
out["bp"] = [float(np.max(np.abs(g - w)[w != 0] / np.abs(w[w != 0]))) for g, w in zip(got, want)]
want = orc.displacedPoleCap_metrics_quad(4, 720, 70, -300.0, -78.0, 80.0, 0.2)
for form in ("literal", "chord"):
    got = ogg.displacedPoleCap_metrics_quad(4, 720, 70, -300.0, -78.0, 80.0, 0.2, arc_form=form)
    out["dp_" + form] = [float(np.max(np.abs(g[36:] - w[36:]) / np.abs(w[36:]))) for g, w in zip(got, want)]
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("env", [{}, {"OGG_BP_GUARD_K": "0"}])
def test_literal_kernels_in_fresh_process(hip, env):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", _LITERAL_SCRIPT % {"root": root}], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    record("literal_env_%d" % len(env), **{k: max(v) for k, v in res.items()})
    assert max(res["bp"]) < 5e-14 and max(res["dp_literal"]) < 2e-12 * 720 and max(res["dp_chord"]) < 2e-12 * 720

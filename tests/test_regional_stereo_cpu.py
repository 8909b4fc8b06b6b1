"""The stereographic regional grids without a GPU: the numpy definition (tests/regional_stereo_definition.py) against the 50-digit
truth, its closed-form area, conformality, symmetries, the order of the analytic angle_dx and of the edge lengths, the defined values of
a pole at the centre, and the library's refusals (ogg_regional_stereo_check does no device work)."""
import os

import numpy as np
import pytest

import regional_stereo_definition as sd
from oracle import ogg_oracle as oo

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regional_stereo_truth.npz")


@pytest.fixture(scope="module")
def truth():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def S():
    from ocean_model_grid_generator_amd import regional_stereo
    return regional_stereo


def test_the_truth_covers_the_cases(truth):
    assert list(truth["cases"]) == [c[0] for c in sd.CASES] and tuple(truth["fields"]) == sd.FIELDS and int(truth["dps"]) == 50
    assert {c[2] for c in sd.CASES} == {0.0, 45.0, -60.0, 90.0, -90.0, 89.97} and {c[1] for c in sd.CASES} == {0.0, 179.9, -300.0}
    assert {c[3] for c in sd.CASES} == {0.0, 37.3, 90.0, -180.0} and {c[4] for c in sd.CASES} >= {4.0, 1.0, 0.0625}
    assert {(c[5], c[6]) for c in sd.CASES} >= {(2, 2), (130, 2), (2, 130), (62, 4), (64, 6), (128, 4), (258, 10), (8, 8), (10, 8)}
    assert set(sd.POLAR) == {c[0] for c in sd.CASES if abs(c[2]) in (90.0, 89.97)} and len(sd.POLAR) == 4
    assert 2000 < sum((c[5] + 1) * (c[6] + 1) for c in sd.CASES) < 10000


@pytest.mark.parametrize("k", range(len(sd.CASES)), ids=[c[0] for c in sd.CASES])
def test_definition_against_the_truth(truth, k):
    """The fp64 definition here is no further from the truth than 4 times what it was when the table was made, plus one rounding of
    the value (x, y, angle_dx: an ulp of the value; dx, dy, area: 2 eps), as tests/test_regional_cpu.py holds the other kinds."""
    case = sd.CASES[k]
    got = sd.stereo(**sd.case_args(case))
    for f, name in enumerate(sd.FIELDS):
        hi, lo = truth["%s/%s" % (case[0], name)]
        assert got[name].shape == hi.shape, name
        e = sd.error(name, got[name], hi, lo)
        floor = 2.0 * EPS if name in sd.RELATIVE else np.spacing(np.abs(hi))
        assert np.all(e <= 4.0 * truth["eref"][k, f] + floor), (case[0], name, e.max(), truth["eref"][k, f])


def test_the_entries_take_eight_scalars(S):
    """the scalars of the other regional entries without kind, the same in every entry; the nine-scalar entries are what they were"""
    import ctypes
    from ocean_model_grid_generator_amd import _lib as L
    eight = [ctypes.c_long, ctypes.c_long] + [ctypes.c_double] * 5 + [ctypes.c_int]
    assert L.REGIONAL_STEREO_ARGS == eight and S.Params._fields == ("nx", "ny", "lon_c", "lat_c", "tilt", "delta", "Re", "metrics")
    for name in ("ogg_regional_stereo_check", "ogg_regional_stereo_tables_dev", "ogg_regional_stereo_band_dev", "ogg_regional_stereo_grid"):
        assert L.SIGNATURES[name][:8] == eight, name
    assert L.LONG_GETTERS["ogg_regional_stereo_workspace_bytes"] == eight
    assert len(L.SIGNATURES["ogg_regional_stereo_band_dev"]) == 8 + 11 and len(L.SIGNATURES["ogg_regional_stereo_grid"]) == 8 + 6
    assert len(L.REGIONAL_ARGS) == 9


def POLE_STEP(k, delta=0.25):
    """the colatitude in degrees of a point k plane steps from the centre: 2 atan(k d / 2)"""
    return float(np.degrees(2.0 * np.arctan(0.5 * k * np.radians(delta))))


REFUSALS = [
    (dict(nx=3), "nx and ny even"), (dict(ny=0), "nx and ny even"), (dict(nx=1 << 23), "nx and ny even"),
    (dict(delta=0.0), "delta > 0"), (dict(delta=-0.25), "delta > 0"), (dict(delta=float("nan")), "not finite"),
    (dict(lon_c=float("inf")), "not finite"), (dict(lat_c=90.5), "|lat_c| <= 90"), (dict(Re=0.0), "Re > 0"),
    (dict(lon_c=2.0e6), "at most 1e6 in magnitude"), (dict(tilt=-2.0e6), "at most 1e6 in magnitude"),
    (dict(nx=230, ny=2, delta=1.0), "degrees from the centre: at most 90"),      # 115 degrees of plane width: rho = 2.007
    (dict(nx=164, ny=164, delta=1.0), "degrees from the centre: at most 90"),    # the corner, not the edge: 82 sqrt(2) degrees
    (dict(lat_c=90.0 - POLE_STEP(1), tilt=0.0, delta=0.25), "(j, i) = (4, 4) lies"),      # the north pole is the point (ny/2 + 1, nx/2)
    (dict(lat_c=POLE_STEP(2) - 90.0, tilt=90.0, delta=0.25), "from the south pole"),      # two points from the centre along x
    (dict(lat_c=90.0 - 1e-10, delta=0.25), "(j, i) = (3, 4) lies"),              # the centre point, but lat_c is not 90 exactly
]


@pytest.mark.parametrize("change, text", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals(S, change, text):
    from ocean_model_grid_generator_amd import _lib as L
    args = dict(lon_c=-70.0, lat_c=40.0, nx=8, ny=6, delta=0.25, tilt=10.0)
    S.params(**args)
    args.update(change)
    with pytest.raises(ValueError) as e:
        S.params(**args)
    assert text in str(e.value) and "regional stereo:" in str(e.value), str(e.value)
    p = S.Params(args["nx"], args["ny"], args["lon_c"], args["lat_c"], args["tilt"], args["delta"], args.get("Re", sd.RE), 1)
    lib = L.load()
    assert lib.ogg_regional_stereo_check(*p) == L.OGG_EARG and text.encode() in lib.ogg_last_error()
    assert lib.ogg_regional_stereo_workspace_bytes(*p) == -1
    # the device entries and the host-pointer entry refuse the same parameters before they look at a pointer
    assert lib.ogg_regional_stereo_tables_dev(*(list(p) + [None, 0, None])) == L.OGG_EARG
    assert lib.ogg_regional_stereo_band_dev(*(list(p) + [0, 1, None, 0, None, None, None, None, None, None, None])) == L.OGG_EARG
    assert lib.ogg_regional_stereo_grid(*(list(p) + [None] * 6)) == L.OGG_EARG and text.encode() in lib.ogg_last_error()


def test_more_refusals_and_what_is_admitted(S):
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import regional as R
    lib = L.load()
    # pole-holding domains: the centre point, a cell corner next to it, inside a cell, and far from the centre
    for kw in (dict(lat_c=90.0), dict(lat_c=-90.0, tilt=33.0), dict(lat_c=89.97), dict(lat_c=89.875, tilt=0.0), dict(lat_c=80.0, nx=200, ny=200)):
        args = dict(lon_c=10.0, lat_c=0.0, nx=8, ny=8, delta=0.25, tilt=0.0)
        args.update(kw)
        p = S.params(**args)
        assert lib.ogg_regional_stereo_workspace_bytes(*p) > 0 and len(S.poles(p)) == 1
    assert S.poles(S.params(0.0, 90.0, 8, 10, 0.5)) == {"north": {"point": [5, 4]}}
    assert S.poles(S.params(0.0, 89.875, 8, 8, 0.25)) == {"north": {"cell": [4, 4]}}     # half a step up the centre column
    assert S.poles(S.params(0.0, 40.0, 8, 8, 0.25)) == {}
    S.params(0.0, 0.0, 162, 162, 1.0)      # a corner 89.98 degrees from the centre
    p = S.params(0.0, 0.0, 4, 4, 1.0)
    assert lib.ogg_regional_stereo_check(*p._replace(metrics=3)) == L.OGG_EARG and b"metrics 3" in lib.ogg_last_error()
    q = list(p)
    for j0, n in ((-1, 2), (0, 6), (4, 2)):      # 5 point rows
        assert lib.ogg_regional_stereo_band_dev(*(q + [j0, n, 8, 1 << 20, 8, 8, 8, 8, 8, 8, None])) == L.OGG_EARG
        assert b"point rows" in lib.ogg_last_error()
    assert lib.ogg_regional_stereo_band_dev(*(q + [0, 5, 8, 16, 8, 8, 8, 8, 8, 8, None])) == L.OGG_EARG and b"workspace" in lib.ogg_last_error()
    assert lib.ogg_regional_stereo_band_dev(*(q + [0, 5, 8, 1 << 20, 8, 8, None, 8, 8, 8, None])) == L.OGG_EARG and b"null" in lib.ogg_last_error()
    # the other regional entries are what they were: kind 2 is refused, "lambert" and "stereographic" are no kinds of theirs
    assert lib.ogg_regional_check(*R.params(0.0, 0.0, 4, 4, 1.0)._replace(kind=2)) == L.OGG_EARG and b"kind 2" in lib.ogg_last_error()
    assert sorted(R.KINDS) == ["latlon", "mercator"]
    with pytest.raises(ValueError, match="kind must be one of latlon, mercator"):
        R.params(0.0, 0.0, 4, 4, 1.0, kind="lambert")


@pytest.mark.parametrize("case", sd.CASES, ids=[c[0] for c in sd.CASES])
def test_area_sums_to_its_closed_form(case):
    name, lon_c, lat_c, tilt, delta, nx, ny = case
    g = sd.stereo(**sd.case_args(case))
    exact = sd.closed_form_area(nx, ny, delta)
    assert abs(g["area"].sum() - exact) / exact <= 1e-12
    assert np.all(g["area"] > 0.0) and np.all(g["dx"] > 0.0) and np.all(g["dy"] > 0.0)


def test_closed_form_area_tends_to_the_sphere(S):
    """the plane is the whole sphere but the centre's antipode: 8 [(B/a) atan(A/a) + (A/b) atan(B/b)] -> 4 pi"""
    rel = [abs(sd.closed_form_area(n, n, 1.0, Re=1.0) / (4.0 * np.pi) - 1.0) for n in (10 ** 3, 10 ** 5, 10 ** 7)]
    assert rel[0] > rel[1] > rel[2] and rel[2] < 1e-4
    p = S.Params(64, 48, 0.0, 0.0, 0.0, 0.5, sd.RE, 1)
    assert abs(S.closed_form_area(p) / sd.closed_form_area(64, 48, 0.5) - 1.0) <= 4 * EPS


def test_conformal():
    """dx(j, i) and dy(j, i) leave the same point along the two grid directions.  The scale 1/m is the same in both, so the two lengths
    differ only through the change of m over half a step: by O(d^2) in units of Re (O(d) relative to either).  Halving delta over the
    same domain quarters the largest difference (between 3 and 5)."""
    worst = []
    for nx, ny, delta in ((32, 24, 1.0), (64, 48, 0.5)):
        g = sd.stereo(20.0, 70.0, nx, ny, delta, tilt=15.0, Re=1.0)
        worst.append(np.abs(g["dx"][:-1, :] - g["dy"][:, :-1]).max())
    assert worst[0] < np.radians(1.0) ** 2 and 3.0 <= worst[0] / worst[1] <= 5.0, worst


def test_mirror_image():
    """(lat_c, tilt) -> (-lat_c, -tilt): the domain mirrored in the equator: y negated with the rows reversed, x the same, and the metrics
    the same (dx, dy, area do not depend on the rotation at all)"""
    a = sd.stereo(-55.5, 33.0, 12, 10, 0.375, tilt=21.0)
    b = sd.stereo(-55.5, -33.0, 12, 10, 0.375, tilt=-21.0)
    assert np.allclose(b["y"][::-1], -a["y"], rtol=0, atol=1e-12) and np.allclose(b["x"][::-1], a["x"], rtol=0, atol=1e-12)
    assert np.allclose(b["angle_dx"][::-1], -a["angle_dx"], rtol=0, atol=1e-12)
    for f in ("dx", "dy", "area"):
        assert np.allclose(b[f][::-1], a[f], rtol=1e-13, atol=0), f
    c = sd.stereo(100.0, 89.0, 12, 10, 0.375, tilt=-140.0)
    for f in ("dx", "dy", "area"):
        assert np.array_equal(c[f], a[f]), f


@pytest.mark.parametrize("lat_c, tilt", [(45.0, 37.3), (-60.0, 90.0), (0.0, 0.0), (80.0, -20.0)])
def test_angle_dx_is_second_order_from_the_mesh(lat_c, tilt):
    """angle_dx is the analytic direction; the reference's angle_x of the mesh is a centred difference in interior columns.  Their
    difference is O(delta^2): halving delta over the same domain divides its maximum by about 4 (between 3 and 5)."""
    worst = []
    for nx, ny, delta in ((32, 24, 0.5), (64, 48, 0.25)):
        g = sd.stereo(-70.0, lat_c, nx, ny, delta, tilt=tilt)
        d = np.abs(g["angle_dx"] - oo.angle_x(g["x"], g["y"]))[:, 1:-1]
        worst.append(np.minimum(d, 360.0 - d).max())
    assert 3.0 <= worst[0] / worst[1] <= 5.0, worst


def test_chord_agrees_with_dx_to_third_order():
    """the straight chord between neighbouring points is shorter than the arc dx by O(d^3): halving delta divides the largest relative
    difference (which is O(d^2)) by about 4; dy likewise"""
    worst = []
    for nx, ny, delta in ((32, 24, 1.0), (64, 48, 0.5)):
        g = sd.stereo(33.0, 75.0, nx, ny, delta, tilt=-40.0, Re=1.0)
        lam, phi = np.radians(g["x"]), np.radians(g["y"])
        p = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)])
        cx = np.sqrt(((p[:, :, 1:] - p[:, :, :-1]) ** 2).sum(axis=0))
        cy = np.sqrt(((p[:, 1:, :] - p[:, :-1, :]) ** 2).sum(axis=0))
        assert np.all(cx < g["dx"]) and np.all(cy < g["dy"])
        worst.append(max(np.abs(cx / g["dx"] - 1.0).max(), np.abs(cy / g["dy"] - 1.0).max()))
    assert worst[0] < 1e-4 and 3.0 <= worst[0] / worst[1] <= 5.0, worst


@pytest.mark.parametrize("lat_c, lon_c, tilt", [(90.0, 0.0, 0.0), (-90.0, 179.9, 37.3), (90.0, -300.0, -180.0)])
def test_a_pole_at_the_centre_has_its_defined_values(lat_c, lon_c, tilt):
    g = sd.stereo(lon_c, lat_c, 8, 10, 0.5, tilt=tilt)
    assert g["x"][5, 4] == lon_c and g["y"][5, 4] == lat_c and g["angle_dx"][5, 4] == tilt
    assert all(np.all(np.isfinite(g[f])) for f in sd.FIELDS) and np.count_nonzero(np.abs(g["y"]) == 90.0) == 1
    # every other point is half a degree of plane or more away: 2 atan(d/2) of latitude
    away = np.abs(g["y"]) < 90.0
    assert abs((90.0 - np.abs(g["y"][away]).max()) - np.degrees(2.0 * np.arctan(0.5 * np.radians(0.5)))) < 1e-12


def test_extent_and_forwarding(S, monkeypatch):
    # 1/4 degree model cells at the centre: delta = 1/8 degree.  2000 km: the plane half-width 2 tan(1000 km / (2 Re)) = 0.157283 is
    # 72.09 steps of 0.0021817: 74 after rounding the full width 144.2 up to even
    nx, ny = S.cells_for_extent(2000.0, 1000.0, 0.125)
    d = np.radians(0.125)
    for n, km in ((nx, 2000.0), (ny, 1000.0)):
        assert n % 2 == 0 and 4.0 * np.arctan(0.25 * n * d) * sd.RE >= km * 1e3 > 4.0 * np.arctan(0.25 * (n - 2) * d) * sd.RE
    with pytest.raises(ValueError, match="beyond the hemisphere"):
        S.cells_for_extent(21000.0, 100.0, 0.125)
    from ocean_model_grid_generator_amd import regional as R
    seen = []
    monkeypatch.setattr(S, "main", lambda argv: seen.append(argv) or "forwarded")
    assert R.main(["--lon_c", "0", "--kind", "stereographic", "--lat_c", "90", "-r", "2", "--cells", "4", "4"]) == "forwarded"
    assert R.main(["--lon_c", "0", "--kind=stereographic", "--lat_c", "90"]) == "forwarded"
    assert seen == [["--lon_c", "0", "--lat_c", "90", "-r", "2", "--cells", "4", "4"], ["--lon_c", "0", "--lat_c", "90"]]

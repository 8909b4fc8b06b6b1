"""The regional grids without a GPU: the numpy definition (tests/regional_definition.py) against the 50-digit truth and against the
reference's own lat-lon and Mercator lattices and MIDAS metrics, its symmetries, the order of the analytic angle_dx, and the
library's refusals (ogg_regional_check does no device work)."""
import ctypes
import os

import numpy as np
import pytest

import regional_definition as rd
from oracle import ogg_oracle as oo

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regional_truth.npz")


@pytest.fixture(scope="module")
def truth():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def R():
    from ocean_model_grid_generator_amd import regional
    return regional


def test_the_truth_covers_the_cases(truth):
    assert list(truth["cases"]) == [c[0] for c in rd.CASES] and tuple(truth["fields"]) == rd.FIELDS and int(truth["dps"]) == 50
    assert {c[2] for c in rd.CASES} == {0.0, 45.0, -60.0, 89.0} and {c[1] for c in rd.CASES} == {0.0, 179.9, -300.0}
    assert {c[3] for c in rd.CASES} == {0.0, 37.3, 90.0, -180.0} and {c[4] for c in rd.CASES} == {"latlon", "mercator"}
    assert {c[5] for c in rd.CASES} >= {1.0, 0.0625} and all(c[6] * c[5] <= 0.5 and c[7] * c[5] <= 0.5 for c in rd.CASES if c[2] == 89.0)
    assert 2000 < sum((c[6] + 1) * (c[7] + 1) for c in rd.CASES) < 10000


@pytest.mark.parametrize("k", range(len(rd.CASES)), ids=[c[0] for c in rd.CASES])
def test_definition_against_the_truth(truth, k):
    """The fp64 definition here is no further from the truth than 4 times what it was when the table was made, plus one rounding of
    the value (x, y, angle_dx: an ulp of the value; dx, dy, area: 2 eps): numpy's functions may differ by an ulp or two between builds,
    and an error measured as a maximum over a few points moves by such factors; a wrong statement is off by many orders."""
    case = rd.CASES[k]
    got = rd.regional(**rd.case_args(case))
    for f, name in enumerate(rd.FIELDS):
        hi, lo = truth["%s/%s" % (case[0], name)]
        assert got[name].shape == hi.shape, name
        e = rd.error(name, got[name], hi, lo)
        floor = 2.0 * EPS if name in rd.RELATIVE else np.spacing(np.abs(hi))
        assert np.all(e <= 4.0 * truth["eref"][k, f] + floor), (case[0], name, e.max(), truth["eref"][k, f])


def test_the_entries_take_nine_scalars_and_add_no_struct(R):
    """The parameters travel as nine scalars by value, the same in every entry, and the header gains no struct: the table of
    OGG_ABI_* size codes, which tests/test_runoff_spread_cpu.py pins at 42 entries, is what it was."""
    from ocean_model_grid_generator_amd import _lib as L
    nine = [ctypes.c_long, ctypes.c_long] + [ctypes.c_double] * 5 + [ctypes.c_int, ctypes.c_int]
    assert L.REGIONAL_ARGS == nine and R.Params._fields == ("nx", "ny", "lon_c", "lat_c", "tilt", "delta", "Re", "kind", "metrics")
    for name in ("ogg_regional_check", "ogg_regional_tables_dev", "ogg_regional_band_dev", "ogg_regional_grid"):
        assert L.SIGNATURES[name][:9] == nine, name
    assert L.LONG_GETTERS["ogg_regional_workspace_bytes"] == nine
    assert len(L.SIGNATURES["ogg_regional_band_dev"]) == 9 + 11 and len(L.SIGNATURES["ogg_regional_grid"]) == 9 + 6
    assert not any("REGIONAL" in k for k in L.ABI) and L.load().ogg_abi_sizeof(len(L.ABI)) == -1


REFUSALS = [
    (dict(nx=3), "nx and ny even"), (dict(ny=0), "nx and ny even"), (dict(nx=1 << 23), "nx and ny even"),
    (dict(delta=0.0), "delta > 0"), (dict(delta=-0.25), "delta > 0"), (dict(delta=float("nan")), "not finite"),
    (dict(nx=720, delta=0.5), "|lam'| = 180 degrees at the edge"), (dict(ny=358, delta=0.5, kind="latlon"), "|phi'| = 89.5 degrees at the edge"),
    (dict(ny=546, delta=1.0, kind="mercator"), "degrees at the edge: at most 89"),
    (dict(lat_c=90.5), "|lat_c| <= 90"), (dict(Re=0.0), "Re > 0"),
    (dict(lat_c=88.0, nx=20, ny=20, delta=0.25), "holds the north pole"), (dict(lat_c=-89.0, tilt=30.0, nx=8, ny=8, delta=0.25), "holds the south pole"),
    (dict(lat_c=90.0), "holds the north pole"),
    (dict(lat_c=88.0, tilt=0.0, kind="latlon", nx=16, ny=16, delta=0.25), "holds the north pole"),      # the pole is the corner (ny, nx/2) of a cell, on the edge row
    (dict(lat_c=0.0, tilt=90.0, nx=360, ny=2, delta=0.5, kind="latlon"), "holds the north pole"),   # at lam' = 90, a point of the edge column
]


@pytest.mark.parametrize("change, text", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals(R, change, text):
    from ocean_model_grid_generator_amd import _lib as L
    args = dict(lon_c=-70.0, lat_c=40.0, nx=8, ny=6, delta=0.25, kind="mercator", tilt=10.0)
    R.params(**args)
    args.update(change)
    with pytest.raises(ValueError) as e:
        R.params(**args)
    assert text in str(e.value), str(e.value)
    p = R.Params(args["nx"], args["ny"], args["lon_c"], args["lat_c"], args["tilt"], args["delta"], args.get("Re", rd.RE),
                 R.KINDS[args["kind"]], 1)
    lib = L.load()
    assert lib.ogg_regional_check(*p) == L.OGG_EARG and text.encode() in lib.ogg_last_error()
    assert lib.ogg_regional_workspace_bytes(*p) == -1
    # the device entries and the host-pointer entry refuse the same parameters before they look at a pointer
    assert lib.ogg_regional_tables_dev(*(list(p) + [None, 0, None])) == L.OGG_EARG
    assert lib.ogg_regional_band_dev(*(list(p) + [0, 1, None, 0, None, None, None, None, None, None, None])) == L.OGG_EARG
    assert lib.ogg_regional_grid(*(list(p) + [None] * 6)) == L.OGG_EARG and text.encode() in lib.ogg_last_error()


def test_more_refusals(R):
    from ocean_model_grid_generator_amd import _lib as L
    lib = L.load()
    with pytest.raises(ValueError, match="kind must be one of"):
        R.params(0.0, 0.0, 4, 4, 1.0, kind="lambert")
    p = R.params(0.0, 0.0, 4, 4, 1.0)
    assert lib.ogg_regional_workspace_bytes(*p) > 0
    assert lib.ogg_regional_check(*p._replace(kind=2)) == L.OGG_EARG and b"kind 2" in lib.ogg_last_error()
    assert lib.ogg_regional_check(*p._replace(metrics=3)) == L.OGG_EARG and b"metrics 3" in lib.ogg_last_error()
    q = list(p)
    for j0, n in ((-1, 2), (0, 6), (4, 2)):      # 5 point rows
        assert lib.ogg_regional_band_dev(*(q + [j0, n, 8, 1 << 20, 8, 8, 8, 8, 8, 8, None])) == L.OGG_EARG
        assert b"point rows" in lib.ogg_last_error()
    assert lib.ogg_regional_band_dev(*(q + [0, 5, 8, 16, 8, 8, 8, 8, 8, 8, None])) == L.OGG_EARG and b"workspace" in lib.ogg_last_error()
    assert lib.ogg_regional_band_dev(*(q + [0, 5, 8, 1 << 20, 8, 8, None, 8, 8, 8, None])) == L.OGG_EARG and b"null" in lib.ogg_last_error()


@pytest.mark.parametrize("kind", ["latlon", "mercator"])
@pytest.mark.parametrize("lon_c", [0.0, -300.0])
def test_untilted_equatorial_grid_is_the_reference_lattice(kind, lon_c):
    """lat_c = 0, tilt = 0: the rotation is the identity, x, y are generate_latlon_grid's lattice (or phi_mercator's rows) shifted by
    lon_c, and the metrics are generate_grid_metrics_MIDAS of that grid -- to rounding: x and y within 4 ulp of their largest values;
    the metrics within what the roundings of the mesh do to MIDAS's differences, 8 eps (max|x| / delta + max|phi'| / min dphi')."""
    nx, ny, delta = 64, 40, 0.25
    g = rd.regional(lon_c, 0.0, nx, ny, delta, kind)
    x0, y0 = oo.generate_latlon_grid(nx, ny, -0.5 * nx * delta, nx * delta, -0.5 * ny * delta, ny * delta, ensure_nj_even=False)
    if kind == "mercator":
        y0 = np.tile(oo.phi_mercator(360.0 / delta, np.arange(ny + 1) - ny // 2)[:, None], (1, nx + 1))
    assert np.max(np.abs(g["x"] - (x0 + lon_c))) <= 4 * np.spacing(np.abs(g["x"]).max())
    assert np.max(np.abs(g["y"] - y0)) <= 4 * np.spacing(np.abs(y0).max())
    dx, dy, area = oo.generate_grid_metrics_MIDAS(g["x"], g["y"], Re=rd.RE, latlon_areafix=True)
    tol = 8 * EPS * (np.abs(g["x"]).max() / delta + np.abs(y0).max() / np.diff(y0[:, 0]).min() + 1.0)
    for a, b in ((g["dx"], dx), (g["dy"], dy), (g["area"], area)):
        assert np.max(np.abs(a - b) / b) <= tol
    assert np.max(np.abs(g["angle_dx"])) == 0.0


@pytest.mark.parametrize("case", rd.CASES, ids=[c[0] for c in rd.CASES])
def test_area_sums_to_its_closed_form(case):
    """Every row's sin phi' difference carries at most 2 eps of absolute error and the sum of nx ny terms at most nx ny eps relative."""
    name, lon_c, lat_c, tilt, kind, delta, nx, ny = case
    g = rd.regional(**rd.case_args(case))
    exact = rd.closed_form_area(nx, ny, delta, kind)
    top = 0.5 * ny * delta * rd.NP.D
    bound = EPS * (2 * ny / (2 * np.sin(top)) + nx * ny + 16)
    assert abs(g["area"].sum() - exact) / exact <= bound


@pytest.mark.parametrize("kind", ["latlon", "mercator"])
def test_mirror_image(kind):
    """(lat_c, tilt) -> (-lat_c, -tilt): the domain mirrored in the equator.  Sine and tanh are odd and a negation commutes with every
    rounding, so y is negated with the rows reversed and x is the same, bit for bit; so are dx, dy and area."""
    a = rd.regional(-55.5, 33.0, 12, 10, 0.375, kind, tilt=21.0)
    b = rd.regional(-55.5, -33.0, 12, 10, 0.375, kind, tilt=-21.0)
    assert np.array_equal(b["y"][::-1], -a["y"]) and np.array_equal(b["x"][::-1], a["x"])
    assert np.array_equal(b["dx"][::-1], a["dx"]) and np.array_equal(b["angle_dx"][::-1], -a["angle_dx"])
    assert np.allclose(b["dy"][::-1], a["dy"], rtol=1e-12, atol=0) and np.allclose(b["area"][::-1], a["area"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind, lat_c, tilt", [("mercator", 45.0, 37.3), ("latlon", -60.0, 90.0), ("mercator", 0.0, 0.0)])
def test_angle_dx_is_second_order_from_the_mesh(kind, lat_c, tilt):
    """angle_dx is the analytic direction; the reference's angle_x of the mesh is a centred difference in interior columns.  Their
    difference is O(delta^2): halving delta over the same domain divides its maximum by about 4 (between 3 and 5)."""
    worst = []
    for nx, ny, delta in ((32, 24, 0.5), (64, 48, 0.25)):
        g = rd.regional(-70.0, lat_c, nx, ny, delta, kind, tilt=tilt)
        d = np.abs(g["angle_dx"] - oo.angle_x(g["x"], g["y"]))[:, 1:-1]
        worst.append(np.minimum(d, 360.0 - d).max())
    if lat_c == 0.0 and tilt == 0.0:
        assert worst[0] < 1e-10 and worst[1] < 1e-10       # both are zero there but for rounding
    else:
        assert 3.0 <= worst[0] / worst[1] <= 5.0, worst


def test_band_rows_and_extent(R):
    for ny in (2, 8, 130):
        for bands in (1, 2, 3, 7, 500):
            rows = R.band_rows(ny, bands)
            assert rows[0][0] == 0 and sum(n for _, n in rows) == ny + 1 and all(n >= 1 for _, n in rows)
            assert all(a + n == b for (a, n), (b, _) in zip(rows[:-1], rows[1:])) and len(rows) == min(bands, ny + 1)
    # 1/4 degree model cells: delta = 1/8 degree = 13.9 km; 1000 km is 71.9 supergrid steps: 72
    assert R.cells_for_extent(1000.0, 1000.0, 0.125, "latlon") == (72, 72)
    nx, ny = R.cells_for_extent(1001.0, 3000.0, 0.125, "mercator")
    assert nx == 74 and ny % 2 == 0
    top = np.degrees(np.arctan(np.sinh(0.5 * ny * np.radians(0.125))))
    assert 2 * np.radians(top) * rd.RE >= 3000.0e3 > 2 * np.radians(np.degrees(np.arctan(np.sinh(0.5 * (ny - 2) * np.radians(0.125))))) * rd.RE

"""CPU tests of the hand-made meshes of tests/small_meshes.py: the inputs of tests/test_gpu_small_meshes.py are what they claim, shown
with the numpy definitions alone.  The zoo holds every class of cell and no cell on a knife edge; the four cuts are the four
topologies, and their missing-value regions and land tell the topologies apart (a kernel using the wrong flag cannot pass); the long
specimen is long; the committed extended-precision areas (tests/golden/xgrid_truth.npz) are what scripts/xgrid_truth.py makes, and the
definition's own distance from them is measured; a NaN latitude is an unfilled point in the bilinear definition."""
import importlib.util
import os

import numpy as np
import pytest

import bilinear_definition as BD
import remap_definition as RD
import runoff_definition as ROD
import small_meshes as sm
import xgrid_definition as xd

from ocean_model_grid_generator_amd import ocean_mask as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zoo():
    x, y, where = sm.cell_zoo()
    lon, lat = sm.zoo_atmosphere("regular")
    lst, a_poly, counts = xd.exchange_grid(x, y, lon, lat, Re=sm.RE, threshold=0.0)
    return dict(x=x, y=y, where=where, lst=lst, a_poly=a_poly, counts=counts)


def corners(x, y, n):
    return ([float(x[0, 2 * n]), float(x[0, 2 * n + 2]), float(x[2, 2 * n + 2]), float(x[2, 2 * n])],
            [float(y[0, 2 * n]), float(y[0, 2 * n + 2]), float(y[2, 2 * n + 2]), float(y[2, 2 * n])])


def status(x, y, a_poly, n):
    st, _, npole = xd.polygon(*corners(x, y, n))
    if st == "ok" and not a_poly[0, n] > 0:
        st = "inverted"
    return st, npole


def test_zoo_holds_every_class_and_every_specimen_is_what_it_is_named(zoo):
    c = zoo["counts"]
    assert c["cells"] == 2 * len(sm.SPECIMENS) - 1
    assert c["pole_cells"] > 0 and c["pole_enclosing"] > 0 and c["inverted"] > 0 and c["degenerate"] > 0, c
    _, ocn, _ = xd.as_arrays(zoo["lst"])
    n_entries = np.bincount(ocn[:, 0], minlength=c["cells"])
    assert set(sm.ZOO_STATUS) == set(zoo["where"])
    for name, n in zoo["where"].items():
        st, npole = status(zoo["x"], zoo["y"], zoo["a_poly"], n)
        assert (st, npole, int(n_entries[n])) == sm.ZOO_STATUS[name], name
    # the NaN pattern: degenerate and pole-enclosing cells and those with a NaN corner
    for name in ("three_poles", "four_poles", "enclosing", "nan_lat", "nan_lon"):
        assert np.isnan(zoo["a_poly"][0, zoo["where"][name]]), name
    # the shifted copies of the seam cell meet the same atmosphere cells
    per = {name: [e[:2] for e in zoo["lst"] if e[2] == zoo["where"][name]] for name in ("seam", "seam_m720", "seam_p360")}
    assert per["seam"] == per["seam_m720"] == per["seam_p360"] and len(per["seam"]) == 4


def test_no_cell_of_the_zoo_sits_on_a_knife_edge(zoo):
    """A_poly is exactly +-0.0, NaN, or in magnitude above 1e-6 of the ordinary specimen's, and the winding sum is 0 or +-360 exactly:
    no rounding of a sine decides a class.  The odd cells between the specimens are held to the same."""
    ap = zoo["a_poly"][0]
    a0 = ap[zoo["where"]["ordinary"]]
    assert a0 > 0
    for n in range(ap.size):
        assert np.isnan(ap[n]) or ap[n] == 0.0 or abs(ap[n]) > 1e-6 * a0, (n, ap[n])
        st, verts, npole = xd.polygon(*corners(zoo["x"], zoo["y"], n))
        w = 0.0
        for k in range(len(verts)):
            w = w + xd.wrap180(verts[(k + 1) % len(verts)][0] - verts[k][0])
        assert np.isnan(w) or abs(w) in (0.0, 360.0), (n, w)
    for name in ("point", "parallel"):
        v = ap[zoo["where"][name]]
        assert v == 0.0 and np.signbit(v), name
    # the two pole-epsilon specimens fall on opposite sides of the test, each by a factor of two
    (_, cy_in), (_, cy_out) = (corners(zoo["x"], zoo["y"], zoo["where"][k]) for k in ("eps_inside", "eps_outside"))
    assert 90.0 - max(cy_in) < xd.POLE_EPS / 1.9 and max(cy_in) < 90.0
    assert 90.0 - max(cy_out) > xd.POLE_EPS * 1.9
    assert status(zoo["x"], zoo["y"], zoo["a_poly"], zoo["where"]["eps_inside"])[1] == 1
    assert status(zoo["x"], zoo["y"], zoo["a_poly"], zoo["where"]["eps_outside"])[1] == 0


def test_long_specimen_has_more_than_two_wavefronts_of_entries(zoo):
    n = zoo["where"]["long"]
    kept = sum(1 for e in zoo["lst"] if e[2] == n)
    assert kept > 128 and kept % 64 != 0, kept
    lon, lat = sm.zoo_atmosphere("regular")
    cx, cy = corners(zoo["x"], zoo["y"], n)
    assert max(cx) - min(cx) > 170.0
    cand = np.sum((lon[:-1] < max(cx)) & (lon[1:] > min(cx))) * np.sum((lat[:-1] < max(cy)) & (lat[1:] > min(cy)))
    assert cand > 128


def test_every_atmosphere_of_the_zoo_sees_every_class():
    x, y, _ = sm.cell_zoo()
    for kind in ("gaussian", "one_column", "one_row"):
        lon, lat = sm.zoo_atmosphere(kind)
        assert abs(lon[-1] - lon[0] - 360.0) <= 1e-9
        _, _, c = xd.exchange_grid(x, y, lon, lat, Re=sm.RE, threshold=0.0)
        assert c["pole_enclosing"] > 0 and c["inverted"] > 0 and c["degenerate"] > 0 and c["kept"] > 0, (kind, c)


def test_cuts_and_shapes_are_the_topologies_they_claim():
    cuts = sm.topology_cuts()
    assert {g["topology"] for g in cuts.values()} == {(True, True), (False, True), (True, False), (False, False)}
    for name, g in cuts.items():
        assert OM.detect_topology(g["x"], g["y"], 2) == g["topology"], name
        ny, nx = (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2
        assert g["x"].shape[0] % 2 == 1 and g["x"].shape[1] % 2 == 1 and ny <= 70 and nx <= 90
        assert g["area"].shape == (2 * ny, 2 * nx) and g["angle_dx"].shape == g["x"].shape
    for name in sm.SHAPES:
        g = sm.shape_grid(name)
        assert OM.detect_topology(g["x"], g["y"], 2) == sm.SHAPE_TOPOLOGY.get(name, (False, False)), name
        assert np.all(g["area"] > 0)
    assert sm.SHAPES["fold_5x7"][1] % 2 == 1   # odd nx: the middle cell of the top row is its own neighbour
    nb = RD.neighbours(5, 7, False, True)
    assert nb[3][4 * 7 + 3] == 4 * 7 + 3


def definition_lists(g, lon, lat, mask=None):
    lst, a_poly, _ = xd.exchange_grid(g["x"], g["y"], lon, lat, mask=mask, Re=sm.RE)
    return xd.as_arrays(lst), a_poly.shape


@pytest.mark.parametrize("name", list(sm.CUTS))
def test_missing_regions_and_land_tell_the_topologies_apart(name):
    """the filled remap and the runoff targets under the detected flags differ from those under the other flags: on a cut from (True,
    True), which every earlier GPU test passes, and on the full grid from (False, False)"""
    g = sm.topology_cuts()[name]
    topo = g["topology"]
    other = (False, False) if topo == (True, True) else (True, True)
    f, lon, lat, fills = sm.source_for(g["x"], g["y"], "nonuniform", nrec=3)
    (atm, ocn, area), (ny, nx) = definition_lists(g, lon, lat)
    v, fl = RD.remap(atm, ocn, area, f, ny, nx, fills=fills)
    assert (fl == RD.UNFILLED).sum() > 0 and (fl == RD.REMAPPED).sum() > 0
    assert np.any(fl[:, :, 0] == RD.UNFILLED) and np.any(fl[:, -1, :] == RD.UNFILLED)   # against the left column and the top row
    a = RD.fill(v, fl, *topo)
    b = RD.fill(v, fl, *other)
    assert a[0].tobytes() != b[0].tobytes(), name
    for flip in ((not topo[0], topo[1]), (topo[0], not topo[1])):   # each flag on its own decides some value
        assert RD.fill(v, fl, *flip)[0].tobytes() != a[0].tobytes(), (name, flip)
    wet = sm.wet_mask(ny, nx)
    assert np.any(wet[:, 0] == 0) and np.any(wet[-1] == 0) and wet.any()
    t = ROD.targets(wet, *topo)
    assert not np.array_equal(t, ROD.targets(wet, *other)), name
    for flip in ((not topo[0], topo[1]), (topo[0], not topo[1])):
        assert not np.array_equal(t, ROD.targets(wet, *flip)), (name, flip)
    # the bilinear fill at the h points: the same region, seen through the source's centres, under the wet mask the GPU test uses
    xh, yh = BD.points(g["x"], "h"), BD.points(g["y"], "h")
    bv, bf = BD.interpolate(xh, yh, lon, lat, f, fills=fills, mask=wet)
    assert (bf == BD.UNFILLED).sum() > 0 and (bf == BD.DRY).sum() > 0
    assert BD.fill(bv, bf, *topo)[0].tobytes() != BD.fill(bv, bf, *other)[0].tobytes(), name


@pytest.mark.parametrize("name", ["band_2x2", "band_3x2", "band_2x1", "band_3x1", "129x1", "1x63", "fold_5x7"])
def test_holes_leave_narrow_grids_something_to_fill(name):
    """source_with_holes() leaves points to fill and points to fill them from on grids one and two columns wide.  Two columns wide,
    W and E are the same cell, summed twice: the filled values differ from those without the seam.  One column wide a cell is its
    own W and E, which is never at a smaller distance, so the seam cannot show in a value (only in an index out of bounds)."""
    g = sm.shape_grid(name)
    topo = sm.SHAPE_TOPOLOGY.get(name, (False, False))
    f, lon, lat, fills = sm.source_with_holes(g["x"], g["y"], nrec=3)
    v, fl = BD.interpolate(BD.points(g["x"], "h"), BD.points(g["y"], "h"), lon, lat, f, fills=fills)
    assert (fl == BD.UNFILLED).sum() > 0 and (fl == BD.REMAPPED).sum() > 0
    fv, ff, _ = BD.fill(v, fl, *topo)
    assert (ff == BD.FILLED).sum() == (fl == BD.UNFILLED).sum()
    ny, nx = fl.shape[1:]
    if nx == 2:
        assert topo[0] and BD.fill(v, fl, False, topo[1])[0].tobytes() != fv.tobytes()
        if ny == 3:   # the middle row's hole is filled from S, the doubled W / E, and N together
            nb = RD.neighbours(ny, nx, True, False)
            assert nb[1][2] == nb[2][2] == 3 and nb[0][2] == 0 and nb[3][2] == 4
    if nx == 1 and topo[0]:
        assert BD.fill(v, fl, False, topo[1])[0].tobytes() == fv.tobytes()
        assert RD.neighbours(ny, nx, True, False)[1].tolist() == list(range(ny))


def test_synthetic_flags_tell_the_seam_of_a_two_wide_grid():
    v, fl = sm.synthetic_flags(3, 2, 3, 0)
    assert RD.fill(v, fl, True, False)[0].tobytes() != RD.fill(v, fl, False, False)[0].tobytes()
    assert RD.fill(v, fl, True, True)[0].tobytes() != RD.fill(v, fl, True, False)[0].tobytes()


def test_sources_have_the_shapes_the_kernels_branch_on():
    for kind, (NA, NB) in sm.SOURCE_SHAPES.items():
        lon, lat = sm.source_edges(kind)
        assert (lon.size - 1, lat.size - 1) == (NA, NB)
        assert np.all(np.diff(lon) > 0) and np.all(np.diff(lat) > 0) and abs(lon[-1] - lon[0] - 360.0) <= 1e-9
        assert lat[0] >= -90.0 and lat[-1] <= 90.0
    NA, NB = sm.SOURCE_SHAPES["over_lds"]
    assert (NA + NB) * 8 == 67200 > 64 * 1024            # the tables do not fit in LDS by size
    assert (sm.SOURCE_SHAPES["regular"][0] + sm.SOURCE_SHAPES["regular"][1]) * 8 < 64 * 1024
    g = sm.topology_cuts()["neither"]
    f, lon, lat, fills = sm.source_for(g["x"], g["y"], "regular", nrec=5, dtype=np.float32, two_fills=True)
    assert f.dtype == np.float32 and fills == (-999.0, 1.0e20)
    for r in range(5):
        assert np.isnan(f[r]).any() and (f[r] == np.float32(-999.0)).any() and (f[r] == np.float32(1.0e20)).any()
    # flag words that straddle two records: nrec * ncell is no multiple of 4 on these
    for name, nrec in (("1x1", 3), ("1x63", 5), ("1x65", 6), ("3x3", 3), ("fold_5x7", 5), ("129x1", 1)):
        ny, nx, _ = sm.SHAPES[name]
        assert (nrec * ny * nx) % 4 != 0 and (ny * nx) % 4 != 0, name


def test_nan_latitude_is_an_unfilled_point_in_the_definition():
    """include/ogg_hip.h, "Bilinear interpolation", locate: a NaN latitude lies between no two nodes.  Whatever row the search clips
    to (NB - 2 by np.searchsorted, 0 by a binary search on comparisons), the point is unfilled with the fill value."""
    for kind in ("1x1", "1x5", "3x2", "7x1", "nonuniform"):
        lon, lat = sm.source_edges(kind)
        f = sm.smooth_field(lon, lat, 2, np.float64)
        x = np.array([[10.0, 20.0, np.nan, np.inf]])
        y = np.array([[5.0, np.nan, 5.0, 5.0]])
        with np.errstate(invalid="ignore"):
            v, fl = BD.interpolate(x, y, lon, lat, f)
        assert fl[:, 0, 1].tolist() == [BD.UNFILLED] * 2 and np.all(v[:, 0, 1] == BD.FILL), kind
        assert np.all(fl[:, 0, [0, 2, 3]] == BD.REMAPPED) and np.all(np.isfinite(v[:, 0, [0, 2, 3]])), kind
        assert v[:, 0, 2].tobytes() == v[:, 0, 3].tobytes()   # NaN and infinite longitudes both reduce to t = 0
        mask = np.array([[1, 0, 1, 1]], np.uint8)
        with np.errstate(invalid="ignore"):
            _, flm = BD.interpolate(x, y, lon, lat, f, mask=mask)
        assert np.all(flm[:, 0, 1] == BD.DRY)


def load_truth_script():
    spec = importlib.util.spec_from_file_location("xgrid_truth", os.path.join(ROOT, "scripts", "xgrid_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_truth_file_is_what_the_script_makes_and_the_definition_is_this_far_from_it(zoo, capsys):
    pytest.importorskip("mpmath")
    want = load_truth_script().table()
    got = np.load(sm.TRUTH)
    assert set(got.files) == set(want)
    # what mpmath makes is compared bit for bit; what the fp64 definition adds (which slivers it keeps, its own errors) may move with
    # the host's sin and cos: the pieces are matched by key, those in one table only must be slivers, the errors agree within 2
    assert want["cells"].tolist() == got["cells"].tolist() and want["a_poly"].tobytes() == got["a_poly"].tobytes()
    wk = {tuple(k): i for i, k in enumerate(want["pairs"].tolist())}
    gk = {tuple(k): i for i, k in enumerate(got["pairs"].tolist())}
    common = sorted(set(wk) & set(gk))
    assert want["area"][[wk[k] for k in common]].tobytes() == got["area"][[gk[k] for k in common]].tobytes()
    a_of = dict(zip(got["cells"].tolist(), got["a_poly"][:, 0]))
    for tab, keys in ((want, set(wk) - set(gk)), (got, set(gk) - set(wk))):
        for k in keys:
            i = (wk if tab is want else gk)[k]
            assert tab["area"][i, 0] <= 1e-10 * a_of[k[2]], k
    for k in ("eref_poly", "eref_piece", "eref_poly_rest", "eref_piece_rest"):
        assert 0.5 <= float(want[k]) / float(got[k]) <= 2.0, k
    assert os.path.getsize(sm.TRUTH) < 100 * 1024
    # every finite cell and every kept piece of the zoo has its truth
    ap = zoo["a_poly"][0]
    assert got["cells"].tolist() == np.nonzero(np.isfinite(ap))[0].tolist()
    assert len(common) >= 0.99 * len(zoo["lst"])
    t = got["a_poly"]
    pos = t[:, 0] > 0
    e_poly = np.max(np.abs((ap[got["cells"]][pos] - t[pos, 0]) - t[pos, 1]) / t[pos, 0])
    area = np.array([e[4] for e in zoo["lst"]])
    e_piece = np.max(np.abs((area - got["area"][:, 0]) - got["area"][:, 1]) / ap[got["pairs"][:, 2]])
    with capsys.disabled():
        print("\nzoo, definition against the 50-digit truth: A_poly %.3e, pieces %.3e (relative to A_poly)" % (e_poly, e_piece))
    assert 0.5 <= e_poly / float(got["eref_poly"]) <= 2.0 and 0.5 <= e_piece / float(got["eref_piece"]) <= 2.0
    assert float(got["eref_poly_rest"]) < 0.2 * float(got["eref_poly"])   # the bow-tie alone sets the larger figure
    # the exact areas of the cells that have one in closed form
    D = np.pi / 180.0
    for name, want_a in (("two_opposite", sm.RE ** 2 * 4.0 * D * 2.0),
                         ("on_edges", sm.RE ** 2 * 4.0 * D * (np.sin(18.0 * D) - np.sin(14.0 * D))),
                         ("two_adjacent", sm.RE ** 2 * 4.0 * D * (1.0 - np.sin(85.0 * D)))):
        k = got["cells"].tolist().index(zoo["where"][name])
        assert abs(t[k, 0] / want_a - 1) <= 1e-14, name
    # inverted cells have a negative (or exactly zero) truth as well: the class does not hang on the definition's rounding
    for k, n in enumerate(got["cells"]):
        assert (t[k, 0] > 0) == (ap[n] > 0), n

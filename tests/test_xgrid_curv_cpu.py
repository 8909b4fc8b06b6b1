"""CPU tests of the curvilinear-source exchange grid's definition (tests/xgrid_curv_definition.py, the restatement of include/ogg_hip.h,
"Exchange grid with a curvilinear source grid"): the numpy box search against the plain double loop, every named input of
tests/test_gpu_xgrid_curv.py reaching the branch it is named for, and the definition alone inside the conservation bounds the device
is held to, on the conservation test's source.  No device is needed."""
import numpy as np
import pytest

import xgrid_cs_definition as cd
import xgrid_curv_definition as vd

RE = 6371.0e3


def target(name):
    x, y, _ = cd.zoo()[name]
    return x, y


def per_cell(lst, shape, col):
    """the areas of a list summed per target cell (col 2: (n, m)) or per source cell (col 0: (I, J))"""
    s = np.zeros(shape)
    for e in lst:
        s[e[col + 1], e[col]] += e[4]
    return s


@pytest.mark.parametrize("tname", ["regional_1x1", "regional_2x3", "regional_1x65", "bow_tie", "pole_two_1", "big_25"])
def test_the_box_search_equals_the_double_loop(tname):
    x, y = target(tname)
    for sname, (sx, sy) in vd.sources_for(x, y).items():
        a = vd.exchange_grid_curv(x, y, sx, sy, Re=RE, threshold=0.0)
        b = vd.exchange_grid_curv(x, y, sx, sy, Re=RE, threshold=0.0, brute=True)
        assert a[0] == b[0] and a[3] == b[3], (tname, sname)
        assert a[6] <= 8, (tname, sname, a[6])


def test_the_named_sources_reach_their_branches():
    x, y = target("regional_2x3")
    s = vd.sources_for(x, y)
    base = vd.exchange_grid_curv(x, y, *s["rotated_12x9"], Re=RE)
    lst, a_poly, a_src, counts, status, sstat, nvmax, _ = base
    assert set(status.values()) == {"ok"} and set(sstat.values()) == {"ok"}
    assert counts["kept"] > counts["cells"] and 3 <= nvmax <= 8           # clipped polygons, not whole cells only
    ap = cd.a_poly_array(a_poly)
    assert np.max(np.abs(per_cell(lst, ap.shape, 2) / ap - 1)) <= 1e-11   # the mesh covers the target: the pieces partition every cell
    # the same mesh stored north to south: every cell REVERSED, the list the first one's with J mirrored
    flip = vd.exchange_grid_curv(x, y, *s["north_to_south"], Re=RE)
    assert set(flip[5].values()) == {"reversed"} and flip[3]["src_reversed"] == 12 * 9
    mirrored = sorted((I, 8 - J, n, m, a) for I, J, n, m, a in flip[0])
    want = sorted(lst)
    assert [e[:4] for e in mirrored] == [e[:4] for e in want]
    assert max(abs(a[4] - b[4]) for a, b in zip(mirrored, want)) <= 1e-12 * ap.max()
    # its own pole inside the target: triangles whose north edge is one point, a zero normal that clips nothing
    sx, sy = s["pole_inside"]
    assert np.all(sx[-1] == sx[-1, 0]) and np.all(sy[-1] == sy[-1, 0])
    fan = vd.exchange_grid_curv(x, y, sx, sy, Re=RE, threshold=0.0)
    assert set(fan[5].values()) == {"ok"}
    tri = [e for e in fan[0] if e[1] == sx.shape[0] - 2]
    assert len({e[0] for e in tri}) == 8                                  # all eight triangles overlap the target
    assert np.max(np.abs(per_cell(fan[0], ap.shape, 2) / ap - 1)) <= 1e-11
    # NaN-cornered, FLAT and 31-degree cells
    bad = vd.exchange_grid_curv(x, y, *s["bad_cells"], Re=RE)
    assert bad[5][(0, 0)] == "degenerate" and bad[5][(1, 1)] == "flat" and bad[5][(0, 4)] == bad[5][(1, 4)] == "wide"
    assert (bad[3]["src_degenerate"], bad[3]["src_flat"], bad[3]["src_wide"]) == (1, 1, 2) and bad[3]["kept"] > 0
    assert not {(0, 0), (1, 1), (0, 4), (1, 4)} & {(e[1], e[0]) for e in bad[0]}
    one = vd.exchange_grid_curv(x, y, *s["one_cell"], Re=RE)
    assert one[3]["src_cells"] == 1 and one[3]["kept"] == one[3]["cells"] == 6


def test_whole_turns_disjoint_and_touching_sources():
    x, y = target("regional_2x3")          # 30.25 .. 31.75 E, 20.5 .. 22 N
    sx, sy = vd.regular_mesh(29.75, 20.25, 0.75, 0.5, 4, 5)
    base = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)
    assert np.all((sx + 720.0) - 720.0 == sx)
    away = vd.exchange_grid_curv(x, y, sx + 720.0, sy, Re=RE)
    assert away[0] == base[0] and away[3] == base[3] and base[3]["kept"] > 0
    dis = vd.exchange_grid_curv(x, y, *vd.regular_mesh(100.0, -40.0, 1.0, 1.0, 3, 3), Re=RE)
    assert dis[3]["candidates"] == 0 and dis[3]["kept"] == 0
    touch = vd.exchange_grid_curv(x, y, *vd.regular_mesh(28.25, 20.5, 2.0, 1.5, 1, 1), Re=RE)   # shares the meridian 30.25 E
    assert touch[3]["candidates"] > 0 and touch[3]["kept"] == 0


def test_masks_select_entries():
    x, y = target("regional_2x3")
    sx, sy = vd.sources_for(x, y)["rotated_12x9"]
    base = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)[0]
    rng = np.random.default_rng(3)
    mask, smask = (rng.random((2, 3)) < 0.6).astype(np.uint8), (rng.random((9, 12)) < 0.6).astype(np.uint8)
    got = vd.exchange_grid_curv(x, y, sx, sy, mask=mask, src_mask=smask, Re=RE)
    assert got[0] == [e for e in base if mask[e[3], e[2]] and smask[e[1], e[0]]]
    assert got[3]["masked"] == int((mask == 0).sum()) and got[3]["src_masked"] == int((smask == 0).sum())


def test_the_definition_conserves_on_the_conservation_source():
    """The global 24 x 12 rotated-pole source of the device's conservation test, against a global 10-degree lat-lon target with pole
    triangles (the generated grids of that test need the device): per target cell and per source cell the pieces sum to A_poly and
    A_src within 1e-11, over the sphere within 1e-12, the bounds the device is held to."""
    x, y = cd.regional(-180.0, -90.0, 10.0, 10.0, 36, 18)
    sx, sy = vd.global_rotated()
    lst, a_poly, a_src, counts, status, sstat, nvmax, _ = vd.exchange_grid_curv(x, y, sx, sy, Re=RE, threshold=0.0)
    assert set(status.values()) == {"ok"} and set(sstat.values()) == {"ok"} and counts["src_wide"] == 0 and nvmax <= 8
    ap, asrc = cd.a_poly_array(a_poly), cd.a_poly_array(a_src)
    sphere = 4 * np.pi * RE * RE
    assert abs(ap.sum() / sphere - 1) <= 1e-12 and abs(asrc.sum() / sphere - 1) <= 1e-12
    e_ocn = np.max(np.abs(per_cell(lst, ap.shape, 2) / ap - 1))
    e_src = np.max(np.abs(per_cell(lst, asrc.shape, 0) / asrc - 1))
    e_glob = abs(sum(e[4] for e in lst) / sphere - 1)
    print("definition alone: ocean %.2e, source %.2e, global %.2e" % (e_ocn, e_src, e_glob))
    assert e_ocn <= 1e-11 and e_src <= 1e-11 and e_glob <= 1e-12


def test_without_the_shared_corner_rule_a_mesh_over_itself_loses_slivers(monkeypatch):
    """Why the definition measures a vertex exactly 0 against an edge it is an end of: T(a; a, b) as computed is a rounding-sized
    number of either sign, and where it comes out negative the inclusive test cuts the corner off.  With the rule a mesh laid over
    itself gives every cell whole, bit for bit; with the rule switched off most cells go through the clip and lose up to 1e-12 of
    their area (measured: 180 of 195 half-degree cells, the largest loss 9.7e-13)."""
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 3)[:2]
    sx, sy = x[0::2, 0::2], y[0::2, 0::2]

    def own(lst, ap):
        return [(e[4], ap[e[3], e[2]]) for e in lst if (e[1], e[0]) == (e[3], e[2])]
    with_rule = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)
    ap = cd.a_poly_array(with_rule[1])
    assert with_rule[3]["kept"] == 195 and all(a == b for a, b in own(with_rule[0], ap))
    monkeypatch.setattr(vd, "edge_measure", lambda v, Q, normals, e: vd.measure(v, normals[e]))
    without = own(vd.exchange_grid_curv(x, y, sx, sy, Re=RE)[0], ap)
    assert len(without) == 195
    changed = [abs(a / b - 1) for a, b in without if a != b]
    print("without the rule: %d of 195 cells changed, the largest by %.2e" % (len(changed), max(changed)))
    assert len(changed) > 100 and 1e-13 < max(changed) < 1e-11

"""CPU tests of the every-element check of the generic stencil (tests/stencil_bounds.py over tests/golden/truth_stencil_*.npz), with the oracle
alone:

  * the fixtures: sizes, shapes, the meshes' features (fold row, pole points at exactly 90 degrees, pole row, whole turns, zero dx and dy),
    the builder against the stored meshes, the window shapes;
  * no false alarm: the oracle on this host reproduces every stored R within 2x and passes the checker on every fixture;
  * planted defects on the oracle's arrays, each 4x the new bound of the elements it touches -- one element, one column either side of the
    kernel's tile edge 255 | 256, one row at a tile-row edge, the area formed with one row's sines moved by 4 ulp, a window's first and last
    angle column taken from the mesh around it (two-sided) -- each fail the checker with a planted element named;
  * LET_THROUGH records which of them today's assertions of tests/test_gpu_parity.py::test_midas_ragged_shapes (dx, dy 2e-15 relative, area
    5e-12 of the largest area, angle 1e-11 degrees, all against the oracle) let through: every defect of area and angle but the two-sided window
    columns; the dx and dy defects are caught by both (there the conditioned bound, 0.8e-15 to 2e-15 of a benign value, is about the old one);
  * the plan: with the knobs the GPU tests use, every tile instantiation 4, 6, 8, 12, rows per block 1 .. 12 and the streaming heights 1, 4
    and 16 are planned on the fixtures (ogg_grid_metrics_midas_plan, no device), and the defaults plan what they always did;
  * scripts/truth_table.py --groups stencil --quick runs, and what it computes equals the committed fixtures.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_bounds as sb
import stencil_meshes as sm
import stencil_plans as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}
# planted defect -> do the old assertions (test_midas_ragged_shapes') pass it?
LET_THROUGH = {"one element: area": True, "one element: angle": True, "one element: dx": False,
               "column 255: dy": False, "column 256: dy": False, "column 255: angle": True, "column 256: angle": True,
               "column 255: area": True, "column 254: area_nofix": True,
               "row 6: dx": False, "row 6: area": True, "row 6: angle": True,
               "sines of row 6 moved by 4 ulp: area": True,
               "window columns two-sided: angle": False}
SEEN = {}


def _oracle(name):
    if name not in _ORACLE:
        fx = sb.load(name)
        o = sb.oracle(fx["x"], fx["y"])
        for a in o.values():
            a.setflags(write=False)
        _ORACLE[name] = o
    return _ORACLE[name]


def _copies(name):
    return {f: a.copy() for f, a in _oracle(name).items()}


def _old_assertions_pass(got, want):
    """The lines of tests/test_gpu_parity.py::test_midas_ragged_shapes, against the oracle."""
    def maxrel(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0
    ok = maxrel(got["dx"], want["dx"]) < 2e-15 and maxrel(got["dy"], want["dy"]) < 2e-15
    ok = ok and float(np.abs(got["area"] - want["area"]).max()) <= 5e-12 * np.abs(want["area"]).max()
    ok = ok and float(np.abs(got["area_nofix"] - want["area_nofix"]).max()) <= 5e-12 * np.abs(want["area_nofix"]).max()
    return bool(ok and float(np.abs(got["angle"] - want["angle"]).max()) < 1e-11)


def _planted(label, name, got, field, where):
    """check() must raise and every element it names must be of `field` and satisfy where(j, i); records what the old assertions make of it."""
    with pytest.raises(sb.StencilBoundError) as ex:
        sb.check(name, got, tag=label)
    worst = ex.value.worst
    assert worst and all(w[0] == field and where(w[1], w[2]) for w in worst), (label, worst)
    SEEN[label] = _old_assertions_pass(got, _oracle(name))
    assert SEEN[label] == LET_THROUGH[label], (label, SEEN[label])


def _bound(name, field):
    fx = sb.load(name)
    return sb.K_REF * max(fx["R"][field], 1.0) * sb.scales(fx["x"], fx["y"])[field]


# ---------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------
def test_fixture_files():
    for f in sb.FILES.values():
        path = os.path.join(sb.GOLD, f)
        assert os.path.getsize(path) <= sb.MAX_FILE_BYTES, f
        assert int(sb.scalar(np.load(path)["dps"])) == 50
    assert [sm.WINDOWS[w][3:] for w in sm.WINDOWS] == sm.WINDOW_SHAPES == [(1, 2), (2, 2), (2, 3), (1, 257), (3, 255), (3, 256), (3, 257), (3, 258), (7, 513)]
    assert sb.names() == list(sm.MESHES) + list(sm.WINDOWS) and len(sb.names()) == 13


@pytest.mark.parametrize("name", sm.MESHES)
def test_builder_gives_the_stored_mesh(name):
    """The stored mesh is the input of the truth; the builder documents where it came from (the caps' last bits are the generating host's libm's)."""
    fx = sb.load(name)
    x, y = sm.BUILDERS[name]()
    assert x.shape == fx["x"].shape and np.abs(x - fx["x"]).max() <= 1e-11 and np.abs(y - fx["y"]).max() <= 1e-11
    if name == "edge":
        assert np.array_equal(x, fx["x"]) and np.array_equal(y, fx["y"]) and np.array_equal(np.signbit(y), np.signbit(fx["y"]))      # + - * / only


def test_mesh_features():
    b, d, t, e = (sb.load(n) for n in sm.MESHES)
    assert b["x"].shape == (12, 257) and d["x"].shape == (12, 261) and t["x"].shape == (8, 515) and e["x"].shape == (9, 259)
    # bipolar: pole points at exactly 90 degrees, the fold row mirrors itself, the seam is one meridian 360 degrees apart
    assert b["y"][11, 64] == 90.0 and b["y"][11, 192] == 90.0 and (b["y"] == 90.0).sum() == 2
    assert np.abs(b["y"][11] - b["y"][11, ::-1]).max() < 1e-12 and np.all(b["x"][:, 256] - b["x"][:, 0] == 360.0)
    # displaced pole: row 0 is one point, longitudes unwrap below the first meridian
    assert np.ptp(d["x"][0]) == 0 and np.ptp(d["y"][0]) == 0 and d["x"].min() < -300.0 - 30.0
    assert np.all(d["truth"]["dx"][0][0] == 0) and np.all(d["truth"]["angle"][0][0] == 0)
    # whole turns: neighbours up to four turns apart, mdist undoes them (dx of a smooth mesh), angle_x does not (D of hundreds of degrees)
    jump = np.abs(np.diff(t["x"], axis=1))
    assert jump.max() > 1400.0 and (jump > 300.0).mean() > 0.5
    assert t["truth"]["dx"][0].max() < 6371e3 * np.radians(3.0)
    # edge: rows at +-90 and 1e-10 inside, signed zeros on the equator, exact zeros of dx (two columns, every row) and dy (two rows, even columns)
    assert np.all(e["y"][0] == -90.0) and np.all(e["y"][8] == 90.0) and np.all(e["y"][1] == -(90.0 - 1e-10)) and np.all(e["y"][7] == 90.0 - 1e-10)
    assert np.all(e["y"][3] == 0) and np.signbit(e["y"][3]).sum() == int((np.arange(259) % 4 >= 2).sum())
    dxh, dxl = e["truth"]["dx"]
    assert np.all(dxh[:, sm.ZERO_DX_COLUMNS[0]] == 0) and np.all(dxl[:, sm.ZERO_DX_COLUMNS[0]] == 0) and (dxh == 0).sum() == 9
    dyh = e["truth"]["dy"][0]
    assert np.all(dyh[sm.ZERO_DY_ROWS[0], 0::2] == 0) and np.all(dyh[sm.ZERO_DY_ROWS[0], 1::2][:40] > 0)
    # at exactly +-90 degrees dx is 1e-10 of its neighbours and the relative error of the ORACLE is of order one: only a conditioned bound holds there
    o = _oracle("edge")["dx"]
    rel = np.abs(o[8] - dxh[8])[dxh[8] > 0] / dxh[8][dxh[8] > 0]
    assert rel.max() > 0.1 and 0 < dxh[8].max() < 1e-3


@pytest.mark.parametrize("name", sb.names())
def test_the_lo_words_are_remainders(name):
    fx = sb.load(name)
    for f in sb.FIELDS:
        hi, lo = fx["truth"][f]
        assert np.all(np.abs(lo.astype(np.float64)) <= 0.5000001 * np.spacing(np.abs(hi))), (name, f)
        assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))


# ---------------------------------------------------------------------------------------------------------------
# no false alarm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sb.names())
def test_oracle_reproduces_r_and_passes(name):
    fx = sb.load(name)
    rep = sb.check(name, _oracle(name), tag="oracle")
    assert sorted(rep) == sorted(f for f in sb.FIELDS if fx["truth"][f][0].size)
    for f, r in rep.items():
        print("%-8s %-10s oracle |error| / s: max %.2f median %.2f (fixture %.2f, %.2f); %d held, %d exact zeros, %d left out" % (
            name, f, r["worst_over_s"], r["median_over_s"], fx["R"][f], fx["Rmed"][f], r["n"], r["n_zero"], r["n_singular"]))
        assert r["worst_over_s"] <= 2.0 * fx["R"][f] + 1e-12, (name, f, r)
        if r["n"] >= 100:                                    # ... and the fixture's figure is no looser than the oracle is (a handful of elements: no statistics)
            assert r["worst_over_s"] >= 0.5 * fx["R"][f], (name, f, r)
        assert r["worst_over_bound"] < 1.0 and r["n_singular"] == (fx["n_singular"] if f == "angle" else 0)
        assert fx["R"][f] < 1.0                              # the scale is a worst case: no class was split, the floor of one s governs


def test_what_is_left_out():
    """The angle at the points of +-90 degrees whose N vanishes, nothing else: counted from the mesh alone.  (In the window w1x2 the pole point
    is the first column: its angle is one-sided, N does not vanish, and it is held.)"""
    want = {"bipolar": 2, "dpole": 0, "turns": 0, "edge": 2 * 259, "w1x257": 2, "w3x257": 257}
    for name in sb.names():
        fx = sb.load(name)
        m = sb.angle_singular(fx["x"], fx["y"])
        assert int(m.sum()) == fx["n_singular"] == want.get(name, 0), name
        assert np.all(np.abs(fx["y"][m]) == 90.0)
    assert np.argwhere(sb.angle_singular(sb.load("bipolar")["x"], sb.load("bipolar")["y"])).tolist() == [[11, 64], [11, 192]]


def test_a_wrong_count_of_left_out_points_fails(monkeypatch):
    monkeypatch.setitem(sb._CACHE, "bipolar", dict(sb.load("bipolar"), n_singular=3))
    with pytest.raises(AssertionError, match="left out"):
        sb.check("bipolar", _oracle("bipolar"))


def test_nan_and_wrong_zeros_fail():
    got = _copies("edge")
    got["dy"][1, 7] = np.nan
    with pytest.raises(sb.StencilBoundError) as ex:
        sb.check("edge", got)
    assert ex.value.worst[0][:3] == ("dy", 1, 7)
    got = _copies("edge")
    assert got["dx"][2, 100] == 0 and not np.signbit(got["dx"][2, 100])
    got["dx"][2, 100] = -0.0                                  # the truth is exactly zero: +0.0 or nothing
    with pytest.raises(sb.StencilBoundError) as ex:
        sb.check("edge", got)
    assert ex.value.worst[0][:3] == ("dx", 2, 100)
    got = _copies("edge")
    got["dx"][2, 100] = 1e-300
    with pytest.raises(sb.StencilBoundError):
        sb.check("edge", got)
    # the angle's zero is numpy's: -0.0 where N is -0.0 (the equator row: y = +0.0, +0.0, -0.0, -0.0, ...)
    a = _oracle("edge")["angle"]
    assert np.all(a[3] == 0) and np.signbit(a[3, 1]) and not np.signbit(a[3, 3]) and 100 < np.signbit(a[3]).sum() < 159
    got = _copies("edge")
    got["angle"][3, 1] = 0.0
    with pytest.raises(sb.StencilBoundError) as ex:
        sb.check("edge", got)
    assert ex.value.worst[0][:3] == ("angle", 3, 1)


def test_angles_compare_modulo_360():
    got = _copies("turns")
    k = np.argmax(np.abs(got["angle"]))
    j, i = np.unravel_index(k, got["angle"].shape)
    assert abs(got["angle"][j, i]) > 170.0
    got["angle"][j, i] -= 360.0 * np.sign(got["angle"][j, i])
    sb.check("turns", got)


# ---------------------------------------------------------------------------------------------------------------
# planted defects: 4x the new bound of every element they touch, on the displaced-pole cap (261 columns: the tile edge 255 | 256 is inside
# every field; 12 rows: the default tile's row edge 5 | 6)
# ---------------------------------------------------------------------------------------------------------------
def test_planted_one_element():
    for f, (j, i) in (("area", (4, 77)), ("angle", (7, 130)), ("dx", (9, 200))):
        got = _copies("dpole")
        got[f][j, i] += 4.0 * _bound("dpole", f)[j, i]
        _planted("one element: " + f, "dpole", got, f, lambda a, b: (a, b) == (j, i))


def test_planted_columns_at_the_tile_edge():
    for f, cols in (("dy", (255, 256)), ("angle", (255, 256)), ("area", (255,)), ("area_nofix", (254,))):
        for c in cols:
            got = _copies("dpole")
            got[f][:, c] += 4.0 * _bound("dpole", f)[:, c]
            _planted("column %d: %s" % (c, f), "dpole", got, f, lambda a, b: b == c)


def test_planted_row_at_a_tile_row_edge():
    for f in ("dx", "area", "angle"):
        got = _copies("dpole")
        got[f][6] -= 4.0 * _bound("dpole", f)[6]
        _planted("row 6: " + f, "dpole", got, f, lambda a, b: a == 6)


def test_planted_sines_of_one_row():
    """OGG:711-713 with the sines of edge row 6 four ulp up: the areas of cell rows 5 and 6 move by Re^2 dxi 4 ulp(sin), 5e-13 of a cell."""
    fx = sb.load("dpole")
    x, y = fx["x"], fx["y"]
    lv = (0.5 * (y[:, 1:] + y[:, :-1])) * sb.PI_180
    dxi = sb.mdist(x[:, 1:], x[:, :-1]) * sb.PI_180
    sl = np.sin(lv)
    area = (sb.RE ** 2) * ((0.5 * (dxi[1:] + dxi[:-1])) * (sl[1:] - sl[:-1]))
    assert np.array_equal(area, _oracle("dpole")["area"])
    for _ in range(4):
        sl[6] = np.nextafter(sl[6], 2.0)
    got = _copies("dpole")
    got["area"] = (sb.RE ** 2) * ((0.5 * (dxi[1:] + dxi[:-1])) * (sl[1:] - sl[:-1]))
    assert np.all(got["area"][[5, 6]] != _oracle("dpole")["area"][[5, 6]]) and np.array_equal(np.delete(got["area"], [5, 6], 0), np.delete(_oracle("dpole")["area"], [5, 6], 0))
    _planted("sines of row 6 moved by 4 ulp: area", "dpole", got, "area", lambda a, b: a in (5, 6))


def test_planted_window_columns_two_sided():
    """A window's first and last angle column are one-sided IN THE WINDOW; taken from the mesh around it they are two-sided."""
    m, j0, i0, nj, ni = sm.WINDOWS["w3x258"]
    got = _copies("w3x258")
    got["angle"] = _oracle(m)["angle"][j0:j0 + nj, i0:i0 + ni].copy()
    assert np.array_equal(got["angle"][:, 1:-1], _oracle("w3x258")["angle"][:, 1:-1])
    _planted("window columns two-sided: angle", "w3x258", got, "angle", lambda a, b: b in (0, ni - 1))


def test_every_planted_defect_was_judged():
    """LET_THROUGH names exactly the defects the tests above plant (they are run again here, so this test stands alone in any order)."""
    SEEN.clear()
    for plant in (test_planted_one_element, test_planted_columns_at_the_tile_edge, test_planted_row_at_a_tile_row_edge, test_planted_sines_of_one_row,
                  test_planted_window_columns_two_sided):
        plant()
    assert SEEN == LET_THROUGH


# ---------------------------------------------------------------------------------------------------------------
# meshes without a truth
# ---------------------------------------------------------------------------------------------------------------
def test_check_against_oracle():
    rng = np.random.default_rng(5)
    x = np.tile(-300 + np.arange(65) * 360.0 / 64, (9, 1)) + rng.normal(0, 0.05, (9, 65))
    y = np.tile(np.linspace(-89.99, 89.99, 9).reshape(9, 1), (1, 65)) + rng.normal(0, 0.05, (9, 65))
    o = sb.oracle(x, y)
    rep = sb.check_against_oracle(x, y, o)
    assert all(r["worst_over_bound"] == 0 for r in rep.values()) and sb.r_max("dx") == 1.0
    s = sb.scales(x, y)
    got = {f: a.copy() for f, a in o.items()}
    got["area"][3, 30] += 2.4 * s["area"][3, 30]                  # inside (K_REF + 1) s
    sb.check_against_oracle(x, y, got)
    got["area"][3, 30] = o["area"][3, 30] + 2.6 * s["area"][3, 30]
    with pytest.raises(sb.StencilBoundError) as ex:
        sb.check_against_oracle(x, y, got)
    assert ex.value.worst[0][:3] == ("area", 3, 30)
    # on the latitude range test_midas_ragged_shapes had (+-80 degrees) the conditioned bound of dx and dy, 2.5 s, is 1.4e-15 to 6.4e-15 of the
    # value: about the relative 2e-15 of that test, not always under it -- so that test keeps its relative lines and gains this check
    y80 = np.tile(np.linspace(-80, 80, 9).reshape(9, 1), (1, 65)) + rng.normal(0, 0.05, (9, 65))
    s80, o80 = sb.scales(x, y80), sb.oracle(x, y80)
    q = 2.5 * s80["dx"] / o80["dx"]
    assert 1.2e-15 < q.min() < 2e-15 < q.max() < 8e-15
    qa = 2.5 * s80["area"].max() / (5e-12 * np.abs(o80["area"]).max())
    assert qa < 0.05                                              # the area: at least 20 times tighter than 5e-12 of the largest cell


# ---------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_is_planned_on_the_fixtures():
    from ocean_model_grid_generator_amd import _lib
    tiles, streams = set(), set()
    for name in sb.names():
        nj1, ni1 = sb.load(name)["x"].shape
        for metrics, n in ((True, max(nj1, 2)), (False, nj1)):          # a single row of points runs twice for its dx
            for label, env, want in sp.variants(ni1, n, metrics):
                got = sp.planned(_lib, ni1, n, metrics, env)
                assert got == want, (name, label, metrics, got, want)
                (tiles if got[0] else streams).add(got)
    assert {t[0] for t in tiles} == {4, 6, 8, 12}
    assert {t[1] for t in tiles} == set(range(1, 13))
    assert all(rpb <= tr and (tr == 4 or rpb > {6: 4, 8: 6, 12: 8}[tr]) for tr, rpb in tiles)
    assert {1, 4, 16} <= {s[1] for s in streams} and max(s[1] for s in streams) == 16


def test_default_plan_is_unchanged(monkeypatch):
    from ocean_model_grid_generator_amd import _lib
    monkeypatch.delenv("OGG_MIDAS_TILE_ROWS", raising=False)
    monkeypatch.delenv("OGG_MIDAS_TARGET_WG", raising=False)
    for ni1, n, want in ((5761, 2241, (6, 6)), (5761, 100, (4, 2)), (5761, 300, (4, 4)), (11521, 200, (6, 5)), (2, 1, (4, 1)), (1000, 200, (4, 2)),
                         (5761, 64, (4, 2))):
        assert sp.planned(_lib, ni1, n, True) == want == sp.expected(ni1, n, True, 6, 2048)
    assert sp.planned(_lib, 5761, 2241, True, {"OGG_MIDAS_TILE_ROWS": "0"}) == (0, 16)
    assert sp.planned(_lib, 5761, 100, False, {"OGG_MIDAS_TILE_ROWS": "0"}) == (0, 2)
    assert sp.planned(_lib, 5761, 100, True, {"OGG_MIDAS_TARGET_WG": "0"}) == (4, 2)          # not a count: the default
    assert sp.planned(_lib, 5761, 2241, True, {"OGG_MIDAS_TARGET_WG": str(2 ** 63 - 1)}) == (4, 2) == sp.expected(5761, 2241, True, 6, 2 ** 63 - 1)   # no overflow
    # the shapes of test_midas_tile_heights_and_streaming_kernel_agree_bitwise plan ONE tile height at the default target, whatever the setting;
    # with one workgroup per column tile each setting plans the height its name says, as far as the mesh has rows
    for nj, ni in ((2, 2), (5, 63), (7, 258), (31, 513), (200, 1000), (64, 5761)):
        assert {sp.planned(_lib, ni, nj, True, {"OGG_MIDAS_TILE_ROWS": k}) for k in ("1", "2", "4", "6", "8", "12", "99")} == {(4, 2)}
        assert sp.planned(_lib, ni, nj, True, {"OGG_MIDAS_TILE_ROWS": "0"}) == (0, 4)
        for k in (1, 2, 4, 6, 8, 12, 99):
            env = {"OGG_MIDAS_TILE_ROWS": str(k), "OGG_MIDAS_TARGET_WG": "1"}
            h = min(k, 12, nj)
            assert sp.planned(_lib, ni, nj, True, env) == (4 if h <= 4 else 6 if h <= 6 else 8 if h <= 8 else 12, h) == sp.expected(ni, nj, True, k, 1)
        assert sp.planned(_lib, ni, nj, True, {"OGG_MIDAS_TILE_ROWS": "0", "OGG_MIDAS_TARGET_WG": "1"}) == (0, min(max(nj * ((ni + 255) // 256), 4), 16))
    assert sp.planned(_lib, 2, 1, False, {"OGG_MIDAS_TILE_ROWS": "1"}) == (4, 1) == sp.expected(2, 1, False, 1, 2048)
    assert sp.planned(_lib, 300, 5, True, {"OGG_MIDAS_TILE_ROWS": "1"}) == (4, 2) == sp.expected(300, 5, True, 1, 2048)
    with pytest.raises(Exception):
        sp.planned(_lib, 1, 5, True)


# ---------------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------------
def test_truth_script_quick_run(tmp_path):
    """scripts/truth_table.py --groups stencil --quick (the first three rows of every mesh, the windows of at most three columns) into a temporary
    directory: what it computes is what the committed fixtures hold."""
    before = {n: os.path.getmtime(os.path.join(sb.GOLD, n)) for n in os.listdir(sb.GOLD)}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "truth_table.py"), "--groups", "stencil", "--quick", "--procs", "4",
                        "--metrics-dir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:]
    assert before == {n: os.path.getmtime(os.path.join(sb.GOLD, n)) for n in os.listdir(sb.GOLD)}          # no fixture was touched
    n_cmp = 0
    for key, fname in sb.FILES.items():
        quick = np.load(os.path.join(str(tmp_path), fname.replace(".npz", "_quick.npz")))
        full = np.load(os.path.join(sb.GOLD, fname))
        for k in quick.files:
            if k.endswith("_hi") or k.endswith("_lo"):
                name, f = k.split("_", 1)[0], k.split("_", 1)[1][:-3]
                # the mesh the script built on THIS host may differ from the stored one in the caps' last bits: compare where it does not
                same = key in ("edge", "windows") or np.array_equal(sm.BUILDERS[key]()[0], full[key + "_x"]) and np.array_equal(sm.BUILDERS[key]()[1], full[key + "_y"])
                if same and (key != "windows" or sm.WINDOWS[name][0] == "edge" or all(
                        np.array_equal(a, b) for a, b in zip(sm.BUILDERS[sm.WINDOWS[name][0]](), (sb.load(sm.WINDOWS[name][0])["x"], sb.load(sm.WINDOWS[name][0])["y"])))):
                    q = quick[k]
                    assert np.array_equal(q, full[k][:q.shape[0]]), k
                    n_cmp += q.size
            elif k.endswith("_x") or k.endswith("_y"):
                assert np.abs(quick[k] - full[k]).max() <= 1e-11, k
    assert n_cmp > 3000

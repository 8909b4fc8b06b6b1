"""CPU tests of the every-element check of the small caps' metrics (tests/quad_bounds.py over tests/golden/truth_small_caps_metrics*.npz),
with the oracle alone:

  * the fixtures: sizes, shapes, parameters (those of truth_small_caps.npz), class census, and the unit of the stored integers against the
    smallest bound it feeds;
  * no false alarm: the oracle on this host reproduces every `eref` of the fixtures within 2x and passes the checker, every cap and order;
  * planted defects on the oracle's arrays -- one cell, one image column, the top edge row shifted, the last column lost, a guarded cell
    with its neighbour's value -- each fail the checker with the planted element reported;
  * what tests/test_gpu_parity.py's SUB_TOL, until now the only bound on the PASS's cap metrics, makes of the same defects: on the
    displaced-pole caps (2e-12 * Ni = 7.2e-10 relative) the (1 + 1e-12) scalings, the shifted top edge row and a cell at 10x the reference's
    own error all pass it; on the bipolar cap (area: 1e-6 m^2 + 2e-13 relative) a cell scaled by (1 + 1e-13) does.  (The lost last column
    and the neighbour's value are gross enough for SUB_TOL too; they are here for the checker's own sake.)
  * scripts/truth_table.py --groups small_metrics --quick runs, and what it computes equals the committed fixture.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import quad_bounds as qb
from test_gpu_parity import SUB_TOL, dp_quad_rel_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [(tag, None) for tag in sorted(qb.FILES)] + [(tag, n) for tag in sorted(qb.REDUCED_ORDERS) for n in qb.REDUCED_ORDERS[tag]]
BIPOLAR = [t for t in sorted(qb.KIND) if qb.KIND[t] == "bipolar"]
DPOLE = [t for t in sorted(qb.KIND) if qb.KIND[t] == "dpole"]
_ORACLE = {}


def _oracle(tag, order=None):
    """The oracle's arrays, computed once per set and never modified (the tests work on copies)."""
    if (tag, order) not in _ORACLE:
        o = qb.oracle_arrays(tag, order)
        for a in o:
            a.setflags(write=False)
        _ORACLE[tag, order] = o
    return _ORACLE[tag, order]


def _copies(tag):
    return [a.copy() for a in _oracle(tag)]


def _sub_tol_passes(tag, field, got, want):
    """The bound tests/test_gpu_parity._check_supergrid holds the pass's cap metrics to, against the oracle."""
    ta, tr = SUB_TOL[qb.KIND[tag]][field]
    tr = dp_quad_rel_tol(got.shape[1] - (field == "dy")) if tr is None else tr
    return bool(np.all(np.abs(got - want) <= ta + tr * np.abs(want)))


def _fails_at(tag, arrays, field, cells):
    """check() must raise, and every element it names must be of `field` and among `cells` (a set of (j, i), or a predicate)."""
    with pytest.raises(qb.QuadBoundError) as ex:
        qb.check(*arrays, tag, name="planted")
    worst = ex.value.worst
    assert worst and all(w[1] == field and (cells(w[2], w[3]) if callable(cells) else (w[2], w[3]) in cells) for w in worst), worst
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(qb.FILES))
def test_fixture_layout(tag):
    path = os.path.join(qb.GOLD, qb.FILES[tag])
    assert os.path.getsize(path) <= qb.MAX_FILE_BYTES
    z = np.load(path)
    assert int(qb.scalar(z["dps"])) == 50
    small = np.load(os.path.join(qb.GOLD, "truth_small_caps.npz"))
    assert np.array_equal(z[tag + "params"], small[tag + "params"])              # the caps of truth_small_caps.npz, the same bits
    s = qb.load(tag)
    kind, Ni = s["kind"], int(s["params"][0])
    o = _oracle(tag)
    n_cell = s["shapes"]["area"][0]
    assert s["order"] == qb.MAIN_ORDER[kind] and list(s["rows"]) == list(range(n_cell)) and list(s["dx_rows"]) == list(range(n_cell + 1))
    for k, f in enumerate(qb.FIELDS):
        assert o[k].shape == s["shapes"][f]
        for T in s["truths"]:
            assert s["truths"][T][f].shape == o[k].shape + (2,)
        cl = qb.classes(kind, s["shapes"][f], Ni, n_cell)
        assert sum(m.astype(int) for m in cl.values()).min() == 1 and sum(m.astype(int) for m in cl.values()).max() == 1     # a partition
        fm = qb.fold(s["truths"][sorted(s["truths"])[0]][f][..., 0])
        for nm, m in cl.items():
            assert s["census"][f, nm] == int((m & ~fm).sum()) > 0, (f, nm)          # every class is non-empty
        assert s["census"][f, "fold"] == int(fm.sum())
        assert sum(s["census"][f, nm] for nm in list(cl) + ["fold"]) == o[k].size
        if kind == "bipolar":
            q = Ni // 4
            assert np.argwhere(cl["pole"]).tolist() == [[n_cell - 1, c] for c in (q - 1, q, 3 * q - 1, 3 * q)]
            # what vanishes on the fold lines: dy at columns 0, Ni/2 and Ni, every row; nothing of dx or area
            assert np.argwhere(fm).tolist() == ([[j, c] for j in range(n_cell) for c in (0, Ni // 2, Ni)] if f == "dy" else [])
        else:
            assert not fm.any()
    if kind == "bipolar":
        jg = int(qb.scalar(z[tag + "guard_row"]))
        assert jg == qb.guard_row(int(s["params"][1]), float(s["params"][2])) and 1 < jg < n_cell        # the guard and its fix-up are exercised
        assert (tag, jg) in (("sbp180_", 26), ("sbp360_", 54))


@pytest.mark.parametrize("tag,order", SETS)
def test_unit_of_the_stored_integers(tag, order):
    """truth = k 2^-bits: the unit is at most 1e-3 of the smallest bound it feeds, and no integer is near overflow."""
    s = qb.load(tag, order)
    z = np.load(os.path.join(qb.GOLD, qb.FILES[tag]))
    for T in s["truths"]:
        for f in qb.FIELDS:
            unit = 2.0 ** -s["bits"][f]
            assert unit <= 1e-3 * qb.smallest_bound(s, T, f), (tag, order, T, f, unit, qb.smallest_bound(s, T, f))
            k = z[s["prefix"] + (T + "_" if T else "") + f]
            assert k.dtype == np.int64 and np.abs(k).max() < 2 ** 62
    if order is not None:                                                        # the reduced sets: the rows the issue names
        n_cell = s["shapes"]["area"][0]
        want = [0, n_cell // 2] + (list(range(qb.guard_row(int(s["params"][1]), float(s["params"][2])) - 1, n_cell)) if s["kind"] == "bipolar" else [n_cell - 1])
        assert list(s["rows"]) == want and list(s["dx_rows"]) == want + [n_cell]


# ---------------------------------------------------------------------------------------------------------------
# no false alarm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,order", SETS)
def test_oracle_reproduces_eref_and_passes(tag, order):
    rep = qb.check(*_oracle(tag, order), tag, order=order, name="oracle")
    s = qb.load(tag, order)
    assert len(rep) == sum(1 for v in s["census"].values() if v) * len(s["truths"])
    for key, r in rep.items():
        assert r["n"] > 0 and r["vs_truth"] <= 2.0 * r["oracle_vs_truth"] + 1e-16, (key, r)
        assert r["vs_truth"] >= 0.5 * r["oracle_vs_truth"], (key, r)             # ... and the fixture's figure is no looser than the oracle is


def test_a_nan_fails():
    dx, dy, area = _copies("sbp180_")
    area[3, 100] = np.nan
    _fails_at("sbp180_", (dx, dy, area), "area", {(3, 100)})


def test_image_lines_are_reported():
    s = qb.load("sbp180_")
    image = {f: np.zeros(s["shapes"][f], bool) for f in qb.FIELDS}
    for f in qb.FIELDS:
        image[f][:, 100] = True
    rep = qb.check(*_oracle("sbp180_"), "sbp180_", image=image)
    assert rep["area/regular@image"]["n"] == 30 and rep["area/regular@image"]["bound"] == rep["area/regular"]["bound"]
    assert rep["dx/regular@image"]["n"] == 31 and "dx/pole@image" not in rep


# ---------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", BIPOLAR)
def test_planted_defects_bipolar(tag):
    s = qb.load(tag)
    Ni, Nj = int(s["params"][0]), int(s["params"][1])
    jg = qb.guard_row(Nj, float(s["params"][2]))
    reg = qb.classes("bipolar", s["shapes"]["area"], Ni, Nj)["regular"]
    c_img = Ni // 4 + Ni // 9                                # a mirror-image column of the rows below the guard (test_bipolar_quadrature_vs_truth)
    assert reg[5, Ni // 9] and reg[:, c_img].all() and reg[jg, Ni // 8] and reg[jg, Ni // 8 + 1]
    # one regular cell's area, 1e-12 relative
    dx, dy, area = _copies(tag)
    area[5, Ni // 9] *= 1.0 + 1e-12
    _fails_at(tag, (dx, dy, area), "area", {(5, Ni // 9)})
    # one image column's dx, 1e-12 relative
    dx, dy, area = _copies(tag)
    dx[:, c_img] *= 1.0 + 1e-12
    _fails_at(tag, (dx, dy, area), "dx", lambda j, i: i == c_img)
    # the top edge row of dx, shifted by one column
    dx, dy, area = _copies(tag)
    dx[Nj] = np.roll(dx[Nj], 1)
    _fails_at(tag, (dx, dy, area), "dx", lambda j, i: j == Nj)
    # the last column of dy: on this cap it is a fold line (the truth is 0 to 1e-11 m), so a zero there is no defect and passes; the
    # column before it in its place -- a strip that stops one column short -- is one
    dx, dy, area = _copies(tag)
    dy[:, Ni] = 0.0
    qb.check(dx, dy, area, tag)
    dy[:, Ni] = dy[:, Ni - 1]
    _fails_at(tag, (dx, dy, area), "dy", lambda j, i: i == Ni)
    # one cell of the first guarded row with its neighbour's value
    for k, f in enumerate(qb.FIELDS):
        arrays = _copies(tag)
        arrays[k][jg, Ni // 8] = arrays[k][jg, Ni // 8 + 1]
        _fails_at(tag, arrays, f, {(jg, Ni // 8)})


def test_planted_defect_under_sub_tol_bipolar():
    """SUB_TOL holds the bipolar cap's area to 1e-6 m^2 + 2e-13 relative against the oracle: a regular cell of the SMALLER cap scaled by
    (1 + 1e-13) passes it, and fails here (bound 1.5 * 2e-14 of the truth)."""
    tag = "sbp180_"
    dx, dy, area = _copies(tag)
    area[5, 20] *= 1.0 + 1e-13
    assert area[5, 20] != _oracle(tag)[2][5, 20]
    assert _sub_tol_passes(tag, "area", area, _oracle(tag)[2])
    _fails_at(tag, (dx, dy, area), "area", {(5, 20)})
    # (the 1e-12 scalings, the shifted row and the neighbour's value of test_planted_defects_bipolar do NOT pass SUB_TOL on this cap)
    area[5, 20] = _oracle(tag)[2][5, 20] * (1.0 + 1e-12)
    assert not _sub_tol_passes(tag, "area", area, _oracle(tag)[2])


@pytest.mark.parametrize("tag", DPOLE)
def test_planted_defects_displaced_pole(tag):
    s = qb.load(tag)
    Ni, n_cell = int(s["params"][0]), s["shapes"]["area"][0]
    tol = dp_quad_rel_tol(Ni)
    assert tol == 7.2e-10
    # one cell at (1 + 10 x the reference's own distance from the truth): fails here, every field
    for k, f in enumerate(qb.FIELDS):
        eref = max(s["eref"][T, f, "all", "rel"] for T in "AB")
        arrays = _copies(tag)
        arrays[k][n_cell // 2, 77] *= 1.0 + 10.0 * eref
        _fails_at(tag, arrays, f, {(n_cell // 2, 77)})
        # ... and passes SUB_TOL wherever 10 eref < 2e-12 Ni (all but dx of the --lat_dp cap: 10 x 7.3e-11)
        assert _sub_tol_passes(tag, f, arrays[k], _oracle(tag)[k]) == (10.0 * eref < tol), (f, eref)
        assert 10.0 * eref < tol or (tag, f) == ("sdp_latdp_", "dx")
    # the last column of dy, zeroed
    dx, dy, area = _copies(tag)
    dy[:, Ni] = 0.0
    _fails_at(tag, (dx, dy, area), "dy", lambda j, i: i == Ni)
    # the defects of test_planted_defects_bipolar that SUB_TOL cannot see on this cap: (1 + 1e-12) on a cell's area and on a column of dx,
    # and the top edge row of dx (the joint with the Southern Ocean grid: a circle of latitude, dx constant to the reference's noise)
    # shifted by one column.  They are below the reference's own noise here (5e-11), so the truth cannot see them either: what this
    # file adds on the displaced-pole caps is the step from 7.2e-10 to 1.5 eref, about 1e-10
    dx, dy, area = _copies(tag)
    area[3, 200] *= 1.0 + 1e-12
    dx[:, 200] *= 1.0 + 1e-12
    dx[n_cell] = np.roll(dx[n_cell], 1)
    assert not np.array_equal(dx[n_cell], _oracle(tag)[0][n_cell])
    assert _sub_tol_passes(tag, "area", area, _oracle(tag)[2]) and _sub_tol_passes(tag, "dx", dx, _oracle(tag)[0])
    # a cell with its neighbour's value is gross on this cap (neighbours differ by 1e-3 and more below the joint row)
    arrays = _copies(tag)
    arrays[2][3, 200] = arrays[2][3, 201]
    _fails_at(tag, arrays, "area", {(3, 200)})


# ---------------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------------
def test_truth_script_quick_run(tmp_path):
    """scripts/truth_table.py --groups small_metrics --quick (two rows of sbp180_ at order 5, one at order 2; one row of sdp_rdp_ at orders 4
    and 2) under a time cap, into a temporary directory: the integers it computes are those of the committed fixtures."""
    before = {n: os.path.getmtime(os.path.join(qb.GOLD, n)) for n in os.listdir(qb.GOLD)}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "truth_table.py"), "--groups", "small_metrics", "--quick", "--procs", "4",
                        "--metrics-dir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:]
    assert before == {n: os.path.getmtime(os.path.join(qb.GOLD, n)) for n in os.listdir(qb.GOLD)}          # no fixture was touched
    n_cmp = 0
    for tag in sorted(qb.REDUCED_ORDERS):
        quick = np.load(os.path.join(str(tmp_path), qb.FILES[tag].replace(".npz", "_quick.npz")))
        full = np.load(os.path.join(qb.GOLD, qb.FILES[tag]))
        assert np.array_equal(quick[tag + "params"], full[tag + "params"])
        for p in (tag, "%so%d_" % (tag, qb.REDUCED_ORDERS[tag][0])):
            for T in (("",) if qb.KIND[tag] == "bipolar" else ("A_", "B_")):
                for f in qb.FIELDS:
                    rows_q = quick[p + ("dx_rows" if f == "dx" else "rows")].tolist()
                    rows_f = full[p + ("dx_rows" if f == "dx" else "rows")].tolist()
                    tq = qb.pairs(quick[p + T + f], int(qb.scalar(quick[p + f + "_bits"])))
                    tf = qb.pairs(full[p + T + f], int(qb.scalar(full[p + f + "_bits"])))[[rows_f.index(j) for j in rows_q]]
                    unit = 2.0 ** -min(int(qb.scalar(quick[p + f + "_bits"])), int(qb.scalar(full[p + f + "_bits"])))
                    assert np.abs((tq[..., 0] - tf[..., 0]) + (tq[..., 1] - tf[..., 1])).max() <= unit, (p, T, f)
                    n_cmp += tq[..., 0].size
    assert n_cmp > 3000

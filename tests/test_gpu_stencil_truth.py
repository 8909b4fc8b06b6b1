"""The generic stencil kernels (csrc/ogg_midas.hip: midas_tile_kernel at TR = 4, 6, 8, 12 and the streaming midas_angle_kernel, behind
ogg_grid_metrics_midas, ogg_grid_metrics_midas_dev and ogg_angle_x) against the 50-digit truth of OGG:687-729 at EVERY element of four
hand-made meshes -- a bipolar cap with its fold row and pole points, a displaced-pole cap with its pole row, a mesh moved by whole turns, a
mesh of exact poles, signed zeros and exact zeros of dx and dy -- and nine windows of them (tests/golden/truth_stencil_*.npz, scripts/truth_table.py
--groups stencil), under the conditioned bound of tests/stencil_bounds.py (derivation there; planted defects: tests/test_stencil_bounds_cpu.py).

  * the truth check, both area forms and the angle; then every planned kernel (tests/stencil_plans.py: every tile setting at one workgroup per
    column tile -- TR 4, 6, 8, 12, rows per block 1 .. 12 -- and the streaming kernel at three heights), each asserted through
    ogg_grid_metrics_midas_plan before it is launched, must give the bits of the default;
  * an angle-only ogg_grid_metrics_midas_dev call (dx, dy, area NULL) and ogg_angle_x give the angle of the metrics call, bit for bit;
  * bands on device pointers, cut at tile-row edges and one row either side, with n_pt_rows < nrows_xy and a last band that owns only the last
    point row (n_cell_rows = 0), assemble the whole mesh bit for bit;
  * a NaN, +inf or -inf in x or y at an interior point, at a tile-edge column and in the last row: outputs outside the entry's stencil keep
    their bits; inside it an output the oracle does not change keeps its bits too, the NaN pattern is the oracle's, and the numbers numpy
    gives there (angles of +-0, +-90, +-180 degrees: the library's constants of atan2 through a division that is IEEE's) are numpy's bits.

The measured figures go to the file OGG_STENCIL_TRUTH_REPORT names, if set (profiles/stencil_truth.json is one such run).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import stencil_bounds as sb
import stencil_meshes as sm
import stencil_plans as sp

pytestmark = pytest.mark.gpu

REPORT = {}
KNOBS = ("OGG_MIDAS_TILE_ROWS", "OGG_MIDAS_TARGET_WG")


@pytest.fixture(scope="module")
def ogg(hip):
    import ocean_model_grid_generator_amd.ocean_grid_generator as m
    return m


def _record(name, path, rep):
    """One block of figures per fixture, REPORT[name]["functions"]; a further path whose figures are the same field by field (it gave the same
    bits) is only named, under "paths_with_the_same_figures"; one whose figures differ gets a block of its own."""
    block = {f: {k: r[k] for k in ("worst_over_bound", "worst_over_s", "median_over_s", "R", "n", "n_zero", "n_singular") if k in r} for f, r in rep.items()}
    fx = REPORT.setdefault(name, {})
    first = fx.get("functions")
    if path != "functions" and first and block and all(first.get(f) == b for f, b in block.items()):
        fx["paths_with_the_same_figures"] = sorted(set(fx.get("paths_with_the_same_figures", [])) | {path})
    else:
        fx[path] = block
    out = os.environ.get("OGG_STENCIL_TRUTH_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _fields(ogg, x, y):
    dx, dy, area = ogg.generate_grid_metrics_MIDAS(x, y)
    return {"dx": dx, "dy": dy, "area": area, "area_nofix": ogg.generate_grid_metrics_MIDAS(x, y, latlon_areafix=False)[2], "angle": ogg.angle_x(x, y)}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _default(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _set_plan(hip, monkeypatch, ni1, nj1, env, want_metrics=None, want_angle=None):
    """Set the knobs and assert, through the library's own query, what the metrics call and the angle call of an (nj1, ni1) mesh will launch."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n_m = max(nj1, 2)                                        # a single row of points runs twice for its dx
    got_m, got_a = sp.planned(hip, ni1, n_m, True), sp.planned(hip, ni1, nj1, False)
    tile, target = int(env.get("OGG_MIDAS_TILE_ROWS", 6)), int(env.get("OGG_MIDAS_TARGET_WG", 2048))
    assert got_m == sp.expected(ni1, n_m, True, tile, target) and got_a == sp.expected(ni1, nj1, False, tile, target), (env, got_m, got_a)
    return got_m, got_a


# ---------------------------------------------------------------------------------------------------------------
# the truth, and every planned kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sb.names())
def test_stencil_vs_truth_every_kernel(hip, ogg, name, monkeypatch):
    fx = sb.load(name)
    x, y = np.array(fx["x"]), np.array(fx["y"])
    nj1, ni1 = x.shape
    _default(monkeypatch)
    assert _set_plan(hip, monkeypatch, ni1, nj1, {}) == ((4, min(2, max(nj1, 2))), (4, min(2, nj1)))      # the default: two rows per tile at these sizes
    base = _fields(ogg, x, y)
    rep = {}
    try:
        rep = sb.check(name, base, tag="HIP")
    finally:
        for f, r in sorted(rep.items()):
            print("%-8s %-10s HIP |error| / s: max %.2f median %.2f (oracle %.2f); worst distance / bound %.2f; %d held, %d exact zeros, %d left out" % (
                name, f, r["worst_over_s"], r["median_over_s"], r["R"], r["worst_over_bound"], r["n"], r["n_zero"], r["n_singular"]))
        _record(name, "functions", rep)
    seen = set()
    for label, env, _ in sp.variants(ni1, max(nj1, 2), True):
        seen.update(_set_plan(hip, monkeypatch, ni1, nj1, env))
        got = _fields(ogg, x, y)
        for f in sb.FIELDS:
            assert _same_bits(got[f], base[f]), (name, label, f, float(np.nanmax(np.abs(got[f] - base[f]))))
    REPORT[name]["kernels_bit_identical"] = sorted("%s/%d" % ("stream" if tr == 0 else "tile%d" % tr, rpb) for tr, rpb in seen)
    if nj1 >= 9:
        assert {tr for tr, _ in seen} == {0, 4, 6, 8, 12} and {rpb for tr, rpb in seen if tr} >= set(range(2, 10))
    _record(name, "functions", rep)


# ---------------------------------------------------------------------------------------------------------------
# device pointers: angle-only calls and bands
# ---------------------------------------------------------------------------------------------------------------
def _dev(hip, torch, x, y, a, b, n_cell, out, last_band_null=False):
    """ogg_grid_metrics_midas_dev on the point rows a .. b-1 of the device mesh (x, y), the rows from a on as its xy rows; writes into the rows
    of the assembled device arrays out = {dx, dy, area, angle} (None: NULL)."""
    nrows, ni1 = x.shape
    ni = ni1 - 1

    def p(t, row, width):
        if t is None:
            return None
        assert row * width <= t.numel()
        return t.data_ptr() + 8 * row * width
    hip.call("ogg_grid_metrics_midas_dev", nrows - a, ni1, p(x, a, ni1), p(y, a, ni1), b - a, n_cell, sb.RE, int(out.get("areafix", 1)),
             p(out.get("dx"), a, ni), None if n_cell == 0 else p(out.get("dy"), a, ni1), None if n_cell == 0 else p(out.get("area"), a, ni),
             p(out.get("angle"), a, ni1), None)
    torch.cuda.synchronize()


def _new(torch, shapes, areafix=1):
    out = {f: torch.full(shapes[f], -7.0, dtype=torch.float64, device="cuda:0") for f in ("dx", "dy", "area", "angle")}
    out["areafix"] = areafix
    return out


def _host(out):
    return {f: out[f].cpu().numpy() for f in ("dx", "dy", "area", "angle")}


ANGLE_ENVS = ({}, {"OGG_MIDAS_TILE_ROWS": "12", "OGG_MIDAS_TARGET_WG": "1"}, {"OGG_MIDAS_TILE_ROWS": "0"}, {"OGG_MIDAS_TILE_ROWS": "0", "OGG_MIDAS_TARGET_WG": "1"})


@pytest.mark.parametrize("name", list(sm.MESHES) + ["w3x255", "w3x258"])
def test_angle_only_calls_give_the_angle_of_the_metrics_call(hip, ogg, name, monkeypatch):
    import torch
    fx = sb.load(name)
    nj1, ni1 = fx["x"].shape
    x, y = (torch.from_numpy(np.array(fx[k])).to("cuda:0") for k in ("x", "y"))
    shp = sb.shapes(nj1, ni1)
    for env in ANGLE_ENVS:
        _default(monkeypatch)
        _set_plan(hip, monkeypatch, ni1, nj1, env)
        whole = _new(torch, shp)
        _dev(hip, torch, x, y, 0, nj1, nj1 - 1, whole)
        want = whole["angle"].cpu().numpy()
        only = {"angle": torch.full(shp["angle"], -7.0, dtype=torch.float64, device="cuda:0")}
        _dev(hip, torch, x, y, 0, nj1, 0, only)
        assert _same_bits(only["angle"].cpu().numpy(), want), (name, env)
        assert _same_bits(ogg.angle_x(np.array(fx["x"]), np.array(fx["y"])), want), (name, env)
        if not env:
            rep = sb.check(name, {"angle": want, "dx": whole["dx"].cpu().numpy(), "dy": whole["dy"].cpu().numpy(), "area": whole["area"].cpu().numpy()}, tag="dev")
            _record(name, "dev_one_call", rep)


@pytest.mark.parametrize("areafix", [1, 0])
@pytest.mark.parametrize("name", sm.MESHES)
def test_bands_assemble_the_whole_mesh(hip, name, areafix, monkeypatch):
    """Bands cut at a tile-row edge and one row either side; every band sees the rows above it (n_pt_rows < nrows_xy); the last band owns the
    last point row alone (n_cell_rows = 0)."""
    import torch
    fx = sb.load(name)
    nj1, ni1 = fx["x"].shape
    x, y = (torch.from_numpy(np.array(fx[k])).to("cuda:0") for k in ("x", "y"))
    shp = sb.shapes(nj1, ni1)
    for env, edge, want_plan in (({}, 2, (4, 2)), ({}, 4, (4, 2)), ({"OGG_MIDAS_TILE_ROWS": "6", "OGG_MIDAS_TARGET_WG": "1"}, 6, (6, 6)),
                                 ({"OGG_MIDAS_TILE_ROWS": "0", "OGG_MIDAS_TARGET_WG": "6"}, 4, (0, 4))):
        _default(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr, rpb = sp.planned(hip, ni1, nj1, True)
        assert (tr, rpb) == sp.expected(ni1, nj1, True, int(env.get("OGG_MIDAS_TILE_ROWS", 6)), int(env.get("OGG_MIDAS_TARGET_WG", 2048))) == want_plan, (env, tr, rpb)
        assert edge % rpb == 0                                # `edge` is a tile-row edge of the whole-mesh call
        whole = _new(torch, shp, areafix)
        _dev(hip, torch, x, y, 0, nj1, nj1 - 1, whole)
        want = _host(whole)
        assert not any((want[f] == -7.0).any() for f in want)
        for cut in (edge - 1, edge, edge + 1):
            parts = _new(torch, shp, areafix)
            _dev(hip, torch, x, y, 0, cut, cut, parts)
            _dev(hip, torch, x, y, cut, nj1 - 1, nj1 - 1 - cut, parts)
            _dev(hip, torch, x, y, nj1 - 1, nj1, 0, parts)
            got = _host(parts)
            for f in want:
                assert _same_bits(got[f], want[f]), (name, env, cut, f)
    rep = sb.check(name, {"dx": want["dx"], "dy": want["dy"], "area" if areafix else "area_nofix": want["area"], "angle": want["angle"]}, tag="bands")
    _record(name, "dev_bands_areafix%d" % areafix, rep)


# ---------------------------------------------------------------------------------------------------------------
# non-finite entries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"OGG_MIDAS_TILE_ROWS": "8", "OGG_MIDAS_TARGET_WG": "1"}, {"OGG_MIDAS_TILE_ROWS": "0"}], ids=["default", "tile8", "stream"])
def test_non_finite_entries(hip, ogg, env, monkeypatch):
    fx = sb.load("turns")
    nj1, ni1 = fx["x"].shape
    _default(monkeypatch)
    _set_plan(hip, monkeypatch, ni1, nj1, env)
    base = _fields(ogg, np.array(fx["x"]), np.array(fx["y"]))
    want_base = sb.oracle(np.array(fx["x"]), np.array(fx["y"]))
    n_num = 0
    for (j, i) in ((3, 100), (4, 255), (4, 256), (nj1 - 1, 300)):
        # the outputs that read the point (j, i): its two dx, two dy, four areas and three angles
        sten = {f: np.zeros(base[f].shape, bool) for f in sb.FIELDS}
        sten["dx"][j, i - 1:i + 1] = True
        sten["dy"][max(j - 1, 0):j + 1, i] = True
        for f in ("area", "area_nofix"):
            sten[f][max(j - 1, 0):j + 1, i - 1:i + 1] = True
        sten["angle"][j, i - 1:i + 2] = True
        for which in "xy":
            for bad in (np.nan, np.inf, -np.inf):
                x, y = np.array(fx["x"]), np.array(fx["y"])
                (x if which == "x" else y)[j, i] = bad
                got = _fields(ogg, x, y)
                with np.errstate(all="ignore"):
                    want = sb.oracle(x, y)
                for f in sb.FIELDS:
                    case = (which, bad, j, i, f)
                    out = ~sten[f]
                    assert np.array_equal(got[f].view(np.int64)[out], base[f].view(np.int64)[out]), case
                    g, w, b, wb = got[f][sten[f]], want[f][sten[f]], base[f][sten[f]], want_base[f][sten[f]]
                    kept = w.view(np.int64) == wb.view(np.int64)          # the oracle does not read the entry here (the angle at (j, i) for an x)
                    assert np.array_equal(g.view(np.int64)[kept], b.view(np.int64)[kept]), (case, g, b)
                    assert np.array_equal(np.isnan(g), np.isnan(w)), (case, g, w)
                    num = ~kept & ~np.isnan(w)                             # numpy gives a number: its bits (a NaN's sign and payload are nobody's promise)
                    assert np.array_equal(g.view(np.int64)[num], w.view(np.int64)[num]), (case, g, w)
                    n_num += int(num.sum())
    assert n_num > 0                                         # numpy did give numbers somewhere (atan2 of an infinity)

"""GPU tests of the grid analyses on the hand-made meshes of tests/small_meshes.py, which the generator never makes: a zoo of cells of
every class (pole corners in every arrangement, pole-enclosing, inverted, degenerate, NaN corners, longitudes turns away, one cell
with 176 list entries), four cuts of a tripolar grid that are the four (periodic, fold) combinations, and regional grids of one to
129 cells.  The exchange grid, the remap and its fill, the regrid to lat-lon, the bilinear interpolation and the runoff mapping are
each held to their numpy definition under tests/*_definition.py by the rules of their own GPU tests (bit for bit, or 1e-12 for the
exchange areas), and the exchange areas also to the 50-digit truth of tests/golden/xgrid_truth.npz.
tests/test_small_meshes_cpu.py shows on the CPU that these inputs tell the topologies and the cell classes apart.

Measured on an MI355X: the 100 tests of this file take 8 s; the zoo's areas against the truth are in the comment of
test_zoo_areas_against_the_truth."""
import numpy as np
import pytest

import bilinear_definition as BD
import latlon_regrid_definition as GD
import remap_definition as RD
import runoff_definition as ROD
import small_meshes as sm
import xgrid_definition as xd

pytestmark = pytest.mark.gpu
RE = sm.RE
ATMS = ("regular", "gaussian", "one_column", "one_row")
_CACHE = {}


@pytest.fixture(scope="module")
def api(hip):
    from ocean_model_grid_generator_amd import bilinear as B
    from ocean_model_grid_generator_amd import exchange_grid as X
    from ocean_model_grid_generator_amd import latlon_regrid as G
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO

    class Api:
        pass
    a = Api()
    a.B, a.X, a.G, a.R, a.RO = B, X, G, R, RO
    return a


def grid(name):
    """dict(x, y, area, angle_dx, topology, mask) of the zoo, a cut or a shape (built once)"""
    if name not in _CACHE:
        if name == "zoo":
            x, y, where = sm.cell_zoo()
            g = dict(x=x, y=y, where=where, topology=(False, False), mask=sm.zoo_mask((x.shape[1] - 1) // 2),
                     area=np.ones((x.shape[0] - 1, x.shape[1] - 1)), angle_dx=np.zeros_like(x))
        elif name in sm.CUTS:
            g = sm.topology_cuts()[name]
        else:
            g = sm.shape_grid(name)
            g["topology"] = sm.SHAPE_TOPOLOGY.get(name, (False, False))
        if "mask" not in g:
            g["mask"] = sm.wet_mask((g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2)
        _CACHE[name] = g
    return _CACHE[name]


def definition_xgrid(name, kind, masked, threshold=0.0):
    key = ("xd", name, kind, masked, threshold)
    if key not in _CACHE:
        g = grid(name)
        lon, lat = sm.zoo_atmosphere(kind)
        _CACHE[key] = xd.exchange_grid(g["x"], g["y"], lon, lat, mask=g["mask"] if masked else None, Re=RE, threshold=threshold)
    return _CACHE[key]


GRIDS = ["zoo"] + list(sm.CUTS) + list(sm.SHAPES)


# ---- exchange grid ---------------------------------------------------------------------------------------------
def compare_xgrid(res, want, a_def, counts):
    """test_gpu_xgrid.compare over all rows, with the whole counts dict and the zeros of A_poly bit for bit: pairs above 1e-10 of
    min(A_poly, A_atm) identical and in the same order, |dA| / A_poly <= 1e-12."""
    assert res["counts"] == counts
    ap = res["a_poly"]
    np.testing.assert_array_equal(np.isnan(ap), np.isnan(a_def))
    zero = a_def == 0.0
    assert np.all(ap[zero] == 0.0) and np.array_equal(np.signbit(ap[zero]), np.signbit(a_def[zero]))
    ok = np.isfinite(a_def) & ~zero
    d_poly = float(np.max(np.abs(ap[ok] / a_def[ok] - 1), initial=0.0))
    assert d_poly <= 1e-12, d_poly
    np.testing.assert_array_equal(ap > 0, a_def > 0)
    w_atm, w_ocn, w_area = xd.as_arrays(want)
    g_atm, g_ocn, g_area = res["atm"], res["ocn"], res["area"]
    a_atm = res["a_atm"]

    def significant(atm, ocn, area):
        return area > 1e-10 * np.minimum(ap[ocn[:, 1], ocn[:, 0]], a_atm[atm[:, 1], atm[:, 0]])

    gs, ws = significant(g_atm, g_ocn, g_area), significant(w_atm, w_ocn, w_area)
    np.testing.assert_array_equal(g_atm[gs], w_atm[ws])
    np.testing.assert_array_equal(g_ocn[gs], w_ocn[ws])
    d = np.abs(g_area[gs] - w_area[ws]) / ap[g_ocn[gs][:, 1], g_ocn[gs][:, 0]]
    assert float(d.max(initial=0.0)) <= 1e-12, d.max()
    return d_poly, float(d.max(initial=0.0)), int(gs.sum())


@pytest.mark.parametrize("kind", ATMS)
@pytest.mark.parametrize("name", GRIDS)
def test_exchange_grid_equals_definition(api, name, kind):
    """No specimen needed a wider bound than the 1e-12 of test_gpu_xgrid.py."""
    g = grid(name)
    lon, lat = sm.zoo_atmosphere(kind)
    # the mask as well: on the zoo and the shapes with every atmosphere, on the cuts (0.7 s of definition each) with the regular one
    for masked in ((False, True) if name not in sm.CUTS or kind == "regular" else (False,)):
        want, a_def, counts = definition_xgrid(name, kind, masked)
        res = api.X.exchange_grid(g["x"], g["y"], lon, lat, mask=g["mask"] if masked else None, threshold=0.0, Re=RE)
        compare_xgrid(res, want, a_def, counts)
        if masked:
            assert res["counts"]["masked"] == int((g["mask"] == 0).sum())
    if name == "zoo":
        c = res["counts"]
        assert c["pole_enclosing"] > 0 and c["inverted"] > 0 and c["degenerate"] > 0 and c["pole_cells"] > 0, c


def test_zoo_device_entry_and_classes(api):
    """the device-pointer entries (count and write steps on device tensors) give the host entry's bits, and the named specimens have
    the entry counts of small_meshes.ZOO_STATUS on the device"""
    import torch
    g = grid("zoo")
    lon, lat = sm.zoo_atmosphere("regular")
    host = api.X.exchange_grid(g["x"], g["y"], lon, lat, threshold=0.0, Re=RE)
    dev = torch.device("cuda:0")
    xt, yt = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["y"]).to(dev)
    atm, ocn, area, _ = api.X.whole_grid_lists_dev(xt, yt, lon, lat, None, RE, 0.0, torch.cuda.current_stream(dev).cuda_stream, dev)
    assert atm.cpu().numpy().tobytes() == host["atm"].tobytes() and ocn.cpu().numpy().tobytes() == host["ocn"].tobytes()
    assert area.cpu().numpy().tobytes() == host["area"].tobytes()
    n = np.bincount(host["ocn"][:, 0], minlength=host["a_poly"].shape[1])
    for spec, col in g["where"].items():
        assert n[col] == sm.ZOO_STATUS[spec][2], spec
    c = host["counts"]
    assert (c["pole_enclosing"], c["degenerate"]) == (1, 3) and c["inverted"] >= 6
    assert n[g["where"]["long"]] > 128 and n[g["where"]["long"]] % 64 != 0


def test_zoo_areas_against_the_truth(api, capsys):
    """The device's A_poly and piece areas may be no farther from the 50-digit truth than 1.5 times the definition's own measured
    error over the same cells and pieces (the rule of tests/test_gpu_truth.py).  Relative to A_poly, definition against the truth:
    A_poly 1.266e-13, pieces 1.762e-13 (eref_poly, eref_piece of the fixture).  Both are the bow-tie's, whose two lobes cancel to a
    hundredth of their size, so the bound is also held over every cell and piece but the bow-tie's (eref_poly_rest 1.101e-14,
    eref_piece_rest 6.404e-15), where it bites for the ordinary and the polar specimens.  Measured on an MI355X, device against the
    truth: A_poly 1.266e-13, pieces 1.762e-13 over all 1146 pieces -- the definition's figures to the digits printed."""
    t = np.load(sm.TRUTH)
    g = grid("zoo")
    lon, lat = sm.zoo_atmosphere("regular")
    res = api.X.exchange_grid(g["x"], g["y"], lon, lat, threshold=0.0, Re=RE)
    ap = res["a_poly"][0]
    tp, ta, pairs = t["a_poly"], t["area"], t["pairs"]
    where = {tuple(k): i for i, k in enumerate(np.concatenate([res["atm"], res["ocn"]], axis=1).tolist())}
    idx = np.array([where.get(tuple(k), -1) for k in pairs.tolist()])
    tiny = ta[:, 0] <= 1e-10 * np.minimum(ap[pairs[:, 2]], res["a_atm"][pairs[:, 1], pairs[:, 0]])   # may be missing from one list
    assert np.all((idx >= 0) | tiny)
    have = idx >= 0
    bow = g["where"]["bow_tie"]
    for tag, cells, pieces in (("", tp[:, 0] > 0, have), ("_rest", (tp[:, 0] > 0) & (t["cells"] != bow), have & (pairs[:, 2] != bow))):
        e_poly = float(np.max(np.abs((ap[t["cells"]][cells] - tp[cells, 0]) - tp[cells, 1]) / tp[cells, 0]))
        e_piece = float(np.max(np.abs((res["area"][idx[pieces]] - ta[pieces, 0]) - ta[pieces, 1]) / ap[pairs[pieces, 2]]))
        r_poly, r_piece = float(t["eref_poly" + tag]), float(t["eref_piece" + tag])
        with capsys.disabled():
            print("\nzoo against the truth%s, relative to A_poly: definition A_poly %.3e pieces %.3e; device A_poly %.3e pieces %.3e "
                  "(%d pieces)" % (" without the bow-tie" if tag else "", r_poly, r_piece, e_poly, e_piece, int(pieces.sum())))
        assert e_poly <= 1.5 * r_poly and e_piece <= 1.5 * r_piece, tag


def test_default_threshold_keeps_a_subsequence(api):
    """a regional grid whose columns miss the atmosphere's edges by 1e-7 degrees: slivers of 2.5e-8 of a cell, dropped by the default
    threshold; the kept list is the full list's subsequence above it (the rule of test_gpu_xgrid.py)"""
    g = sm.latlon_grid(3, 5, lon0=-32.0000001, lat0=-10.0, dlon=4.0, dlat=4.0)
    lon, lat = sm.zoo_atmosphere("regular")
    full = api.X.exchange_grid(g["x"], g["y"], lon, lat, threshold=0.0, Re=RE)
    kept = api.X.exchange_grid(g["x"], g["y"], lon, lat, Re=RE)
    ap = full["a_poly"]
    ratio = full["area"] / np.minimum(ap[full["ocn"][:, 1], full["ocn"][:, 0]], full["a_atm"][full["atm"][:, 1], full["atm"][:, 0]])
    assert (ratio <= 1e-6).sum() > 0 and (ratio > 1e-6).sum() > 0
    where = {tuple(k): i for i, k in enumerate(np.concatenate([full["atm"], full["ocn"]], axis=1).tolist())}
    idx = np.array([where[tuple(k)] for k in np.concatenate([kept["atm"], kept["ocn"]], axis=1).tolist()])
    assert np.all(np.diff(idx) > 0)
    assert full["area"][idx].tobytes() == kept["area"].tobytes()
    assert np.all(ratio[idx] > 1e-6 * (1 - 1e-9))
    assert set(np.nonzero(ratio > 1e-6 * (1 + 1e-9))[0]) <= set(idx.tolist())
    want, a_def, counts = xd.exchange_grid(g["x"], g["y"], lon, lat, Re=RE)
    compare_xgrid(kept, want, a_def, counts)


# ---- remap and fill --------------------------------------------------------------------------------------------
# (source shape, dtype, nrec, two fill values plus NaN, masked, fill_max): nrec * ncell is no multiple of 4 on the odd-sized grids.  The
# first case is the one tests/test_small_meshes_cpu.py shows to tell the topologies apart.
REMAP_CASES = [("nonuniform", np.float64, 3, False, False, None), ("regular", np.float32, 3, True, True, None),
               ("nonuniform", np.float32, 5, False, False, 2), ("regular", np.float64, 6, True, True, 1),
               ("3x2", np.float64, 1, False, False, None), ("7x1", np.float32, 5, False, True, 0), ("1x1", np.float64, 1, False, False, None)]


def remap_definition(api, g, src, mask, summary, fill_max):
    lists = api.X.exchange_grid(g["x"], g["y"], src.lon, src.lat, mask=mask, Re=RE)
    ny, nx = lists["a_poly"].shape
    v, fl = RD.remap(lists["atm"], lists["ocn"], lists["area"], src.records, ny, nx, fills=src.fill, mask=mask)
    v, fl, _ = RD.fill(v, fl, summary["periodic"], summary["fold"], fill_max)
    return v, fl, lists


@pytest.mark.parametrize("name", GRIDS)
def test_remap_and_fill_equal_definition(api, name):
    import torch
    g = grid(name)
    filled_somewhere = False
    for k, (kind, dtype, nrec, two, masked, fill_max) in enumerate(REMAP_CASES):
        f, lon, lat, fills = sm.source_for(g["x"], g["y"], kind, nrec=nrec, dtype=dtype, two_fills=two)
        src = api.R.Source(f, lon, lat, fill=fills)
        mask = g["mask"] if masked else None
        res = api.R.remap(g["x"], g["y"], src, mask=mask, fill_max=fill_max, Re=RE)
        s = res["summary"]
        assert (s["periodic"], s["fold"]) == g["topology"], (name, s)
        v, fl, lists = remap_definition(api, g, src, mask, s, fill_max)
        tag = (name, kind, dtype.__name__, nrec, fill_max)
        assert res["values"].tobytes() == v.reshape(res["values"].shape).tobytes(), tag
        np.testing.assert_array_equal(res["flags"], fl.reshape(res["flags"].shape), err_msg=str(tag))
        c = res["counts"]
        ncell = lists["a_poly"].size
        assert c["remapped"] + c["filled"] + c["unfilled"] + c["dry"] == nrec * ncell
        assert c["dry"] == (nrec * int((mask == 0).sum()) if masked else 0) and c["filled"] == int((fl == RD.FILLED).sum())
        if fill_max is not None:
            assert c["max_distance"] <= fill_max
        filled_somewhere |= c["filled"] > 0
        # cells without a list entry are never remapped: unfilled or filled, as the definition says
        n_entries = np.bincount(lists["ocn"][:, 1].astype(np.int64) * lists["a_poly"].shape[1] + lists["ocn"][:, 0], minlength=ncell)
        assert not np.any(res["flags"].reshape(nrec, -1)[:, n_entries == 0] == RD.REMAPPED)
        if name == "zoo" and kind == "regular":   # the long specimen is wet under the mask: 176 entries of this call's own list, the
            col = g["where"]["long"]              # cooperative walk's second and partial third round
            assert mask[0, col] == 1 and n_entries[col] == sm.ZOO_STATUS["long"][2] > 128 and n_entries[col] % 64 != 0
            assert np.all(res["flags"][:, 0, col] == RD.REMAPPED)
        if k < 2:   # the device-pointer path, which finds the topology from device tensors
            dev = torch.device("cuda:0")
            one = api.R.remap_dev(torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["y"]).to(dev), src, mask=mask, fill_max=fill_max, Re=RE)
            assert one["values"].tobytes() == res["values"].tobytes() and one["flags"].tobytes() == res["flags"].tobytes()
            assert one["summary"] == s
    if name in sm.CUTS or name == "zoo":
        assert filled_somewhere


# ---- regrid to lat-lon -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zoo", "fold_only"])
def test_regrid_to_latlon_equals_definition(api, name):
    g = grid(name)
    ny, nx = (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2
    rng = np.random.default_rng(7)
    for kind, dtype, nrec, missing, masked in (("regular", np.float32, 3, True, True), ("gaussian", np.float64, 2, False, False),
                                               ("one_row", np.float32, 1, True, False)):
        lon, lat = sm.zoo_atmosphere(kind)
        f = (10.0 + rng.random((nrec, ny, nx))).astype(dtype)
        fills = ()
        if missing:
            f[rng.random(f.shape) < 0.1] = np.nan
            f[rng.random(f.shape) < 0.1] = -999.0
            fills = (-999.0,)
        mask = g["mask"] if masked else None
        lists = api.X.exchange_grid(g["x"], g["y"], lon, lat, mask=mask, Re=RE)
        for normalize in ("area", "cell"):
            res = api.G.regrid_to_latlon(g["x"], g["y"], f, lon, lat, mask=mask, normalize=normalize, cover=True, fill_values=fills, Re=RE)
            want_v, want_c = GD.regrid(lists["atm"], lists["ocn"], lists["area"], f, lists["a_atm"], fills, normalize)
            frac, n = GD.static(lists["atm"], lists["area"], lists["a_atm"])
            tag = (name, kind, normalize)
            assert res["values"].tobytes() == want_v.reshape(res["values"].shape).tobytes(), tag
            assert res["cover"].tobytes() == want_c.reshape(res["cover"].shape).tobytes(), tag
            assert res["ocean_frac"].tobytes() == frac.tobytes() == lists["ocean_frac"].tobytes(), tag
            assert res["n_entries"].tobytes() == n.tobytes() and res["cell_area"].tobytes() == lists["a_atm"].tobytes(), tag
            c = res["counts"]
            assert c["entries"] == lists["area"].size and c["valid"] + c["empty"] == nrec * n.size
            assert c["cells"] == int((n > 0).sum()) and c["max_entries"] == int(n.max())
    # a constant field over the listed area: a power of two comes back exactly within 4 ulp, and S sums to c times the listed area
    lon, lat = sm.zoo_atmosphere("regular")
    lists = api.X.exchange_grid(g["x"], g["y"], lon, lat, Re=RE)
    const = api.G.regrid_to_latlon(g["x"], g["y"], np.full((ny, nx), 4.0), lon, lat, Re=RE)
    ok = const["n_entries"] > 0
    assert ok.sum() > 0 and np.all(np.abs(const["values"][ok] - 4.0) <= 4 * np.spacing(4.0)) and np.all(const["values"][~ok] == GD.FILL)
    cell = api.G.regrid_to_latlon(g["x"], g["y"], np.full((ny, nx), 3.75), lon, lat, normalize="cell", Re=RE)
    assert abs(np.sum(cell["values"] * cell["cell_area"]) / (3.75 * lists["area"].sum()) - 1) <= 1e-12


# ---- bilinear --------------------------------------------------------------------------------------------------
def same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def over_lds_source():
    if "over_lds" not in _CACHE:
        lon, lat = sm.source_edges("over_lds")
        f = sm.smooth_field(lon, lat, 2, np.float32)
        f[:, 150:260, 1000:3000] = np.nan
        _CACHE["over_lds"] = (f[:1], f[1:], lon, lat)
    return _CACHE["over_lds"]


def bilinear_sources(api, g, kind, dtype, nrec, two):
    """a scalar and the two components of a vector on one source grid, missing against the grid's left column and top row"""
    if kind == "over_lds":
        t, u, lon, lat = over_lds_source()
        fills, v = (), u + np.float32(1.0)
    else:
        t, lon, lat, fills = sm.source_for(g["x"], g["y"], kind, nrec=nrec, dtype=dtype, two_fills=two)
        miss = np.isnan(t)
        for fv in fills:
            miss |= t == dtype(fv)
        u = np.where(miss, t, t * dtype(0.5)).astype(dtype)
        v = np.where(miss, t, t + dtype(1.0)).astype(dtype)
        if t[0].size > 12:
            v[:, ::3, ::4] = np.nan   # a corner is valid only where both components are
    S = api.R.Source
    return (lon, lat), fills, S(t, lon, lat, fill=fills, name="t"), S(u, lon, lat, fill=fills, name="u"), S(v, lon, lat, fill=fills, name="v")


def check_bilinear(api, g, name, kind, dtype, nrec, two, fill_max=None):
    x, y, angle, mask = g["x"], g["y"], g["angle_dx"], g["mask"]
    pts = {k: (BD.points(x, k), BD.points(y, k)) for k in "huv"}
    (lon, lat), fills, t, u, v = bilinear_sources(api, g, kind, dtype, nrec, two)
    tag = (name, kind, np.dtype(dtype).name, nrec)
    with np.errstate(invalid="ignore"):
        for k in "huv":
            m = mask if k == "h" else None
            res = api.B.bilinear(x, y, t, points=k, mask=m, fill=False)
            wv, wf = BD.interpolate(*pts[k], lon, lat, t.records, fills=fills, mask=m)
            same(res["values"], wv.reshape(res["values"].shape), tag + (k, "values"))
            same(res["flags"], wf.reshape(res["flags"].shape), tag + (k, "flags"))
            if k == "h":   # filled, under the detected flags
                fres = api.B.bilinear(x, y, t, mask=m, fill_max=fill_max)
                s = fres["summary"]
                assert (s["periodic"], s["fold"]) == g["topology"], (tag, s)
                fv, ff, _ = BD.fill(wv, wf, s["periodic"], s["fold"], fill_max)
                same(fres["values"], fv.reshape(fres["values"].shape), tag + ("filled values",))
                same(fres["flags"], ff.reshape(fres["flags"].shape), tag + ("filled flags",))
        # a vector at the h points, filled and turned with the cosines and sines the device returns; at the c points, unturned
        (wu, wv2), wf = BD.interpolate(*pts["h"], lon, lat, u.records, v.records, fills=fills, mask=mask)
        res = api.B.bilinear(x, y, u, v, angle_dx=angle, mask=mask, fill_max=fill_max)
        s = res["summary"]
        fu, ff, _ = BD.fill(wu, wf, s["periodic"], s["fold"], fill_max)
        fv, ff2, _ = BD.fill(wv2, wf, s["periodic"], s["fold"], fill_max)
        assert ff.tobytes() == ff2.tobytes()
        ug, vg = BD.rotate(fu, fv, ff, res["rot_cos"], res["rot_sin"])
        for key, want in (("values", ug), ("values2", vg), ("flags", ff), ("flags2", ff)):
            same(res[key], want.reshape(res[key].shape), tag + ("vector h", key))
        ca, sa = BD.rot(BD.points(angle, "h"))
        assert np.abs(res["rot_cos"] - ca).max() <= 4e-16 and np.abs(res["rot_sin"] - sa).max() <= 4e-16
        (uu, _), fu_ = BD.interpolate(*pts["u"], lon, lat, u.records, v.records, fills=fills)
        (_, vv), fv_ = BD.interpolate(*pts["v"], lon, lat, u.records, v.records, fills=fills)
        res = api.B.bilinear(x, y, u, v, points="c", rotate=False)
        for key, want in (("values", uu), ("values2", vv), ("flags", fu_), ("flags2", fv_)):
            same(res[key], want.reshape(res[key].shape), tag + ("vector c", key))
    return fres


BILINEAR_CASES = [("nonuniform", np.float64, 3, False), ("regular", np.float32, 5, True), ("1x1", np.float64, 1, False),
                  ("1x5", np.float32, 6, False), ("3x2", np.float64, 3, False), ("7x1", np.float32, 5, False)]


@pytest.mark.parametrize("name", list(sm.CUTS) + list(sm.SHAPES))
def test_bilinear_equals_definition(api, name):
    g = grid(name)
    filled = 0
    for k, (kind, dtype, nrec, two) in enumerate(BILINEAR_CASES):
        fres = check_bilinear(api, g, name, kind, dtype, nrec, two, fill_max=2 if k == 1 else None)
        filled += fres["counts"]["filled"]
    if name in sm.CUTS:
        assert filled > 0


@pytest.mark.parametrize("name", ["neither", "1x1", "1x63", "fold_5x7"])
def test_bilinear_with_tables_too_large_for_lds(api, name, monkeypatch):
    """8000 + 400 nodes are 67 200 bytes: the kernel forms every node from the edges in global memory, without any knob"""
    monkeypatch.delenv("OGG_BILINEAR_LDS", raising=False)
    check_bilinear(api, grid(name), name, "over_lds", np.float32, 1, False)


def test_bilinear_nan_and_infinite_targets(api):
    """Targets of +-inf and NaN longitude reduce to t = 0 on both sides.  A NaN latitude lies between no two nodes (include/ogg_hip.h,
    "Bilinear interpolation", locate): the point is unfilled with the fill value whatever the corners hold, dry under a dry mask cell,
    and filled from its neighbours at the h points."""
    g = sm.latlon_grid(3, 5)
    x, y = g["x"].copy(), g["y"].copy()
    x[1, 1], x[1, 3], x[3, 5] = np.nan, np.inf, -np.inf           # h points (0, 0), (0, 1), (1, 2)
    y[3, 3], y[5, 9], y[1, 7] = np.nan, np.nan, np.inf            # h points (1, 1), (2, 4); (0, 3) above every node
    y[2, 5], x[3, 4] = np.nan, np.nan                             # the v point (1, 2) and the u point (1, 2)
    mask = np.ones((3, 5), np.uint8)
    mask[2, 4] = 0
    pts = {k: (BD.points(x, k), BD.points(y, k)) for k in "huv"}
    for kind, dtype, nrec in (("nonuniform", np.float64, 2), ("regular", np.float32, 5), ("3x2", np.float64, 1), ("1x1", np.float32, 3),
                              ("1x5", np.float64, 1)):
        lon, lat = sm.source_edges(kind)
        f = sm.smooth_field(lon, lat, nrec, dtype)
        if f[0].size > 1:            # missing corners in the first and last rows: were the NaN-latitude rows to differ, the flags would
            f[:, 0, 0] = np.nan
            f[:, -1, -1] = np.nan
        src = api.R.Source(f, lon, lat)
        with np.errstate(invalid="ignore"):
            for k in "huv":
                m = mask if k == "h" else None
                res = api.B.bilinear(x, y, src, points=k, mask=m, fill=False)
                wv, wf = BD.interpolate(*pts[k], lon, lat, f, mask=m)
                same(res["values"], wv, (kind, k, "values"))
                same(res["flags"], wf, (kind, k, "flags"))
            res = api.B.bilinear(x, y, src, points="h", mask=mask, fill=False)
            assert np.all(res["flags"][:, 1, 1] == BD.UNFILLED) and np.all(res["values"][:, 1, 1] == BD.FILL)
            assert np.all(res["flags"][:, 2, 4] == BD.DRY)
            assert np.all(res["flags"][:, 0, :3] == BD.REMAPPED)   # NaN and infinite longitudes are t = 0: points like any other
            fres = api.B.bilinear(x, y, src, points="h", mask=mask)
            wv, wf = BD.interpolate(*pts["h"], lon, lat, f, mask=mask)
            fv, ff, _ = BD.fill(wv, wf, False, False)
            same(fres["values"], fv, (kind, "filled values"))
            same(fres["flags"], ff, (kind, "filled flags"))
            assert np.all(fres["flags"][:, 1, 1] == BD.FILLED)
            rv = api.B.bilinear(x, y, src, points="v", fill=False)
            assert np.all(rv["flags"][:, 1, 2] == BD.UNFILLED) and np.all(rv["values"][:, 1, 2] == BD.FILL)


NARROW = ["band_2x1", "band_2x2", "band_3x1", "band_3x2", "129x1", "1x63", "1x65", "3x3", "fold_5x7"]


@pytest.mark.parametrize("name", NARROW)
def test_bilinear_fill_on_narrow_grids(api, name):
    """One hole per record (small_meshes.source_with_holes) instead of a missing left column, which is the whole grid when it is one
    or two columns wide: the fill really runs, with W and E the same cell on the two-wide bands (summed twice, claimed twice) and a
    cell its own W and E on the one-wide ones.  No mask."""
    g = grid(name)
    x, y = g["x"], g["y"]
    for dtype, nrec, fill_max in ((np.float64, 3, None), (np.float32, 5, 1)):
        f, lon, lat, fills = sm.source_with_holes(x, y, nrec=nrec, dtype=dtype)
        src = api.R.Source(f, lon, lat, fill=fills)
        res = api.B.bilinear(x, y, src, fill_max=fill_max)
        s = res["summary"]
        assert (s["periodic"], s["fold"]) == g["topology"], s
        wv, wf = BD.interpolate(BD.points(x, "h"), BD.points(y, "h"), lon, lat, f, fills=fills)
        fv, ff, _ = BD.fill(wv, wf, s["periodic"], s["fold"], fill_max)
        same(res["values"], fv, (name, nrec, "values"))
        same(res["flags"], ff, (name, nrec, "flags"))
        assert res["counts"]["filled"] > 0 and res["counts"]["interpolated"] > 0, (name, res["counts"])
        if fill_max is None:
            assert res["counts"]["unfilled"] == 0


FILL_SHAPES = [(3, 1), (3, 2), (2, 1), (2, 2), (129, 1), (1, 1), (1, 65), (5, 7), (4, 3)]


@pytest.mark.parametrize("ny, nx", FILL_SHAPES)
def test_fill_step_on_synthetic_flags(api, ny, nx):
    """The remap's fill step through its params-level entry (ogg_remap_fill_dev), under all four (periodic, fold) combinations on
    every shape: on a band one or two cells wide the exchange grid gives no cell an entry (a cell 180 or 360 degrees wide is no
    polygon), so the array-level remap() cannot seed a fill there.  nrec = 3 and 5: flag words that straddle two records."""
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    dev = torch.device("cuda:0")
    lon, lat = sm.source_edges("3x2")
    filled = 0
    for nrec in (3, 5):
        src = api.R.Source(sm.smooth_field(lon, lat, nrec, np.float64), lon, lat)
        v, fl = sm.synthetic_flags(ny, nx, nrec, 11 * ny + nx)
        for periodic in (False, True):
            for fold in (False, True):
                for fill_max in (None, 1):
                    tv = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                    tf = api.R.flags_buffer(torch, tv.numel(), dev).view(v.shape)
                    tf.copy_(torch.from_numpy(fl))
                    counts = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
                    api.R.fill_dev(api.R.params(ny, nx, src, 0, periodic, fold, fill_max), tv, tf, counts,
                                   torch.cuda.current_stream(dev).cuda_stream, dev)
                    wv, wf, wd = RD.fill(v, fl, periodic, fold, fill_max)
                    tag = (ny, nx, nrec, periodic, fold, fill_max)
                    assert tv.cpu().numpy().tobytes() == wv.tobytes(), tag
                    assert tf.cpu().numpy().tobytes() == wf.tobytes(), tag
                    c = api.R.counts_dict(counts.cpu().numpy())
                    assert c["filled"] == int((wf == RD.FILLED).sum()) and c["max_distance"] == wd, tag
                    filled += c["filled"]
    assert filled > 0 or ny * nx == 1


# ---- runoff ----------------------------------------------------------------------------------------------------
def runoff_field(lon, lat, nrec, dtype, prob, seed):
    """sparse positive records with NaN and -999 holes (as tests/test_gpu_runoff.py)"""
    rng = np.random.default_rng(seed)
    NB, NA = lat.size - 1, lon.size - 1
    f = np.where(rng.random((nrec, NB, NA)) < prob, rng.random((nrec, NB, NA)) * 1e-4, 0.0).astype(dtype)
    f[rng.random((nrec, NB, NA)) < 0.02] = np.nan
    f[rng.random((nrec, NB, NA)) < 0.02] = -999.0
    return f


def run_runoff(api, g, src, wet, mode):
    import torch
    from test_gpu_runoff import check_against_definition
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    res = api.RO.runoff_dev(to(g["x"]), to(g["y"]), to(g["area"]), src, wet, targets=mode, Re=RE, keep_lists=True)
    s = res["summary"]
    assert (s["periodic"], s["fold"]) == g["topology"], s
    check_against_definition(res, src, wet, g, mode)   # the target set bit for bit under those flags, then values and distances
    host = api.RO.runoff(g["x"], g["y"], g["area"], src, wet, targets=mode, Re=RE)
    for k in ("values", "n_sources", "src_cell", "src_target", "src_d2"):
        assert host[k].tobytes() == res[k].tobytes(), k
    return res


@pytest.mark.parametrize("name", list(sm.CUTS))
def test_runoff_equals_definition_on_every_topology(api, name):
    g = grid(name)
    wet = g["mask"]
    assert np.any(wet[:, 0] == 0) and np.any(wet[-1] == 0)
    for k, (kind, dtype, mode, prob) in enumerate((("regular", np.float32, "coast", 0.2), ("nonuniform", np.float64, "coast", 0.3),
                                                   ("regular", np.float64, "wet", 0.05))):
        lon, lat = sm.source_edges(kind)
        src = api.R.Source(runoff_field(lon, lat, 3, dtype, prob, k), lon, lat, fill=(-999.0,))
        res = run_runoff(api, g, src, wet, mode)
        assert res["counts"]["mapped"] > 50 and res["counts"]["targets"] > 10


@pytest.mark.parametrize("name", ["1x1", "1x65"])
def test_runoff_onto_a_single_target_cell(api, name):
    g = grid(name)
    ny, nx = g["mask"].shape
    wet = np.zeros((ny, nx), np.uint8)
    wet[0, nx // 2] = 1
    lon, lat = sm.source_edges("nonuniform")
    src = api.R.Source(runoff_field(lon, lat, 2, np.float32, 0.2, 5), lon, lat, fill=(-999.0,))
    res = run_runoff(api, g, src, wet, "coast")
    c = res["counts"]
    assert c["targets"] == 1 and c["cells"] == 1 and c["max_sources"] == c["mapped"] > 10
    assert np.all(res["src_target"] == nx // 2) and res["n_sources"][0, nx // 2] == c["mapped"]


def test_runoff_exact_distance_tie_goes_to_the_smaller_cell(api):
    """the mirrored +-10 degree case of tests/test_runoff_cpu.py on the device: a source on the equator midway between two coastal
    cells whose unit vectors mirror each other bit for bit"""
    g = sm.latlon_grid(1, 3, lon0=-15.0, lat0=-5.0, dlon=10.0, dlat=10.0)
    g["topology"] = (False, False)
    wet = np.array([[1, 0, 1]], np.uint8)
    lon, lat = -185.0 + 10.0 * np.arange(37), np.array([-90.0, -5.0, 5.0, 90.0])
    f = np.zeros((1, 3, 36))
    f[0, 1, 18] = 2.5e-5                                       # the source cell centred on (0, 0)
    assert (lon[18] + lon[19]) / 2.0 == 0.0
    res = run_runoff(api, g, api.R.Source(f, lon, lat), wet, "coast")
    assert res["tgt_cell"].tolist() == [0, 2] and res["src_cell"].tolist() == [36 + 18]
    d = ROD.d2(res["src_u"], res["tgt_u"])[0]
    assert d[0] == d[1]                                        # a bit-exact tie on the device's own unit vectors
    assert res["src_target"].tolist() == [0] and res["src_d2"][0] == d[0]
    assert res["n_sources"].tolist() == [[1, 0, 0]]

"""GPU tests of the curvilinear-source exchange grid (csrc/ogg_xgrid_curv.hip, exchange_grid_curv.py, remap.CurvilinearSource): the
device's lists against the definition in tests/xgrid_curv_definition.py on the zoo of hand-made cells under five source meshes each,
the particular cases (a disjoint and a touching source, a band without a model row), large lists and the sort, truths that do not
come from the definition (a mesh laid over itself, conservation on generated grids), and the same bits for any index, capacity and
entry."""
import ctypes
import os

import numpy as np
import pytest

import xgrid_cs_definition as cd
import xgrid_curv_definition as vd
from test_gpu_xgrid_cs import compare

pytestmark = pytest.mark.gpu
RE = 6371.0e3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH = os.path.join(ROOT, "tests", "golden", "xgrid_curv_truth.npz")
LIST_KEYS = ("src", "ocn", "area", "a_poly", "a_src")
SOURCES = ("rotated_12x9", "north_to_south", "pole_inside", "bad_cells", "one_cell")
CONFIGS = {
    "r05": dict(inverse_resolution=0.5, ensure_nj_even=True),
    "r05_dp": dict(inverse_resolution=0.5, lon_dp=80.0, lat_dp=-85.85, ensure_nj_even=True),
}


@pytest.fixture(scope="module")
def XC(hip):
    from ocean_model_grid_generator_amd import exchange_grid_curv
    return exchange_grid_curv


@pytest.fixture(scope="module")
def RM(hip):
    from ocean_model_grid_generator_amd import remap
    return remap


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def as_cs(res):
    """a result in the shape test_gpu_xgrid_cs.compare reads: one face, the source cells its atmosphere"""
    return dict(res, atm=np.hstack([res["src"], np.zeros((res["src"].shape[0], 1), np.int32)]), a_atm=res["a_src"][None])


def want_cs(lst):
    return [(I, J, 0, n, m, a) for I, J, n, m, a in lst]


def defined(counts):
    return {k: counts[k] for k in vd.COUNT_FIELDS}


def against_definition(res, want):
    lst, a_poly, a_src, counts = want[:4]
    d = compare(as_cs(res), want_cs(lst), cd.a_poly_array(a_poly))
    assert defined(res["counts"]) == counts
    a_def = cd.a_poly_array(a_src)
    np.testing.assert_array_equal(np.isnan(res["a_src"]), np.isnan(a_def))
    ok = np.isfinite(a_def) & (a_def > 0)
    assert np.all(np.abs(res["a_src"][ok] / a_def[ok] - 1) <= 1e-12)
    return d


def same_bits(a, b, what=""):
    for k in LIST_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert defined(a["counts"]) == defined(b["counts"]), what


@pytest.fixture(scope="module")
def zoo_runs(XC):
    """{(target, source): (device result, the definition's tuple)} of the whole zoo under its five sources, computed once"""
    out = {}
    for tname, (x, y, _) in cd.zoo().items():
        for sname, (sx, sy) in vd.sources_for(x, y).items():
            out[(tname, sname)] = (XC.exchange_grid_curv(x, y, sx, sy, Re=RE), vd.exchange_grid_curv(x, y, sx, sy, Re=RE))
    return out


@pytest.mark.parametrize("sname", SOURCES)
def test_zoo_lists_against_the_definition(zoo_runs, sname):
    """pole corners in every arrangement, triangles, clockwise, collapsed, bow-tie and NaN-cornered cells, cells stated whole turns
    away and regional grids of 1 x 1, 63 x 1, 64 x 1 and 65 x 1 cells, under each source mesh"""
    zoo = cd.zoo()
    assert {"regional_1x1", "regional_1x63", "regional_1x64", "regional_1x65"} <= set(zoo)
    for tname, (x, y, expect) in zoo.items():
        res, want = zoo_runs[(tname, sname)]
        assert set(want[4].values()) == {expect}, (tname, want[4])
        against_definition(res, want)
        c = res["counts"]
        if expect == "ok":
            assert c["kept"] > 0 and c["candidates"] >= c["kept"], (tname, sname, c)
        else:
            assert c["kept"] == c["candidates"] == 0 and c[expect] == c["cells"], (tname, sname, c)
        sstat = set(want[5].values())
        if sname == "north_to_south":
            assert sstat == {"reversed"} and c["src_reversed"] == c["src_cells"] == 108
        elif sname == "bad_cells":
            assert (c["src_degenerate"], c["src_flat"], c["src_wide"]) == (1, 1, 2)
        else:
            assert sstat == {"ok"}, (tname, sname)


def test_a_mesh_stored_north_to_south_gives_the_mirrored_list(zoo_runs):
    for tname in ("regional_2x3", "regional_1x65", "pole_one_0"):
        a, b = zoo_runs[(tname, "rotated_12x9")][0], zoo_runs[(tname, "north_to_south")][0]

        def significant(r, flip):
            J = 8 - r["src"][:, 1] if flip else r["src"][:, 1]
            ap = r["a_poly"][r["ocn"][:, 1], r["ocn"][:, 0]]
            big = r["area"] > 1e-10 * np.minimum(ap, r["a_src"][r["src"][:, 1], r["src"][:, 0]])
            keys = np.stack([r["ocn"][:, 1], r["ocn"][:, 0], J, r["src"][:, 0]], axis=1)[big]
            order = np.lexsort(keys.T[::-1])
            return keys[order], r["area"][big][order], ap[big][order]
        ka, aa, ap = significant(a, False)
        kb, ab, _ = significant(b, True)
        np.testing.assert_array_equal(ka, kb)
        assert np.all(np.abs(aa - ab) <= 1e-12 * ap)


def test_whole_turns_disjoint_touching_and_a_band_without_a_model_row(XC, hip):
    import torch
    x, y, _ = cd.zoo()["regional_2x3"]          # 30.25 .. 31.75 E, 20.5 .. 22 N
    sx, sy = vd.regular_mesh(29.75, 20.25, 0.75, 0.5, 4, 5)
    base = XC.exchange_grid_curv(x, y, sx, sy, Re=RE)
    against_definition(base, vd.exchange_grid_curv(x, y, sx, sy, Re=RE))
    assert np.all((sx + 720.0) - 720.0 == sx) and base["counts"]["kept"] > 0
    same_bits(XC.exchange_grid_curv(x, y, sx + 720.0, sy, Re=RE), base, "720 degrees away")
    dis = XC.exchange_grid_curv(x, y, *vd.regular_mesh(100.0, -40.0, 1.0, 1.0, 3, 3), Re=RE)
    assert dis["counts"]["candidates"] == 0 and dis["counts"]["kept"] == 0 and dis["area"].size == 0
    assert dis["counts"]["src_cells"] == 9 and np.all(dis["a_src"] > 0)
    tsx, tsy = vd.regular_mesh(28.25, 20.5, 2.0, 1.5, 1, 1)   # shares the meridian 30.25 E
    touch = XC.exchange_grid_curv(x, y, tsx, tsy, Re=RE)
    assert touch["counts"]["candidates"] > 0 and touch["counts"]["kept"] == 0
    against_definition(touch, vd.exchange_grid_curv(x, y, tsx, tsy, Re=RE))
    # cell row 1 alone holds no model row: an empty list, the source's counts and areas all the same
    dev = "cuda:0"
    xt, yt, sxt, syt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, y, sx, sy))
    band = hip.XgridBand(nx=x.shape[1] - 1, ny=x.shape[0] - 1, j0=1, n_cell_rows=1, Re=RE, threshold=1e-6)
    band.x, band.y = xt[1:].data_ptr(), yt[1:].data_ptr()
    band.x_next, band.y_next = xt[2:].data_ptr(), yt[2:].data_ptr()
    desc = XC.src_desc(sxt.data_ptr(), syt.data_ptr(), 4, 5)
    m0, counts, a_poly, a_src, sij, ocn, area = XC.band_lists_dev(band, desc, torch.cuda.current_stream().cuda_stream, dev)
    c = XC.counts_dict(counts)
    assert c["cells"] == c["candidates"] == c["kept"] == 0 and area.numel() == 0 and a_poly.numel() == 0
    assert c["src_cells"] == 20 and a_src.cpu().numpy().tobytes() == base["a_src"].tobytes()


# ---- large lists and the sort --------------------------------------------------------------------------------------
def in_order(res, NA):
    key = (res["ocn"][:, 1].astype(np.int64) * res["a_poly"].shape[1] + res["ocn"][:, 0]) * (1 << 32) + \
        res["src"][:, 1].astype(np.int64) * NA + res["src"][:, 0]
    return bool(np.all(np.diff(key) > 0))


def test_one_coarse_cell_over_a_fine_source(XC):
    """a 20-degree cell over half-degree cells: more than 1600 pairs in one model cell"""
    x, y = cd.one_cell([(0.0, -10.0), (20.0, -10.0), (20.0, 10.0), (0.0, 10.0)])
    sx, sy = vd.regular_mesh(-1.25, -11.25, 0.5, 0.5, 45, 45)
    res = XC.exchange_grid_curv(x, y, sx, sy, Re=RE)
    want = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)
    against_definition(res, want)
    assert res["counts"]["cells"] == 1 and res["counts"]["kept"] >= 1600 and in_order(res, 45)
    assert abs(res["area"].sum() / res["a_poly"][0, 0] - 1) <= 1e-11


def test_one_coarse_source_cell_on_the_large_list(XC, monkeypatch):
    """a 25-degree source cell over quarter-degree cells with 128 cubes per axis: the cell touches more cubes than a registered cell
    may and goes on the large-cells list"""
    monkeypatch.setenv("OGG_XGRID_CURV_CUBES", "128")
    x, y = cd.regional(-13.0, -7.0, 0.25, 0.25, 108, 56)[:2]
    sx, sy = np.array([[-12.0, 13.0], [-12.0, 13.0]]), np.array([[-6.0, -6.0], [6.0, 6.0]])
    res = XC.exchange_grid_curv(x, y, sx, sy, Re=RE)
    want = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)
    against_definition(res, want)
    c = res["counts"]
    assert c["src_large"] == 1 and c["kept"] > 4000 and in_order(res, 1)
    assert abs(res["area"].sum() / res["a_src"][0, 0] - 1) <= 1e-11


def subset_with_sum(values, total):
    """indices of a subset of ``values`` (small positive ints) that sums to ``total`` (dynamic programming over the sums)"""
    reach = {0: None}
    for i, v in enumerate(values):
        for s in sorted(reach, reverse=True):
            if s + v <= total and s + v not in reach:
                reach[s + v] = (i, s)
    assert total in reach, (total, sum(values))
    out, s = [], total
    while reach[s] is not None:
        i, s = reach[s]
        out.append(i)
    return out


@pytest.fixture(scope="module")
def many(XC):
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 3)[:2]
    sx, sy = vd.rotated_mesh(46.5, 21.625, 36.0, 6.0, 96, 16, angle=0.05)
    return x, y, sx, sy, XC.exchange_grid_curv(x, y, sx, sy, Re=RE), vd.exchange_grid_curv(x, y, sx, sy, Re=RE)


@pytest.mark.parametrize("total", [255, 256, 257, 1025])
def test_candidate_totals_around_the_sort_runs(XC, many, total):
    """one run of 256 keys, the run boundary, and three merge passes: a target mask picks model cells whose candidates sum to the
    total; the masked list is the unmasked one's entries of those cells, in (m, n, q) order"""
    x, y, sx, sy, base, want = many
    cells = sorted(want[7])
    assert sum(want[7].values()) > 1025
    mask = np.zeros(base["a_poly"].shape, np.uint8)
    for i in subset_with_sum([want[7][c] for c in cells], total):
        mask[cells[i]] = 1
    res = XC.exchange_grid_curv(x, y, sx, sy, mask=mask, Re=RE)
    assert res["counts"]["candidates"] == total
    sel = mask[base["ocn"][:, 1], base["ocn"][:, 0]] != 0
    for k in ("src", "ocn", "area"):
        assert res[k].tobytes() == base[k][sel].tobytes(), k
    assert in_order(res, 96) and res["counts"]["masked"] == int((mask == 0).sum())


def test_many_pairs_against_the_definition_and_masks(XC, many):
    x, y, sx, sy, base, want = many
    against_definition(base, want)
    assert in_order(base, 96)
    rng = np.random.default_rng(11)
    smask = (rng.random((16, 96)) < 0.6).astype(np.uint8)
    res = XC.exchange_grid_curv(x, y, sx, sy, src_mask=smask, Re=RE)
    sel = smask[base["src"][:, 1], base["src"][:, 0]] != 0
    assert 0 < sel.sum() < sel.size
    for k in ("src", "ocn", "area"):
        assert res[k].tobytes() == base[k][sel].tobytes(), k
    assert res["a_src"].tobytes() == base["a_src"].tobytes() and res["counts"]["src_masked"] == int((smask == 0).sum())


# ---- the same bits -------------------------------------------------------------------------------------------------
def test_same_bits_for_any_index_capacity_and_entry(XC, many, hip, monkeypatch):
    import torch
    x, y, sx, sy, base, _ = many
    for cubes in ("2", "7", "128"):
        monkeypatch.setenv("OGG_XGRID_CURV_CUBES", cubes)
        same_bits(XC.exchange_grid_curv(x, y, sx, sy, Re=RE), base, "cubes " + cubes)
    monkeypatch.delenv("OGG_XGRID_CURV_CUBES")
    monkeypatch.setenv("OGG_XGRID_CURV_BRUTE", "1")
    brute = XC.exchange_grid_curv(x, y, sx, sy, Re=RE)
    same_bits(brute, base, "brute")
    assert brute["counts"]["src_large"] == brute["counts"]["src_cells"]
    monkeypatch.delenv("OGG_XGRID_CURV_BRUTE")
    # the host entry at exact and at short capacity
    n = base["counts"]["kept"]
    for cap in (n, 1):
        same_bits(XC.exchange_grid_curv(x, y, sx, sy, Re=RE, capacity=cap), base, "capacity %d" % cap)
    nyp, nxp = x.shape
    band = hip.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=RE, threshold=1e-6)
    xc, yc = np.ascontiguousarray(x), np.ascontiguousarray(y)
    band.x, band.y = hip.ptr(xc), hip.ptr(yc)
    band.x_next, band.y_next = hip.ptr(xc[nyp - 1:]), hip.ptr(yc[nyp - 1:])
    sxc, syc = np.ascontiguousarray(sx), np.ascontiguousarray(sy)
    desc = XC.src_desc(sxc.ctypes.data, syc.ctypes.data, 96, 16)
    a_poly, a_src, counts = np.full(base["a_poly"].shape, -1.0), np.full((16, 96), -1.0), hip.XgridCurvCounts()
    one = [np.empty((1, 2), np.int32), np.empty((1, 2), np.int32), np.empty(1)]
    rc = hip.load().ogg_xgrid_curv(ctypes.byref(band), ctypes.byref(desc), 1, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data,
                                   a_poly.ctypes.data, a_src.ctypes.data, ctypes.byref(counts))
    assert rc == hip.OGG_ESHAPE and XC.counts_dict(counts) == base["counts"]
    assert a_poly.tobytes() == base["a_poly"].tobytes() and a_src.tobytes() == base["a_src"].tobytes()
    # device tensors, the source's rows padded
    dev = "cuda:0"
    xt, yt = torch.from_numpy(xc).to(dev), torch.from_numpy(yc).to(dev)
    pad = torch.full((17, 97 + 5), float("nan"), dtype=torch.float64, device=dev)
    sxt, syt = pad.clone(), pad.clone()
    sxt[:, :97], syt[:, :97] = torch.from_numpy(sxc).to(dev), torch.from_numpy(syc).to(dev)
    got = XC.exchange_grid_curv_dev(xt, yt, sxt[:, :97], syt[:, :97], Re=RE)
    for k in LIST_KEYS:
        assert got[k].cpu().numpy().tobytes() == base[k].tobytes(), k
    assert got["counts"] == base["counts"]


# ---- truths that do not come from the definition -------------------------------------------------------------------
def rotated_supergrid(nx, ny):
    return vd.rotated_mesh(40.0, 30.0, 20.0, 10.0, 2 * nx, 2 * ny)


@pytest.mark.parametrize("name", ["regional", "rotated"])
def test_a_mesh_laid_over_itself(XC, RM, name):
    """The source is the target's own model cells: one entry per cell, its own, with A_poly bit for bit (the cell holds all four
    corners; the neighbours' slivers fall under the threshold), and a remapped field comes back within 2 ulp."""
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 3)[:2] if name == "regional" else rotated_supergrid(40, 20)
    sx, sy = np.ascontiguousarray(x[0::2, 0::2]), np.ascontiguousarray(y[0::2, 0::2])
    res = XC.exchange_grid_curv(x, y, sx, sy, Re=RE)
    ny, nx = res["a_poly"].shape
    c = res["counts"]
    assert c["kept"] == c["cells"] == ny * nx and c["candidates"] > c["kept"]
    np.testing.assert_array_equal(res["ocn"], res["src"])
    np.testing.assert_array_equal(res["ocn"][:, 1] * nx + res["ocn"][:, 0], np.arange(ny * nx))
    assert res["area"].tobytes() == res["a_poly"].tobytes() == res["a_src"].tobytes()
    f = np.random.default_rng(2).normal(size=(ny, nx)) * 100.0
    out = RM.remap(x, y, RM.CurvilinearSource(f, sx, sy), fill=False)
    assert np.all(out["flags"] == 1)
    assert np.all(np.abs(out["values"] - f) <= 2 * np.spacing(np.abs(f)))


@pytest.mark.parametrize("name", ["r05", "r05_dp"])
def test_conservation_on_generated_grids(sg, XC, RM, name, capsys):
    """A generated tripolar grid at inverse_resolution 0.5, and the same with the displaced pole, under a global 24 x 12 rotated-pole
    source of 15-degree cells, threshold 0: per model cell and per source cell inside the grid the pieces sum to A_poly / A_src
    within 1e-11, over the grid within 1e-12 (the bounds of the cubed-sphere test); a constant field remaps to the constant within
    4 ulp with no cell unfilled."""
    plan = sg.SupergridPlan(**CONFIGS[name])
    ranks = []
    g = sg.Supergrid(plan, rank=0, world=1, device="cuda:0", halo="local", peers=ranks)
    ranks.append(g)
    g.run_pass()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = np.ascontiguousarray(out["x"]), np.ascontiguousarray(out["y"])
    sx, sy = vd.global_rotated()
    res = XC.exchange_grid_curv(x, y, sx, sy, Re=float(plan.Re), threshold=0.0)
    c = res["counts"]
    assert c["degenerate"] == c["wide"] == c["inverted"] == 0 and c["src_wide"] == c["src_flat"] == c["src_degenerate"] == 0, c
    ap, asrc = res["a_poly"], res["a_src"]
    e_ocn = float(np.max(np.abs(res["ocn_frac"] - 1)))
    inside = np.minimum(np.minimum(sy[:-1, :-1], sy[:-1, 1:]), np.minimum(sy[1:, :-1], sy[1:, 1:])) > y[0].max() + 2.0
    assert inside.sum() > inside.size // 2
    e_src = float(np.max(np.abs(res["src_frac"][inside] - 1)))
    e_glob = abs(res["area"].sum() / ap.sum() - 1)
    with capsys.disabled():
        print("\n%s: %d exchange cells of %d candidates; conservation ocean %.2e, source %.2e, global %.2e"
              % (name, c["kept"], c["candidates"], e_ocn, e_src, e_glob))
    assert e_ocn <= 1e-11 and e_src <= 1e-11 and e_glob <= 1e-12
    # the definition alone on the same x, y (a sample of rows: the first and last three, the fold's among them, and every ninth):
    # its own pieces partition its own A_poly within the same bound, and the device's list is the definition's there
    ny = ap.shape[0]
    rows = sorted(set(range(3)) | set(range(ny - 3, ny)) | set(range(0, ny, 9)))
    want = vd.exchange_grid_curv(x, y, sx, sy, Re=float(plan.Re), threshold=0.0, rows=rows)
    a_def = cd.a_poly_array(want[1])
    s_def = np.zeros(ap.shape)
    for I, J, n, m, a in want[0]:
        s_def[m, n] += a
    d_ocn = float(np.max(np.abs(s_def[rows] / a_def[rows] - 1)))
    with capsys.disabled():
        print("%s: the definition alone on %d rows: conservation ocean %.2e" % (name, len(rows), d_ocn))
    assert d_ocn <= 1e-11
    sel = np.isin(res["ocn"][:, 1], rows)
    keep = np.zeros(ny, bool)
    keep[rows] = True
    sub = dict(res, src=res["src"][sel], ocn=res["ocn"][sel], area=res["area"][sel], a_poly=np.where(keep[:, None], ap, np.nan))
    from test_gpu_xgrid_cs import conditioned_bound
    compare(as_cs(sub), want_cs(want[0]), a_def, conditioned_bound(x, y, a_def))
    const = RM.remap(x, y, RM.CurvilinearSource(np.full(asrc.shape, 3.7), sx, sy), fill=False, threshold=0.0, Re=float(plan.Re))
    assert np.all(const["flags"] == 1)
    assert np.all(np.abs(const["values"] - 3.7) <= 4 * np.spacing(3.7))


def test_same_bits_for_any_rank_count(sg, XC, RM):
    """Supergrid.exchange_grid_curv and Supergrid.remap with a curvilinear source on 1, 2 and 3 ranks, and the host entry on the
    stitched grid: the source whole on every rank, the target banded"""
    sx, sy = vd.global_rotated()
    f = np.random.default_rng(5).normal(size=(2, 12, 24))
    source = RM.CurvilinearSource(f, sx, sy)
    want = None
    for world in (1, 2, 3):
        plan = sg.SupergridPlan(**CONFIGS["r05_dp"])
        ranks = []
        for r in range(world):
            ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
        for g in ranks:
            g.run_pass()
        cut = ranks[0].south_cut()
        res = ranks[0].exchange_grid_curv(cut, sx, sy)
        rem = ranks[0].remap(cut, source)
        for other in ranks[1:]:
            assert other.exchange_grid_curv(other.south_cut(), sx, sy) is None and other.remap(other.south_cut(), source) is None
        got = [res[k].tobytes() for k in LIST_KEYS] + [defined(res["counts"]), rem["values"].tobytes(), rem["flags"].tobytes()]
        if want is None:
            want = got
            out = sg.stitch(plan, [ranks[0].bands_to_host()])
        else:
            assert got == want, world
    x, y = np.ascontiguousarray(out["x"]), np.ascontiguousarray(out["y"])
    host = XC.exchange_grid_curv(x, y, sx, sy, Re=float(plan.Re))
    assert [host[k].tobytes() for k in LIST_KEYS] + [defined(host["counts"])] == want[:6]
    rem = RM.remap(x, y, source, Re=float(plan.Re))
    assert [rem["values"].tobytes(), rem["flags"].tobytes()] == want[6:]
    assert np.all(rem["flags"] == 1)


def test_zoo_areas_against_the_truth(zoo_runs, capsys):
    """The device is no farther from the 50-digit truth (scripts/xgrid_curv_truth.py) than 1.5 x the fp64 definition's own error over
    the same pieces, relative to A_poly: the rule of tests/test_gpu_truth.py and tests/test_gpu_xgrid_cs.py."""
    t = np.load(TRUTH)
    e = {"dev_poly": 0.0, "def_poly": 0.0, "dev_piece": 0.0, "def_piece": 0.0}
    n_piece = 0
    for k, case in enumerate(t["cases"].tolist()):
        res, want = zoo_runs[tuple(case.split("/"))]
        ap = t["a_poly"][t["cell_off"][k]:t["cell_off"][k + 1]]
        dev, ref = res["a_poly"].reshape(-1), cd.a_poly_array(want[1]).reshape(-1)
        pos = ap[:, 0] > 0
        if pos.any():
            e["dev_poly"] = max(e["dev_poly"], float(np.max(np.abs((dev[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0])))
            e["def_poly"] = max(e["def_poly"], float(np.max(np.abs((ref[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0])))
        pieces = t["pieces"][t["piece_off"][k]:t["piece_off"][k + 1]]
        area = t["area"][t["piece_off"][k]:t["piece_off"][k + 1]]
        nx = res["a_poly"].shape[1]
        got_dev = {tuple(a.tolist()) + tuple(o.tolist()): v for a, o, v in zip(res["src"], res["ocn"], res["area"])}
        got_def = {e_[:4]: e_[4] for e_ in want[0]}
        for p, (hi, lo) in zip(pieces.tolist(), area.tolist()):
            p = tuple(p)
            if p in got_dev and p in got_def:   # the same pieces for both
                scale = ap[p[3] * nx + p[2], 0]
                e["dev_piece"] = max(e["dev_piece"], abs((got_dev[p] - hi) - lo) / scale)
                e["def_piece"] = max(e["def_piece"], abs((got_def[p] - hi) - lo) / scale)
                n_piece += 1
    with capsys.disabled():
        print("\ncurvilinear zoo against the truth over %d pieces: A_poly device %.3e, definition %.3e; pieces device %.3e, "
              "definition %.3e (of A_poly)" % (n_piece, e["dev_poly"], e["def_poly"], e["dev_piece"], e["def_piece"]))
    assert n_piece > 2000
    assert e["dev_poly"] <= 1.5 * e["def_poly"]
    assert e["dev_piece"] <= 1.5 * e["def_piece"]


# ---- files ---------------------------------------------------------------------------------------------------------
def test_main_flags_write_the_bytes_of_the_file_commands(hip, XC, RM, tmp_path, capsys):
    """main(--remap_source_grid) and main(--xgrid_curv_grid) against the file-based commands on the grid file main() wrote, on both of
    main()'s paths; the curvilinear source is a smaller generated grid written by the package and a field on its cells.  Without
    the new flags a run writes what it wrote: the same call with the flags absent and with their defaults spelled out."""
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg

    def main(argv):
        ogg.main(**vars(ogg.build_parser().parse_args(argv)))
        return capsys.readouterr().out

    def read(*paths):
        return [open(str(p), "rb").read() for p in paths]
    common = ["--ensure_nj_even", "--no_changing_meta"]
    srcgrid, field = str(tmp_path / "src_hgrid.nc"), str(tmp_path / "field.nc")
    main(["-r", "0.5", "-f", srcgrid] + common)
    sx, sy = XC.read_source_corners(srcgrid)
    NB, NA = sx.shape[0] - 1, sx.shape[1] - 1
    f = (10.0 + np.cos(np.radians(sy[:-1, :-1])) * np.sin(np.radians(2 * sx[:-1, :-1]))).astype(np.float32)
    f[0, :3] = np.nan
    ds = netcdf3.Dataset(field, [("nyc", NB), ("nxc", NA)])
    ds.def_var("t", netcdf3.NC_FLOAT, ("nyc", "nxc"), [("units", "degC")], f)
    ds.write()
    grid, rem, xg = (str(tmp_path / n) for n in ("ocean_hgrid.nc", "remapped.nc", "xgrid_curv.nc"))
    text = main(["-r", "1", "-f", grid, "--remap_source", field, "--remap_var", "t", "--remap_source_grid", srcgrid, "--remap_file", rem,
                 "--xgrid_curv_grid", srcgrid, "--xgrid_curv_file", xg] + common)
    assert "curvilinear exchange grid:" in text and "remap: t" in text
    want = read(rem, xg)
    rem2, xg2 = str(tmp_path / "remapped2.nc"), str(tmp_path / "xgrid_curv2.nc")
    RM.main([grid, field, "--var", "t", "--source_grid", srcgrid, "-o", rem2])
    XC.main([grid, srcgrid, "-o", xg2])
    capsys.readouterr()
    assert read(rem2, xg2) == want
    # the other path of main()
    rem3, xg3 = str(tmp_path / "remapped3.nc"), str(tmp_path / "xgrid_curv3.nc")
    ogg.main(1.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, remap_source=field, remap_var=["t"],
             remap_source_grid=srcgrid, remap_file=rem3, xgrid_curv_grid=srcgrid, xgrid_curv_file=xg3, path="functions")
    capsys.readouterr()
    assert read(rem3, xg3) == want
    # corner variables named on the command line: the same corners from a file of two 2-D variables
    corners = str(tmp_path / "corners.nc")
    ds = netcdf3.Dataset(corners, [("nyp", NB + 1), ("nxp", NA + 1)])
    ds.def_var("glon", netcdf3.NC_DOUBLE, ("nyp", "nxp"), [], sx)
    ds.def_var("glat", netcdf3.NC_DOUBLE, ("nyp", "nxp"), [], sy)
    ds.write()
    xg4 = str(tmp_path / "xgrid_curv4.nc")
    XC.main([grid, corners, "--source_corners", "glon", "glat", "-o", xg4])
    capsys.readouterr()
    assert read(xg4) == want[1:]
    # the values: the source covers the grid, so every cell is remapped from it or filled, and stays within the field's range
    res = netcdf3.read_doubles(rem, names=("t",))["t"]
    assert res.shape == ((netcdf3.read_doubles(grid, names=("x",))["x"].shape[0] - 1) // 2, 360)
    assert np.nanmin(f) - 1e-6 <= res.min() and res.max() <= np.nanmax(f) + 1e-6
    # without the new flags: the same bytes whether the flags are absent or at their defaults
    lon = -180.0 + 2.0 * (np.arange(180) + 0.5)
    lat = -90.0 + 2.0 * (np.arange(90) + 0.5)
    ll = str(tmp_path / "latlon.nc")
    ds = netcdf3.Dataset(ll, [("lat", 90), ("lon", 180)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "degrees_north")], lat)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "degrees_east")], lon)
    ds.def_var("t", netcdf3.NC_DOUBLE, ("lat", "lon"), [], np.cos(np.radians(lat))[:, None] * np.sin(np.radians(lon))[None, :])
    ds.write()
    outs = []
    for tag, extra in (("a", {}), ("b", dict(remap_source_grid=None, remap_source_corners=None, xgrid_curv_grid=None,
                                              xgrid_curv_corners=None))):
        g2, r2, x2 = (str(tmp_path / (tag + n)) for n in ("_hgrid.nc", "_remapped.nc", "_xgrid.nc"))
        ogg.main(1.0, gridfilename=g2, no_changing_meta=True, ensure_nj_even=True, remap_source=ll, remap_var=["t"], remap_file=r2,
                 xgrid_atm=(36, 18), xgrid_file=x2, **extra)
        outs.append(read(g2, r2, x2))
    capsys.readouterr()
    assert outs[0] == outs[1] and outs[0][0] == read(grid)[0]

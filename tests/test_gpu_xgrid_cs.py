"""GPU tests of the cubed-sphere exchange grid (csrc/ogg_xgrid_cs.hip, exchange_grid_cs.py, Supergrid.exchange_grid_cs): the device's
lists against the definition in tests/xgrid_cs_definition.py on a zoo of hand-made cells and on generated grids, against the 50-digit
truth of tests/golden/xgrid_cs_truth.npz, conservation, independence of the rank split, the host-pointer entry and its capacity
protocol, and main()'s --xgrid_cs against the file-based command."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xgrid_cs_definition as cd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE = 6371.0e3
TRUTH = os.path.join(ROOT, "tests", "golden", "xgrid_cs_truth.npz")

CONFIGS = {
    "r1": dict(inverse_resolution=1.0, ensure_nj_even=True),
    "r2": dict(inverse_resolution=2.0, ensure_nj_even=True),
    "r2_dp": dict(inverse_resolution=2.0, lon_dp=80.0, lat_dp=-85.85, ensure_nj_even=True),
    "om4": dict(inverse_resolution=4.0, r_dp=0.2, south_cutoff_row=83, ensure_nj_even=True),
}
ATMS = [(N, sp) for N in (1, 2, 3, 5, 48) for sp in ("equiangular", "edge_equidistant")]
LIST_KEYS = ("atm", "ocn", "area", "a_poly")


@pytest.fixture(scope="module")
def XC(hip):
    from ocean_model_grid_generator_amd import exchange_grid_cs
    return exchange_grid_cs


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def case_name(name, N, sp):
    return "%s/C%d%s" % (name, N, {"equiangular": "e", "edge_equidistant": "d"}[sp])


@pytest.fixture(scope="module")
def zoo_runs(XC):
    """{case: (device result, the definition's (list, A_poly, counts, statuses))} of the whole zoo, computed once"""
    out = {}
    zoo = cd.zoo()
    for N, sp in ATMS + [(96, "equiangular")]:
        atm = XC.cubed_sphere_atm(N, sp)
        for name, (x, y, _) in zoo.items():
            if N == 96 and name != "big_25":
                continue
            out[case_name(name, N, sp)] = (XC.exchange_grid_cs(x, y, atm, Re=RE), cd.exchange_grid_cs(x, y, atm["t"], atm["frames"], Re=RE))
    return out


def compare(res, want, a_def, bound=1e-12):
    """the device's list and A_poly against the definition's: the entry sets among significant pieces, the areas (within ``bound``
    of A_poly: one number, or one per model cell); returns the largest |dA| / A_poly"""
    bound = np.broadcast_to(bound, a_def.shape)
    w_atm, w_ocn, w_area = cd.as_arrays(want)
    ap, a_atm = res["a_poly"], res["a_atm"]
    np.testing.assert_array_equal(np.isnan(ap), np.isnan(a_def))
    ok = np.isfinite(a_def) & (a_def > 0)
    if ok.any():
        assert np.all(np.abs(ap[ok] / a_def[ok] - 1) <= bound[ok]), np.max(np.abs(ap[ok] / a_def[ok] - 1) / bound[ok])
    bad = np.isfinite(a_def) & ~ok   # INVERTED cells: the same sign
    assert np.all(ap[bad] <= 0)

    def significant(atm, ocn, area):
        return area > 1e-10 * np.minimum(ap[ocn[:, 1], ocn[:, 0]], a_atm[atm[:, 2], atm[:, 1], atm[:, 0]])

    g_atm, g_ocn, g_area = res["atm"], res["ocn"], res["area"]
    gs, ws = significant(g_atm, g_ocn, g_area), significant(w_atm, w_ocn, w_area)
    np.testing.assert_array_equal(g_atm[gs], w_atm[ws])
    np.testing.assert_array_equal(g_ocn[gs], w_ocn[ws])
    if not gs.any():
        return 0.0
    d = np.abs(g_area[gs] - w_area[ws]) / ap[g_ocn[gs][:, 1], g_ocn[gs][:, 0]]
    assert np.all(d <= bound[g_ocn[gs][:, 1], g_ocn[gs][:, 0]]), np.max(d / bound[g_ocn[gs][:, 1], g_ocn[gs][:, 0]])
    return float(d.max())


@pytest.mark.parametrize("N,sp", ATMS + [(96, "equiangular")])
def test_zoo_lists_against_the_definition(zoo_runs, N, sp):
    zoo = cd.zoo()
    seen = 0
    for name, (x, y, expect) in zoo.items():
        key = case_name(name, N, sp)
        if key not in zoo_runs:
            continue
        res, (want, a_poly, counts, status) = zoo_runs[key]
        seen += 1
        assert set(status.values()) == {expect}, (key, status)
        compare(res, want, cd.a_poly_array(a_poly))
        assert res["counts"] == counts, key
        assert counts["face_candidates"] <= 3 * counts["cells"], key   # a face and its opposite are never both candidates
        if expect == "ok":
            assert counts["kept"] > 0 and counts["face_candidates"] >= counts["cells"], key
        else:
            assert counts["kept"] == 0 and counts[expect] == counts["cells"], key
    assert seen == (1 if N == 96 else len(zoo))
    if N == 96:   # hundreds of candidates in one lane's cell, spread over the wavefront
        c = zoo_runs[case_name("big_25", 96, sp)][0]["counts"]
        assert c["cells"] == 1 and c["candidates"] > 300 and c["kept"] > 300, c
    else:         # the cube-corner cell lies on three faces
        res = zoo_runs[case_name("cube_corner", N, sp)][0]
        assert sorted(set(res["atm"][:, 2].tolist())) == [0, 1, 4]
        assert res["counts"]["face_candidates"] >= 3


def test_zoo_areas_against_the_truth(zoo_runs, capsys):
    """The device is no farther from the 50-digit truth than 1.5 x the fp64 definition's own error over the same pieces (relative to
    A_poly), the rule of tests/test_gpu_truth.py.  Measured on an MI355X over 4774 pieces: A_poly device 2.266e-14, definition
    2.511e-14; pieces device 2.266e-14, definition 2.621e-14 (the bow-tie, whose lobes cancel in part, gives all four)."""
    t = np.load(TRUTH)
    e = {"dev_poly": 0.0, "def_poly": 0.0, "dev_piece": 0.0, "def_piece": 0.0}
    n_piece = 0
    for k, case in enumerate(t["cases"].tolist()):
        res, (want, a_poly, _, _) = zoo_runs[case]
        ap = t["a_poly"][t["cell_off"][k]:t["cell_off"][k + 1]]
        dev, ref = res["a_poly"].reshape(-1), cd.a_poly_array(a_poly).reshape(-1)
        pos = ap[:, 0] > 0
        if pos.any():
            e["dev_poly"] = max(e["dev_poly"], float(np.max(np.abs((dev[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0])))
            e["def_poly"] = max(e["def_poly"], float(np.max(np.abs((ref[pos] - ap[pos, 0]) - ap[pos, 1]) / ap[pos, 0])))
        pieces = t["pieces"][t["piece_off"][k]:t["piece_off"][k + 1]]
        area = t["area"][t["piece_off"][k]:t["piece_off"][k + 1]]
        nx = res["a_poly"].shape[1]
        got_dev = {tuple(a.tolist()) + tuple(o.tolist()): v for a, o, v in zip(res["atm"], res["ocn"], res["area"])}
        got_def = {e_[:5]: e_[5] for e_ in want}
        for p, (hi, lo) in zip(pieces.tolist(), area.tolist()):
            p = tuple(p)
            if p in got_dev and p in got_def:   # the same pieces for both
                scale = ap[p[4] * nx + p[3], 0]
                e["dev_piece"] = max(e["dev_piece"], abs((got_dev[p] - hi) - lo) / scale)
                e["def_piece"] = max(e["def_piece"], abs((got_def[p] - hi) - lo) / scale)
                n_piece += 1
    with capsys.disabled():
        print("\ncubed-sphere zoo against the truth over %d pieces: A_poly device %.3e, definition %.3e; pieces device %.3e, "
              "definition %.3e (of A_poly)" % (n_piece, e["dev_poly"], e["def_poly"], e["dev_piece"], e["def_piece"]))
    assert n_piece > 2000
    assert e["dev_poly"] <= 1.5 * e["def_poly"]
    assert e["dev_piece"] <= 1.5 * e["def_piece"]


def test_whole_turns_and_a_mask(XC):
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 2)   # (x + 720 and x - 360 are exact for these values)
    atm = XC.cubed_sphere_atm(5, "edge_equidistant")
    base = XC.exchange_grid_cs(x, y, atm, Re=RE)
    for shift in (720.0, -360.0):
        assert np.all((x + shift) - shift == x)
        other = XC.exchange_grid_cs(x + shift, y, atm, Re=RE)
        for k in LIST_KEYS:
            assert other[k].tobytes() == base[k].tobytes(), (shift, k)
        assert other["counts"] == base["counts"]
    mask = (np.random.default_rng(5).random(base["a_poly"].shape) < 0.6).astype(np.uint8)
    masked = XC.exchange_grid_cs(x, y, atm, mask=mask, Re=RE)
    sel = mask[base["ocn"][:, 1], base["ocn"][:, 0]] != 0
    assert 0 < sel.sum() < sel.size
    np.testing.assert_array_equal(masked["ocn"], base["ocn"][sel])
    np.testing.assert_array_equal(masked["atm"], base["atm"][sel])
    assert masked["area"].tobytes() == base["area"][sel].tobytes()
    assert masked["counts"]["masked"] == int((mask == 0).sum())
    assert masked["a_poly"].tobytes() == base["a_poly"].tobytes()
    want, _, counts, _ = cd.exchange_grid_cs(x, y, atm["t"], atm["frames"], mask=mask, Re=RE)
    assert masked["counts"] == counts


def device_grid(sg, name, world=1):
    plan = sg.SupergridPlan(**CONFIGS[name])
    ranks = []
    for r in range(world):
        ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
    for g in ranks:
        g.run_pass()
    return plan, ranks


def sample_rows(ny, every):
    return sorted(set(range(3)) | set(range(ny - 3, ny)) | set(range(0, ny, every)))


def conditioned_bound(x, y, a_def):
    """The bound on |dA| / A_poly between two fp64 evaluations of the definition on different libms, per model cell.  Each component
    of a corner's unit vector carries the rounding of sin and cos, up to an ulp (1.1e-16) each side, so two evaluations differ by
    2.2e-16 per component and a difference of two corners by 4.4e-16 per component, 7.6e-16 in length.  The area is half the cross
    product of such differences over two triangles, so it moves by at most 7.6e-16 (|u| + |v|) / 2 per triangle, 1.6e-15 d_max for
    the cell, d_max its longest corner separation; relative to the cell's solid angle that is 1.6e-15 d_max / (A_poly / Re^2).  The
    1/4 degree cells are at 1e-12; the slivers next to the bipolar cap's singular points (0.008 degrees tall, 0.2 wide) at 1e-11.
    The projected pieces are cross products of differences of the same vectors' ratios and scale the same way.  1e-12, the bound of
    the well-conditioned zoo, covers the roundings that follow."""
    lam, phi = np.radians(x[0::2, 0::2] % 360.0), np.radians(y[0::2, 0::2])
    P = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)], axis=-1)
    c = [P[:-1, :-1], P[:-1, 1:], P[1:, 1:], P[1:, :-1]]
    d_max = np.max([np.linalg.norm(c[i] - c[j], axis=-1) for i in range(4) for j in range(i + 1, 4)], axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1e-12 + 1.6e-15 * d_max / (a_def / (RE * RE))


def conservation(XC, res, atm, y):
    """Relative errors per ocean cell, per atmosphere cell wholly inside the grid, and globally; threshold 0.  An atmosphere cell is
    inside when its four corners lie 2 degrees north of the grid's first row: its great-circle edges bulge poleward of the corners by
    0.6 degrees at most for a C12 cell at 78 S."""
    ap, fij, ocn, area = res["a_poly"], res["atm"], res["ocn"], res["area"]
    ny, nx = ap.shape
    per_ocn = np.bincount(ocn[:, 1].astype(np.int64) * nx + ocn[:, 0], weights=area, minlength=ny * nx).reshape(ny, nx)
    ok = np.isfinite(ap)
    e_ocn = float(np.max(np.where(ok, np.abs(per_ocn / np.where(ok, ap, 1.0) - 1), 0.0)))
    _, clat = XC.cubed_sphere_corners(atm)
    cmin = np.minimum(np.minimum(clat[:, :-1, :-1], clat[:, :-1, 1:]), np.minimum(clat[:, 1:, :-1], clat[:, 1:, 1:]))
    inside = cmin > y[0].max() + 2.0
    assert inside.sum() > inside.size // 2
    e_atm = float(np.max(np.abs(res["ocean_frac"][inside] - 1)))
    e_glob = abs(area.sum() / ap[ok].sum() - 1)
    return e_ocn, e_atm, e_glob


@pytest.mark.parametrize("name", ["r1", "r2", "r2_dp", "om4"])
def test_generated_grids_against_definition_and_conservation(sg, XC, name, capsys):
    plan, ranks = device_grid(sg, name)
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y = out["x"], out["y"]
    ny = (x.shape[0] - 1) // 2
    rows = sample_rows(ny, 9 if name != "om4" else 23)
    for atm in (XC.cubed_sphere_atm(12, "equiangular"), XC.cubed_sphere_atm(48, "edge_equidistant", lon_shift=-10.0)):
        res = g.exchange_grid_cs(cut, atm, threshold=0.0)
        c = res["counts"]
        assert c["degenerate"] == c["wide"] == c["inverted"] == 0, c
        assert c["cells"] <= c["face_candidates"] <= 3 * c["cells"], c
        want, a_poly, _, _ = cd.exchange_grid_cs(x, y, atm["t"], atm["frames"], Re=RE, threshold=0.0, rows=rows)
        a_def = cd.a_poly_array(a_poly)
        sel = np.isin(res["ocn"][:, 1], rows)
        sub = dict(res, atm=res["atm"][sel], ocn=res["ocn"][sel], area=res["area"][sel])
        keep = np.zeros(ny, bool)
        keep[rows] = True
        sub["a_poly"] = np.where(keep[:, None], res["a_poly"], np.nan)
        dmax = compare(sub, want, a_def, conditioned_bound(x, y, a_def))
        e_ocn, e_atm, e_glob = conservation(XC, res, atm, y)
        with capsys.disabled():
            print("\n%s C%d %s: %d exchange cells, %d candidates on %d cell faces; max |dA|/A_poly %.2e on %d rows; conservation "
                  "ocean %.2e, atm %.2e, global %.2e" % (name, atm["N"], atm["spacing"], c["kept"], c["candidates"], c["face_candidates"],
                                                        dmax, len(rows), e_ocn, e_atm, e_glob))
        assert e_ocn <= 1e-11 and e_atm <= 1e-11 and e_glob <= 1e-12
        if name == "r2":   # the default grid reaches both poles: it covers the whole sphere
            assert abs(res["a_poly"].sum() / (4 * np.pi * RE * RE) - 1) <= 1e-12
            assert np.max(np.abs(res["ocean_frac"] - 1)) <= 1e-11
            assert np.max(np.abs(res["land_frac"])) <= 1e-11


def test_same_bits_for_any_rank_count_and_the_host_entry(sg, XC, hip):
    import ctypes
    L = hip
    atm = XC.cubed_sphere_atm(48, "edge_equidistant", lon_shift=-10.0)
    want = None
    for world in (1, 2, 3):
        plan, ranks = device_grid(sg, "r2", world=world)
        res = ranks[0].exchange_grid_cs(ranks[0].south_cut(), atm)
        for other in ranks[1:]:
            assert other.exchange_grid_cs(other.south_cut(), atm) is None
        got = [res[k].tobytes() for k in LIST_KEYS] + [res["counts"]]
        if want is None:
            want = got
            out = sg.stitch(plan, [ranks[0].bands_to_host()])
        else:
            assert got == want, world
    x, y = np.ascontiguousarray(out["x"]), np.ascontiguousarray(out["y"])
    # the host-pointer entry: the same bits, with a first capacity that fits and with one that does not
    for cap in (None, 1):
        host = XC.exchange_grid_cs(x, y, atm, capacity=cap)
        assert [host[k].tobytes() for k in LIST_KEYS] + [host["counts"]] == want, cap
    # the protocol itself: capacity 1 gives OGG_ESHAPE with the counts and A_poly filled, the second call succeeds
    nyp, nxp = x.shape
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=float(plan.Re), threshold=1e-6)
    band.x, band.y = L.ptr(x), L.ptr(y)
    band.x_next, band.y_next = L.ptr(x[nyp - 1:]), L.ptr(y[nyp - 1:])
    desc = XC.atm_desc(atm, atm["t"].ctypes.data)
    a_poly = np.full(((nyp - 1) // 2, (nxp - 1) // 2), -1.0)
    counts = L.XgridCsCounts()
    lib = L.load()
    one = [np.empty((1, 3), np.int32), np.empty((1, 2), np.int32), np.empty(1)]
    rc = lib.ogg_xgrid_cs(ctypes.byref(band), ctypes.byref(desc), 1, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data,
                          a_poly.ctypes.data, ctypes.byref(counts))
    assert rc == L.OGG_ESHAPE
    assert XC.counts_dict(counts) == want[4] and a_poly.tobytes() == want[3]
    n = int(counts.kept)
    full = [np.empty((n, 3), np.int32), np.empty((n, 2), np.int32), np.empty(n)]
    rc = lib.ogg_xgrid_cs(ctypes.byref(band), ctypes.byref(desc), n, full[0].ctypes.data, full[1].ctypes.data, full[2].ctypes.data,
                          a_poly.ctypes.data, ctypes.byref(counts))
    assert rc == L.OGG_OK
    assert [a.tobytes() for a in full] == want[:3]


def _files(tmp, tag):
    pat = str(tmp / (tag + "_tile%d.nc"))
    return pat, [pat % k for k in range(1, 7)], str(tmp / (tag + "_frac.nc"))


def test_main_xgrid_cs_files_equal_the_file_based_command(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg

    def main(argv):
        ogg.main(**vars(ogg.build_parser().parse_args(argv)))
        return capsys.readouterr().out

    def command(grid, extra, tag):
        pat, files, frac = _files(tmp_path, tag)
        r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.exchange_grid_cs", grid, "--cs", "6", "-o", pat,
                            "--frac", frac, "--json", str(tmp_path / (tag + ".json"))] + extra, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return files + [frac]

    grid = str(tmp_path / "ocean_hgrid.nc")
    pat, files, frac = _files(tmp_path, "m")
    text = main(["-r", "1", "--ensure_nj_even", "--no_changing_meta", "-f", grid, "--xgrid_cs", "6", "--xgrid_cs_file", pat,
                 "--xgrid_cs_frac_file", frac])
    assert "cubed-sphere exchange grid:" in text
    want = [open(p, "rb").read() for p in files + [frac]]
    assert [open(p, "rb").read() for p in command(grid, [], "c")] == want
    # the other path of main(), and --skip_metrics
    pat2, files2, frac2 = _files(tmp_path, "f")
    ogg.main(1.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, xgrid_cs=6, xgrid_cs_file=pat2, xgrid_cs_frac_file=frac2,
             path="functions")
    assert [open(p, "rb").read() for p in files2 + [frac2]] == want
    pat3, files3, frac3 = _files(tmp_path, "s")
    ogg.main(1.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, skip_metrics=True, xgrid_cs=6, xgrid_cs_file=pat3,
             xgrid_cs_frac_file=frac3)
    assert [open(p, "rb").read() for p in files3 + [frac3]] == want
    capsys.readouterr()
    # with a synthetic topography in the same call: the wet set of topog.nc
    lon = -180.0 + 0.5 * (np.arange(720) + 0.5)
    lat = -90.0 + 0.5 * (np.arange(360) + 0.5)
    z = (3000.0 * np.sin(np.radians(2 * lon))[None, :] * np.cos(np.radians(lat))[:, None] - 500.0).astype(np.int16)
    srcf, topog = str(tmp_path / "src.nc"), str(tmp_path / "topog.nc")
    ds = netcdf3.Dataset(srcf, [("lat", 360), ("lon", 720)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], lat)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], lon)
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], z)
    ds.write()
    pat4, files4, frac4 = _files(tmp_path, "t")
    main(["-r", "1", "--ensure_nj_even", "--no_changing_meta", "-f", grid, "--topog_source", srcf, "--topog_file", topog, "--xgrid_cs", "6",
          "--xgrid_cs_file", pat4, "--xgrid_cs_frac_file", frac4])
    wet = [open(p, "rb").read() for p in files4 + [frac4]]
    assert wet != want
    assert [open(p, "rb").read() for p in command(grid, ["--topog", topog], "ct")] == wet

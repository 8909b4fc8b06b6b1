"""GPU tests of face topography (csrc/ogg_topog.hip, face_topography.py, Supergrid.face_topography): every byte of every record
equal to the numpy definition of tests/topog_faces_definition.py on small grids, and truths that are not the definition: the exact
combination of the existing supergrid-cell records of ogg_topog, planted ridges, closed forms in Python integers; every split of the
output rows; seam, fold, edges and the pole; the host, device and Supergrid entries, main() and the file command."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import small_grids as G
import small_meshes as sm
import topog_faces_cases as C
import topog_faces_definition as fd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# model cells -> supergrid cells; 1 x 65: 130 supergrid columns, more than one take of faces and more than a wavefront of them
GRIDS = {"1x1": (2, 2), "1x2": (2, 4), "2x1": (4, 2), "3x2": (6, 4), "1x65": (2, 130)}
REFINES = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65)
RASTERS = ("int16", "int16_fill2", "window", "float32_q0.01")


@pytest.fixture(scope="module")
def FT(hip):
    from ocean_model_grid_generator_amd import face_topography
    return face_topography


@pytest.fixture(scope="module")
def T(hip):
    from ocean_model_grid_generator_amd import topography
    return topography


def source(T, kind):
    r = G.raster(kind)
    return T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])


def definition(x, y, kind, **kw):
    r = G.raster(kind)
    return fd.records(x, y, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], **kw)


def recs(res):
    return {fam: res[fam]["records"] for fam in ("u", "v")}


def same(got, want, what):
    for fam in ("u", "v"):
        g, w = got[fam], want[fam]
        assert g.shape == w.shape, (what, fam, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = [(f, np.argwhere(g[f] != w[f])[:3].tolist()) for f in fd.FIELDS if np.any(g[f] != w[f])]
            raise AssertionError("%s: %s records differ in %s" % (what, fam, bad))


# ---- byte equality with the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shear", [False, True])
@pytest.mark.parametrize("kind", RASTERS)
@pytest.mark.parametrize("name", list(GRIDS))
def test_every_record_is_the_definitions(FT, T, name, kind, shear):
    ny, nx = GRIDS[name]
    x, y = G.grid(ny, nx, shear=shear)
    src = source(T, kind)
    for refine in REFINES + ((256,) if name == "1x1" else ()):
        for topology in ((0, 3) if refine == 8 else (0,)):     # a lat-lon grid told to be periodic and folded: the partners at the far end
            got = FT.face_topography(x, y, src, refine=refine, sea_level=-200.0, topology=topology)
            want = definition(x, y, kind, refine=refine, sea_level=-200.0, topology=topology)
            same(recs(got), want, "%s %s shear=%s refine=%d topology=%d" % (name, kind, shear, refine, topology))
    if kind == "window":     # the regional raster leaves one-sided and all-missing lines on the grid across its west edge
        x, y = G.grid(ny, nx, lon0=98.5 - nx // 2, shear=shear)
        got = recs(FT.face_topography(x, y, src, refine=8, topology=0))
        same(got, definition(x, y, kind, refine=8), "%s across the window's edge" % name)
        if nx >= 4:
            assert np.any(got["v"]["n_lines_missing"] > 0) and np.any((got["u"]["n_missing"] > 0) & (got["u"]["n"] > 0))


@pytest.mark.parametrize("kind", ["int16", "window"])
def test_automatic_refinement_where_the_cells_of_a_block_differ(FT, T, kind):
    import topog_definition as td
    x, y = C.mixed_grid()
    r = G.raster(kind)
    c = td.cells(x, y, r["box"][1], r["box"][3])
    differ = 0
    for fam, n_rows, n_cols in (("u", 2, 4), ("v", 3, 3)):
        for row in range(n_rows):
            for col in range(n_cols):
                differ += len({int(c["R"][j, i]) for _, j, i, _ in fd.block(fam, row, col, 4, 6, 0)[0]}) > 1
    assert differ >= 6
    for oversample in (2.0, 0.7, 11.0):
        got = recs(FT.face_topography(x, y, source(T, kind), oversample=oversample, topology=0))
        same(got, definition(x, y, kind, oversample=oversample), "%s oversample %g" % (kind, oversample))
    # cells too large for 256 samples a side are clamped and counted
    x, y = G.grid(2, 4, d=40.0, lat0=-40.0)
    got = recs(FT.face_topography(x, y, source(T, kind), topology=0))
    same(got, definition(x, y, kind), "%s clamped" % kind)
    assert np.all(got["u"]["R"] == 256) and got["u"]["n_clamped"].tolist() == [[2, 4, 2]]


# ---- truths that are not the definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16_fill2", "window", "float32_q0.01"])
@pytest.mark.parametrize("topology", [0, 1, 3])
def test_counts_and_extremes_combine_the_supergrid_cell_records(FT, T, kind, topology):
    """n, n_missing, hi and q_min of a face are the exact combination of the records ogg_topog gives the block's supergrid cells"""
    x, y = G.grid(6, 8, lon0=97.0, shear=True)
    src = source(T, kind)
    for refine in (1, 5, 33):
        cell = T.topography(x, y, src, cells="supergrid", refine=refine)["records"]
        got = recs(FT.face_topography(x, y, src, refine=refine, topology=topology))
        for fam in ("u", "v"):
            for row in range(got[fam].shape[0]):
                for col in range(got[fam].shape[1]):
                    block = [cell[j, i] for _, j, i, _ in fd.block(fam, row, col, 6, 8, topology)[0]]
                    f = got[fam][row, col]
                    want = (sum(int(b["n"]) for b in block), sum(int(b["n_missing"]) for b in block), max(int(b["max"]) for b in block),
                            min(int(b["min"]) for b in block))
                    assert (int(f["n"]), int(f["n_missing"]), int(f["hi"]), int(f["q_min"])) == want, (kind, refine, fam, row, col)


@pytest.mark.parametrize("kind", C.PLANTED_KINDS)
def test_planted_ridges(FT, T, kind):
    x, y = C.planted_grid()
    got = FT.face_topography(x, y, T.Source(C.planted(kind), *C.BOX), refine=C.PLANTED_R, topology=0)
    C.assert_planted(kind, recs(got))
    fam, row, col = ("v", 1, 1) if kind.startswith("row") else ("u", 1, 1)
    assert got[fam]["depth_max"][row, col] == -float(C.RIDGE) and got[fam]["open_fraction"][row, col] == 0.0


@pytest.mark.parametrize("kind", ["index_js", "index_is"])
def test_closed_forms_in_python_integers(FT, T, kind):
    x, y = C.closed_grid()
    for R in (2, 4, 16, 64, 128):
        C.assert_closed_forms(kind, R, recs(FT.face_topography(x, y, source(T, kind), refine=R, topology=0)))


# ---- splits of the output rows -----------------------------------------------------------------------------------------------------
def test_every_split_of_the_row_ranges(FT, T, hip):
    import torch
    x, y = G.grid(6, 4, shear=True)
    xd, yd = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    dev = T.DeviceSource(source(T, "int16_fill2"), "cuda:0")
    whole = recs(FT.face_topography_dev(xd, yd, dev, refine=7, topology=3))
    same(whole, definition(x, y, "int16_fill2", refine=7, topology=3), "the one call")
    for k in range(4):
        for m in range(5):
            lo = recs(FT.face_topography_dev(xd, yd, dev, refine=7, topology=3, u_rows=(0, k), v_rows=(0, m)))
            hi = recs(FT.face_topography_dev(xd, yd, dev, refine=7, topology=3, u_rows=(k, 3), v_rows=(m, 4)))
            assert lo["u"].shape[0] == k and hi["v"].shape[0] == 4 - m
            for fam in ("u", "v"):
                assert np.concatenate([lo[fam], hi[fam]]).tobytes() == whole[fam].tobytes(), (k, m, fam)
    mid = recs(FT.face_topography_dev(xd, yd, dev, refine=7, topology=3, u_rows=(1, 2), v_rows=(2, 3)))
    assert mid["u"].tobytes() == whole["u"][1:2].tobytes() and mid["v"].tobytes() == whole["v"][2:3].tobytes()
    # empty ranges write nothing
    p = FT.params(6, 4, 3, refine=7, u_rows=(2, 2), v_rows=(1, 1), desc=dev.desc, device=True)
    p.points(xd.data_ptr(), yd.data_ptr())
    out = torch.full((2, 64), -7, dtype=torch.int64, device="cuda:0")
    ws = torch.zeros(int(hip.load().ogg_topog_workspace_bytes()), dtype=torch.uint8, device="cuda:0")
    hip.call("ogg_topog_faces_dev", *p.args(), ctypes.byref(dev.desc), ws.data_ptr(), ws.numel(), out[0].data_ptr(), out[1].data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((out == -7).all())


# ---- seam, fold, edges and the pole ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", list(sm.CUTS))
def test_seam_fold_and_edges_of_the_tripolar_cuts(FT, T, cut):
    from ocean_model_grid_generator_amd import ocean_mask as M
    g = sm.topology_cuts()[cut]
    periodic, fold = g["topology"]
    r = G.raster("int16")
    got = FT.face_topography(g["x"], g["y"], source(T, "int16"), refine=2)     # the topology detected
    assert got["summary"]["topology"] == M.topology_flags(periodic, fold)
    ny, nx = g["x"].shape[0] - 1, g["x"].shape[1] - 1
    C.assert_edges(lambda fam, row, col: got[fam]["records"][row, col], ny, nx, periodic, fold)
    want = C.edge_records(g["x"], g["y"], r["data"], r["box"], M.topology_flags(periodic, fold), 2)
    for (fam, row, col), w in want.items():
        assert got[fam]["records"][row, col].tobytes() == w.tobytes(), (cut, fam, row, col)
    s = got["summary"]
    assert s["u"]["n_one_sided"] == (0 if periodic else 2 * (ny // 2)) and s["v"]["n_one_sided"] == (1 if fold else 2) * (nx // 2)


@pytest.mark.parametrize("kind", ["int16", "window"])
def test_pole_faces_have_no_lines(FT, T, kind):
    x, y = G.pole_block()
    for refine in (None, 4):
        got = recs(FT.face_topography(x, y, source(T, kind), refine=refine, topology=0))
        same(got, definition(x, y, kind, refine=refine), "pole block")
        assert [bool(f & fd.F_POLE) for f in got["u"]["flags"][0]] == [True, False]
        assert [bool(f & fd.F_POLE) for f in got["v"]["flags"][:, 0]] == [True, False]
        assert got["u"]["n"][0, 0] == got["u"]["n_lines"][0, 0] == 0 and got["u"]["lo"][0, 0] == fd.INT_MAX
    x, y = G.grid(2, 2, lon0=30.0, lat0=88.0, d=1.0)     # pole corners only
    got = recs(FT.face_topography(x, y, source(T, kind), refine=4, topology=0))
    same(got, definition(x, y, kind, refine=4), "pole corners")
    assert not np.any(got["u"]["flags"] & fd.F_POLE) and not np.any(got["v"]["flags"] & fd.F_POLE)
    x, y = G.pole_block()
    same(recs(FT.face_topography(x, -y[::-1], source(T, kind), refine=4, topology=0)), definition(x, -y[::-1], kind, refine=4), "south pole block")


# ---- hosts and commands ------------------------------------------------------------------------------------------------------------
def synthetic_raster(path):
    from ocean_model_grid_generator_amd import netcdf3
    lon = -180.0 + 0.25 * (np.arange(1440) + 0.5)
    lat = -90.0 + 0.25 * (np.arange(720) + 0.5)
    z = 3000.0 * np.sin(np.radians(3 * lon))[None, :] * np.cos(np.radians(2 * lat))[:, None] - 1500.0
    z += (np.arange(720)[:, None] * 7919 + np.arange(1440)[None, :] * 104729) % 301 - 150
    ds = netcdf3.Dataset(path, [("lat", lat.size), ("lon", lon.size)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], lat)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], lon)
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], z.astype(np.int16))
    ds.write()


def test_host_device_and_supergrid_entries_give_the_same_bytes(FT, T, tmp_path):
    import ocean_model_grid_generator_amd.supergrid as sg
    src_path = str(tmp_path / "src.nc")
    synthetic_raster(src_path)
    src = T.read_source(src_path)
    plan = sg.SupergridPlan(inverse_resolution=1.0, ensure_nj_even=True)
    want = None
    for world in (1, 3):
        ranks = []
        for r in range(world):
            ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
        for g in ranks:
            g.run_pass()
        cut = ranks[0].south_cut()
        res = ranks[0].face_topography(cut, T.DeviceSource(src, "cuda:0", sea_level=-20.0))
        assert all(g.face_topography(cut, src) is None for g in ranks[1:])
        if want is None:
            want = res
            xy = ranks[0].stitched_xy(cut)
            assert res["summary"]["topology"] == 3 and res["summary"]["sea_level"] == -20.0
            host = FT.face_topography(xy[0].cpu().numpy(), xy[1].cpu().numpy(), src, sea_level=-20.0)
            dev = FT.face_topography_dev(xy[0], xy[1], src, sea_level=-20.0)
            for other in (host, dev):
                same(recs(other), recs(res), "entries")
                for fam in ("u", "v"):
                    for k in ("depth_max", "depth_min", "depth_ave", "open_fraction", "n_lines", "R", "flag"):
                        assert other[fam][k].tobytes() == res[fam][k].tobytes(), (fam, k)
                assert other["summary"] == res["summary"]
            assert res["u"]["records"][:, 0].tobytes() == res["u"]["records"][:, -1].tobytes()     # the seam
        else:
            same(recs(res), recs(want), "world %d" % world)
    with pytest.raises(ValueError, match="not made from a list"):
        ranks[0].face_topography(cut, T.SourceList([src, src]))


def test_main_and_the_file_command_write_the_same_files(hip, tmp_path, capsys):
    import ocean_model_grid_generator_amd.ocean_grid_generator as ogg
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "grid0", "t0", "t1", "f1", "t2", "f2", "t3", "f3")}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src)
    ogg.main(1.0, gridfilename=f["grid0"], topog_file=f["t0"], **kw)                                   # without the flag
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["t1"], topog_faces_file=f["f1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], topog_faces_file=f["f2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert "face topography:" in out and "u faces" in out and "largest sill-to-mean gap" in out
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.topography", f["grid"], src, "-o", f["t3"], "--faces", f["f3"]],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "face topography:" in r.stdout
    read = lambda k: open(f[k], "rb").read()   # noqa: E731
    assert read("f1") == read("f2") == read("f3")
    assert read("t0") == read("t1") == read("t2") == read("t3") and read("grid0") == read("grid")     # every other output is what it was
    with pytest.raises(ValueError, match="--topog_faces_file: .*not made from a list"):
        ogg.main(1.0, gridfilename=None, topog_faces_file=f["f1"], no_changing_meta=True, ensure_nj_even=True, topog_source=[src, src])

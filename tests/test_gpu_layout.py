"""GPU tests of the processor layouts and mask tables (csrc/ogg_layout.hip, layout.py, Supergrid.layouts / mask_table): the records
and the per-block counts bit for bit against the cell-by-cell definition of tests/layout_definition.py (exhaustively on tiny
grids; on grids around a wavefront's 64 lanes, the 32-row tile of the table's column pass and the 256 columns of its workgroups
under a fixed list of layouts), truths that need no definition, the status bits and the limits, the knobs, and main(), the
function-level path, the file command and Supergrid.mask_table writing the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import layout_definition as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGIES = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def LY(hip):
    from ocean_model_grid_generator_amd import layout as m
    return m


def random_wet(ny, nx, density, seed=0):
    return (np.random.default_rng(1000 * ny + nx + seed).random((ny, nx)) < density).astype(np.uint8)


def check(LY, wet, layouts, periodic, fold, halo, blocks_up_to=1 << 30, host=False):
    """the sweep's records of ``layouts``, and the per-block counts of those of at most blocks_up_to blocks, against the definition"""
    t = LY.DeviceTable(wet, periodic, fold, halo)
    res = LY.layouts_dev(None, candidates=layouts, table=t)
    rec = res["records"]
    assert rec.shape[0] == len(layouts)
    for k, (px, py) in enumerate(layouts):
        keep = {}
        want = D.record(wet, px, py, periodic, fold, halo, keep)
        got = {f: int(rec[k][f]) for f in D.FIELDS}
        assert got == want, ((px, py), periodic, fold, halo)
        assert (int(rec[k]["px"]), int(rec[k]["py"])) == (px, py)
        if keep and px * py <= blocks_up_to:
            tab = LY.mask_table_dev(None, px, py, table=t)
            assert np.array_equal(tab["block_wet"], keep["block_wet"]) and np.array_equal(tab["block_nbr"], keep["block_nbr"]), (px, py)
            assert [tuple(m) for m in tab["masked"].tolist()] == D.masked_blocks(keep["block_nbr"])
            assert {f: tab["record"][f] for f in D.FIELDS} == want
    if host:   # the host-pointer entry gives the same bytes
        assert LY.layouts(wet, candidates=layouts, periodic=periodic, fold=fold, halo=halo)["records"].tobytes() == rec.tobytes()
    return res


# ---- records against the definition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic,fold", TOPOLOGIES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (5, 7), (9, 12)])
def test_every_layout_of_tiny_grids(LY, shape, periodic, fold):
    ny, nx = shape
    wet = random_wet(ny, nx, 0.12)
    layouts = [(px, py) for px in range(1, nx + 1) for py in range(1, ny + 1)]
    for halo in (0, 1, 2, 13):
        check(LY, wet, layouts, periodic, fold, halo, blocks_up_to=1 << 30 if halo < 2 else 12, host=halo == 1)


def layout_list(ny, nx):
    """about 40 layouts: the ends, the asymmetric (4, *) on odd nx and (3, *) on even nx, sizes about 64 and 256, too fine ones"""
    want = [(1, 1), (nx, ny), (nx, 1), (1, ny), (4, 1), (4, 3), (3, 1), (3, 2), (2, 2), (2, 1), (1, 2), (7, 5), (16, 8), (64, 1), (65, 2),
            (63, 3), (5, 64), (128, 1), (129, 1), (nx - 1, 1), (1, ny - 1), (nx // 2, ny // 2), (33, 17), (12, 9), (8, 8), (6, 11), (13, 7),
            (32, 4), (5, 5), (9, 3), (3, 9), (24, 16), (48, 2), (2, 48), (100, 1), (1, 100), (31, 31), (256, 1), (257, 2), (nx, 2), (2, ny),
            (nx + 1, 1), (1, ny + 1), (4097, 1)]
    out = []
    for px, py in want:
        px, py = max(px, 1), max(py, 1)
        if (px > nx or py > ny) and (px, py) not in ((nx + 1, 1), (1, ny + 1), (4097, 1)):
            px, py = min(px, nx), min(py, ny)
        if (px, py) not in out:
            out.append((px, py))
    return out


# rows 17, 64 (two tiles of 32 to the row), 129, 130; columns 1, 33 (a fold of odd width), 65 and 257 (one past a wavefront and one
# past the 256 columns of a workgroup of the column pass)
@pytest.mark.parametrize("density,periodic,fold", [(0.02, True, True), (0.5, True, True), (0.98, True, True), (0.5, False, True),
                                                   (0.02, True, False), (0.5, False, False)])
@pytest.mark.parametrize("shape", [(17, 33), (129, 1), (64, 65), (130, 257)])
def test_grids_around_the_wavefront_and_the_tiles(LY, shape, density, periodic, fold):
    ny, nx = shape
    wet = random_wet(ny, nx, density)
    layouts = layout_list(ny, nx)
    assert (nx, ny) in layouts and (4097, 1) in layouts
    check(LY, wet, layouts, periodic, fold, 0)
    small = [l for l in layouts if l[0] * l[1] <= 400]
    check(LY, wet, small, periodic, fold, 2, host=density == 0.5)
    check(LY, wet, small[::3], periodic, fold, 40)


# ---- truths that do not come from the definition -----------------------------------------------------------------------------
SHAPES = [(9, 12), (17, 33), (64, 65)]


def all_layouts(ny, nx, step=1):
    return [(px, py) for px in range(1, nx + 1, step) for py in range(1, ny + 1, step)]


@pytest.mark.parametrize("shape", SHAPES)
def test_all_wet_and_all_land(LY, shape):
    ny, nx = shape
    for halo in (0, 3):
        r = LY.layouts_dev(np.ones(shape, np.uint8), candidates=all_layouts(ny, nx, 3), periodic=True, fold=True, halo=halo)["records"]
        assert np.all(r["masked"] == 0) and np.all(r["max_wet"] == r["max_block_cells"]) and np.all(r["pes"] == r["blocks"])
        assert np.all(r["wet_total"] == ny * nx) and np.all(r["masked_cells"] == 0)
        r = LY.layouts_dev(np.zeros(shape, np.uint8), candidates=all_layouts(ny, nx, 3), periodic=True, fold=True, halo=halo)["records"]
        assert np.all(r["masked"] == r["blocks"]) and np.all(r["pes"] == 0) and np.all(r["max_wet"] == 0)
        assert np.all(r["masked_cells"] == ny * nx) and np.all(r["wet_total"] == 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_wet_cell_leaves_one_block(LY, shape):
    ny, nx = shape
    cells = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (ny // 2, 0), (ny // 2, nx - 1), (ny - 1, nx // 2), (ny - 1, nx // 2 - 1)]
    for j, i in cells:   # the corners, the seam columns, the fold row
        wet = np.zeros(shape, np.uint8)
        wet[j, i] = 1
        for periodic, fold in ((True, True), (False, False)):
            r = LY.layouts_dev(wet, candidates=all_layouts(ny, nx, 2), periodic=periodic, fold=fold)["records"]
            assert np.all(r["masked"] == r["blocks"] - 1) and np.all(r["max_wet"] == 1) and np.all(r["wet_total"] == 1), (j, i)


def test_the_fold_and_the_seam_unmask_their_partners_only_when_set(LY):
    ny, nx, px, py = 6, 12, 6, 3   # blocks of 2 x 2 cells: block (a, b) holds columns 2a, 2a+1 and rows 2b, 2b+1
    every = {(a, b) for a in range(px) for b in range(py)}

    def unmasked(wet, periodic, fold, h):
        return every - {tuple(m) for m in LY.mask_table_dev(wet, px, py, periodic=periodic, fold=fold, halo=h)["masked"].tolist()}
    wet = np.zeros((ny, nx), np.uint8)
    wet[ny - 1, 2] = 1   # on the fold row, the first cell of block (1, 2); its fold partner is column 9, in block (4, 2)
    assert unmasked(wet, False, False, 0) == unmasked(wet, True, True, 0) == {(1, 2)}
    assert unmasked(wet, False, False, 1) == unmasked(wet, True, False, 1) == {(0, 2), (1, 2)}
    # row 6 is row 5 at the mirrored column: the halo of the blocks holding column 9 +- 1 (8 .. 10: blocks 4 and 5) reaches the cell
    assert unmasked(wet, False, True, 1) == unmasked(wet, True, True, 1) == {(0, 2), (1, 2), (4, 2), (5, 2)}
    wet = np.zeros((ny, nx), np.uint8)
    wet[2, 0] = 1   # on the seam, the first cell of block (0, 1)
    assert unmasked(wet, False, False, 1) == unmasked(wet, False, True, 1) == {(0, 0), (0, 1)}
    assert unmasked(wet, True, False, 1) == unmasked(wet, True, True, 1) == {(0, 0), (0, 1), (5, 0), (5, 1)}   # column 12 is column 0


@pytest.mark.parametrize("shape", [(1, 1), (31, 63), (32, 64), (33, 65), (65, 255), (64, 256), (63, 257), (129, 1), (1, 300)])
def test_the_finest_layout_is_the_wet_set_itself(LY, shape):
    ny, nx = shape
    wet = random_wet(ny, nx, 0.4)
    t = LY.mask_table_dev(wet, nx, ny, periodic=True, fold=True)
    assert np.array_equal(t["block_wet"], wet) and np.array_equal(t["block_nbr"], wet)
    assert t["record"]["masked"] == int((wet == 0).sum()) and t["masked"].shape[0] == int((wet == 0).sum())
    r = LY.layouts_dev(wet, candidates=[(nx, ny)], periodic=True, fold=True)["records"][0]
    assert r["masked"] == int((wet == 0).sum()) == r["masked_cells"] and r["wet_total"] == int(wet.sum()) and r["max_block_cells"] == 1


@pytest.mark.parametrize("shape", SHAPES)
def test_sums_and_halo_monotony(LY, shape):
    ny, nx = shape
    wet = random_wet(ny, nx, 0.05)
    layouts = all_layouts(ny, nx, 2)
    prev = None
    for halo in (0, 1, 2, 5, 100):
        t = LY.DeviceTable(wet, True, True, halo)
        r = LY.layouts_dev(None, candidates=layouts, table=t)["records"]
        assert np.all(r["wet_total"] == int(wet.sum()))
        assert prev is None or np.all(r["masked"] <= prev)   # masked never grows with the halo
        prev = r["masked"].copy()
        for px, py in layouts[::17]:
            bw, bn = t.blocks(px, py)
            assert int(bw.sum()) == int(wet.sum()) and np.all(bn >= bw) and np.all(bn <= int(wet.sum()))
    assert np.all(prev == 0)   # a halo wider than the grid reaches every cell


def test_explicit_extents_equal_to_the_rule_give_its_bytes(LY):
    wet = random_wet(17, 33, 0.1)
    for px, py in ((4, 3), (5, 2), (33, 17), (1, 1), (7, 6)):
        for halo in (0, 2):
            sx, sy = (np.diff(np.append(LY.extent(n, d)[0], n)) for n, d in ((33, px), (17, py)))
            a = LY.mask_table_dev(wet, px, py, periodic=True, fold=True, halo=halo)
            b = LY.mask_table_dev(wet, px, py, periodic=True, fold=True, halo=halo, xextent=sx, yextent=sy)
            c = LY.mask_table(wet, px, py, periodic=True, fold=True, halo=halo, xextent=list(sx))
            for k in ("block_wet", "block_nbr", "masked", "xbegin", "ybegin"):
                assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()
            assert a["record"] == b["record"] == c["record"] and b["explicit"] and not a["explicit"]
    # extents of the caller's own: against the definition with the same begins
    t = LY.mask_table_dev(wet, 3, 2, periodic=True, fold=True, halo=1, xextent=[20, 1, 12], yextent=[16, 1])
    own, nbr, _ = D.blocks(wet, 3, 2, True, True, 1, xb=[0, 20, 21], yb=[0, 16])
    assert np.array_equal(t["block_wet"], own) and np.array_equal(t["block_nbr"], nbr) and t["record"]["status"] == D.FOLD_ASYMMETRIC
    with pytest.raises(ValueError, match="xextent holds"):
        LY.mask_table_dev(wet, 3, 2, xextent=[20, 1, 11])


# ---- status and limits ---------------------------------------------------------------------------------------------------
def test_status_bits(LY):
    wet = random_wet(9, 12, 0.3)
    cands = [(13, 1), (1, 10), (4097, 1), (1, 4097), (12, 9), (2**31 - 1, 2)]
    r = LY.layouts_dev(wet, candidates=cands, periodic=True, fold=True)["records"]
    assert r["status"].tolist() == [1, 1, 1, 1, 0, 1]
    for f in D.FIELDS[:-1]:
        assert np.all(r[f][[0, 1, 2, 3, 5]] == 0)
    for nx in (12, 13, 33):   # FOLD_ASYMMETRIC exactly where the rule's extents are no mirror images
        wet = random_wet(5, nx, 0.3)
        cands = [(px, 1) for px in range(1, nx + 1)]
        want = []
        for px, _ in cands:
            b, e = D.extent(nx, px)
            want.append(D.FOLD_ASYMMETRIC if any(b[a] + e[px - 1 - a] != nx - 1 for a in range(px)) else 0)
        assert LY.layouts_dev(wet, candidates=cands, periodic=True, fold=True)["records"]["status"].tolist() == want
        assert any(want) and not all(want) and want[3] == (D.FOLD_ASYMMETRIC if nx % 2 else 0)
        assert not LY.layouts_dev(wet, candidates=cands, periodic=True, fold=False)["records"]["status"].any()


def test_candidate_limit_and_a_grid_dimension_above_65535(LY):
    wet = random_wet(9, 12, 0.12)
    base = [(px, py) for px in range(1, 14) for py in range(1, 11)]   # the 108 layouts and the too fine ones around them
    want = np.array([[D.record(wet, px, py, True, True, 1)[f] for f in D.FIELDS] for px, py in base])
    for n in (70000, 1 << 20):
        idx = np.arange(n) % len(base)
        r = LY.layouts_dev(wet, candidates=np.array(base)[idx], periodic=True, fold=True, halo=1)["records"]
        got = np.stack([r[f] for f in D.FIELDS], axis=1)
        assert np.array_equal(got, want[idx])
    with pytest.raises(ValueError, match="1048577 candidates"):
        LY.layouts_dev(wet, candidates=np.ones(((1 << 20) + 1, 2), np.int64), periodic=True, fold=True)


# ---- whole paths -----------------------------------------------------------------------------------------------------------
def test_knobs_change_no_bit(LY, monkeypatch):
    cases = [(random_wet(130, 257, 0.03), True, True, 2), (random_wet(64, 65, 0.5), False, True, 0), (random_wet(9, 12, 0.2), True, False, 1)]
    run = lambda: [(LY.layouts_dev(w, max_blocks=300, periodic=p, fold=f, halo=h, min_block=1)["records"].tobytes(),   # noqa: E731
                    LY.mask_table_dev(w, 5, 4, periodic=p, fold=f, halo=h)["block_nbr"].tobytes()) for w, p, f, h in cases]
    want = run()
    for env in (dict(OGG_LAYOUT_TILE_ROWS="4"), dict(OGG_LAYOUT_TILE_ROWS="7"), dict(OGG_LAYOUT_TILE_ROWS="1024"), dict(OGG_LAYOUT_GRID="1"),
                dict(OGG_LAYOUT_GRID="3"), dict(OGG_LAYOUT_GRID="1000", OGG_LAYOUT_TILE_ROWS="33")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert run() == want, env
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setenv("OGG_LAYOUT_TILE_ROWS", "3")
    with pytest.raises(Exception, match="OGG_LAYOUT_TILE_ROWS=3"):
        LY.DeviceTable(cases[2][0])


def test_main_function_level_file_command_and_supergrid_write_the_same_bytes(LY, hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import read, synthetic_raster
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    f = {k: str(tmp_path / k) for k in ("grid.nc", "topog.nc", "t2.nc", "t3.nc", "r0.json", "r1.json", "r2.json", "r3.json", "m1.json", "m2.json",
                                        "m3.json", "tm.nc", "tm2.nc", "mask.nc", "mask2.nc")}
    d = {k: str(tmp_path / k) for k in ("d0", "d1", "d2", "d3", "d4", "e1", "e2", "e3")}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src, layout_sweep=200)
    # a process count the sweep reaches only by masking: the largest whose best layout has masked blocks
    ogg.main(1.0, gridfilename=f["grid.nc"], topog_file=f["topog.nc"], layout_target_pes=200, mask_table_dir=d["d0"], layout_report=f["r0.json"], **kw)
    T = [r["pes"] for r in json.load(open(f["r0.json"]))["sweep"]["by_pes"] if r["masked"] > 0][0]
    capsys.readouterr()
    kw.update(layout_target_pes=T, mask_table_layout=None)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2.nc"], mask_table_dir=d["d1"], layout_report=f["r1.json"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t3.nc"], mask_table_dir=d["d2"], layout_report=f["r2.json"], path="functions", **kw)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "   layout:" in ln and "wrote" not in ln]
    assert lines[:len(lines) // 2] == lines[len(lines) // 2:] and out.index("topography:") < out.index("   layout:")
    assert sum(ln.startswith("   layout: LAYOUT = ") for ln in lines) == 2 and sum(ln.startswith("   layout: MASKTABLE = mask_table.") for ln in lines) == 2

    def command(*args):
        r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.layout", "--layout_sweep", "200"] + list(args),
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return [ln for ln in r.stdout.splitlines() if "   layout:" in ln and "wrote" not in ln]
    assert command("--topog", f["topog.nc"], "--grid", f["grid.nc"], "--layout_target_pes", str(T), "--mask_table_dir", d["d3"],
                   "--layout_report", f["r3.json"]) == lines[:len(lines) // 2]
    rep = json.load(open(f["r1.json"]))
    best = rep["sweep"]["best"]
    name = rep["tables"][0]["file"]
    assert best["pes"] == T and best["status"] == 0 and name == LY.default_name(best["masked"], best["px"], best["py"]) and os.listdir(d["d1"]) == [name]
    table = open(os.path.join(d["d1"], name), "rb").read()
    assert all(open(os.path.join(d[k], name), "rb").read() == table for k in ("d2", "d3"))
    assert open(f["r1.json"], "rb").read() == open(f["r2.json"], "rb").read() == open(f["r3.json"], "rb").read()
    # the file holds what the definition gives on the wet set as written, and the winner is the definition's
    wet = (read(f["topog.nc"], "depth") > 0).astype(np.uint8)
    assert rep["sweep"]["periodic"] is True and rep["sweep"]["fold"] is True
    keep = {}
    want = D.record(wet, best["px"], best["py"], True, True, 0, keep)
    assert {k: best[k] for k in D.FIELDS} == want and want["masked"] > 0
    assert table.decode() == D.table_text(best["px"], best["py"], D.masked_blocks(keep["block_nbr"]))
    px, py, masked = LY.read_mask_table(os.path.join(d["d1"], name))
    assert (px, py) == (best["px"], best["py"]) and masked.shape[0] == best["masked"]
    cands = LY.sweep_candidates(wet.shape[0], wet.shape[1], 200, 2)
    assert rep["sweep"]["candidates"] == cands.shape[0] > 100
    recs = [dict(D.record(wet, int(c["px"]), int(c["py"]), True, True, 0), px=int(c["px"]), py=int(c["py"])) for c in cands]
    assert D.best(recs, T)[0] == best
    # Supergrid.mask_table and Supergrid.layouts on the generated grid; rank 0 holds the result whatever the rank count
    from test_gpu_runoff import stitched
    import ocean_model_grid_generator_amd.supergrid as sg
    for world in (1, 2):
        plan, ranks, cut, _ = stitched(sg, "r1", world)
        res = ranks[0].mask_table(cut, wet, best["px"], best["py"])
        assert all(r.mask_table(cut, wet, best["px"], best["py"]) is None for r in ranks[1:])
        assert open(LY.write_mask_table(d["d4"] if os.path.isdir(d["d4"]) else (os.makedirs(d["d4"]) or d["d4"]), res), "rb").read() == table
        assert LY.summary_lines(res) == [ln for ln in lines[:len(lines) // 2] if "layouts of at most" not in ln and "for %d processes" % T not in ln]
        sweep = ranks[0].layouts(cut, wet, max_blocks=200)
        assert LY.best_layouts(sweep, T)["best"] == best and all(r.layouts(cut, wet, max_blocks=200) is None for r in ranks[1:])
    # with --ocean_mask_file the edited wet set is used; an explicit layout with a halo, on the three paths
    mk = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src, mask_min_depth=10.0, skip_metrics=True, mask_table_layout=[(12, 8), (5, 3)],
              layout_halo=1)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm.nc"], ocean_mask_file=f["mask.nc"], mask_table_dir=d["e1"], layout_report=f["m1.json"], **mk)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm2.nc"], ocean_mask_file=f["mask2.nc"], mask_table_dir=d["e2"], layout_report=f["m2.json"],
             path="functions", **mk)
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.layout", "--mask", f["mask.nc"], "--periodic", "--fold",
                        "--mask_table_layout", "12", "8", "--mask_table_layout", "5", "3", "--layout_halo", "1", "--mask_table_dir", d["e3"],
                        "--layout_report", f["m3.json"]], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(f["m1.json"], "rb").read() == open(f["m2.json"], "rb").read() == open(f["m3.json"], "rb").read()
    mwet = (read(f["mask.nc"], "mask") != 0).astype(np.uint8)
    assert sorted(os.listdir(d["e1"])) == sorted(os.listdir(d["e2"])) == sorted(os.listdir(d["e3"])) and len(os.listdir(d["e1"])) == 2
    for px, py in ((12, 8), (5, 3)):
        nbr = D.blocks(mwet, px, py, True, True, 1)[1]
        name = LY.default_name(int((nbr == 0).sum()), px, py)
        text = D.table_text(px, py, D.masked_blocks(nbr)).encode()
        assert all(open(os.path.join(d[k], name), "rb").read() == text for k in ("e1", "e2", "e3"))

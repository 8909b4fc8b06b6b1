"""CPU tests of the sill depths: the two formulations of the definition (tests/sill_definition.py: a heap-based widest path, and
Kruskal in descending weight) agree on the GPU tests' kinds of cases; the named cases reach what they are named for; the package's
quantiser, face weights, default seed, basin list, file writer and flag refusals, none of which needs a device."""
import numpy as np
import pytest

import sill_definition as D
from ocean_model_grid_generator_amd import _lib as L
from ocean_model_grid_generator_amd import netcdf3
from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
from ocean_model_grid_generator_amd import sill_depth as S


def both(wu, wv, seeds, topology, bits=None):
    a = D.sill(wu, wv, seeds, topology, bits)
    b = D.sill(wu, wv, seeds, topology, bits, search=D.sill_kruskal)
    for k in ("b", "region", "gate_u", "gate_v"):
        assert np.array_equal(a[k], b[k]), k
    assert a["counts"] == b["counts"]
    return a


@pytest.mark.parametrize("topology", [0, 1, 2, 3])
def test_the_two_formulations_agree(topology):
    rng = np.random.default_rng(topology)
    for ny, nx in [(1, 1), (1, 2), (2, 2), (1, 130), (3, 130), (70, 3), (9, 7), (33, 64)]:
        for bits in (1, 2, 21, 30):
            top = (1 << bits) - 1
            vals = np.array([0, max(top // 2, 1), top])
            for wu, wv in ((rng.integers(0, top + 1, (ny, nx + 1)), rng.integers(0, top + 1, (ny + 1, nx))),
                           (vals[rng.integers(0, 3, (ny, nx + 1))], vals[rng.integers(0, 3, (ny + 1, nx))]),
                           (rng.integers(-top - 2, 2 * top + 2, (ny, nx + 1)), rng.integers(-top - 2, 2 * top + 2, (ny + 1, nx)))):
                seeds = rng.integers(-1, ny * nx + 1, int(rng.integers(1, 4)))
                r = both(wu, wv, seeds, topology, bits)
                b, region = r["b"].reshape(-1), r["region"].reshape(-1)
                gated = set()   # the enclosed side's region of every gate
                for (a, q, w, faces) in D.passages(ny, nx, wu, wv, topology, bits)[0]:
                    kind, row, col, _ = faces[0]
                    code = (r["gate_u"] if kind == "u" else r["gate_v"])[row, col]
                    if code:
                        gated.add(int(region[a if code == 1 else q]))
                assert set(int(v) for v in region[(b > 0) & (b < D.SEED)]) <= gated   # every such region has a gate
                assert np.all((b == 0) == (region == -1))


def test_a_basin_reached_only_across_the_seam():
    ny, nx = 3, 8
    wu, wv = np.zeros((ny, nx + 1), np.int64), np.zeros((ny + 1, nx), np.int64)
    wu[1, 1] = 9          # (1, 0) ~ (1, 1)
    wu[1, 0], wu[1, nx] = 5, 7   # the seam (1, 7) ~ (1, 0): min = 5
    open_ = both(wu, wv, [1 * nx + 1], D.PERIODIC)
    shut = both(wu, wv, [1 * nx + 1], 0)
    assert open_["b"][1, 0] == 9 and open_["b"][1, 7] == 5 and shut["b"][1, 7] == 0
    assert open_["gate_u"][1, 0] == open_["gate_u"][1, nx] == 1 and shut["gate_u"].sum() == 1   # the west cell (1, 7) is enclosed
    assert open_["counts"]["n_connected"] == 2 and shut["counts"]["n_connected"] == 1 and shut["counts"]["n_cut_off"] == 0
    two = np.zeros((1, 3), np.int64) + 4
    assert both(two, np.zeros((2, 2), np.int64), [0], D.PERIODIC)["gate_u"].tolist() == [[0, 2, 0]]   # nx = 2: the seam adds nothing


def test_a_basin_reached_only_across_the_fold():
    ny, nx = 3, 7
    wu, wv = np.zeros((ny, nx + 1), np.int64), np.zeros((ny + 1, nx), np.int64)
    wv[ny, 1], wv[ny, 5] = 6, 8      # (2, 1) ~ (2, 5): min = 6
    wv[ny, 3] = 99                   # the middle cell has no partner: never read
    open_ = both(wu, wv, [2 * nx + 5], D.FOLD)
    shut = both(wu, wv, [2 * nx + 5], 0)
    assert open_["b"][2, 1] == 6 and shut["b"][2, 1] == 0 and open_["b"][2, 3] == 0
    assert open_["gate_v"][ny, 1] == 1 and open_["gate_v"][ny, 5] == 2 and open_["gate_v"][ny, 3] == 0   # the roles swapped
    assert open_["counts"]["n_gate_faces"] == 2 and open_["counts"]["n_clamped"] == 0


def test_the_quantiser():
    d = np.array([0.005, 0.015, 0.025, -3.0, np.nan, np.inf, -np.inf, 1.0e20, 1.0e19, 123.456, 0.0])
    q = S.quantise(d, 0.01)
    assert q.dtype == np.int64
    assert q.tolist() == [0, 2, 2, 0, 0, 0, 0, 0, (1 << 30) - 1, 12346, 0]   # ties to even; NaN, inf and the fill are 0; the clamp
    assert np.array_equal(q, D.quantise(d, 0.01))
    assert S.quantise(np.array([5.0]), 0.25).tolist() == [20]


def test_the_face_weights_of_both_modes():
    rng = np.random.default_rng(5)
    q = rng.integers(1, 50, (4, 6))
    wet = rng.random((4, 6)) > 0.3
    qw = np.where(wet, q, 0)
    for topology in range(4):
        wu, wv = S.cell_face_weights(qw, bool(topology & 1), bool(topology & 2))
        du, dv = D.cell_weights(q, wet, topology)
        assert np.array_equal(wu, du) and np.array_equal(wv, dv)
        fu, fv = rng.random((4, 7)) * 10, rng.random((5, 6)) * 10
        fu[0, 2] = 1.0e20     # a face without a line
        ru, rv = S.raster_face_weights(fu, fv, qw, bool(topology & 1), bool(topology & 2), 0.01)
        assert ru[0, 2] == 0 and np.all(ru[:, 1:6][~(wet[:, :-1] & wet[:, 1:])] == 0)
        both_wet = wet[:-1] & wet[1:]
        assert np.array_equal(rv[1:4][both_wet], D.quantise(fv[1:4], 0.01)[both_wet])
    assert S.bits_for(0) == 1 and S.bits_for(1) == 1 and S.bits_for(2) == 2 and S.bits_for((1 << 21) - 1) == 21 and S.bits_for(1 << 40) == 30


def test_the_default_seed_takes_the_first_of_the_deepest():
    q = np.array([[0, 5, 9], [9, 2, 9]])
    assert S.default_seed(q) == 2
    with pytest.raises(ValueError, match="no wet cell"):
        S.default_seed(np.zeros((2, 2), np.int64))


def made_result(min_cells=2):
    """a result as sill_depth() makes it, from the definition in place of the device: the seed's basin, two basins behind sills one
    cell wide, a one-cell region, and a cut-off slope"""
    ny, nx = 4, 9
    depth = np.array([[50, 50, 3, 20, 20, 20, 2, 30, 30],
                      [50, 50, 0, 20, 20, 20, 0, 30, 1],
                      [0, 0, 0, 0, 0, 0, 0, 0, 0],
                      [9, 8, 7, 6, 5, 4, 3, 2, 1]], dtype=np.float64)
    q = S.quantise(depth, 1.0)
    wet = (q > 0).astype(np.uint8)
    wu, wv = S.cell_face_weights(q, False, False)
    raw = D.sill(wu, wv, [0], 0)
    x, y = np.meshgrid(np.arange(2 * nx + 1) * 0.5, np.arange(2 * ny + 1) * 0.5)
    res = S.result(raw, q, wet, [0], [None], x, y, False, False, 1.0, "cells", area=np.ones((ny, nx)), min_cells=min_cells)
    return res, depth


def test_the_result_and_the_basin_list():
    res, depth = made_result()
    assert res["sill_depth"][0, 0] == 50.0 and res["sill_depth"][0, 4] == 3.0 and res["sill_depth"][0, 7] == 2.0
    assert res["sill_depth"][3, 0] == 1.0e20 and res["reach"][3, 0] == 3 and res["reach"][2, 0] == 0 and res["reach"][0, 0] == 2
    assert res["reach"][0, 1] == 1 and res["counts"]["n_cut_off"] == 9
    assert [(k["sill_depth"], k["cells"]) for k in res["basins"]] == [(3.0, 7), (2.0, 4), (50.0, 3)]
    first = res["basins"][0]
    assert first["area_m2"] == 7.0 and first["deepest_cell"] == {"j": 0, "i": 3, "depth": 20.0} and first["n_gates"] == 1
    assert first["gates"] == [{"face": "u", "j": 0, "i": 2, "lon": 2.0, "lat": 0.5, "behind_region": 1, "behind_sill_depth": 50.0}]
    # the filter: the one-cell region (1, 8) is no basin at min_cells 2, and is one at 1
    assert [len(made_result(m)[0]["basins"]) for m in (1, 2, 4, 5, 8)] == [4, 3, 2, 1, 0]
    lines = S.summary_lines(res)
    assert "3 basins of at least 2 cells" in lines[0] and lines[1].startswith("   sill depth: sill 3.00 m, 7 cells, gate u(0, 2) at 2.0000, 0.5000")


def test_the_file_writer(tmp_path):
    res, _ = made_result()
    path = str(tmp_path / "sill_depth.nc")
    S.write_sill_depth(path, res)
    h = netcdf3.read_header(path)
    assert list(h.vars) == ["sill_depth", "reach", "region", "b", "gate_u", "gate_v"]
    assert h.vars["sill_depth"].shape == (4, 9) and h.vars["gate_u"].shape == (4, 10) and h.vars["gate_v"].shape == (5, 9)
    assert [h.vars[v].nc_type for v in h.vars] == [netcdf3.NC_DOUBLE, netcdf3.NC_BYTE, netcdf3.NC_INT, netcdf3.NC_INT, netcdf3.NC_BYTE,
                                                   netcdf3.NC_BYTE]
    g = h.gatts
    assert g["weights"] == "cells" and g["seeds"] == "0" and float(np.asarray(g["quantum"]).reshape(-1)[0]) == 1.0
    assert int(np.asarray(g["bits"]).reshape(-1)[0]) == 6
    back = netcdf3.read_doubles(path, names=("sill_depth",))["sill_depth"]
    assert back.tobytes() == res["sill_depth"].tobytes()
    b = np.frombuffer(netcdf3.read_var_bytes(path, h, "b", dtype=netcdf3.NC_INT), dtype=">i4").reshape(4, 9)
    assert np.array_equal(b, res["b"])
    S.write_report(str(tmp_path / "basins.json"), res)
    import json
    assert [k["cells"] for k in json.load(open(str(tmp_path / "basins.json")))["basins"]] == [7, 4, 3]


def test_every_flag_refusal():
    check = lambda **f: ogg._validate_all((), 0.0, -99.0, f.pop("skip_metrics", False), ogg.AnalysisFlags(**f))   # noqa: E731
    a = ogg.AnalysisFlags()
    assert a.sill_depth_file is None and a.sill_seed is None and a.sill_weights == "cells" and a.sill_min_cells == 16 and a.sill_report is None
    check(sill_depth_file="s.nc", topog_source="t.nc", skip_metrics=True)
    check(sill_depth_file="s.nc", topog_source="t.nc", ocean_mask_file="m.nc", sill_seed=[(10.0, -20.0)], sill_min_cells=4,
          sill_report="b.json")
    check(sill_depth_file="s.nc", topog_source="t.nc", sill_weights="faces", topog_faces_file="f.nc")
    for flags, text in (
            (dict(sill_seed=[(1.0, 2.0)]), "--sill_seed, --sill_weights, --sill_min_cells and --sill_report need --sill_depth_file"),
            (dict(sill_weights="faces"), "need --sill_depth_file"),
            (dict(sill_min_cells=3), "need --sill_depth_file"),
            (dict(sill_report="b.json"), "need --sill_depth_file"),
            (dict(sill_depth_file="s.nc"), "--sill_depth_file needs --topog_source"),
            (dict(sill_depth_file="s.nc", topog_source="t.nc", sill_weights="faces"), "--sill_weights faces needs --topog_faces_file"),
            (dict(sill_depth_file="s.nc", topog_source="t.nc", sill_weights="edges"), "--sill_weights must be cells or faces"),
            (dict(sill_depth_file="s.nc", topog_source="t.nc", sill_min_cells=0), "--sill_min_cells must be >= 1"),
            (dict(sill_depth_file="s.nc", topog_source="t.nc", sill_seed=[(10.0, 95.0)]), "--sill_seed needs a longitude and a latitude")):
        with pytest.raises(ValueError, match=text):
            check(**flags)
    p = ogg.build_parser().parse_args(["-r", "4", "--sill_depth_file", "s.nc", "--sill_seed", "1", "2", "--sill_seed", "3", "4",
                                       "--sill_weights", "faces", "--sill_min_cells", "5", "--sill_report", "r.json"])
    assert (p.sill_depth_file, p.sill_seed, p.sill_weights, p.sill_min_cells, p.sill_report) == ("s.nc", [[1.0, 2.0], [3.0, 4.0]], "faces", 5,
                                                                                                  "r.json")


def test_argument_refusals_need_no_device():
    assert S.params(3, 4, True, True, 30, 1) == (3, 4, 3, 30, 1, 0)
    for args, text in (((3, 4, False, False, 0, 1), "0 bits"), ((3, 4, False, False, 31, 1), "31 bits"), ((3, 4, False, False, 8, 0), "0 seeds"),
                       ((0, 4, False, False, 8, 1), "0 x 4 cells"), ((1 << 16, 1 << 15, False, False, 8, 1), "2\\^31")):
        with pytest.raises(ValueError, match=text):
            S.params(*args)
    with pytest.raises(ValueError, match="tile_rows 65"):
        S.params(3, 4, False, False, 8, 1, tile_rows=65)
    assert L.load().ogg_sill_workspace_bytes(1 << 16, 1 << 15) == -1 and L.load().ogg_sill_workspace_bytes(0, 5) == -1
    assert L.load().ogg_sill_workspace_bytes(3, 5) == 4 * 256
    assert not any("SILL" in k for k in L.ABI) and len(L.SILL_COUNT_FIELDS) == 7     # no struct: the table of size codes is unchanged
    with pytest.raises(ValueError, match="weights must be"):
        S.sill_depth(np.ones((2, 2)), np.zeros((5, 5)), np.zeros((5, 5)), weights="edges")
    with pytest.raises(ValueError, match="needs the face topography"):
        S.sill_depth(np.ones((2, 2)), np.zeros((5, 5)), np.zeros((5, 5)), weights="faces")
    with pytest.raises(ValueError, match="quantum must be > 0"):
        S.sill_depth(np.ones((2, 2)), np.zeros((5, 5)), np.zeros((5, 5)), quantum=0.0)
    with pytest.raises(ValueError, match="needs a supergrid of"):
        S.sill_depth(np.ones((2, 2)), np.zeros((4, 5)), np.zeros((4, 5)))

"""GPU tests of the distance to the coast (csrc/ogg_coast.hip, coast_distance.py, Supergrid.coast_distance) on generated grids: flag
bytes, coastal lists, nearest and d2 bit for bit against the definition in tests/coast_distance_definition.py run on the device's own
unit vectors (every cell at 1 degree; the coastal cells, 2000 random cells and the 100 farthest on the larger grids, where the indexed
search is also held to the brute-force one on every cell); the runoff mapping's search given the same queries and targets; the same
bits on two runs, for every knob and for any rank count; main(), the function-level path and the file command writing the same bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import coast_distance_definition as D
from test_gpu_runoff import stitched, wet_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE = 6371.0e3
KNOBS = ("OGG_COAST_BRUTE", "OGG_COAST_CUBES", "OGG_COAST_TILE_X", "OGG_COAST_TILE_Y", "OGG_COAST_CHUNK")
_CACHE = {}


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def computed(sg, name):
    """the grid ``name`` on one rank, its wet mask and the device result with the lists (computed once and left unchanged)"""
    if name not in _CACHE:
        from ocean_model_grid_generator_amd import coast_distance as CD
        plan, ranks, cut, out = stitched(sg, name)
        wet = wet_of(out["x"], out["y"])
        xy = ranks[0].stitched_xy(cut)
        res = CD.coast_distance_dev(xy[0], xy[1], wet, Re=RE, keep_lists=True)
        _CACHE[name] = (ranks[0], cut, out, wet, xy, res)
    return _CACHE[name]


def check_sets(res, out, wet):
    s = res["summary"]
    fl = D.flags(out["x"], out["y"], wet, s["periodic"], s["fold"])
    assert np.array_equal(res["flags"], fl)
    L, W = D.sets(fl)
    assert np.array_equal(res["land_cell"], L) and np.array_equal(res["wet_cell"], W) and L.size > 100 and W.size > 100
    assert res["land_u"].tobytes() == res["u"][L].tobytes() and res["wet_u"].tobytes() == res["u"][W].tobytes()
    lon, lat = D.centres(out["x"], out["y"])
    assert np.max(np.abs(res["u"] - D.unit(lon.reshape(-1), lat.reshape(-1)))) <= 4e-16   # within a few ulp of numpy's
    c = res["counts"]
    assert (c["coast_wet"], c["coast_land"], c["queries"], c["answered"]) == (W.size, L.size, fl.size, fl.size)
    assert np.array_equal(res["wet"], wet) and np.array_equal(res["coast"] != 0, D.coastal(wet, s["periodic"], s["fold"]))
    return fl, L, W


def test_device_equals_definition_on_every_cell_of_r1(sg):
    g, cut, out, wet, xy, res = computed(sg, "r1")
    assert res["summary"]["periodic"] and res["summary"]["fold"]
    fl, L, W = check_sets(res, out, wet)
    n, d2 = D.coast_distance(res["u"], fl)
    assert np.array_equal(res["nearest"], n) and res["d2"].tobytes() == d2.tobytes()
    assert res["counts"]["cubes"] > 0 and res["counts"]["tests"] < 0.25 * (fl.size * (L.size + W.size) / 2)   # the index prunes
    far = res["summary"]["farthest"]
    assert far["km"] * 1000.0 == pytest.approx(res["distance"][wet != 0].max(), rel=1e-14) and 1000.0 < far["km"] < 10000.0


@pytest.mark.parametrize("name", ["r2", "r2_dp", "r2_nosc", "om4"])
def test_larger_grids_against_definition_and_brute_force(sg, name, monkeypatch):
    from ocean_model_grid_generator_amd import coast_distance as CD
    g, cut, out, wet, xy, res = computed(sg, name)
    fl, L, W = check_sets(res, out, wet)
    rng = np.random.default_rng(11)
    only = np.unique(np.concatenate([L, W, rng.choice(fl.size, 2000, replace=False), np.argsort(res["d2"].reshape(-1))[-100:]]))
    n, d2 = D.coast_distance(res["u"], fl, only=only)
    assert np.array_equal(res["nearest"].reshape(-1)[only], n.reshape(-1)[only])
    assert res["d2"].reshape(-1)[only].tobytes() == d2.reshape(-1)[only].tobytes()
    monkeypatch.setenv("OGG_COAST_BRUTE", "1")
    brute = CD.coast_distance_dev(xy[0], xy[1], wet, Re=RE)
    assert brute["counts"]["cubes"] == 0 and brute["counts"]["tests"] > 20 * res["counts"]["tests"]
    assert brute["nearest"].tobytes() == res["nearest"].tobytes() and brute["d2"].tobytes() == res["d2"].tobytes()
    assert brute["distance"].tobytes() == res["distance"].tobytes()


def test_runoff_search_gives_the_same_answers(sg, hip):
    """the runoff mapping's ogg_runoff_search_dev fed the same query and target unit vectors: the same formula and the same key"""
    import torch
    L = hip
    g, cut, out, wet, xy, res = computed(sg, "r2")
    fl = res["flags"]
    nc = fl.size
    p = L.RunoffParams(ny=fl.shape[0], nx=fl.shape[1], NA=nc, NB=1, nrec=1, dtype=L.REMAP_FLOAT32, n_fill=0, topology=0,
                       targets=L.RUNOFF_WET, Re=RE)
    wsb = int(L.load().ogg_runoff_workspace_bytes(ctypes.byref(p)))
    assert wsb > 0
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    qw, ql = D.queries(fl)
    for q, tc, tu in ((qw, res["land_cell"], res["land_u"]), (ql, res["wet_cell"], res["wet_u"])):
        su, dtc, dtu = to(res["u"][q]), to(tc), to(tu)
        tgt = torch.empty(q.size, dtype=torch.int32, device="cuda:0")
        d2 = torch.empty(q.size, dtype=torch.float64, device="cuda:0")
        counts = torch.zeros(len(L.RUNOFF_COUNT_FIELDS), dtype=torch.int64, device="cuda:0")
        L.call("ogg_runoff_search_dev", ctypes.byref(p), dtc.data_ptr(), dtu.data_ptr(), tc.size, su.data_ptr(), q.size, ws.data_ptr(), wsb,
               tgt.data_ptr(), d2.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(tgt.cpu().numpy(), res["nearest"].reshape(-1)[q])
        assert d2.cpu().numpy().tobytes() == res["d2"].reshape(-1)[q].tobytes()


def test_same_bits_on_two_runs_and_for_every_knob(sg, monkeypatch):
    from ocean_model_grid_generator_amd import coast_distance as CD
    g, cut, out, wet, xy, want = computed(sg, "r2")
    settings = [{}] + [dict(OGG_COAST_TILE_X=a, OGG_COAST_TILE_Y=b) for a, b in (("8", "32"), ("32", "8"), ("256", "1"), ("1", "256"), ("5", "3"))]
    settings += [dict(OGG_COAST_CUBES=v) for v in ("1", "2", "7", "33", "128")] + [dict(OGG_COAST_CHUNK=v) for v in ("7", "64", "512")]
    for env in settings:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res = CD.coast_distance_dev(xy[0], xy[1], wet, Re=RE)
        for k in ("nearest", "d2", "flags", "distance"):
            assert res[k].tobytes() == want[k].tobytes(), (env, k)
        if "OGG_COAST_CUBES" in env:
            assert res["counts"]["cubes"] == int(env["OGG_COAST_CUBES"])
        if not env:
            assert res["summary"] == want["summary"]   # the counts too: the same work on the same input
        for k in env:
            monkeypatch.delenv(k)
    for sides, sel in (("wet", wet != 0), ("land", wet == 0)):
        res = CD.coast_distance_dev(xy[0], xy[1], wet, sides=sides, Re=RE)
        assert np.array_equal(res["nearest"][sel], want["nearest"][sel]) and res["d2"][sel].tobytes() == want["d2"][sel].tobytes()
        assert np.all(res["nearest"][~sel] == -1) and np.all(np.isposinf(res["d2"][~sel])) and np.all(res["distance"][~sel] == 1e20)
        assert res["counts"]["queries"] == int(sel.sum()) == res["counts"]["answered"]


def test_same_bits_for_any_rank_count(sg):
    want = computed(sg, "r2")[5]
    for world in (1, 2, 4):
        plan, ranks, cut, out = stitched(sg, "r2", world)
        wet = wet_of(out["x"], out["y"])
        res = ranks[0].coast_distance(cut, wet)
        assert all(g.coast_distance(cut, wet) is None for g in ranks[1:])
        for k in ("nearest", "d2", "flags", "distance", "nearest_j", "nearest_i"):
            assert res[k].tobytes() == want[k].tobytes(), (world, k)
        assert res["summary"] == want["summary"]


def test_main_function_level_and_file_command_write_the_same_bytes(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import read, synthetic_raster
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    names = ("grid", "topog", "t2", "c1", "c2", "c3", "tm", "tm2", "mask", "mask2", "m1", "m2", "m3", "land")
    f = {k: str(tmp_path / (k + ".nc")) for k in names}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], coast_distance_file=f["c1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], coast_distance_file=f["c2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert out.count("coast distance: the wet cell farthest from land") == 2 and out.index("topography:") < out.index("coast distance:")

    def command(*args):
        r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.coast_distance", f["grid"]] + list(args), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout
    assert "coast distance:" in command("--topog", f["topog"], "-o", f["c3"])
    b1 = open(f["c1"], "rb").read()
    assert b1 == open(f["c2"], "rb").read() and b1 == open(f["c3"], "rb").read()
    # with --ocean_mask_file the edited wet set is used: the lake and the sea behind the sill are land
    mk = dict(kw, mask_min_depth=10.0, skip_metrics=True)   # (the metrics are not needed)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm"], ocean_mask_file=f["mask"], coast_distance_file=f["m1"], **mk)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm2"], ocean_mask_file=f["mask2"], coast_distance_file=f["m2"], path="functions", **mk)
    capsys.readouterr()
    command("--mask", f["mask"], "-o", f["m3"])
    bm = open(f["m1"], "rb").read()
    assert bm == open(f["m2"], "rb").read() and bm == open(f["m3"], "rb").read() and bm != b1
    mask = read(f["mask"], "mask")
    assert np.array_equal(read(f["m1"], "wet"), (mask != 0).astype(np.int8)) and not np.array_equal(read(f["c1"], "wet"), read(f["m1"], "wet"))
    # the file holds what the definition gives on the grid and wet set as written
    g = netcdf3.read_doubles(f["grid"], names=("x", "y"))
    wet = read(f["c1"], "wet")
    fl, n, d2, _ = D.define(g["x"], g["y"], wet, True, True)
    assert np.array_equal(read(f["c1"], "coast") != 0, (fl & D.F_COAST) != 0)
    nx = wet.shape[1]
    got = read(f["c1"], "nearest_j").astype(np.int64) * nx + read(f["c1"], "nearest_i")
    same = got == n   # (numpy's unit vectors are not the device's to the last bit: a near tie may go the other way)
    assert same.mean() > 0.999
    dist = read(f["c1"], "distance").astype(np.float64)
    assert np.all(dist < 1e20) and np.allclose(dist[same], RE * 2 * np.arcsin(np.minimum(1, 0.5 * np.sqrt(d2[same]))), rtol=1e-9)
    command("--topog", f["topog"], "--sides", "land", "-o", f["land"])
    dl = read(f["land"], "distance").astype(np.float64)
    assert np.all(dl[wet != 0] == 1e20) and np.array_equal(dl[wet == 0], dist[wet == 0])


def test_struct_layout(hip):
    L = hip
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["COAST_PARAMS"]) == ctypes.sizeof(L.CoastParams) == 24
    assert lib.ogg_abi_sizeof(L.ABI["COAST_COUNTS"]) == ctypes.sizeof(L.CoastCounts) == 8 * len(L.COAST_COUNT_FIELDS)
    assert [L.CoastParams.ny.offset, L.CoastParams.nx.offset, L.CoastParams.topology.offset, L.CoastParams.sides.offset] == [0, 8, 16, 20]
    # the host-pointer entry fills the ctypes counts in the header's order
    from ocean_model_grid_generator_amd import coast_distance as CD
    import small_meshes as sm
    g = sm.latlon_grid(6, 7)
    wet = np.ones((6, 7), np.uint8)
    wet[2, 3] = 0
    c = CD.coast_distance(g["x"], g["y"], wet)["counts"]
    assert c == dict(coast_wet=4, coast_land=1, queries=42, answered=42, tests=41 + 4, tiles=1, cubes=1)

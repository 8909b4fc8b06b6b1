"""GPU tests of the ocean mask (csrc/ogg_mask.hip, ocean_mask.py, Supergrid.ocean_mask): every root bit-identical to the numpy
definition in tests/ocean_mask_definition.py on random wet sets around the percolation threshold, on edge shapes, on shapes around the
64 x 32 tile, under every combination of seam and fold, on a serpentine channel that fills a 1/8 degree grid, and under every setting
of the tile knob; main()'s --ocean_mask_file at 1 degree with a lake, a sea behind a sill and an open ocean, against the definition, the function path, the
file-based command and the virtual ranks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ocean_mask_definition as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_mask(depth, periodic=False, fold=False, min_depth=0.0, mode="mask", keep_min_cells=0, components=None):
    """ogg_ocean_mask with the topology given (no seeds): (root, depth, wet, counts); components: an int64 array that takes the
    component list, (cells << 32) | (INT32_MAX - root), largest first"""
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import ocean_mask as M
    d = np.ascontiguousarray(depth, dtype=np.float64)
    p = M.params(d.shape[0], d.shape[1], periodic, fold, min_depth, mode, keep_min_cells)
    root = np.empty(d.shape, np.int32)
    out = np.empty_like(d)
    wet = np.empty(d.shape, np.uint8)
    c = L.MaskCounts()
    L.call("ogg_ocean_mask", ctypes.byref(p), d.ctypes.data, None, None, 0, None, out.ctypes.data, wet.ctypes.data, root.ctypes.data,
           None, None if components is None else components.ctypes.data, 0 if components is None else components.size, ctypes.byref(c))
    return root, out, wet, {f: int(getattr(c, f)) for f in L.MASK_COUNT_FIELDS}


def check(wet_set, periodic=False, fold=False):
    d = np.where(wet_set, 100.0, 0.0)
    root, out, wet, counts = lib_mask(d, periodic, fold)
    want = D.ocean_mask(d, periodic=periodic, fold=fold)
    np.testing.assert_array_equal(root, want["root"])
    np.testing.assert_array_equal(out, want["depth"])
    np.testing.assert_array_equal(wet, want["wet"])
    assert counts["components"] == want["n_components"] and counts["removed"] == want["removed"]
    return root, counts


def serpentine(ny, nx):
    s = np.zeros((ny, nx), bool)
    s[::2] = True
    for k, j in enumerate(range(1, ny, 2)):
        s[j, nx - 1 if k % 2 == 0 else 0] = True
    return s


@pytest.mark.parametrize("density", [0.45, 0.5927, 0.7])
@pytest.mark.parametrize("periodic,fold", [(False, False), (True, False), (False, True), (True, True)])
def test_random_wet_sets_match_definition(hip, density, periodic, fold):
    rng = np.random.default_rng(int(density * 1e4) + 2 * periodic + fold)
    check(rng.random((301, 257)) < density, periodic, fold)


@pytest.mark.parametrize("shape", [(1, 1), (1, 1000), (1000, 1), (3, 3), (77, 129), (2196, 2880)])
def test_shapes_match_definition(hip, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for periodic, fold in ((False, False), (True, True)):
        check(rng.random(shape) < 0.5927, periodic, fold)


@pytest.mark.parametrize("ny", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("nx", [1, 2, 63, 64, 65, 129])
def test_shapes_around_the_tile_match_definition(hip, ny, nx):
    """one tile and the first cells of a second one in each direction; bands one and two cells wide, where the seam adds no face"""
    rng = np.random.default_rng(1000 * ny + nx)
    for periodic, fold in ((False, False), (True, True)):
        check(rng.random((ny, nx)) < 0.5927, periodic, fold)


@pytest.mark.parametrize("periodic,fold", [(False, False), (True, True)])
def test_all_wet_and_all_land(hip, periodic, fold):
    root, counts = check(np.ones((130, 200), bool), periodic, fold)
    assert counts["components"] == 1 and np.all(root == 0)
    root, counts = check(np.zeros((130, 200), bool), periodic, fold)
    assert counts["components"] == 0 and np.all(root == -1) and counts["kept"] == 0


def test_serpentine_channel_is_one_component(hip):
    s = serpentine(2196, 2880)
    root, counts = check(s, True, True)
    assert counts["components"] == 1 and np.all(root[s] == 0) and counts["wet_out"] == s.sum()


def test_same_bits_on_two_runs_and_every_tile_knob(hip, monkeypatch):
    rng = np.random.default_rng(11)
    d = np.where(rng.random((1100, 1500)) < 0.5927, rng.random((1100, 1500)) * 20.0, 0.0)
    first = lib_mask(d, True, True, min_depth=3.0)
    again = lib_mask(d, True, True, min_depth=3.0)
    for a, b in zip(first[:3], again[:3]):
        assert a.tobytes() == b.tobytes()
    want = D.ocean_mask(d, min_depth=3.0, periodic=True, fold=True)
    np.testing.assert_array_equal(first[0], want["root"])
    for rows in ("1", "7", "64"):
        monkeypatch.setenv("OGG_MASK_TILE_ROWS", rows)
        got = lib_mask(d, True, True, min_depth=3.0)
        for a, b in zip(first[:3], got[:3]):
            assert a.tobytes() == b.tobytes(), rows
    monkeypatch.setenv("OGG_MASK_TILE_ROWS", "65")
    with pytest.raises(Exception, match="OGG_MASK_TILE_ROWS"):
        lib_mask(d, True, True)


def test_seeds_keep_min_cells_and_device_entry(hip):
    """seeds through the host entry and the device-tensor entry: the same result as the definition"""
    import torch
    from ocean_model_grid_generator_amd import ocean_mask as M
    ny, nx = 60, 90
    X, Y = np.meshgrid(np.linspace(-300.0, 60.0, 2 * nx + 1), np.linspace(-80.0, 70.0, 2 * ny + 1))
    rng = np.random.default_rng(3)
    d = np.where(rng.random((ny, nx)) < 0.5, 50.0 + rng.random((ny, nx)), 0.0)
    want_root = D.roots(d > 0, True, False)
    big = np.bincount(want_root[want_root >= 0]).argmax()
    j, i = divmod(int(np.flatnonzero(want_root.ravel() == big)[0]), nx)
    seeds = [(float(X[2 * j + 1, 2 * i + 1]), float(Y[2 * j + 1, 2 * i + 1]))]
    for kw in (dict(), dict(seeds=seeds), dict(keep_min_cells=5), dict(seeds=seeds, keep_min_cells=3)):
        want = D.ocean_mask(d, X, Y, periodic=True, **kw)
        res = M.ocean_mask(d, X, Y, **kw)
        dev = M.ocean_mask_dev(torch.from_numpy(d).cuda(), torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), **kw)
        for r in (res, dev):
            np.testing.assert_array_equal(r["root"], want["root"])
            np.testing.assert_array_equal(r["depth"], want["depth"])
            np.testing.assert_array_equal(r["wet"], want["wet"])
            assert r["summary"]["periodic"] and not r["summary"]["fold"]
        assert res["summary"] == dev["summary"]
    land = np.flatnonzero(d.ravel() == 0)[0]
    j, i = divmod(int(land), nx)
    for f in (M.ocean_mask, lambda *a, **k: M.ocean_mask_dev(*[torch.from_numpy(v).cuda() for v in a], **k)):
        with pytest.raises(Exception, match="lies on land: cell \\(j, i\\) = \\(%d, %d\\) has depth 0" % (j, i)):
            f(d, X, Y, seeds=[(float(X[2 * j + 1, 2 * i + 1]), float(Y[2 * j + 1, 2 * i + 1]))])


# ---- main() at 1 degree ------------------------------------------------------------------------------------------
LAKE = (20.0, 30.0, 0.0, 10.0)      # lon0, lon1, lat0, lat1: a lake 50 m below sea level inside the continent
SEA = (38.0, 52.0, 18.0, 40.0)      # a sea 1000 m deep inside the continent ...
SILL = (52.0, 62.0, 27.0, 33.0)     # ... joined to the open ocean by a 5 m deep channel
CONTINENT = (0.0, 60.0, -30.0, 50.0)


def synthetic_raster(path):
    from ocean_model_grid_generator_amd import netcdf3
    lon = -180.0 + 0.25 * (np.arange(1440) + 0.5)
    lat = -90.0 + 0.25 * (np.arange(720) + 0.5)
    L, A = np.meshgrid(lon, lat)
    z = np.full(L.shape, -4000.0)
    inside = lambda b: (L >= b[0]) & (L < b[1]) & (A >= b[2]) & (A < b[3])   # noqa: E731
    z[inside(CONTINENT)] = 500.0
    z[inside(LAKE)] = -50.0
    z[inside(SEA)] = -1000.0
    z[inside(SILL)] = -5.0
    z[A > 84.0] = 300.0
    ds = netcdf3.Dataset(path, [("lat", lat.size), ("lon", lon.size)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], lat)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], lon)
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], z.astype(np.int16))
    ds.write()


def read(path, name):
    from ocean_model_grid_generator_amd import netcdf3
    h = netcdf3.read_header(path)
    v = h.vars[name]
    return np.frombuffer(netcdf3.read_var_bytes(path, h, name, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)


def centres_in(x, y, box):
    cx, cy = x[1::2, 1::2], y[1::2, 1::2]
    lon = (cx - box[0]) % 360.0 + box[0]
    return (lon > box[0] + 1) & (lon < box[1] - 1) & (cy > box[2] + 1) & (cy < box[3] - 1)


def test_main_removes_lake_and_sea_behind_sill(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "topog", "mask", "xg", "topog_d", "mask_d", "xg2")}
    ogg.main(1.0, gridfilename=f["grid"], no_changing_meta=True, ensure_nj_even=True, topog_source=src, topog_file=f["topog"],
             ocean_mask_file=f["mask"], mask_min_depth=10.0, xgrid_atm=(36, 18), xgrid_file=f["xg"])
    out = capsys.readouterr().out
    assert "ocean mask:" in out and "removed a basin of" in out
    assert out.index("topography:") < out.index("ocean mask:") < out.index("exchange grid:")
    g = netcdf3.read_doubles(f["grid"], names=("x", "y"))
    x, y = g["x"], g["y"]
    sampled = read(f["topog"], "depth_sampled").astype(np.float64)
    depth = read(f["topog"], "depth").astype(np.float64)
    mask = read(f["mask"], "mask").astype(np.float64)
    want = D.ocean_mask(sampled, x, y, min_depth=10.0, periodic=True, fold=True)
    np.testing.assert_array_equal(depth, want["depth"])
    np.testing.assert_array_equal(mask, want["wet"].astype(np.float64))
    lake, sea = centres_in(x, y, LAKE), centres_in(x, y, SEA)
    assert lake.sum() > 20 and sea.sum() > 100
    assert np.all(sampled[lake] > 0) and np.all(sampled[sea] > 0)
    assert np.all(mask[lake] == 0) and np.all(mask[sea] == 0) and np.all(depth[lake] == 0) and np.all(depth[sea] == 0)
    ocean = want["root"] == want["kept_roots"][0]
    assert ocean.sum() > 0.5 * (sampled > 0).sum()
    # the exchange grid lists no cell of a removed basin, and equals the file-based command on the edited topog.nc
    ocn = read(f["xg"], "tile2_cell").astype(np.int64) - 1
    assert np.all(mask[ocn[:, 1], ocn[:, 0]] == 1)
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.exchange_grid", f["grid"], "--atm", "36", "18", "--topog",
                        f["topog"], "-o", f["xg2"]], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(f["xg"], "rb").read() == open(f["xg2"], "rb").read()
    # --mask_deepen keeps the sea: its channel is deepened to 10 m
    ogg.main(1.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, topog_source=src, topog_file=f["topog_d"],
             ocean_mask_file=f["mask_d"], mask_min_depth=10.0, mask_deepen=True)
    capsys.readouterr()
    mask_d = read(f["mask_d"], "mask")
    depth_d = read(f["topog_d"], "depth").astype(np.float64)
    want_d = D.ocean_mask(sampled, x, y, min_depth=10.0, mode="deepen", periodic=True, fold=True)
    np.testing.assert_array_equal(depth_d, want_d["depth"])
    assert np.all(mask_d[sea] == 1) and np.all(mask_d[lake] == 0) and np.any(depth_d == 10.0)


def test_function_path_and_file_command_write_the_same_bytes(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "t_plain", "t1", "m1", "t2", "m2", "t3", "m3")}
    seeds = [[-150.0, 0.0], [45.0, 30.0]]
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src, mask_min_depth=10.0, mask_seed=seeds, mask_keep_cells=40)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["t1"], ocean_mask_file=f["m1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], ocean_mask_file=f["m2"], path="functions", **kw)
    ogg.main(1.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, topog_source=src, topog_file=f["t_plain"])
    out = capsys.readouterr().out
    assert "2 seeds" in out
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.ocean_mask", f["t_plain"], "--grid", f["grid"],
                        "--min_depth", "10", "--seed", "-150", "0", "--seed", "45", "30", "--keep_min_cells", "40", "-o", f["t3"],
                        "--mask", f["m3"], "--json", str(tmp_path / "s.json")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for a, b in (("t1", "t2"), ("m1", "m2"), ("t1", "t3"), ("m1", "m3")):
        assert open(f[a], "rb").read() == open(f[b], "rb").read(), (a, b)
    # the unmasked topog.nc is byte for byte what it was before the stage existed: no depth_sampled
    from ocean_model_grid_generator_amd import netcdf3
    assert "depth_sampled" not in netcdf3.read_header(f["t_plain"]).vars
    assert np.array_equal(read(f["t1"], "depth_sampled"), read(f["t_plain"], "depth"))


def test_same_result_for_any_rank_count(hip):
    import ocean_model_grid_generator_amd.supergrid as sg
    from ocean_model_grid_generator_amd import topography as T
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "src.nc")
        synthetic_raster(src)
        dev = T.DeviceSource(T.read_source(src), "cuda:0")
    plan = sg.SupergridPlan(inverse_resolution=1.0, ensure_nj_even=True)
    want = None
    for world in (1, 2, 4):
        ranks = []
        for r in range(world):
            ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
        for g in ranks:
            g.run_pass()
        cut = ranks[0].south_cut()
        topo = ranks[0].topography(cut, dev)
        res = ranks[0].ocean_mask(cut, topo, min_depth=10.0, seeds=[(-150.0, 0.0)])
        assert all(g.ocean_mask(cut, topo) is None for g in ranks[1:])
        if want is None:
            want = res
        else:
            for k in ("depth", "wet", "root"):
                assert res[k].tobytes() == want[k].tobytes(), (world, k)
            assert res["summary"] == want["summary"]

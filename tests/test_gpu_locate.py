"""GPU tests of point location (csrc/ogg_locate.hip, locate.py, Supergrid.locate / Supergrid.sample) on generated grids: the smallest
tripolar configuration of the suite (that of tests/golden/ref_small_r0.25_even.npz), with and without a displaced pole, held to the
definition in tests/locate_definition.py on the device's own corner table and query vectors, bit for bit and at every point; the same
bits for any rank count against locate() on the gathered arrays; main(), the function-level path and the file command writing the
same bytes, and main() without the new flag writing what it wrote."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import locate_inputs as LI
from test_locate_cpu import cut_queries

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"r025": dict(inverse_resolution=0.25, ensure_nj_even=True), "r025_dp": dict(inverse_resolution=0.25, ensure_nj_even=True, r_dp=0.2)}
KEYS = ("cell", "s", "t", "margin", "cell_j", "cell_i")
_CACHE = {}


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def device_grid(sg, name, world=1):
    plan = sg.SupergridPlan(**CONFIGS[name])
    ranks = []
    for r in range(world):
        ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
    for g in ranks:
        g.run_pass()
    return plan, ranks


def generated(sg, name):
    """the grid on one rank: its rank, cut, stitched host arrays and device points (computed once and left unchanged)"""
    if name not in _CACHE:
        plan, ranks = device_grid(sg, name)
        cut = ranks[0].south_cut()
        out = sg.stitch(plan, [g.bands_to_host() for g in ranks])
        _CACHE[name] = (ranks[0], cut, out, ranks[0].stitched_xy(cut))
    return _CACHE[name]


def queries(out, seed):
    lon, lat = cut_queries(dict(x=out["x"], y=out["y"], topology=(True, True)), seed)
    ll, la = LI.line_points(out["x"], out["y"], True)
    return np.concatenate([lon, ll, [np.nan, 10.0]]), np.concatenate([lat, la, [0.0, np.inf]])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_generated_grid_against_the_definition(sg, name):
    from ocean_model_grid_generator_amd import locate as LOC
    g, cut, out, xy = generated(sg, name)
    if name == "r025":
        gold = np.load(os.path.join(ROOT, "tests", "golden", "ref_small_r0.25_even.npz"))
        assert out["x"].shape == gold["x"].shape and np.abs(out["y"] - gold["y"]).max() < 1e-6
    ny, nx = LI.shape_of(out["x"])
    lon, lat = queries(out, 21)
    rng = np.random.default_rng(22)
    f = np.stack([np.cos(np.radians(out["y"][1::2, 1::2])) * (3 + r) + np.sin(np.radians(2 * out["x"][1::2, 1::2])) for r in range(3)])
    wet = (rng.random((ny, nx)) > 0.2).astype(np.uint8)
    res = LI.check(LOC, out["x"], out["y"], lon, lat, True, True, field=f.astype(np.float32), wet=wet, xy_dev=xy)
    assert np.all(res["cell"][:-2] >= 0) and np.all(res["cell"][-2:] == -1)
    assert res["summary"]["periodic"] and res["summary"]["fold"] and res["counts"]["cubes"] > 1
    # the cell's own centre returns that cell
    centre = np.zeros(out["x"].shape, bool)
    centre[1::2, 1::2] = True
    assert np.array_equal(res["cell"][np.nonzero(centre.reshape(-1))[0]], np.arange(ny * nx))


def test_same_bits_for_any_rank_count_and_on_the_gathered_arrays(sg):
    from ocean_model_grid_generator_amd import locate as LOC
    g, cut, out, xy = generated(sg, "r025_dp")
    lon, lat = queries(out, 23)
    ny, nx = LI.shape_of(out["x"])
    f = np.arange(ny * nx, dtype=np.float64).reshape(ny, nx)
    want = LOC.sample(out["x"], out["y"], lon, lat, f)
    for world in (1, 2):
        plan, ranks = device_grid(sg, "r025_dp", world)
        c = ranks[0].south_cut()
        res = ranks[0].sample(c, lon, lat, f)
        assert all(r.sample(c, lon, lat, f) is None for r in ranks[1:])
        assert all(res[k].tobytes() == want[k].tobytes() for k in KEYS), world
        assert res["samples"][0]["values"].tobytes() == want["samples"][0]["values"].tobytes()
        assert res["samples"][0]["flags"].tobytes() == want["samples"][0]["flags"].tobytes()
        only = ranks[0].locate(c, lon, lat)
        assert all(only[k].tobytes() == want[k].tobytes() for k in KEYS) and only["samples"] == []
        for k in ("located", "outside", "invalid", "large_cells", "cubes", "tests", "points", "shape"):
            assert res["summary"][k] == want["summary"][k], k


def test_main_function_level_and_file_command_write_the_same_bytes(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import read, synthetic_raster
    src = str(tmp_path / "src.nc")
    synthetic_raster(src)
    pts = str(tmp_path / "points.txt")
    with open(pts, "w") as fh:
        fh.write("# gauges and moorings\n-140.0 0.5 TAO\n10.25 -40.0\n-299.9 -60.0 seam\n60.0 89.5 fold\n30.0 30.0 on_land\n25.0 5.0 lake\n0 nan bad\n")
    names = ("grid", "topog", "t2", "p1", "p2", "p3", "p4", "g0", "t0", "tm", "tm2", "mask", "mask2", "m1", "m2", "m3")
    f = {k: str(tmp_path / (k + ".nc")) for k in names}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=src)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], locate_points=pts, locate_file=f["p1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], locate_points=pts, locate_file=f["p2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert out.count("locate: 7 points on") == 2 and out.count("point 6 (bad)") == 2 and out.index("topography:") < out.index("locate:")
    # without the flag the grid and the topography are the same bytes
    ogg.main(1.0, gridfilename=f["g0"], topog_file=f["t0"], **kw)
    assert open(f["g0"], "rb").read() == open(f["grid"], "rb").read() and open(f["t0"], "rb").read() == open(f["topog"], "rb").read()
    assert "locate:" not in capsys.readouterr().out

    def command(*args):
        r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.locate", f["grid"], pts] + list(args), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout
    assert "locate: 7 points on" in command("--topog", f["topog"], "-o", f["p3"])
    b1 = open(f["p1"], "rb").read()
    assert b1 == open(f["p2"], "rb").read() and b1 == open(f["p3"], "rb").read()
    cj, ci, wet, depth, flag = (read(f["p1"], k) for k in ("cell_j", "cell_i", "wet", "depth", "depth_locate_flag"))
    assert np.all(cj[:6] >= 0) and cj[6] == -1 and ci[6] == -1 and list(wet) == [1, 1, 1, 0, 0, 1, -1]
    assert list(flag) == [1, 1, 1, 3, 3, 1, 0] and np.all(depth[:3] > 3000.0) and np.all(depth[[3, 4, 6]] == 1e20) and 40.0 < depth[5] < 60.0
    from ocean_model_grid_generator_amd import netcdf3
    assert netcdf3.read_var_bytes(f["p1"], netcdf3.read_header(f["p1"]), "name", dtype=netcdf3.NC_CHAR).split(b"\0")[0] == b"TAO"
    x, y = read(f["grid"], "x"), read(f["grid"], "y")
    k = 0   # the point lies within the corners of its cell
    assert x[2 * cj[k], 2 * ci[k]] <= -140.0 <= x[2 * cj[k], 2 * ci[k] + 2] and y[2 * cj[k], 2 * ci[k]] <= 0.5 <= y[2 * cj[k] + 2, 2 * ci[k]]
    # --locate_mode cell, --skip_metrics and the edited wet set of --ocean_mask_file
    mk = dict(kw, mask_min_depth=10.0, skip_metrics=True, locate_mode="cell")
    ogg.main(1.0, gridfilename=None, topog_file=f["tm"], ocean_mask_file=f["mask"], locate_points=pts, locate_file=f["m1"], **mk)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm2"], ocean_mask_file=f["mask2"], locate_points=pts, locate_file=f["m2"],
             path="functions", **mk)
    capsys.readouterr()
    command("--topog", f["tm"], "--mode", "cell", "-o", f["m3"])
    bm = open(f["m1"], "rb").read()
    assert bm == open(f["m2"], "rb").read() and bm == open(f["m3"], "rb").read() and bm != b1
    command("--mask", f["mask"], "-o", f["p4"])                       # a mask alone: the wet byte, no depth
    assert np.array_equal(read(f["p4"], "wet"), read(f["m1"], "wet")) and list(read(f["m1"], "wet")) == [1, 1, 1, 0, 0, 0, -1]   # the lake is land
    assert "depth" not in netcdf3.read_header(f["p4"]).vars


def test_struct_layout(hip):
    L = hip
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["LOCATE_PARAMS"]) == ctypes.sizeof(L.LocateParams) == 64
    assert lib.ogg_abi_sizeof(L.ABI["LOCATE_COUNTS"]) == ctypes.sizeof(L.LocateCounts) == 8 * len(L.LOCATE_COUNT_FIELDS)
    P = L.LocateParams
    assert [P.ny.offset, P.nx.offset, P.n.offset, P.nrec.offset, P.topology.offset, P.mode.offset, P.dtype.offset, P.n_fill.offset,
            P.fill.offset] == [0, 8, 16, 24, 32, 36, 40, 44, 48]
    # a workspace that is too small, and a search without an index, are refused or answer nothing: never read out of bounds
    p = L.LocateParams(ny=4, nx=5, n=3, nrec=0, topology=0, mode=1, dtype=1, n_fill=0)
    assert lib.ogg_locate_workspace_bytes(ctypes.byref(p)) > 0
    assert lib.ogg_locate_sets_dev(ctypes.byref(p), 8, 8, 11, 8, 100, 8, 8, None) == L.OGG_EARG
    assert b"workspace of 100 bytes" in lib.ogg_last_error()

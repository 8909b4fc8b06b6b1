"""GPU tests of the sill depths in the pipeline: main() on both of its paths and the file command write the same sill_depth.nc bytes
(both weight modes, with and without the ocean mask) on the 1-degree tripolar grid of the other pipeline tests, whose synthetic raster
has a sea behind a 5 m sill; Supergrid.sill_depth gives the same bits on one and on three ranks; the file holds what the definition of
tests/sill_definition.py gives on the depth as written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sill_definition as D
from test_gpu_runoff import stitched, wet_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def depth_of(x, y):
    """a depth for every model cell: the wet set of the runoff tests, a smooth bottom with ties, and a shelf"""
    cx, cy = x[1::2, 1::2], y[1::2, 1::2]
    d = np.rint(3000.0 + 2000.0 * np.sin(np.radians(3.0 * cx)) * np.cos(np.radians(2.0 * cy)))
    d[(cy > 60.0) & (cy < 70.0)] = 37.5
    return np.where(wet_of(x, y) != 0, d, 0.0)


def test_same_bits_for_one_and_three_ranks(sg):
    want = None
    for world in (1, 3):
        plan, ranks, cut, out = stitched(sg, "r2", world)
        depth = depth_of(out["x"], out["y"])
        wet = wet_of(out["x"], out["y"])
        res = ranks[0].sill_depth(cut, depth, wet, seeds=[(-150.0, -30.0), (20.0, -50.0)], min_cells=4)
        assert all(g.sill_depth(cut, depth, wet, seeds=[(-150.0, -30.0)]) is None for g in ranks[1:])
        if want is None:
            want = res
            q = D.quantise(depth, 0.01)
            s = res["summary"]
            assert s["periodic"] and s["fold"] and len(s["seeds"]) == 2 and res["basins"] and res["basins"][0]["area_m2"] > 0.0
            wu, wv = D.cell_weights(q, wet, 3)
            ref = D.sill(wu, wv, [k["cell"] for k in s["seeds"]], 3)
            for k in ("b", "region", "gate_u", "gate_v"):
                assert np.array_equal(res[k], ref[k]), k
            assert res["counts"] == ref["counts"]
        for k in ("sill_depth", "reach", "region", "gate_u", "gate_v", "b"):
            assert res[k].tobytes() == want[k].tobytes(), (world, k)
        assert res["summary"] == want["summary"] and res["basins"] == want["basins"]


SEED = [(-150.0, -30.0)]
KW = dict(no_changing_meta=True, ensure_nj_even=True)


@pytest.fixture(scope="module")
def raster(hip, tmp_path_factory):
    from test_gpu_ocean_mask import synthetic_raster
    src = str(tmp_path_factory.mktemp("sill") / "src.nc")
    synthetic_raster(src)
    return src


def command(grid, *args):
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.sill_depth", grid] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def same_bytes(*paths):
    b = [open(p, "rb").read() for p in paths]
    assert all(v == b[0] for v in b[1:])
    return b[0]


def test_main_function_level_and_file_command_write_the_same_bytes(raster, tmp_path, capsys):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import read
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "topog", "t2", "s1", "s2", "s3")}
    rep = str(tmp_path / "basins.json")
    ogg.main(1.0, gridfilename=f["grid"], topog_source=raster, topog_file=f["topog"], sill_depth_file=f["s1"], sill_seed=SEED, sill_report=rep,
             **KW)
    ogg.main(1.0, gridfilename=None, topog_source=raster, topog_file=f["t2"], sill_depth_file=f["s2"], sill_seed=SEED, path="functions", **KW)
    out = capsys.readouterr().out
    assert out.count("sill depth: ") >= 2 and out.index("topography:") < out.index("sill depth:")
    assert "sill depth:" in command(f["grid"], "--topog", f["topog"], "--seed", "-150", "-30", "-o", f["s3"])
    same_bytes(f["s1"], f["s2"], f["s3"])
    # the file holds what the definition gives on the depth as written
    depth = read(f["topog"], "depth").astype(np.float64)
    q = D.quantise(depth, 0.01)
    b = read(f["s1"], "b").astype(np.int32)
    seeds = np.flatnonzero(b.reshape(-1) == D.SEED)
    assert seeds.size == 1
    wu, wv = D.cell_weights(q, q > 0, 3)
    ref = D.sill(wu, wv, seeds, 3)
    assert np.array_equal(b, ref["b"]) and np.array_equal(read(f["s1"], "region").astype(np.int32), ref["region"])
    assert np.array_equal(read(f["s1"], "gate_u").astype(np.uint8), ref["gate_u"])
    assert np.array_equal(read(f["s1"], "gate_v").astype(np.uint8), ref["gate_v"])
    sd = read(f["s1"], "sill_depth").astype(np.float64)
    assert np.array_equal(sd[(b > 0) & (b < D.SEED)], b[(b > 0) & (b < D.SEED)] * 0.01) and np.all(sd[b == 0] == 1.0e20)
    # the sea behind the 5 m sill is a basin whose sill depth is that of the sill's cells, far below its own depth; the lake is cut off
    basins = json.load(open(rep))["basins"]
    shallow = [k for k in basins if k["sill_depth"] <= 10.0 and k["deepest_cell"]["depth"] >= 500.0]
    assert shallow and all(k["gates"] and k["area_m2"] > 0.0 for k in shallow)
    assert np.any(read(f["s1"], "reach") == 3)


def test_main_with_face_weights(raster, tmp_path, capsys):
    """faces: main() needs --topog_faces_file in the same call; the file command reads the file it wrote"""
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "topog", "t2", "f1", "f2", "sf1", "sf2", "sf3", "sc")}
    fk = dict(KW, topog_source=raster, sill_weights="faces", sill_seed=SEED)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], topog_faces_file=f["f1"], sill_depth_file=f["sf1"], **fk)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], topog_faces_file=f["f2"], sill_depth_file=f["sf2"], path="functions", skip_metrics=True,
             **fk)   # (allowed: the areas are left out of the report, the file is the same)
    capsys.readouterr()
    command(f["grid"], "--topog", f["topog"], "--faces", f["f1"], "--weights", "faces", "--seed", "-150", "-30", "-o", f["sf3"])
    command(f["grid"], "--topog", f["topog"], "--seed", "-150", "-30", "-o", f["sc"])
    assert same_bytes(f["sf1"], f["sf2"], f["sf3"]) != open(f["sc"], "rb").read()


def test_main_with_the_ocean_mask(raster, tmp_path, capsys):
    """with --ocean_mask_file the edited depth and wet set are used: the sea behind the sill is land"""
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from test_gpu_ocean_mask import read
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "tm", "tm2", "mask", "mask2", "m1", "m2", "m3")}
    mk = dict(KW, topog_source=raster, mask_min_depth=10.0, sill_seed=SEED)
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["tm"], ocean_mask_file=f["mask"], sill_depth_file=f["m1"], **mk)
    ogg.main(1.0, gridfilename=None, topog_file=f["tm2"], ocean_mask_file=f["mask2"], sill_depth_file=f["m2"], path="functions",
             skip_metrics=True, **mk)
    capsys.readouterr()
    command(f["grid"], "--mask", f["mask"], "--topog", f["tm"], "--seed", "-150", "-30", "-o", f["m3"])
    same_bytes(f["m1"], f["m2"], f["m3"])
    assert np.array_equal(read(f["m1"], "reach") != 0, read(f["mask"], "mask") != 0) and not np.any(read(f["m1"], "reach") == 3)

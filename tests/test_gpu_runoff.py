"""GPU tests of the runoff mapping (csrc/ogg_runoff.hip, runoff.py, Supergrid.runoff): values, n_sources, targets and distances bit
for bit against the definition in tests/runoff_definition.py run on the device's own unit vectors, for the remap tests' grids, float32
and fp64 sources with missing values and both target modes; the device's unit vectors within a few ulp of numpy's; the indexed search
equal to the brute-force one for every bin count on adversarial sources; the same bits for any rank count and on two runs;
conservation; main(), the function-level path and the file command writing the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import runoff_definition as D
from test_gpu_remap import device_grid, edges

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE = 6371.0e3


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def wet_of(x, y):
    """a wet mask of the model cells: two continents, an island row on the seam and land north of 80N and next to the fold"""
    cx, cy = x[1::2, 1::2] % 360, y[1::2, 1::2]
    land = (((cx > 100) & (cx < 140) & (cy > -20) & (cy < 30)) | ((cx > 250) & (cx < 300) & (cy > 10) & (cy < 60)) | (cy > 80)
            | ((cx > 55) & (cx < 65) & (cy > -40) & (cy < -30)))
    wet = (~land).astype(np.uint8)
    wet[-1, : wet.shape[1] // 8] = 0
    return wet


def field(lon, lat, nrec, dtype, prob, seed=0):
    """sparse positive records with NaN and -999 holes"""
    rng = np.random.default_rng(seed)
    NB, NA = lat.size - 1, lon.size - 1
    f = np.where(rng.random((nrec, NB, NA)) < prob, rng.random((nrec, NB, NA)) * 1e-4, 0.0).astype(dtype)
    f[rng.random((nrec, NB, NA)) < 0.02] = np.nan
    f[rng.random((nrec, NB, NA)) < 0.02] = -999.0
    return f


def stitched(sg, name, world=1):
    plan, ranks = device_grid(sg, name, world)
    cut = ranks[0].south_cut()
    out = sg.stitch(plan, [g.bands_to_host() for g in ranks])
    return plan, ranks, cut, out


def check_against_definition(res, src, wet, out, mode):
    from ocean_model_grid_generator_amd import runoff as RO
    s = res["summary"]
    x, y = out["x"], out["y"]
    want_t = np.nonzero(D.targets(wet, s["periodic"], s["fold"], mode).reshape(-1))[0]
    assert np.array_equal(res["tgt_cell"], want_t)
    # the device's unit vectors and ds_J within a few ulp of numpy's
    tu_np = D.unit(x[1::2, 1::2].reshape(-1)[want_t], y[1::2, 1::2].reshape(-1)[want_t])
    assert np.max(np.abs(res["tgt_u"] - tu_np), initial=0.0) <= 4e-16
    mapped, skipped, missing = D.classify(src.records, src.fill)
    sc = np.nonzero(mapped)[0]
    assert np.array_equal(res["src_cell"], sc)
    J, I = np.divmod(sc, src.lon.size - 1)
    su_np = D.unit((src.lon[I] + src.lon[I + 1]) / 2.0, (src.lat[J] + src.lat[J + 1]) / 2.0)
    assert np.max(np.abs(res["src_u"] - su_np), initial=0.0) <= 4e-16
    assert np.max(np.abs(res["ds"] - D.ds_of(src.lat)) / np.abs(D.ds_of(src.lat))) <= 4e-16
    c = res["counts"]
    assert (c["mapped"], c["skipped"], c["missing"], c["targets"]) == (mapped.sum(), skipped.sum(), missing.sum(), want_t.size)
    v, n, _, tgt, dd = D.runoff(src.records, src.fill, src.lon, src.lat, res["ds"], RE, res["src_u"], res["tgt_u"], res["tgt_cell"],
                                out["area"])
    assert np.array_equal(res["src_target"], tgt) and res["src_d2"].tobytes() == dd.tobytes()
    assert res["values"].tobytes() == v.reshape(res["values"].shape).tobytes()
    assert np.array_equal(res["n_sources"], n)
    assert c["cells"] == int((n > 0).sum()) and c["max_sources"] == int(n.max())
    assert max(s["conservation"]) <= 1e-12, s["conservation"]
    assert np.array_equal(res["area"], RO.cell_area(out["area"]))


CASES = [("regular", np.float32, "coast", 0.05), ("gaussian", np.float64, "coast", 0.05), ("regular", np.float64, "wet", 0.005),
         ("gaussian", np.float32, "wet", 0.005)]


@pytest.mark.parametrize("name", ["r1", "r2", "r2_dp", "r2_nosc", "om4"])
def test_device_equals_definition(sg, name):
    import torch
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    plan, ranks, cut, out = stitched(sg, name)
    g = ranks[0]
    wet = wet_of(out["x"], out["y"])
    xy, area = g.stitched_xy(cut), g.stitched_area(cut)
    assert xy[0].cpu().numpy().tobytes() == out["x"].tobytes() and area.cpu().numpy().tobytes() == out["area"].tobytes()
    for k, (kind, dtype, mode, prob) in enumerate(CASES):
        lon, lat = edges(kind)
        src = R.Source(field(lon, lat, 3, dtype, prob, seed=k), lon, lat, fill=(-999.0,))
        res = RO.runoff_dev(xy[0], xy[1], area, src, wet, targets=mode, Re=RE, keep_lists=True)
        check_against_definition(res, src, wet, out, mode)
        assert res["counts"]["mapped"] > 100
        via = g.runoff(cut, src, wet, targets=mode)
        assert via["values"].tobytes() == res["values"].tobytes() and np.array_equal(via["n_sources"], res["n_sources"])
    torch.cuda.synchronize()


def adversarial_sources(out):
    """sources whose centres lie midway between model cells, in rows reaching the poles, on the seam and next to the fold"""
    from ocean_model_grid_generator_amd import remap as R
    x, y = out["x"], out["y"]
    lon0 = float(x[0, 0])
    cy = y[1::2, 1::2][:, 0]
    srcs = []
    # 1: a 1-degree source whose centres fall halfway between the 1-degree model centres in longitude and on the equator rows
    lon = lon0 + np.arange(361.0)
    lat = np.r_[-90.0, np.arange(-89.0, 90.0, 1.0) + 0.5, 90.0]
    lat = np.unique(np.clip(lat, -90, 90))
    f = np.ones((1, lat.size - 1, 360))
    srcs.append(R.Source(f, lon, lat, name="midway"))
    # 2: thin polar rows (centres within 5e-4 degrees of the poles), everything mapped
    lat = np.r_[-90.0, -89.999, np.linspace(-89.0, 89.0, 90), 89.999, 90.0]
    srcs.append(R.Source(np.ones((2, lat.size - 1, 180)), np.linspace(lon0, lon0 + 360.0, 181), lat, name="poles"))
    # 3: centres on the seam meridian (lon0) and on the rows next to the fold
    lon = lon0 - 0.25 + 0.5 * np.arange(721)
    top = float(cy[-1])
    lat = np.r_[-90.0, np.linspace(min(top, 89.0) - 3.0, min(top + 0.5, 89.9), 15), 90.0]
    f = np.zeros((1, lat.size - 1, 720))
    f[0, :, 0] = 1.0
    f[0, :, 360] = 2.0
    f[0, -5:-1, :] = 3.0
    srcs.append(R.Source(f, lon, lat, name="seam_fold"))
    return srcs


def test_indexed_search_equals_brute_force_for_every_bin_count(sg, monkeypatch):
    from ocean_model_grid_generator_amd import runoff as RO
    plan, ranks, cut, out = stitched(sg, "r2")
    g = ranks[0]
    xy, area = g.stitched_xy(cut), g.stitched_area(cut)
    wet = wet_of(out["x"], out["y"])
    # a whole continent of runoff: every 1-degree source cell over the two land boxes maps somewhere, most to the few coastal cells
    # of a land mass with a short coast (thousands of sources in one segment)
    cont = wet.copy()
    ny, nx = cont.shape
    cont[ny // 8: 7 * ny // 8, :] = 0
    cont[ny // 2, nx // 2] = 1   # a one-cell lake: the only coast for thousands of sources
    lon, lat = edges("regular")
    from ocean_model_grid_generator_amd import remap as R
    whole = R.Source(np.ones((2, 180, 360)), lon, lat, name="continent")
    cases = [(s, wet, "coast") for s in adversarial_sources(out)] + [(whole, cont, "coast"), (whole, cont, "wet")]
    for src, w, mode in cases:
        monkeypatch.setenv("OGG_RUNOFF_BRUTE", "1")
        want = RO.runoff_dev(xy[0], xy[1], area, src, w, targets=mode, Re=RE, keep_lists=True)
        monkeypatch.delenv("OGG_RUNOFF_BRUTE")
        assert want["counts"]["bins"] == 0
        if mode == "coast":   # (the definition's brute force over every wet cell is too slow in numpy here)
            check_against_definition(want, src, w, out, mode)
        for bins in ("1", "2", "7", "33", "160", None):
            if bins is not None:
                monkeypatch.setenv("OGG_RUNOFF_BINS", bins)
            res = RO.runoff_dev(xy[0], xy[1], area, src, w, targets=mode, Re=RE)
            for k in ("src_target", "src_d2", "values", "n_sources"):
                assert res[k].tobytes() == want[k].tobytes(), (src.name, mode, bins, k)
            assert bins is None or res["counts"]["bins"] == int(bins)
            monkeypatch.delenv("OGG_RUNOFF_BINS", raising=False)
        if src is whole and mode == "coast":
            assert want["counts"]["max_sources"] > 1000, want["counts"]["max_sources"]


def test_same_bits_for_any_rank_count_and_on_two_runs(sg):
    from ocean_model_grid_generator_amd import remap as R
    lon, lat = edges("gaussian")
    src = R.Source(field(lon, lat, 2, np.float32, 0.05), lon, lat, fill=(-999.0,))
    want = None
    for world in (1, 2, 4):
        plan, ranks, cut, out = stitched(sg, "r2", world)
        wet = wet_of(out["x"], out["y"])
        res = ranks[0].runoff(cut, src, wet)
        assert all(g.runoff(cut, src, wet) is None for g in ranks[1:])
        if want is None:
            want = res
            again = ranks[0].runoff(cut, src, wet)
            assert again["values"].tobytes() == res["values"].tobytes()
        for k in ("values", "n_sources", "src_target", "src_d2"):
            assert res[k].tobytes() == want[k].tobytes(), (world, k)
        assert res["summary"] == want["summary"]


def test_empty_target_set_is_refused(sg):
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    plan, ranks, cut, out = stitched(sg, "r1")
    lon, lat = edges("regular")
    src = R.Source(field(lon, lat, 1, np.float64, 0.05), lon, lat, fill=(-999.0,))
    dry = np.zeros(((out["x"].shape[0] - 1) // 2, (out["x"].shape[1] - 1) // 2), np.uint8)
    with pytest.raises(ValueError, match="no target cell"):
        RO.runoff(out["x"], out["y"], out["area"], src, dry)
    with pytest.raises(ValueError, match="no target cell"):
        ranks[0].runoff(cut, src, dry)
    nothing = R.Source(np.zeros((1, 180, 360)), lon, lat)
    res = RO.runoff(out["x"], out["y"], out["area"], nothing, dry)
    assert res["counts"]["mapped"] == 0 and not res["values"].any() and not np.signbit(res["values"]).any()


def write_sources(tmp_path):
    """a bathymetry raster and a runoff source with an unlimited time axis and two record variables, NetCDF-3"""
    from scipy.io import netcdf_file
    from test_gpu_remap import write_sources as remap_sources
    topo, _ = remap_sources(tmp_path)
    src = str(tmp_path / "jra.nc")
    lo, la = -180.0 + 0.5 * (np.arange(720) + 0.5), -90.0 + 0.5 * (np.arange(360) + 0.5)
    L, A = np.meshgrid(lo, la)
    land = ((L > 0) & (L < 60) & (A > -30) & (A < 50)) | (A > 84)
    rng = np.random.default_rng(3)
    with netcdf_file(src, "w", version=2) as nc:
        nc.createDimension("time", None)
        nc.createDimension("lat", 360)
        nc.createDimension("lon", 720)
        t = nc.createVariable("time", "d", ("time",))
        t.units = "days since 1958-01-01"
        a = nc.createVariable("lat", "d", ("lat",))
        a.units = "degrees_north"
        a[:] = la
        b = nc.createVariable("lon", "d", ("lon",))
        b.units = "degrees_east"
        b[:] = lo
        v = nc.createVariable("friver", "f", ("time", "lat", "lon"))
        v.units = "kg m-2 s-1"
        v._FillValue = np.float32(1e20)
        w = nc.createVariable("licalvf", "f", ("time", "lat", "lon"))
        w.units = "kg m-2 s-1"
        for r in range(3):
            t[r] = 15.0 + 30.0 * r
            v[r] = np.where(land & (rng.random(land.shape) < 0.3), rng.random(land.shape) * 1e-3, 0.0).astype(np.float32)
            w[r] = np.where(np.abs(A) > 60, 1e-5 * (r + 1), 0.0).astype(np.float32)
    return topo, src


def test_main_function_level_and_file_command_write_the_same_bytes(hip, tmp_path, capsys):
    from scipy.io import netcdf_file
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    topo, src = write_sources(tmp_path)
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "topog", "o1", "o2", "o3", "t2")}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=topo, runoff_source=src, runoff_var=["friver", "licalvf"])
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], runoff_file=f["o1"], **kw)
    ogg.main(1.0, gridfilename=None, topog_file=f["t2"], runoff_file=f["o2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert "runoff: friver, 3 records" in out and "runoff: licalvf, 3 records" in out
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.runoff", f["grid"], src, "--var", "friver", "--var", "licalvf",
                        "--topog", f["topog"], "-o", f["o3"]], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    b1 = open(f["o1"], "rb").read()
    assert b1 == open(f["o2"], "rb").read() and b1 == open(f["o3"], "rb").read()
    with netcdf_file(f["o1"], "r", mmap=False) as nc:
        assert nc.dimensions["time"] is None and nc.variables["friver"].shape[0] == 3
        n = nc.variables["n_sources"][:]
        depth = netcdf_file(f["topog"], "r", mmap=False).variables["depth"][:]
        wet = (depth > 0) & (depth != 1e20)
        assert n.sum() > 0 and np.all(n[~wet] == 0)
        v = np.array(nc.variables["friver"][:])
        assert np.all(v[:, ~wet] == 0) and np.all(v >= 0)

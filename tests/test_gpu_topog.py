"""GPU tests of topography by refined sampling (csrc/ogg_topog.hip, topography.py, Supergrid.topography): every integer of every
record bit-identical to the numpy definition in tests/topog_definition.py on generated grids and three kinds of raster, the refine
override and the clamp, independence of the rank split, main()'s --topog_source against the file-based command, and the cost at
1/8 degree."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import topog_definition as td

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = td.RECORD_FIELDS


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def raster(kind):
    """(data, box, fill): a periodic int16 raster (0.25 deg), a regional float64 raster with fill values (0.2 deg, lon -100 .. 20,
    lat -80 .. 60), a periodic float32 raster (0.5 deg) with NaN and a _FillValue."""
    if kind == "int16":
        lon = -180.0 + 0.25 * (np.arange(1440) + 0.5)
        lat = -90.0 + 0.25 * (np.arange(720) + 0.5)
        z = 4000.0 * np.sin(np.radians(3 * lon))[None, :] * np.cos(np.radians(2 * lat))[:, None] - 1500.0
        h = (np.arange(720)[:, None] * 7919 + np.arange(1440)[None, :] * 104729) % 301 - 150
        return (z + h).astype(np.int16), (-180.0, 0.25, -90.0, 0.25), ()
    if kind == "float64_regional":
        lon = -100.0 + 0.2 * (np.arange(600) + 0.5)
        lat = -80.0 + 0.2 * (np.arange(700) + 0.5)
        z = 2500.0 * np.cos(np.radians(4 * lon))[None, :] * np.sin(np.radians(3 * lat))[:, None] - 800.123
        z[::17, ::13] = -99999.0
        return z, (-100.0, 0.2, -80.0, 0.2), (-99999.0,)
    lon = -180.0 + 0.5 * (np.arange(720) + 0.5)
    lat = -90.0 + 0.5 * (np.arange(360) + 0.5)
    z = (3000.0 * np.sin(np.radians(2 * lon))[None, :] * np.cos(np.radians(lat))[:, None] - 500.0).astype(np.float32)
    z[5::23, 7::29] = np.nan
    z[11::31, 3::37] = 1.0e30
    return z, (-180.0, 0.5, -90.0, 0.5), (1.0e30,)


CONFIGS = {
    "r1": dict(inverse_resolution=1.0, ensure_nj_even=True),
    "r2": dict(inverse_resolution=2.0, ensure_nj_even=True),
    "r2_dp": dict(inverse_resolution=2.0, r_dp=0.2, ensure_nj_even=True),
    "r2_nosc": dict(inverse_resolution=2.0, no_south_cap=True, ensure_nj_even=True),
    "om4": dict(inverse_resolution=4.0, r_dp=0.2, south_cutoff_row=83, ensure_nj_even=True),
}


def device_grid(sg, name, world=1):
    plan = sg.SupergridPlan(**CONFIGS[name])
    ranks = []
    for r in range(world):
        ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
    for g in ranks:
        g.run_pass()
    return plan, ranks


def assert_records_equal(got, want):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f].astype(np.int64), want[f], err_msg=f)


@pytest.mark.parametrize("name,kind", [("r1", "int16"), ("r2", "int16"), ("r2_dp", "int16"), ("r2_nosc", "float64_regional"),
                                       ("om4", "float32"), ("r2_dp", "float64_regional"), ("r1", "float32")])
def test_pipeline_records_match_definition(sg, name, kind):
    from ocean_model_grid_generator_amd import topography as T
    plan, ranks = device_grid(sg, name)
    g = ranks[0]
    cut = g.south_cut()
    data, box, fill = raster(kind)
    src = T.Source(data, *box, fill=fill)
    res = g.topography(cut, T.DeviceSource(src, "cuda:0"))
    out = sg.stitch(plan, [g.bands_to_host()])
    want = td.records(out["x"], out["y"], data, *box, fill=fill)
    assert_records_equal(res["records"], want)
    ref = T.fields_from_records(res["records"], src.quantum)
    for k in ("height", "h_std", "h_min", "h_max", "wet_fraction", "depth", "n_samples"):
        assert res[k].tobytes() == ref[k].tobytes(), k
    assert res["summary"]["n_samples"] == int((want["n"] + want["n_missing"]).sum())
    # the host-array entry gives the same records
    host = T.topography(out["x"], out["y"], src)
    assert host["records"].tobytes() == res["records"].tobytes()


def test_supergrid_cells_and_odd_rows(sg):
    """Without --ensure_nj_even, cutting one more south row flips the parity of ny: of south_cutoff_row 1 and 2 one gives an odd
    number of supergrid rows.  On that grid supergrid cells match the definition and model cells are refused with a pointer to
    --ensure_nj_even."""
    from ocean_model_grid_generator_amd import topography as T
    data, box, fill = raster("int16")
    src = T.Source(data, *box)
    grids = []
    for cut_rows in (1, 2):
        plan = sg.SupergridPlan(inverse_resolution=2.0, r_dp=0.2, south_cutoff_row=cut_rows)
        g = sg.Supergrid(plan, device="cuda:0")
        g.run_pass()
        grids.append((plan, g, g.stitched_rows(g.south_cut()) - 1))
    odd = [t for t in grids if t[2] % 2 == 1]
    assert odd, [t[2] for t in grids]
    plan, g, ny = odd[0]
    out = sg.stitch(plan, [g.bands_to_host()])
    assert out["x"].shape[0] - 1 == ny
    res = g.topography(g.south_cut(), T.DeviceSource(src, "cuda:0"), cells="supergrid")
    assert_records_equal(res["records"], td.records(out["x"], out["y"], data, *box, cells_="supergrid"))
    with pytest.raises(ValueError, match="ensure_nj_even"):
        g.topography(g.south_cut(), T.DeviceSource(src, "cuda:0"))


def test_pole_enclosing_cells_on_the_device(sg, capsys):
    """The kernel's pole branch against the definition: a hand-built cell around the south pole (the CPU test's), and the
    displaced-pole southern cap, where the geographic pole lies inside a cell."""
    from ocean_model_grid_generator_amd import topography as T
    raw = np.arange(180 * 360).reshape(180, 360).astype(np.float64)
    x, y = np.array([[0.0, 90.0], [270.0, 180.0]]), np.full((2, 2), -89.0)
    for refine in (None, 4):
        res = T.topography(x, y, raw, -180.0, 1.0, -90.0, 1.0, quantum=1.0, cells="supergrid", refine=refine)
        assert res["summary"]["n_pole_cells"] == 1
        assert_records_equal(res["records"], td.records(x, y, raw, -180.0, 1.0, -90.0, 1.0, quantum=1.0, cells_="supergrid",
                                                       refine=refine))
    # the generated caps: each pole is either a grid point (its cells take the row neighbour's longitude) or inside exactly one cell
    data, box, fill = raster("int16")
    for name in ("r2_dp", "om4", "r2"):
        plan, ranks = device_grid(sg, name)
        g = ranks[0]
        res = g.topography(g.south_cut(), T.DeviceSource(T.Source(data, *box), "cuda:0"), cells="supergrid")
        out = sg.stitch(plan, [g.bands_to_host()])
        y = out["y"]
        on_point = [bool(np.any(y >= 90.0 - td.POLE_EPS)), bool(np.any(y <= -90.0 + td.POLE_EPS))]
        c = td.cells(out["x"], y, box[1], box[3])
        inside = [int(np.sum(c["pole"] > 0)), int(np.sum(c["pole"] < 0))]
        with capsys.disabled():
            print("\n%s: north pole a grid point %s, in %d cells; south pole a grid point %s, in %d cells; max |y| of the southmost row %.12g"
                  % (name, on_point[0], inside[0], on_point[1], inside[1], float(np.abs(y[0]).max())))
        assert res["summary"]["n_pole_cells"] == inside[0] + inside[1]
        for k in range(2):
            if y.min() < -89.0 if k else y.max() > 89.0:   # the cap reaches the pole's neighbourhood
                assert inside[k] <= 1
        assert_records_equal(res["records"], td.records(out["x"], y, data, *box, cells_="supergrid"))


def test_refine_override_and_clamp(sg):
    from ocean_model_grid_generator_amd import topography as T
    plan, ranks = device_grid(sg, "r1")
    out = sg.stitch(plan, [ranks[0].bands_to_host()])
    x, y = out["x"][:41], out["y"][:41]
    data, box, fill = raster("int16")
    for kw in (dict(refine=5), dict(refine=1), dict(oversample=300.0)):
        res = T.topography(x, y, data, *box, **kw)
        assert_records_equal(res["records"], td.records(x, y, data, *box, **kw))
    assert res["summary"]["R_max"] == 256 and res["summary"]["n_clamped_cells"] > 0
    with pytest.raises(Exception, match="2\\^21|exceeds"):
        T.topography(x, y, np.full((180, 360), 1.0e5, dtype=np.float32), -180.0, 1.0, -90.0, 1.0, quantum=0.01)


@pytest.mark.parametrize("name", ["r2_dp", "om4"])
def test_same_bits_for_any_rank_count(sg, name):
    from ocean_model_grid_generator_amd import topography as T
    data, box, fill = raster("int16")
    src = T.Source(data, *box)
    dev = T.DeviceSource(src, "cuda:0")
    want = None
    for world in (1, 2, 4):
        plan, ranks = device_grid(sg, name, world=world)
        res = ranks[0].topography(ranks[0].south_cut(), dev)
        for other in ranks[1:]:
            assert other.topography(other.south_cut(), dev) is None
        if want is None:
            want = res
        else:
            assert res["records"].tobytes() == want["records"].tobytes(), world
            assert res["summary"] == want["summary"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, q):
    """One rank of an N-rank run on cuda:0 with the collectives over gloo: the torch.distributed gather of Supergrid.topography."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import ocean_model_grid_generator_amd.supergrid as m
        from ocean_model_grid_generator_amd import topography as T
        plan = m.SupergridPlan(**CONFIGS["r2_dp"])
        g = m.Supergrid(plan, rank=rank, world=world, device="cuda:0", halo="rccl")
        g.run_pass()
        data, box, fill = raster("int16")
        res = g.topography(g.south_cut(), T.DeviceSource(T.Source(data, *box), "cuda:0"))
        q.put((rank, None if res is None else res["records"].tobytes()))
    except Exception as e:   # reported to the parent, which fails the test
        q.put((rank, "error: %r" % (e,)))
    finally:
        dist.destroy_process_group()


def test_same_bits_over_torch_distributed(sg):
    """Two processes on cuda:0, gloo: rank 1 sends its records, rank 0 assembles the same bytes as one rank does."""
    import torch.multiprocessing as mp
    from ocean_model_grid_generator_amd import topography as T
    plan, ranks = device_grid(sg, "r2_dp")
    data, box, fill = raster("int16")
    want = ranks[0].topography(ranks[0].south_cut(), T.DeviceSource(T.Source(data, *box), "cuda:0"))["records"].tobytes()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert got[1] is None, got[1]
    assert isinstance(got[0], bytes), got[0]
    assert got[0] == want


def test_main_topog_file_equals_file_based_command(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    data, box, fill = raster("int16")
    srcf = str(tmp_path / "src.nc")
    ds = netcdf3.Dataset(srcf, [("lat", data.shape[0]), ("lon", data.shape[1])])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [], box[2] + box[3] * (np.arange(data.shape[0]) + 0.5))
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [], box[0] + box[1] * (np.arange(data.shape[1]) + 0.5))
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], data)
    ds.write()
    a, b, t1, t2 = (str(tmp_path / n) for n in ("a.nc", "b.nc", "t1.nc", "t2.nc"))
    ogg.main(2.0, gridfilename=a, no_changing_meta=True, ensure_nj_even=True)
    plain = capsys.readouterr().out
    ogg.main(2.0, gridfilename=b, no_changing_meta=True, ensure_nj_even=True, topog_source=srcf, topog_file=t1)
    with_t = capsys.readouterr().out
    assert open(a, "rb").read() == open(b, "rb").read()
    assert "topography" not in plain and "topography:" in with_t
    strip = [ln.replace(b, a) for ln in with_t.splitlines() if "topography" not in ln and "runtime" not in ln and "src.nc" not in ln]
    assert strip == [ln for ln in plain.splitlines() if "runtime" not in ln]
    r = subprocess.run([sys.executable, "-m", "ocean_model_grid_generator_amd.topography", b, srcf, "-o", t2, "--json",
                        str(tmp_path / "s.json")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(t1, "rb").read() == open(t2, "rb").read()
    t3 = str(tmp_path / "t3.nc")
    ogg.main(2.0, gridfilename=None, no_changing_meta=True, ensure_nj_even=True, topog_source=srcf, topog_file=t3, path="functions")
    assert open(t1, "rb").read() == open(t3, "rb").read()


def test_cost_at_one_eighth_degree(sg, capsys):
    from ocean_model_grid_generator_amd import topography as T
    plan = sg.SupergridPlan(inverse_resolution=8.0, ensure_nj_even=True)
    g = sg.Supergrid(plan, device="cuda:0")
    g.run_pass()
    data, box, fill = raster("int16")
    dev = T.DeviceSource(T.Source(data, *box), "cuda:0")
    t0 = time.perf_counter()
    res = g.topography(g.south_cut(), dev)
    dt = time.perf_counter() - t0
    with capsys.disabled():
        print("\n-r 8 topography against a 0.25 deg raster: %.3f s for %d samples" % (dt, res["summary"]["n_samples"]))
    assert dt < 60.0
    assert res["summary"]["n_cells"] == (plan.Ni // 2) * ((g.stitched_rows(g.south_cut()) - 1) // 2)

"""Every device entry held to the stream it is given (include/ogg_hip.h: an ogg_*_dev entry enqueues its work on ``stream`` and
returns without synchronising, unless its comment says "Waits for the stream").  On the default stream, which every other test
passes, a launch that forgot its stream argument, an internal synchronous copy and a host read of a count ahead of the stream all
give the right bytes.  Here every analysis runs through its device wrapper on a non-blocking side stream, with its tensors in the
arena of tests/guarded_memory.py under the all-zero pattern, and _lib.call is wrapped (``observe``): before an entry is called the
stream it will be given is drained and a delay is enqueued on it, the arena is copied on an observer stream before and after the
call, and the stream must still be busy afterwards.  Nothing the entry does may touch device memory before the stream reaches it
(the two copies are the same bytes), and the entry must have returned without waiting (the stream is still inside the delay).
The entries that wait by contract stand in WAITS (tests/test_stream_contract_cpu.py holds that table to the header's list): they
get the delay but no copies.  Every case is also compared, array by array and count by count, between the side-stream run, a plain
run on the default stream and a guarded all-zero run on the default stream: a count read ahead of the stream is 0 there, and the
cases' counts are asserted non-zero.

The null stream is drained before the second copy (a write it carries must have landed to be seen); a write from another
unordered stream of the library's own would be seen only if it lands in time, or in the comparison of the results.

The delay: STREAM_DELAY_MS, 20 times the largest host time of one observation (copy, call, copy) measured on an MI355X: the figures
stand above the constant, and the module's last test prints those of the run.  An observation that outlasts the delay is reported as
void, never passed over.  Streams share the device's few hardware queues: the observer is chosen as a stream whose copies are seen to
run beside the sleeping side stream (the ``streams`` fixture).
"""
import ctypes
import os
import time

import numpy as np
import pytest

import guarded_memory as gm
import test_gpu_extents as TE
from test_gpu_extents import api, differences, frozen, up   # noqa: F401  (fixture and helpers of the harness)

pytestmark = pytest.mark.gpu
DEV = TE.DEV

# Measured on an MI355X with the library of the commit before this module (the module's last test prints the figures of every run):
# 192 observations of 60 entries; their median host time 0.074 ms, the longest 0.573 ms (ogg_topog_band_dev; ogg_sill_depth_dev 0.526 ms,
# every other one under 0.2 ms); the largest arena use copied, 34 430 784 bytes (the runoff case), took 0.16 ms with its call.
# 20 x 0.573 ms = 11.5 ms.  (ogg_runoff_search_dev, which then still waited for its stream, is not among them: its observation took
# the whole delay and was reported.)  With this delay and the library as it is now: 198 observations, the longest 0.521 ms, and with the
# 37 calls of the entries that wait the module sleeps 2.7 s of its 6.4 s.
STREAM_DELAY_MS = 11.5
ARENA_BYTES = 64 << 20
VERBOSE = bool(os.environ.get("OGG_STREAMS_VERBOSE"))      # with pytest -s: every case's counts and every observation's times

# ogg_*_dev entries that wait for the stream by contract: the header says so in their comment and lists them in its conventions
WAITS = {
    "ogg_workspace_error_flag_dev": "reads the workspace's error word on the host: csrc/ogg_dpole.hip:538",
    "ogg_supergrid_pass_plan_flags_dev": "reads the look-back words of both slots on the host: csrc/ogg_pass.hip:865",
    "ogg_supergrid_pass_dev": "plan + run + destroy, and the destroy waits for the run before it frees the plan's workspaces: csrc/ogg_pass.hip:647",
    "ogg_tripolar_pass_dev": "ogg_supergrid_pass_dev without a southern cap: csrc/ogg_pass.hip:647",
    "ogg_spread_sets_dev": "refuses a mouth that is no candidate and sizes the cube index by the candidates' count: csrc/ogg_spread.hip:439",
    "ogg_remap_fill_dev": "launches fronts until the queue's head, read on the host, is empty: csrc/ogg_remap.hip:463",
    "ogg_layout_blocks_dev": "copies the block begins from vectors of its own frame: csrc/ogg_layout.hip:421",
}
# ... and those that no case of this module observes, each with its reason
NO_STREAM = "takes no stream: it builds the plan of a pass (device allocations of its own, cleared synchronously) before any run"
NOT_OBSERVED = dict(TE.NOT_GUARDED, ogg_supergrid_pass_plan_dev=NO_STREAM)

S = {"active": False, "arena": None, "obs": None, "snap": None, "cycles_per_ms": None}
OBSERVED, WAITED = {}, {}          # entry -> calls
REPORTS = []                       # (entry, what) of every observation that failed
TIMES = {"max_s": 0.0, "max_entry": None, "n": 0, "peak_used": 0}


# ---- the harness -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena(hip):
    return gm.Arena(DEV, ARENA_BYTES)


@pytest.fixture(scope="module")
def streams(hip, arena):
    """the side stream, the observer stream, the two snapshot buffers and the rate of torch.cuda._sleep's clock"""
    import torch
    side = torch.cuda.Stream(DEV)
    S["arena"] = arena
    S["snap"] = [gm._REAL["empty"](ARENA_BYTES, dtype=torch.uint8, device=DEV) for _ in range(2)]
    n = 4000000
    with torch.cuda.stream(side):
        torch.cuda._sleep(1000)
        side.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        torch.cuda._sleep(n)
        e1.record(side)
        side.synchronize()
    S["cycles_per_ms"] = n / e0.elapsed_time(e1)
    # streams share the device's few hardware queues, and a copy on a stream that shares the side stream's queue waits behind the
    # delay: the observer is the first stream whose copy of the arena's first block ends while the side stream still sleeps
    tried = []
    for k in range(16):
        obs = torch.cuda.Stream(DEV)
        S["obs"] = obs
        snapshot(0, gm.BLOCK)
        with torch.cuda.stream(side):
            torch.cuda._sleep(int(STREAM_DELAY_MS * S["cycles_per_ms"]))
        t0 = time.perf_counter()
        snapshot(1, gm.BLOCK)
        torch.cuda.default_stream(torch.device(DEV)).synchronize()
        busy, dt = not side.query(), time.perf_counter() - t0
        side.synchronize()
        tried.append((busy, round(dt * 1e3, 3)))
        if busy:
            break
    S["tried"] = tried
    assert tried[-1][0], "no stream found whose copies run beside a sleeping side stream (busy, ms of the copy): %s" % tried
    torch.cuda.synchronize()
    return side, obs


def snapshot(k, n):
    import torch
    with torch.cuda.stream(S["obs"]):
        S["snap"][k][:n].copy_(S["arena"].buf[:n])
    S["obs"].synchronize()


def changed_bytes(n):
    """the bytes that differ between the two snapshots, as a text ('' if none): how many, the first's offset and its tensor"""
    import torch
    with torch.cuda.stream(S["obs"]):
        a, b = S["snap"][0][:n], S["snap"][1][:n]
        if torch.equal(a, b):
            return ""
        bad = (a != b).nonzero().view(-1)
        first, count = int(bad[0]), int(bad.numel())
    owner = [r[0] for r in S["arena"].records if r[1] <= first < r[2]]
    return "%d bytes of the arena changed before the stream reached the entry, the first at offset %d (%s)" % (
        count, first, owner[0] if owner else "a guard band")


def observe(name, fn):
    """One entry, called by ``fn``, on the current stream: drained, a delay enqueued, [the arena copied,] the call, [the arena copied
    again, the stream still busy].  What fails goes to REPORTS."""
    import torch
    cur = torch.cuda.current_stream(torch.device(DEV))
    cur.synchronize()
    waits = name in WAITS
    n = S["arena"].used(guards=True)
    torch.cuda._sleep(int(STREAM_DELAY_MS * S["cycles_per_ms"]))
    t0 = time.perf_counter()
    if not waits:
        snapshot(0, n)
    t_call = time.perf_counter()
    out = fn()
    t_call = time.perf_counter() - t_call
    if waits:
        WAITED[name] = WAITED.get(name, 0) + 1
        return out
    torch.cuda.default_stream(torch.device(DEV)).synchronize()     # a write the null stream carries has landed
    snapshot(1, n)
    busy = not cur.query()
    dt = time.perf_counter() - t0
    OBSERVED[name] = OBSERVED.get(name, 0) + 1
    TIMES["n"] += 1
    TIMES["peak_used"] = max(TIMES["peak_used"], n)
    if dt > TIMES["max_s"]:
        TIMES.update(max_s=dt, max_entry=name)
    what = changed_bytes(n)
    if VERBOSE:
        print("%s: %d bytes, %.3f ms of which the call %.3f ms, busy %s %s" % (name, n, dt * 1e3, t_call * 1e3, busy, what))
    ms = (dt * 1e3, t_call * 1e3, STREAM_DELAY_MS)
    if (dt - t_call) * 1e3 >= STREAM_DELAY_MS:
        REPORTS.append((name, "the observation is void, the delay was too short: it took %.3f ms, %.3f ms of them in the call; the delay is %.3f ms" % ms))
    elif dt * 1e3 >= STREAM_DELAY_MS:      # the delay ran out during the call: what the copies show is what the entry then enqueued
        REPORTS.append((name, "the entry waited for the stream (or its call is slower on the host than the delay allows): the observation took "
                        "%.3f ms, %.3f ms of them in the call; the delay is %.3f ms" % ms))
    elif not busy:
        REPORTS.append((name, "the observation is void, the delay ended early: the stream was idle %.3f ms after the delay was enqueued, %.3f ms "
                        "of them in the call; the delay is %.3f ms" % ms))
    elif what:
        REPORTS.append((name, what))
    return out


@pytest.fixture(autouse=True)
def observe_entries(hip, monkeypatch):
    """_lib.call wrapped: while a side-stream run is under way every ogg_*_dev entry goes through observe"""
    real = hip.call

    def call(name, *args):
        if S["active"] and name.startswith("ogg_") and name.endswith("_dev") and name not in NOT_OBSERVED:
            return observe(name, lambda: real(name, *args))     # real raises unless the entry returned OGG_OK
        return real(name, *args)
    monkeypatch.setattr(hip, "call", call)


def side_run(fn, arena, streams, monkeypatch, freeze=frozen):
    """fn() on the side stream under ``guarded`` with the all-zero pattern and every entry observed: (result frozen, reports)"""
    import torch
    side = streams[0]
    arena.reset("00")
    torch.cuda.synchronize()
    first = len(REPORTS)
    S["active"] = True
    try:
        with torch.cuda.stream(side), gm.guarded(monkeypatch, arena):
            got = freeze(fn())
            side.synchronize()
    finally:
        S["active"] = False
    bad = arena.check()
    assert bad == [], TE.violations(bad)
    return got, REPORTS[first:]


@pytest.fixture
def three_streams(arena, streams, monkeypatch):
    """run(fn, case): fn() plain on the default stream, guarded all-zero on the default stream, and observed on the side stream;
    no report, and the three results the same"""
    import torch

    def run(fn, case):
        plain = frozen(fn())
        if VERBOSE:
            print("\n%s: %s" % (case, counts_of(plain)))
        arena.reset("00")
        torch.cuda.synchronize()
        with gm.guarded(monkeypatch, arena):
            zero = frozen(fn())
        torch.cuda.synchronize()
        got, reports = side_run(fn, arena, streams, monkeypatch)
        assert reports == [], (case, reports[:8])
        for other, what in ((zero, "guarded on the default stream"), (got, "on the side stream")):
            diff = differences(plain, other)
            assert diff == [], (case, what, diff[:8])
        return plain
    return run


def counts_of(v, path="result"):
    """the integers of every dict inside a frozen result, by the dict's path"""
    out = {}
    if isinstance(v, dict):
        ints = {k: e for k, e in v.items() if isinstance(e, int) and not isinstance(e, bool)}
        if ints:
            out[path] = ints
        for k, e in v.items():
            out.update(counts_of(e, "%s[%r]" % (path, k)))
    elif isinstance(v, list):
        for k, e in enumerate(v):
            out.update(counts_of(e, "%s[%d]" % (path, k)))
    return out


def nonzero(res, *keys):
    """the counts named by ``keys`` occur in the result and none is 0: a count read ahead of the stream would be"""
    found = {}
    for d in counts_of(res).values():
        found.update({k: d[k] for k in keys if k in d and k not in found})
    assert sorted(found) == sorted(keys) and all(found[k] > 0 for k in keys), (keys, counts_of(res))


# ---- the harness must be able to fail ---------------------------------------------------------------------------------
def test_the_harness_reports_an_early_write_and_a_wait(arena, streams, monkeypatch):
    """Two entries played by torch: one fills an arena tensor on the DEFAULT stream (ordinary, but not where the caller's stream is),
    one waits for the side stream.  The first must be reported as changed bytes, the second as a wait, and a well-behaved one not at all."""
    import torch
    side = streams[0]
    torch.zeros(8, dtype=torch.float64, device=DEV).fill_(1.0).add_(1.0)      # the first launch of a kernel loads its code: not in the observation
    torch.cuda.synchronize()

    def run():
        t = torch.zeros(1000, dtype=torch.float64, device=DEV)

        def early():
            with torch.cuda.stream(torch.cuda.default_stream(torch.device(DEV))):
                t.fill_(1.0)
        observe("test_early_write_dev", early)
        observe("test_wait_dev", side.synchronize)
        observe("test_good_dev", lambda: t.add_(1.0))
        return t
    times = dict(TIMES)
    got, reports = side_run(run, arena, streams, monkeypatch)
    assert got[3] == np.full(1000, 2.0).tobytes()
    del REPORTS[len(REPORTS) - len(reports):]       # the three are no entries of the library: out of the module's census
    TIMES.update(times)
    for name in ("test_early_write_dev", "test_wait_dev", "test_good_dev"):
        del OBSERVED[name]
    assert [r[0] for r in reports] == ["test_early_write_dev", "test_wait_dev"], reports
    assert "bytes of the arena changed before the stream reached the entry" in reports[0][1] and "test_gpu_streams.py:" in reports[0][1], reports
    assert reports[1][1].startswith("the entry waited for the stream"), reports


# ---- the analyses: one small case each ---------------------------------------------------------------------------------
def test_exchange_grid(api, three_streams):
    import small_meshes as sm
    g = TE.grid("3x3")
    lon, lat = sm.zoo_atmosphere("regular")

    def run():
        x, y = up(g["x"]), up(g["y"])
        return api.X.whole_grid_lists_dev(x, y, lon, lat, g["mask"], sm.RE, 0.0, TE.stream(), x.device)
    res = three_streams(run, "xgrid 3x3")
    assert res[2][2][0] > 0      # the list of areas is not empty


def test_exchange_grid_cs(api, three_streams):
    g = TE.grid("3x3")
    atm = api.XC.cubed_sphere_atm(5, "edge_equidistant")
    res = three_streams(lambda: TE.cs_lists(api, g["x"], g["y"], atm, g["mask"], 1e-6), "xgrid_cs 3x3 N=5")
    assert res[5][2][0] > 0      # the list of areas is not empty


def test_exchange_grid_curv(hip, api, three_streams):
    import test_gpu_curv_extents as TC
    import xgrid_cs_definition as cd
    import xgrid_curv_definition as vd
    from ocean_model_grid_generator_amd import exchange_grid_curv
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 3)[:2]
    sx, sy = vd.rotated_mesh(46.5, 21.625, 36.0, 6.0, 96, 16, angle=0.05)
    res = three_streams(lambda: TC.lists(hip, exchange_grid_curv, x, y, sx, sy, [(0, 6)]), "xgrid_curv 65x3")
    assert res[0][6][2][0] > 1025


def test_remap(api, three_streams):
    import small_meshes as sm
    g = TE.grid("3x3")
    f, lon, lat, fills = sm.source_with_holes(g["x"], g["y"], nrec=3)     # one hole per record: cells to remap and cells to fill
    src = api.R.Source(f, lon, lat, fill=fills)
    res = three_streams(lambda: api.R.remap_dev(up(g["x"]), up(g["y"]), src, mask=g["mask"], Re=sm.RE), "remap 3x3")
    nonzero(res, "dry", "remapped", "filled", "fronts", "launches")


def test_regrid_to_latlon(api, three_streams):
    import small_meshes as sm
    g = TE.grid("3x3")
    rng = np.random.default_rng(7)
    lon, lat = sm.zoo_atmosphere("regular")
    f = (10.0 + rng.random((3, 3, 3))).astype(np.float32)
    f[0, 1, 1], f[1, 0, 2] = np.nan, -999.0
    res = three_streams(lambda: api.G.regrid_to_latlon_dev(up(g["x"]), up(g["y"]), f, lon, lat, mask=g["mask"], normalize="area", cover=True,
                                                           fill_values=(-999.0, 1.0e20), Re=sm.RE), "regrid 3x3")
    nonzero(res, "entries", "cells", "valid")


def test_bilinear(api, three_streams):
    import test_gpu_small_meshes as TSM
    g = TE.grid("3x3")
    _, _, t, u, v = TSM.bilinear_sources(api, g, "regular", np.float32, 5, True)
    with np.errstate(invalid="ignore"):
        res = three_streams(lambda: TE.bilinear_all(api, g, t, u, v, 2), "bilinear 3x3")
    nonzero(res[0], "dry", "interpolated", "filled", "unfilled")


def test_runoff(api, three_streams):
    import small_meshes as sm
    import test_gpu_small_meshes as TSM
    g = TE.grid("3x3")
    wet = np.ones_like(g["mask"])
    wet[1, 1] = 0
    lon, lat = sm.source_edges("regular")
    src = api.R.Source(TSM.runoff_field(lon, lat, 3, np.float32, 0.2, 0), lon, lat, fill=(-999.0, 1.0e20))
    res = three_streams(lambda: api.RO.runoff_dev(up(g["x"]), up(g["y"]), up(g["area"]), src, up(wet), targets="coast", Re=sm.RE, keep_lists=True),
                        "runoff 3x3")
    nonzero(res, "targets", "mapped", "cells", "bins", "tests")


def test_runoff_spread(api, three_streams):
    import small_meshes as sm
    g = sm.shape_grid("3x3")
    wet = np.ones((3, 3), np.uint8)
    load = np.zeros((3, 3), np.int32)
    load[0, 0] = load[2, 1] = 1
    v = np.random.default_rng(6).standard_normal((2, 3, 3)) * load
    res = three_streams(lambda: api.RO.spread_dev(v, up(g["x"]), up(g["y"]), up(g["area"]), wet, load=load, radius_km=2500.0, Re=6371.0e3,
                                                  keep_lists=True), "spread 3x3")
    nonzero(res, "mouths", "pairs", "candidates")
    assert res["counts"]["mouths"] == 2 and res["counts"]["pairs"] > 2


def test_coast_distance(api, three_streams):
    import small_meshes as sm
    g = TE.grid("3x3")
    wet = np.ones_like(g["mask"])
    wet[1, 1] = 0
    res = three_streams(lambda: api.CD.coast_distance_dev(up(g["x"]), up(g["y"]), up(wet), sides="both", Re=sm.RE, keep_lists=True), "coast 3x3")
    nonzero(res, "coast_wet", "coast_land", "queries", "answered")


def test_basin_codes(api, three_streams):
    import small_meshes as sm
    import test_gpu_basin_codes as TB
    c = TE.grid("3x3")
    lon, lat = float(c["x"][3, 3]), float(c["y"][3, 3])
    rules = [(7, lon, lat) + (-180.0, 180.0, lat - 30.0, 90.0), (9, lon + 40.0, lat) + TB.FULL]
    wet = np.ones_like(c["mask"])
    res = three_streams(lambda: api.BC.basin_codes_dev(up(c["x"]), up(c["y"]), up(wet), rules, Re=sm.RE), "basin 3x3")
    nonzero(res, "wet", "coded", "passes")


def test_ocean_mask(api, three_streams):
    g = TE.grid("3x3")
    depth = np.full((3, 3), 30.0)
    depth[1, 2], depth[0, 1] = 0.0, 2.0
    seeds = [(float(g["x"][1, 1]), float(g["y"][1, 1]))] * 3
    res = three_streams(lambda: api.M.ocean_mask_dev(up(depth), up(g["x"]), up(g["y"]), seeds=seeds, keep_min_cells=3, min_depth=5.0), "mask 3x3")
    assert counts_of(res), sorted(res)


def test_layouts_and_mask_table(api, three_streams):
    ny, nx = 5, 8
    wet = (np.random.default_rng(13).random((ny, nx)) < 0.6).astype(np.uint8)
    wet[-1] = wet[-1] | wet[-1, ::-1]

    def run():
        out = [api.LY.layouts_dev(up(wet), max_blocks=12, periodic=True, fold=True, halo=1, min_block=1)]
        t = api.LY.DeviceTable(up(wet), True, True, 1)
        out.append(api.LY.layouts_dev(None, candidates=[(1, 1), (3, 2)], table=t))
        out.append(api.LY.mask_table_dev(None, 4, 3, table=t))
        return out
    res = three_streams(run, "layout 5x8")
    nonzero(res, "blocks", "pes", "wet_total")


def test_locate_and_sample(api, three_streams):
    import locate_inputs as LI
    g = TE.grid("3x3")
    rng = np.random.default_rng(11)
    lon, lat, _ = LI.interior_points(g["x"], g["y"], rng, 63)
    lon[1], lat[2] = np.nan, np.inf
    f = 5.0 + rng.random((5, 3, 3))
    f[0, 0, 0], f[1, 1, 1] = np.nan, -999.0
    with np.errstate(invalid="ignore"):
        res = three_streams(lambda: api.LOC.locate_dev(up(g["x"]), up(g["y"]), up(lon), up(lat), keep_vectors=True, field=up(f), wet=up(g["mask"]),
                                                       mode="bilinear", fill_values=(-999.0, 1.0e20)), "locate 3x3 n=63")
    nonzero(res, "located", "invalid", "cubes", "tests")


def test_topography(api, three_streams):
    """one source (the band and the plane-fit band), a layered source (the layers' band, their ranges and their projection), the faces"""
    import small_grids as G
    import test_gpu_small_topog as TT
    import test_gpu_topog_layers as TTL
    import topog_layers_inputs as TI
    from ocean_model_grid_generator_amd import face_topography as FT
    L = api.L
    x, y = G.shape_grid("2x2")
    src = TT.source(api.T, "int16_fill2")

    def single():
        dev = api.T.DeviceSource(src, DEV, sea_level=0.5)
        return [TE.topog_band(api, x, y, dev.desc, L.TOPOG_MODEL_CELLS, 9, plane) for plane in (False, True)]
    three_streams(single, "topog 2x2")
    gx, gy, lys = TI.two_layers()
    sl = TTL.to_list(api.T, lys)
    px, py = TI.patch(37.3, -84.1, ny=2, nx=2, dlat=0.011, dlon=0.6)

    def layered():
        dev = api.T.DeviceSourceList(sl, DEV, sea_level=-50.0)
        return TE.topog_band(api, px, py, dev.desc, L.TOPOG_MODEL_CELLS, 9)
    three_streams(layered, "topog two layers 2x2")
    fx, fy = G.grid(2, 2, lon0=97.0, shear=True)

    def faces():
        dev = api.T.DeviceSource(src, DEV, sea_level=0.5)
        res = FT.face_topography_dev(up(fx), up(fy), dev, refine=9, topology=3)
        return {fam: res[fam]["records"] for fam in ("u", "v")}
    three_streams(faces, "faces 2x2")


def test_grid_quality(api, three_streams):
    import small_grids as G
    g = G.quality_shape(1, 127)
    three_streams(lambda: api.Q.grid_quality_dev(*[up(g[k]) for k in ("x", "y", "dx", "dy", "area")], Re=6371.0e3), "quality 1x127")


def test_sill_depth(api, three_streams):
    from ocean_model_grid_generator_amd import sill_depth
    rng = np.random.default_rng(233)
    top = (1 << 30) - 1
    wu, wv = rng.integers(-1, top + 2, (2, 3)), rng.integers(-1, top + 2, (3, 2))
    seeds = np.array([3, 0, 4, -7], dtype=np.int64)
    res = three_streams(lambda: sill_depth.sill_depth_faces_dev(up(wu), up(wv), up(seeds), True, True, 30), "sill 2x2 topology=3")
    nonzero(res, "rounds", "n_connected", "n_regions", "n_gate_faces")


def test_regional_grids(api, three_streams):
    from ocean_model_grid_generator_amd import regional, regional_stereo
    three_streams(lambda: regional.regional_grid_dev(-140.5, 55.0, 2, 2, 0.25, "mercator", tilt=40.0, metrics=True, bands=3), "regional 2x2")
    three_streams(lambda: regional_stereo.stereo_grid_dev(-140.5, 90.0, 2, 2, 0.25, tilt=40.0, metrics=True, bands=3), "regional stereo 2x2")


def test_elementwise_entries(api, three_streams):
    """the projection of the layers and the byte swap of the file stream, called on their own"""
    import torch
    import topog_layers_inputs as TI
    L = api.L
    n = 65
    p = TI.stereo("south_wgs84", lat_gate=60.0)
    rng = np.random.default_rng(n)
    lon, lat = 360.0 * rng.random(n) - 180.0, -90.0 + 40.0 * rng.random(n)

    def run():
        d = [up(lon), up(lat)]
        X, Y, swapped = torch.empty_like(d[0]), torch.empty_like(d[0]), torch.empty_like(d[0])
        ok = torch.zeros(n, dtype=torch.int32, device=DEV)
        desc = L.TopogProjection(h=p.h, lon0=p.lon0, a=p.a, e=p.e, K=p.K, lat_gate=p.lat_gate)
        L.call("ogg_topog_project_dev", ctypes.byref(desc), n, d[0].data_ptr(), d[1].data_ptr(), X.data_ptr(), Y.data_ptr(), ok.data_ptr(), TE.stream())
        L.call("ogg_bswap64_dev", n, d[0].data_ptr(), swapped.data_ptr(), TE.stream())
        return X, Y, ok, swapped
    res = three_streams(run, "project and bswap n=65")
    assert res[3][3] == lon.astype(">f8").tobytes()


# ---- the pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_dp", [None, 0.2])
def test_the_pass(api, hip, arena, streams, monkeypatch, r_dp):
    """Supergrid.run_pass three times on the side stream with the plan built under ``guarded`` (ogg_supergrid_pass_run_dev is called
    through the bound function: it is wrapped where the Supergrid binds it), the look-back flags clean, the fields the bytes of a pass on
    the default stream; then the one-call forms, quality, topography and the metrics self-check on those buffers."""
    flags = dict(inverse_resolution=0.25, ensure_nj_even=True)
    if r_dp is not None:
        flags["r_dp"] = r_dp
    plan, ranks = TE.build_ranks(api, flags, 1)
    ranks[0].run_pass()
    want = TE.host_bands(ranks)
    want_after = TE.after_pass(api, plan, ranks)
    ranks[0].close()
    lib = hip.load()
    real_run = lib.ogg_supergrid_pass_run_dev

    def run_dev(handle, events, alg_bytes, st):
        if not S["active"]:
            return real_run(handle, events, alg_bytes, st)
        return observe("ogg_supergrid_pass_run_dev", lambda: real_run(handle, events, alg_bytes, st))
    monkeypatch.setattr(lib, "ogg_supergrid_pass_run_dev", run_dev)

    def run():
        import torch
        plan, ranks = TE.build_ranks(api, flags, 1)
        g = ranks[0]
        assert g.launch == "pass"
        out = []
        for k in range(3):
            g.run_pass()
            torch.cuda.current_stream().synchronize()
            out.append(frozen(g.bands_to_host()))
            g.check_lookback_flags()
            TE.poison(plan, ranks)
        TE.one_shot_pass(api, plan, g)
        torch.cuda.current_stream().synchronize()
        out.append(frozen(g.bands_to_host()))
        after = TE.after_pass(api, plan, ranks)
        g.close()
        return out, after
    (passes, after), reports = side_run(run, arena, streams, monkeypatch, freeze=lambda v: v)
    assert reports == [], reports[:8]
    assert OBSERVED.get("ogg_supergrid_pass_run_dev", 0) >= 3
    for k, got in enumerate(passes):
        diff = differences(want[0], got)
        assert diff == [], ("pass %d" % k, diff[:8])
    diff = differences(want_after, after)
    assert diff == [], diff[:8]


@pytest.mark.parametrize("mode", list(TE.KERNEL_MODES))
def test_the_stand_alone_kernels_of_a_pass(api, arena, streams, monkeypatch, mode):
    """the entries a pass uses when it is not one fused launch (tests/test_gpu_extents.py has the list), one rank, two passes"""
    flags = dict(inverse_resolution=0.25, ensure_nj_even=True, r_dp=0.2)
    if mode == "skip_metrics":
        flags["skip_metrics"] = True
    if mode == "fused_rows":
        monkeypatch.setenv("OGG_LATLON_ROWS", "1")

    def run():
        plan, ranks = TE.build_ranks(api, flags, 1, **TE.KERNEL_MODES[mode])
        g = ranks[0]
        if mode != "skip_metrics":
            g.launch = "kernels"
        out = []
        for k in range(2):
            g.phase_a()
            g.exchange_halo()
            g.phase_b()
            if mode == "skip_metrics":
                g.run_pass()
            g.torch.cuda.current_stream().synchronize()
            out.append(frozen(g.bands_to_host()))
            g.check_lookback_flags()
        g.close()
        return out
    want = run()
    got, reports = side_run(run, arena, streams, monkeypatch, freeze=lambda v: v)
    assert reports == [], reports[:8]
    diff = differences(want, got)
    assert diff == [], diff[:8]


# ---- completeness ------------------------------------------------------------------------------------------------------
def test_every_device_entry_is_observed_or_waits(hip, capsys):
    """The last test of the module (it needs the others to have run): every ogg_*_dev entry of _lib.SIGNATURES was observed on the side
    stream, waits by contract and ran there, or stands in NOT_OBSERVED with a reason.  A device entry added later fails here until it
    has a case."""
    entries = {n for n in hip.SIGNATURES if n.startswith("ogg_") and n.endswith("_dev")}
    with capsys.disabled():
        print("\nstreams: %d observations of %d entries; the longest took %.3f ms of host time (%s) with %d bytes of the arena copied twice; "
              "delay %.3f ms, %.0f cycles of torch.cuda._sleep per ms; observer streams tried %s" % (
                  TIMES["n"], len(OBSERVED), TIMES["max_s"] * 1e3, TIMES["max_entry"], TIMES["peak_used"], STREAM_DELAY_MS,
                  S["cycles_per_ms"] or 0.0, S.get("tried")))
        print("observed: %s" % " ".join("%s(%d)" % (k, v) for k, v in sorted(OBSERVED.items())))
        print("waits: %s" % " ".join("%s(%d)" % (k, WAITED.get(k, 0)) for k in sorted(WAITS)))
        print("not observed: %s" % " ".join(sorted(NOT_OBSERVED)))
    assert REPORTS == [], REPORTS[:8]
    assert set(WAITS) <= entries and set(NOT_OBSERVED) <= entries, sorted((set(WAITS) | set(NOT_OBSERVED)) - entries)
    assert not set(OBSERVED) & (set(WAITS) | set(NOT_OBSERVED)) and not set(WAITS) & set(NOT_OBSERVED)
    assert set(WAITS) <= set(WAITED), "entries that wait by contract and never ran on the side stream: %s" % sorted(set(WAITS) - set(WAITED))
    missing = entries - set(OBSERVED) - set(WAITS) - set(NOT_OBSERVED)
    assert not missing, "device entries never observed on a side stream: %s" % sorted(missing)

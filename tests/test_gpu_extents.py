"""Every device entry held to its extents: no write outside an output or a workspace, no result that depends on what torch.empty
memory held, and the row stride ``ld`` of the supergrid arrays honoured.  None of this needs a definition; it needs memory whose
surroundings are known (tests/guarded_memory.py; its harness is proved on the CPU by tests/test_guarded_memory_cpu.py).

Every analysis runs three times through its device wrapper: plain; under ``guarded`` with every byte of the arena 0xFF; under
``guarded`` with seeded random bytes.  In the guarded runs every tensor the wrapper allocates and every device input it is given is an
exact-size view of the arena, flush against 64 KiB of guard.  The guards must be intact, every array of the result must have the
same bytes in all three runs, and every counts or summary dict must compare equal.  The pass (Supergrid.run_pass) is built under
``guarded`` and run three times back to back, then quality() and topography() on its buffers.  The seven entries that take a row
stride are called directly with padded rows.  test_every_device_entry_ran_guarded, the last test of the module, asserts that
every ogg_*_dev entry of _lib.SIGNATURES ran under ``guarded`` in this module but for the list NOT_GUARDED.

No element of any result is masked: the wrappers return their lists cut to their counts, and the strided calls are compared with
contiguous calls whose outputs lie at the same arena addresses under the same pattern, so that an element no kernel writes holds
the same poison in both.

Measured on an MI355X (test_every_device_entry_ran_guarded prints them): the largest case, the bilinear interpolation of the
``over_lds`` source on the ``neither`` cut, has 117 015 180 bytes handed out, its peak used(), and takes 120 888 288 bytes of the
arena with its guard bands; the arena is twice that, 241 776 576 bytes.  27 480 guarded allocations in all; 55 of the 69 device
entries covered, 14 excepted (NOT_GUARDED).  The first run found no changed guard byte and no difference between the three runs;
the 163 tests take 7 s together, none more than 0.3 s.
"""
import ctypes
import os
import struct

import numpy as np
import pytest

import guarded_memory as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANDOM = ("random", 20240611)
PATTERNS = ("ff", RANDOM)
PEAK_USED = 120888288              # the largest case's used(guards=True): the end of the module docstring
ARENA_BYTES = 2 * PEAK_USED

ACTIVE = [False]        # a guarded run is under way: _lib.call records the entry
COVERED = set()
STATS = {"peak": 0, "peak_case": None, "allocations": 0, "handed": 0}

# ogg_*_dev entries of _lib.SIGNATURES that no guarded case of this module runs, each with its reason
TEST_ONLY = "test-only: evaluates device math helpers for tests/test_gpu_math_helpers.py and smoke(), no analysis calls it"
FUNCTIONS = "function-level generator entry: only the path='functions' orchestrator's host-pointer twin is called by the package, with " \
            "the library's own staging; its extents are those of one elementwise launch over n outputs"
NOT_GUARDED = {
    "ogg_math_eval_dev": TEST_ONLY,
    "ogg_libm_check_dev": TEST_ONLY,
    "ogg_y_mercator_rounded_dev": FUNCTIONS,
    "ogg_phi_mercator_dev": FUNCTIONS,
    "ogg_y_mercator_dev": FUNCTIONS,
    "ogg_affine_index_dev": FUNCTIONS,
    "ogg_mdist_dev": FUNCTIONS,
    "ogg_haversine_dev": FUNCTIONS,
    "ogg_monotonic_bounding_dev": FUNCTIONS,
    "ogg_bipolar_projection_dev": FUNCTIONS,
    "ogg_bipolar_cap_ij_array_dev": FUNCTIONS,
    "ogg_displaced_pole_projection_dev": FUNCTIONS,
    "ogg_displaced_pole_mesh_dev": FUNCTIONS,
    "ogg_displaced_pole_numerical_h_dev": FUNCTIONS,
}


# ---- the harness -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena(hip):
    return gm.Arena(DEV, ARENA_BYTES)


@pytest.fixture(autouse=True)
def record_entries(hip, monkeypatch):
    """_lib.call wrapped: the entries that run while a guarded run is under way"""
    real = hip.call

    def call(name, *args):
        if ACTIVE[0]:
            COVERED.add(name)
        return real(name, *args)
    monkeypatch.setattr(hip, "call", call)


def up(a):
    """a host array on the device: under ``guarded`` an exact-size view of the arena (Tensor.to is one of the patched forms)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    import torch
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def frozen(v):
    """a result as something that compares with ==: arrays and tensors as (dtype, shape, bytes), floats as their bits (NaN == NaN),
    dicts, lists and tuples walked, objects the wrappers pass through (a Source, a rule table) as their type's name"""
    if hasattr(v, "data_ptr") and hasattr(v, "cpu"):
        v = v.cpu().numpy()
    if isinstance(v, np.ndarray):
        if v.dtype == object:
            return [frozen(e) for e in v.tolist()]
        return ("array", str(v.dtype), tuple(v.shape), np.ascontiguousarray(v).tobytes())
    if isinstance(v, dict):
        return {k: frozen(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [frozen(e) for e in v]
    if isinstance(v, (float, np.floating)):
        return ("float", struct.pack("<d", float(v)))
    if isinstance(v, (bool, int, str, bytes, type(None), np.integer, np.bool_)):
        return v if not isinstance(v, (np.integer, np.bool_)) else v.item()
    return ("object", type(v).__name__)


def differences(a, b, path="result"):
    """the paths at which two frozen results differ"""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [] if set(a) == set(b) else ["%s: keys %s" % (path, sorted(set(a) ^ set(b), key=str))]
        for k in a:
            if k in b:
                out += differences(a[k], b[k], "%s[%r]" % (path, k))
        return out
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [d for k, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, "%s[%d]" % (path, k))]
    if isinstance(a, tuple) and isinstance(b, tuple) and a[:1] == b[:1] == ("array",) and a[1:3] == b[1:3]:
        if a[3] == b[3]:
            return []
        x, y = (np.frombuffer(t[3], dtype=np.uint8) for t in (a, b))
        bad = np.nonzero(x != y)[0]
        return ["%s: %s %s differs in %d bytes, the first at byte %d" % (path, a[1], a[2], bad.size, int(bad[0]))]
    return [] if type(a) is type(b) and a == b else ["%s: %r != %r" % (path, str(a)[:80], str(b)[:80])]


def violations(bad):
    return "%d guard bytes changed: %s" % (len(bad), bad[:12])


def note(arena, case):
    used = arena.used(guards=True)
    if used > STATS["peak"]:
        STATS.update(peak=used, peak_case=case, handed=arena.used())
    STATS["allocations"] += arena.count()


@pytest.fixture
def three_runs(arena, monkeypatch):
    """run(fn, case): fn() plain, then under ``guarded`` with each pattern; guards intact, results the same"""
    def run(fn, case):
        plain = frozen(fn())
        for pattern in PATTERNS:
            arena.reset(pattern)
            ACTIVE[0] = True
            try:
                with gm.guarded(monkeypatch, arena):
                    got = frozen(fn())
            finally:
                ACTIVE[0] = False
            bad = arena.check()
            note(arena, case)
            assert bad == [], (case, pattern, violations(bad))
            diff = differences(plain, got)
            assert diff == [], (case, pattern, diff[:8])
        return plain
    return run


class Api(object):
    pass


@pytest.fixture(scope="module")
def api(hip):
    from ocean_model_grid_generator_amd import (basin_codes, bilinear, coast_distance, exchange_grid, exchange_grid_cs, grid_quality,
                                                latlon_regrid, layout, locate, ocean_mask, remap, runoff, supergrid, topography)
    a = Api()
    a.L, a.B, a.X, a.XC, a.G, a.R, a.RO, a.CD, a.BC, a.M, a.LY, a.LOC, a.T, a.Q, a.SG = (
        hip, bilinear, exchange_grid, exchange_grid_cs, latlon_regrid, remap, runoff, coast_distance, basin_codes, ocean_mask, layout,
        locate, topography, grid_quality, supergrid)
    return a


def grid(name):
    import test_gpu_small_meshes as TSM
    return TSM.grid(name)


def small_names():
    import small_meshes as sm
    return ["zoo"] + list(sm.CUTS) + list(sm.SHAPES)


# the shapes the issue names (all of small_meshes.SHAPES but the 1x64 control are there; it stays in)
SHAPES = ["1x1", "1x63", "1x64", "1x65", "129x1", "3x3", "fold_5x7", "band_2x1", "band_2x2", "band_3x1", "band_3x2"]
CUTS = ["full", "fold_only", "periodic_only", "neither"]


def test_the_named_shapes_exist():
    import small_meshes as sm
    assert set(SHAPES) <= set(sm.SHAPES) and set(CUTS) == set(sm.CUTS)


def test_the_harness_on_the_device(arena, monkeypatch):
    """What tests/test_guarded_memory_cpu.py shows on the CPU, once on the device, with torch operations playing the faulty kernels
    (every write stays inside the arena's own allocation): a tail that forgets its k < n test, a step that reads a torch.empty word
    before anyone wrote it, and a kernel that indexes rows with 2 nx + 1 where it should use ld."""
    import torch
    n, nx = 1000, 7
    rows = np.arange(3.0 * (2 * nx + 1)).reshape(3, 2 * nx + 1)
    summed, wrong_stride = [], []
    for pattern in PATTERNS:
        arena.reset(pattern)
        with gm.guarded(monkeypatch, arena):
            out = torch.empty(n, dtype=torch.float64, device=DEV)
            assert out.data_ptr() % 256 == 0 and arena.buf.data_ptr() <= out.data_ptr() < arena.buf.data_ptr() + arena.nbytes
            counter = torch.empty(1, dtype=torch.int64, device=DEV)
            z = torch.zeros(5, dtype=torch.int32, device=DEV)
            out.fill_(1.0)
            assert arena.check() == [] and z.tolist() == [0] * 5
            tail = torch.as_strided(out, (n + 1,), (1,))[n:].view(torch.uint8)   # one element past the end: every byte of it flipped
            tail ^= 0xFF
            bad = arena.check()
            assert [b[1:] for b in bad] == [("after", k) for k in range(1, 9)] and bad[0][0].startswith("test_gpu_extents.py:")
            counter += 5                                                     # a counter nobody zeroed
            summed.append(counter.cpu().numpy().tobytes())
        x = arena.take(rows.shape, torch.float64, ld=2 * nx + 1 + 3)
        x.copy_(torch.from_numpy(rows))
        assert x.cpu().numpy().tobytes() == rows.tobytes()
        wrong_stride.append(torch.as_strided(x, rows.shape, (2 * nx + 1, 1)).cpu().numpy().tobytes())
        for r in range(3):   # the element after every row: the first padding column of rows 0 and 1, the guard after row 2
            pad = torch.as_strided(x, (1,), (1,), x.storage_offset() + r * (2 * nx + 4) + 2 * nx + 1).view(torch.uint8)
            pad ^= 0xFF
        assert [b[1:] for b in arena.check()[8:]] == [("padding", r * (2 * nx + 4) * 8 + (2 * nx + 1) * 8 + k) for r in range(2) for k in range(8)] + \
            [("after", k) for k in range(1, 9)]
    assert summed[0] != summed[1]
    assert wrong_stride[0] != wrong_stride[1] and rows.tobytes() not in wrong_stride
    assert torch.empty is gm._REAL["empty"]


# ---- exchange grids --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zoo"] + CUTS + SHAPES)
def test_exchange_grid(api, three_runs, name):
    import small_meshes as sm
    g = grid(name)
    kinds = ("regular", "gaussian", "one_column", "one_row") if name == "zoo" else ("regular",)
    for kind in kinds:
        lon, lat = sm.zoo_atmosphere(kind)
        for masked in (False, True):
            def run():
                x, y = up(g["x"]), up(g["y"])
                atm, ocn, area, mt = api.X.whole_grid_lists_dev(x, y, lon, lat, g["mask"] if masked else None, sm.RE, 0.0, stream(), x.device)
                return atm, ocn, area, mt
            three_runs(run, "xgrid %s %s" % (name, kind))


def cs_lists(api, x, y, atm, mask, threshold):
    """exchange_grid_cs.band_lists_dev of a whole grid as one band, with the table, the grid and the mask on the device"""
    L = api.L
    nyp, nxp = x.shape
    xt, yt, tt = up(x), up(y), up(atm["t"])
    mt = None if mask is None else up(mask)
    band = L.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=0, n_cell_rows=nyp - 1, Re=6371.0e3, threshold=threshold)
    band.x, band.y = xt.data_ptr(), yt.data_ptr()
    band.x_next, band.y_next = xt[nyp - 1:].data_ptr(), yt[nyp - 1:].data_ptr()
    band.mask = None if mt is None else mt.data_ptr()
    return api.XC.band_lists_dev(band, api.XC.atm_desc(atm, tt.data_ptr()), stream(), xt.device)


@pytest.mark.parametrize("N, spacing", [(1, "equiangular"), (5, "edge_equidistant"), (12, "equiangular")])
def test_exchange_grid_cs(api, three_runs, N, spacing):
    import xgrid_cs_definition as cd
    atm = api.XC.cubed_sphere_atm(N, spacing)
    for name, (x, y, _) in cd.zoo().items():
        three_runs(lambda: cs_lists(api, x, y, atm, None, 0.0), "xgrid_cs %s N=%d" % (name, N))
    for name in ("zoo", "fold_only", "1x65", "fold_5x7"):
        g = grid(name)
        three_runs(lambda: cs_lists(api, g["x"], g["y"], atm, g["mask"], 1e-6), "xgrid_cs %s N=%d masked" % (name, N))


# ---- remap, fill, regrid ---------------------------------------------------------------------------------------------
# (source shape, dtype, nrec, two fill values plus NaN, masked, fill_max): nrec 3 and 5, both dtypes
REMAP_CASES = [("nonuniform", np.float64, 3, False, False, None), ("regular", np.float32, 5, True, True, 2), ("3x2", np.float64, 1, False, False, None),
               ("1x1", np.float32, 3, True, True, 0)]


@pytest.mark.parametrize("name", ["zoo"] + CUTS + SHAPES)
def test_remap(api, three_runs, name):
    import small_meshes as sm
    g = grid(name)
    for kind, dtype, nrec, two, masked, fill_max in REMAP_CASES:
        f, lon, lat, fills = sm.source_for(g["x"], g["y"], kind, nrec=nrec, dtype=dtype, two_fills=two)
        src = api.R.Source(f, lon, lat, fill=fills)
        three_runs(lambda: api.R.remap_dev(up(g["x"]), up(g["y"]), src, mask=g["mask"] if masked else None, fill_max=fill_max, Re=sm.RE),
                   "remap %s %s" % (name, kind))


@pytest.mark.parametrize("ny, nx", [(3, 1), (2, 2), (129, 1), (1, 1), (1, 65), (5, 7), (4, 3)])
def test_fill_step(api, three_runs, ny, nx):
    """remap.fill_dev alone on synthetic flags: nrec * ny * nx no multiple of 4 (the fill changes flag bytes by 32-bit compare-and-swap)"""
    import small_meshes as sm
    import torch
    lon, lat = sm.source_edges("3x2")
    for nrec in (3, 5):
        src = api.R.Source(sm.smooth_field(lon, lat, nrec, np.float64), lon, lat)
        v, fl = sm.synthetic_flags(ny, nx, nrec, 11 * ny + nx)
        for periodic, fold, fill_max in ((False, False, None), (True, True, None), (True, False, 1), (False, True, 1)):
            def run():
                tv = up(v)
                tf = api.R.flags_buffer(torch, tv.numel(), tv.device).view(v.shape)
                tf.copy_(torch.from_numpy(fl))
                counts = torch.zeros(len(api.L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=tv.device)
                api.R.fill_dev(api.R.params(ny, nx, src, 0, periodic, fold, fill_max), tv, tf, counts, stream(), tv.device)
                return tv, tf, api.R.counts_dict(counts.cpu().numpy())
            three_runs(run, "fill %dx%d nrec=%d" % (ny, nx, nrec))


@pytest.mark.parametrize("name", ["zoo", "fold_only", "1x65", "129x1", "fold_5x7", "1x1"])
def test_regrid_to_latlon(api, three_runs, name):
    import small_meshes as sm
    g = grid(name)
    ny, nx = (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2
    rng = np.random.default_rng(7)
    for kind, dtype, nrec, missing, masked, normalize in (("regular", np.float32, 3, True, True, "area"), ("gaussian", np.float64, 5, False, False, "cell"),
                                                          ("one_row", np.float32, 1, True, False, "cell"), ("one_column", np.float64, 3, True, True, "area")):
        lon, lat = sm.zoo_atmosphere(kind)
        f = (10.0 + rng.random((nrec, ny, nx))).astype(dtype)
        fills = ()
        if missing:
            f[rng.random(f.shape) < 0.1] = np.nan
            f[rng.random(f.shape) < 0.1] = -999.0
            f[rng.random(f.shape) < 0.1] = 1.0e20
            fills = (-999.0, 1.0e20)
        three_runs(lambda: api.G.regrid_to_latlon_dev(up(g["x"]), up(g["y"]), f, lon, lat, mask=g["mask"] if masked else None, normalize=normalize,
                                                      cover=True, fill_values=fills, Re=sm.RE), "regrid %s %s" % (name, kind))
    lon, lat = sm.zoo_atmosphere("regular")
    three_runs(lambda: api.G.regrid_to_latlon_dev(up(g["x"]), up(g["y"]), None, lon, lat, Re=sm.RE), "regrid %s fraction only" % name)


# ---- bilinear --------------------------------------------------------------------------------------------------------
def bilinear_all(api, g, t, u, v, fill_max):
    """a scalar at the h (masked, filled), u and v points; a vector at the h points, filled and turned; at the c points unturned and
    turned (the cross terms)"""
    x, y, ang = up(g["x"]), up(g["y"]), up(g["angle_dx"])
    out = [api.B.bilinear_dev(x, y, t, points="h", mask=g["mask"], fill_max=fill_max),
           api.B.bilinear_dev(x, y, t, points="u", fill=False), api.B.bilinear_dev(x, y, t, points="v", fill=False),
           api.B.bilinear_dev(x, y, u, v, angle_dx=ang, mask=g["mask"], fill_max=fill_max),
           api.B.bilinear_dev(x, y, u, v, points="c", rotate=False),
           api.B.bilinear_dev(x, y, u, v, angle_dx=ang, points="c")]
    return out


@pytest.mark.parametrize("name", CUTS + SHAPES)
def test_bilinear(api, three_runs, name):
    import test_gpu_small_meshes as TSM
    g = grid(name)
    for kind, dtype, nrec, two, fill_max in (("nonuniform", np.float64, 3, False, None), ("regular", np.float32, 5, True, 2), ("1x1", np.float64, 1, False, None),
                                             ("7x1", np.float32, 5, False, 0)):
        _, _, t, u, v = TSM.bilinear_sources(api, g, kind, dtype, nrec, two)
        with np.errstate(invalid="ignore"):
            three_runs(lambda: bilinear_all(api, g, t, u, v, fill_max), "bilinear %s %s" % (name, kind))


@pytest.mark.parametrize("name", ["neither", "1x1", "1x63", "fold_5x7"])
def test_bilinear_with_tables_too_large_for_lds(api, three_runs, name, monkeypatch):
    """the 8000 + 400 node source: the kernel's global-memory path"""
    import test_gpu_small_meshes as TSM
    monkeypatch.delenv("OGG_BILINEAR_LDS", raising=False)
    g = grid(name)
    _, _, t, u, v = TSM.bilinear_sources(api, g, "over_lds", np.float32, 1, False)
    with np.errstate(invalid="ignore"):
        three_runs(lambda: bilinear_all(api, g, t, u, v, None), "bilinear %s over_lds" % name)


# ---- runoff, coast distance, basin codes, ocean mask -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CUTS + ["1x1", "1x65", "3x3", "129x1", "fold_5x7"])
def test_runoff(api, three_runs, name):
    import small_meshes as sm
    import test_gpu_small_meshes as TSM
    g = grid(name)
    ny, nx = g["mask"].shape
    wet = g["mask"]
    if name not in CUTS:      # a single target cell
        wet = np.zeros((ny, nx), np.uint8)
        wet[ny // 2, nx // 2] = 1
    for k, (kind, dtype, nrec, mode, prob) in enumerate((("regular", np.float32, 3, "coast", 0.2), ("nonuniform", np.float64, 5, "wet", 0.05))):
        lon, lat = sm.source_edges(kind)
        src = api.R.Source(TSM.runoff_field(lon, lat, nrec, dtype, prob, k), lon, lat, fill=(-999.0, 1.0e20))
        three_runs(lambda: api.RO.runoff_dev(up(g["x"]), up(g["y"]), up(g["area"]), src, up(wet), targets=mode, Re=sm.RE, keep_lists=True),
                   "runoff %s %s" % (name, mode))


def coast_cases():
    import coast_inputs as CI
    import small_meshes as sm
    out = {k: f() for k, f in CI.CASES.items()}
    out["coast_of_1"], out["coast_of_65"] = CI.coast_of(1), CI.coast_of(65)
    for name in CUTS + ["1x1", "1x65", "129x1", "3x3", "fold_5x7", "band_2x1", "band_3x2"]:
        g = grid(name)
        out[name] = dict(x=g["x"], y=g["y"], wet=g["mask"], periodic=None, fold=None)
    assert sm.RE > 0
    return out


@pytest.mark.parametrize("sides", ["both", "wet", "land"])
def test_coast_distance(api, three_runs, sides):
    import small_meshes as sm
    for name, c in coast_cases().items():
        three_runs(lambda: api.CD.coast_distance_dev(up(c["x"]), up(c["y"]), up(c["wet"]), sides=sides, periodic=c["periodic"], fold=c["fold"],
                                                     Re=sm.RE, keep_lists=True), "coast %s %s" % (name, sides))


@pytest.mark.parametrize("ny, nx", [(1, 1), (1, 65), (33, 2), (31, 63), (65, 129), (5, 7)])
def test_basin_codes(api, three_runs, ny, nx):
    import small_meshes as sm
    import test_gpu_basin_codes as TB
    g = sm.latlon_grid(ny, nx, lon0=-33.0, lat0=-21.0, dlon=1.0, dlat=1.0)
    ie, iw = (3 * nx) // 5, (2 * nx) // 5
    rules = [(1,) + TB.centre(g, 0, 0) + TB.cell_box(g, 0, ny - 1, 0, ie), (2,) + TB.centre(g, ny - 1, nx - 1) + TB.cell_box(g, 0, ny - 1, iw, nx - 1),
             (3,) + TB.centre(g, ny // 2, nx // 2) + TB.FULL, (1,) + TB.centre(g, 0, nx - 1) + TB.cell_box(g, 0, ny // 2, 0, nx - 1),
             (4, 170.0, 80.0) + TB.FULL]     # a seed far off the grid
    j, i = np.indices((ny, nx))
    wall = np.ones((ny, nx), np.uint8)
    wall[:, nx // 2] = 0
    for wet in (np.ones((ny, nx), np.uint8), ((i + j) % 2 == 0).astype(np.uint8), wall):
        for kw in (dict(periodic=False, fold=False), dict(periodic=False, fold=False, seed_max_distance=500.0e3, area=g["area"][::2, ::2])):
            three_runs(lambda: api.BC.basin_codes_dev(up(g["x"]), up(g["y"]), up(wet), rules, Re=sm.RE, **kw), "basin %dx%d" % (ny, nx))


def test_basin_codes_serpentine_and_topologies(api, three_runs):
    import small_meshes as sm
    import test_gpu_basin_codes as TB
    g, wet, rules = TB.serpentine()
    three_runs(lambda: api.BC.basin_codes_dev(up(g["x"]), up(g["y"]), up(wet), rules, periodic=False, fold=False, Re=sm.RE), "basin serpentine")
    for name in CUTS + ["fold_5x7", "band_3x2"]:
        c = grid(name)
        ny, nx = c["mask"].shape
        lon, lat = float(c["x"][2 * (ny // 2) + 1, 2 * (nx // 2) + 1]), float(c["y"][2 * (ny // 2) + 1, 2 * (nx // 2) + 1])
        rules = [(7, lon, lat) + (-180.0, 180.0, lat - 30.0, 90.0), (9, lon + 40.0, lat) + TB.FULL]
        three_runs(lambda: api.BC.basin_codes_dev(up(c["x"]), up(c["y"]), up(c["mask"]), rules, Re=sm.RE), "basin %s" % name)


@pytest.mark.parametrize("name", CUTS + ["1x1", "1x65", "129x1", "3x3", "fold_5x7", "band_2x2"])
def test_ocean_mask(api, three_runs, name):
    g = grid(name)
    ny, nx = g["mask"].shape
    rng = np.random.default_rng(ny * 1000 + nx)
    depth = np.where((g["mask"] != 0) & (rng.random((ny, nx)) < 0.8), 1.0 + 50.0 * rng.random((ny, nx)), 0.0)
    depth.flat[0] = 25.0
    seeds = [(float(g["x"][1, 1]), float(g["y"][1, 1]))]      # the centre of cell (0, 0), wet
    for kw in (dict(), dict(seeds=seeds), dict(keep_min_cells=2, min_depth=10.0, mode="deepen"), dict(seeds=seeds * 3, keep_min_cells=3, min_depth=5.0)):
        three_runs(lambda: api.M.ocean_mask_dev(up(depth), up(g["x"]), up(g["y"]), **kw), "mask %s %s" % (name, sorted(kw)))
    # supergrid cells (no seeds): depth on every cell of the supergrid
    d2 = np.repeat(np.repeat(depth, 2, axis=0), 2, axis=1)
    three_runs(lambda: api.M.ocean_mask_dev(up(d2), up(g["x"]), up(g["y"])), "mask %s supergrid cells" % name)


# ---- layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny, nx, periodic, fold, halo", [(1, 1, False, False, 0), (13, 20, True, True, 1), (64, 65, True, False, 2), (33, 128, False, True, 0),
                                                          (129, 3, False, False, 1)])
def test_layouts_and_mask_table(api, three_runs, ny, nx, periodic, fold, halo):
    rng = np.random.default_rng(ny + nx)
    wet = (rng.random((ny, nx)) < 0.4).astype(np.uint8)
    wet[ny // 2:, : nx // 2] = 0
    if fold:   # a folded top row mirrors itself
        wet[-1] = wet[-1] | wet[-1, ::-1]

    def run():
        out = [api.LY.layouts_dev(up(wet), max_blocks=60, periodic=periodic, fold=fold, halo=halo, min_block=1)]
        t = api.LY.DeviceTable(up(wet), periodic, fold, halo)
        out.append(api.LY.layouts_dev(None, candidates=list(dict.fromkeys([(1, 1), (min(nx, 3), min(ny, 2)), (min(nx, 5), 1)])), table=t))
        for px, py in ((1, 1), (min(nx, 4), min(ny, 3)), (min(nx, 7), min(ny, 5))):
            out.append(api.LY.mask_table_dev(None, px, py, table=t))
        out.append(api.LY.mask_table_dev(up(wet), min(nx, 2), min(ny, 2), periodic=periodic, fold=fold, halo=halo))
        return out
    three_runs(run, "layout %dx%d" % (ny, nx))


# ---- point location --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CUTS + ["1x1", "1x63", "1x65", "129x1", "3x3", "fold_5x7", "band_2x1", "band_3x2"])
def test_locate_and_sample(api, three_runs, name):
    import locate_inputs as LI
    g = grid(name)
    ny, nx = g["mask"].shape
    rng = np.random.default_rng(11)
    for n, dtype, nrec, mode in ((0, np.float64, 1, "bilinear"), (1, np.float32, 3, "cell"), (63, np.float64, 5, "bilinear"), (65, np.float32, 5, "cell"),
                                 (257, np.float32, 3, "bilinear")):
        lon, lat, _ = LI.interior_points(g["x"], g["y"], rng, n) if n else (np.zeros(0), np.zeros(0), None)
        if n > 2:
            lon[1], lat[2] = np.nan, np.inf            # an invalid query and one more
            lon[0], lat[0] = lon[0] + 170.0, -lat[0]   # most likely outside a regional grid
        f = (5.0 + rng.random((nrec, ny, nx))).astype(dtype)
        f[rng.random(f.shape) < 0.15] = np.nan
        f[rng.random(f.shape) < 0.15] = -999.0
        f[rng.random(f.shape) < 0.15] = 1.0e20

        def run(device_inputs):
            x, y = up(g["x"]), up(g["y"])
            if device_inputs:
                return api.LOC.locate_dev(x, y, up(lon), up(lat), keep_vectors=True, field=up(f), wet=up(g["mask"]), mode=mode, fill_values=(-999.0, 1.0e20))
            return api.LOC.locate_dev(x, y, lon, lat, keep_vectors=True, field=f, wet=g["mask"], mode=mode, fill_values=(-999.0, 1.0e20))
        with np.errstate(invalid="ignore"):
            three_runs(lambda: run(True), "locate %s n=%d" % (name, n))
            if n in (1, 257):
                three_runs(lambda: run(False), "locate %s n=%d host points" % (name, n))
    three_runs(lambda: api.LOC.locate_dev(up(g["x"]), up(g["y"]), up(np.array([10.0, 20.0])), up(np.array([0.0, 5.0]))), "locate %s no field" % name)


# ---- topography, grid quality ----------------------------------------------------------------------------------------
def topog_band(api, x, y, desc, cells, refine, plane=False):
    L = api.L
    xd, yd = up(x), up(y)
    ny, nx = x.shape[0] - 1, x.shape[1] - 1
    band = L.TopogBand(nx=nx, j0=0, n_cell_rows=ny, cells=cells, refine=refine, oversample=2.0)
    band.x, band.y, band.x_next, band.y_next = xd.data_ptr(), yd.data_ptr(), xd[ny].data_ptr(), yd[ny].data_ptr()
    m0, out, ws = api.T.band_records_dev(band, desc, stream(), xd.device, plane)
    return m0, out


@pytest.mark.parametrize("kind", ["int16_fill2", "float32_q0.01", "float64_q0.5", "window", "1x1_regional"])
def test_topography(api, three_runs, kind):
    import small_grids as G
    import test_gpu_small_topog as TT
    L = api.L
    src = TT.source(api.T, kind)
    for name, (ny, nx, _) in G.TOPOG_SHAPES.items():
        x, y = G.shape_grid(name)
        even = ny % 2 == 0 and nx % 2 == 0
        for refine in (1, 9, 65) if name in ("1x1", "2x2", "1x65", "5x3") else (0,):
            for plane in (False, True):
                def run():
                    dev = api.T.DeviceSource(src, DEV, sea_level=0.5)
                    out = [topog_band(api, x, y, dev.desc, L.TOPOG_SUPERGRID_CELLS, refine, plane)]
                    if even:
                        out.append(topog_band(api, x, y, dev.desc, L.TOPOG_MODEL_CELLS, refine, plane))
                    return out
                three_runs(run, "topog %s %s refine=%d plane=%s" % (kind, name, refine, plane))
    x, y = G.placed("across_180")
    three_runs(lambda: topog_band(api, x, y, api.T.DeviceSource(src, DEV).desc, L.TOPOG_MODEL_CELLS, 0, True), "topog %s across_180" % kind)


@pytest.mark.parametrize("layers", ["two_layers", "three_layers", "four_layers"])
def test_layered_topography(api, three_runs, layers):
    import test_gpu_topog_layers as TTL
    import topog_layers_inputs as TI
    L = api.L
    x, y, lys = getattr(TI, layers)()
    sl = TTL.to_list(api.T, lys)
    strips = [(xs, ys) for n, xs, ys, _ in TI.strips() if n in (1, 63, 65, 129)]
    for gx, gy in [(x, y), TI.patch(37.3, -84.1, ny=65, nx=8, dlat=0.011, dlon=0.6)] + strips:
        even = (gx.shape[0] - 1) % 2 == 0 and (gx.shape[1] - 1) % 2 == 0
        for refine in (0, 9):
            def run():
                dev = api.T.DeviceSourceList(sl, DEV, sea_level=-50.0)
                out = [topog_band(api, gx, gy, dev.desc, L.TOPOG_SUPERGRID_CELLS, refine)]
                if even:
                    out.append(topog_band(api, gx, gy, dev.desc, L.TOPOG_MODEL_CELLS, refine))
                return out
            three_runs(run, "topog %s %s refine=%d" % (layers, gx.shape, refine))


@pytest.mark.parametrize("ny, nx", [(1, 1), (1, 127), (2, 254), (31, 126), (32, 128), (33, 253), (33, 1), (65, 255)])
def test_grid_quality(api, three_runs, ny, nx):
    import small_grids as G
    g = G.quality_shape(ny, nx) if (ny, nx) in G.QUALITY_PAIRS else G.quality_grid(ny, nx, shear=0.125)
    fields = ("x", "y", "dx", "dy", "area")
    for metrics in (True, False):
        three_runs(lambda: api.Q.grid_quality_dev(*[up(g[k]) for k in (fields if metrics else fields[:2])], Re=6371.0e3), "quality %dx%d" % (ny, nx))


@pytest.mark.parametrize("n", [1, 63, 65, 513, 4099])
def test_projection_and_byte_swap(api, three_runs, n):
    """the two elementwise entries the analyses call on whole arrays: the layers' polar-stereographic projection and the file
    stream's byte swap, at sizes around a wavefront and a workgroup"""
    import torch
    import topog_layers_inputs as TI
    L = api.L
    p = TI.stereo("south_wgs84", lat_gate=60.0)
    rng = np.random.default_rng(n)
    lon, lat = 360.0 * rng.random(n) - 180.0, -90.0 + 40.0 * rng.random(n)
    lat[0] = -90.0
    if n > 2:
        lon[1], lat[2] = np.nan, np.inf

    def project():
        d = [up(lon), up(lat)]
        X, Y = torch.empty_like(d[0]), torch.empty_like(d[0])
        ok = torch.zeros(n, dtype=torch.int32, device=DEV)
        desc = L.TopogProjection(h=p.h, lon0=p.lon0, a=p.a, e=p.e, K=p.K, lat_gate=p.lat_gate)
        L.call("ogg_topog_project_dev", ctypes.byref(desc), n, d[0].data_ptr(), d[1].data_ptr(), X.data_ptr(), Y.data_ptr(), ok.data_ptr(), stream())
        return X, Y, ok

    def swap():
        src = up(lon)
        dst = torch.empty(n, dtype=torch.float64, device=DEV)
        L.call("ogg_bswap64_dev", n, src.data_ptr(), dst.data_ptr(), stream())
        return dst
    three_runs(project, "project n=%d" % n)
    got = three_runs(swap, "bswap n=%d" % n)
    assert got[3] == lon.astype(">f8").tobytes()


# ---- the pass ----------------------------------------------------------------------------------------------------------
FIELDS =("x", "y", "dx", "dy", "area", "angle_dx")


def build_ranks(api, flags, world, **kw):
    plan = api.SG.SupergridPlan(**flags)
    ranks = []
    for r in range(world):
        ranks.append(api.SG.Supergrid(plan, rank=r, world=world, device=DEV, halo="local", peers=ranks, **kw))
    return plan, ranks


def host_bands(ranks):
    import torch
    torch.cuda.synchronize()
    return frozen([g.bands_to_host() for g in ranks])


def one_shot_pass(api, plan, g):
    """the pass's one-call forms on the descriptors the plan was built from: ogg_supergrid_pass_dev, and without a displaced pole
    ogg_tripolar_pass_dev as well"""
    L = api.L
    bands, arr, cap, scap, _ = g._pass_args
    capref = ctypes.byref(cap) if cap is not None else None
    metrics = 0 if plan.skip_metrics else 1
    L.call("ogg_supergrid_pass_dev", len(bands), arr, plan.Ni + 1, plan.lon0, plan.lenlon, plan.Re, metrics, capref,
           ctypes.byref(scap) if scap is not None else None, None, None, stream())
    if scap is None:
        L.call("ogg_tripolar_pass_dev", len(bands), arr, plan.Ni + 1, plan.lon0, plan.lenlon, plan.Re, metrics, capref, stream())


def poison(plan, ranks):
    for g in ranks:
        for s in plan.subs:
            for f in FIELDS:
                g.buf[s.name][f].fill_(float("nan"))


def topog_source(api):
    import small_grids as G
    r = G.raster("int16_fill2")
    return api.T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])


def after_pass(api, plan, ranks):
    """quality(cut), one topography(cut, dev) and the self-check's sums on the buffers the pass left"""
    g = ranks[0]
    cut = g.south_cut()
    dev = api.T.DeviceSource(topog_source(api), DEV)
    return frozen({"quality": g.quality(cut), "topography": g.topography(cut, dev), "plane": g.topography(cut, dev, cells="supergrid", plane=True),
                   "metrics_error": g.metrics_error()})


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("r_dp", [None, 0.2])
def test_the_pass_three_times_then_quality_and_topography(api, arena, monkeypatch, world, r_dp):
    """Supergrid(plan).run_pass() three times back to back with the fields, axes and workspaces in the arena: guards intact after
    every pass and the bands' bytes the plain run's; then the pass's one-call forms, quality(cut), topography(cut, dev) and the
    metrics self-check on those buffers."""
    flags = dict(inverse_resolution=0.25, ensure_nj_even=True)
    if r_dp is not None:
        flags["r_dp"] = r_dp
    case = "pass world=%d r_dp=%s" % (world, r_dp)
    plan, ranks = build_ranks(api, flags, world)
    for g in ranks:
        g.run_pass()
    want = host_bands(ranks)
    want_after = after_pass(api, plan, ranks)
    for g in ranks:
        g.close()
    for pattern in PATTERNS:
        arena.reset(pattern)
        ACTIVE[0] = True
        try:
            with gm.guarded(monkeypatch, arena):
                plan, ranks = build_ranks(api, flags, world)
                assert all(g.launch == "pass" for g in ranks)
                for k in range(3):
                    for g in ranks:
                        g.run_pass()
                        COVERED.add("ogg_supergrid_pass_run_dev")    # called through the bound function, not through _lib.call
                    bad = arena.check()
                    assert bad == [], (case, pattern, "pass %d" % k, violations(bad))
                    diff = differences(want, host_bands(ranks))
                    assert diff == [], (case, pattern, "pass %d" % k, diff[:8])
                    for g in ranks:
                        g.check_lookback_flags()
                    poison(plan, ranks)
                for g in ranks:
                    one_shot_pass(api, plan, g)
                    bad = arena.check()
                    assert bad == [], (case, pattern, "one-call pass", violations(bad))
                    diff = differences(want[g.rank], host_bands([g])[0])
                    assert diff == [], (case, pattern, "one-call pass", diff[:8])
                got_after = after_pass(api, plan, ranks)
                bad = arena.check()
                for g in ranks:
                    g.close()
        finally:
            ACTIVE[0] = False
        note(arena, case)
        assert bad == [], (case, pattern, "quality and topography", violations(bad))
        diff = differences(want_after, got_after)
        assert diff == [], (case, pattern, diff[:8])


KERNEL_MODES = {"stencil": dict(latlon="stencil"), "fused_kernels": dict(), "fused_rows": dict(), "skip_metrics": dict()}


@pytest.mark.parametrize("mode", list(KERNEL_MODES))
def test_the_stand_alone_kernels_of_a_pass(api, arena, monkeypatch, mode):
    """The entries a pass uses when it is not one fused launch: the stencil path (axes, tiles, the generic metrics kernel, the caps'
    mesh and quadrature kernels with their workspaces), the fused lat-lon launch on its own, its row-ordered form, and the -1 fill
    of skip_metrics; one rank and three, with the displaced pole."""
    flags = dict(inverse_resolution=0.25, ensure_nj_even=True, r_dp=0.2)
    if mode == "skip_metrics":
        flags["skip_metrics"] = True
    if mode == "fused_rows":
        monkeypatch.setenv("OGG_LATLON_ROWS", "1")

    def run(world):
        plan, ranks = build_ranks(api, flags, world, **KERNEL_MODES[mode])
        for g in ranks:
            if mode != "skip_metrics":
                g.launch = "kernels"
        out = []
        for k in range(2):
            for g in ranks:
                g.phase_a()
            for g in ranks:
                g.exchange_halo()
            for g in ranks:
                g.phase_b()
            if mode == "skip_metrics":
                for g in ranks:
                    g.run_pass()
            out.append(host_bands(ranks))
            for g in ranks:
                g.check_lookback_flags()
        for g in ranks:
            g.close()
        return out

    for world in (1, 3):
        case = "kernels %s world=%d" % (mode, world)
        want = run(world)
        assert differences(want[0], want[1]) == []
        for pattern in PATTERNS:
            arena.reset(pattern)
            ACTIVE[0] = True
            try:
                with gm.guarded(monkeypatch, arena):
                    got = run(world)
            finally:
                ACTIVE[0] = False
            bad = arena.check()
            note(arena, case)
            assert bad == [], (case, pattern, violations(bad))
            diff = differences(want, got)
            assert diff == [], (case, pattern, diff[:8])


# ---- the row stride ---------------------------------------------------------------------------------------------------------
class Strided(object):
    """One call of an ``ld`` entry with every buffer in the arena: the outputs and workspaces first, in a fixed order and at their
    exact sizes, so that they lie at the same addresses whatever the inputs' stride; then the supergrid arrays, contiguous (pad 0) or
    with ``pad`` poisoned columns after every row."""

    def __init__(self, arena, pad):
        self.arena, self.pad, self.outputs = arena, pad, []

    def out(self, shape, dtype, zero=False, compare=True):
        t = self.arena.take(shape, dtype, owner="output %d" % len(self.outputs))
        if zero:
            t.zero_()
        if compare:
            self.outputs.append(t)
        return t

    def const(self, a):
        import torch
        a = np.ascontiguousarray(a)
        t = self.arena.take(a.shape, torch.from_numpy(a).dtype, owner="input")
        t.copy_(torch.from_numpy(a))
        return t

    def rows(self, a):
        import torch
        t = self.arena.take(a.shape, torch.float64, ld=(a.shape[1] + self.pad) if self.pad else None, owner="strided input")
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return t

    def ld(self, a):
        return a.shape[1] + self.pad

    def bytes(self):
        return [t.cpu().numpy().tobytes() for t in self.outputs]


def stride_cases(api):
    """{entry: fn(S, g, ld_override)}: each takes its buffers from the Strided S and calls the entry"""
    import torch
    L, lib = api.L, api.L.load()
    u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64

    def shape(g):
        return g["mask"].shape

    def mask_seed(S, g, ld=None):
        ny, nx = shape(g)
        p = api.M.params(ny, nx, False, False)
        seeds = np.array([[g["x"][1, 1], g["y"][1, 1]], [g["x"][-2, -2] + 0.3, g["y"][-2, -2] - 0.2], [0.0, 89.0]])
        so = S.out(2 * len(seeds), i64)
        ll, x, y = S.const(seeds), S.rows(g["x"]), S.rows(g["y"])
        L.call("ogg_mask_seed_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]), len(seeds), ll.data_ptr(), so.data_ptr(), stream())

    def runoff_targets(S, g, ld=None):
        import small_meshes as sm
        ny, nx = shape(g)
        lon, lat = sm.source_edges("3x2")
        src = api.R.Source(sm.smooth_field(lon, lat, 1, np.float64), lon, lat)
        p = api.RO.params(ny, nx, src, "coast", False, g["topology"][1], sm.RE)
        wsb = int(lib.ogg_runoff_workspace_bytes(ctypes.byref(p)))
        ws = S.out(wsb, u8, compare=False)
        tc, tu, counts = S.out(ny * nx, i32), S.out((ny * nx, 3), f64), S.out(len(L.RUNOFF_COUNT_FIELDS), i64, zero=True)
        wet, x, y = S.const(g["mask"]), S.rows(g["x"]), S.rows(g["y"])
        L.call("ogg_runoff_targets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]), wet.data_ptr(), ws.data_ptr(), wsb,
               tc.data_ptr(), tu.data_ptr(), counts.data_ptr(), stream())

    def bilinear_source(g):
        import small_meshes as sm
        f, lon, lat, fills = sm.source_for(g["x"], g["y"], "regular", nrec=3, dtype=np.float32, two_fills=True)
        return api.R.Source(f, lon, lat, fill=fills), api.R.Source(f + np.float32(1.0), lon, lat, fill=fills)

    def bilinear(S, g, ld=None, rotate=False):
        ny, nx = shape(g)
        s1, s2 = bilinear_source(g)
        p = api.B.params(ny, nx, s1, "c", 2, 0, False, False, None, False)
        t = {}
        for sfx, kind in zip(("", "2"), ("u", "v")):
            shp = (3,) + api.B.point_shape(ny, nx, kind)
            t["values" + sfx], t["flags" + sfx] = S.out(shp, f64), S.out(shp, u8)
        t["cross"], t["cross2"] = S.out(tuple(t["values"].shape), f64), S.out(tuple(t["values2"].shape), f64)
        for sfx, kind in zip(("", "2"), ("u", "v")):
            for k in ("rot_cos", "rot_sin"):
                t[k + sfx] = S.out(api.B.point_shape(ny, nx, kind), f64) if rotate else None
        lon, lat, f, f2 = S.const(s1.lon), S.const(s1.lat), S.const(s1.records), S.const(s2.records)
        x, y = S.rows(g["x"]), S.rows(g["y"])
        ang = S.rows(g["angle_dx"]) if rotate else None
        dp = lambda k: t[k].data_ptr()   # noqa: E731
        # (the rotation's refusal comes with ld given to it alone: the interpolation before it gets the true stride)
        L.call("ogg_bilinear_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), S.ld(g["x"]) if rotate else (ld or S.ld(g["x"])), lon.data_ptr(),
               lat.data_ptr(), f.data_ptr(), f2.data_ptr(), None, dp("values"), dp("flags"), dp("values2"), dp("flags2"), dp("cross"), dp("cross2"),
               stream())
        if rotate:
            L.call("ogg_bilinear_rotate_dev", ctypes.byref(p), ang.data_ptr(), ld or S.ld(g["x"]), dp("values"), dp("flags"), dp("values2"),
                   dp("flags2"), dp("cross"), dp("cross2"), dp("rot_cos"), dp("rot_sin"), dp("rot_cos2"), dp("rot_sin2"), 1, stream())

    def coast_sets(S, g, ld=None):
        ny, nx = shape(g)
        p = api.CD.params(ny, nx, "both", False, g["topology"][1])
        wsb = int(lib.ogg_coast_workspace_bytes(ctypes.byref(p)))
        nc = ny * nx
        ws = S.out(wsb, u8, compare=False)
        flags, u = S.out((ny, nx), u8), S.out((nc, 3), f64)
        lc, lu, wc, wu = S.out(nc, i32), S.out((nc, 3), f64), S.out(nc, i32), S.out((nc, 3), f64)
        counts = S.out(len(L.COAST_COUNT_FIELDS), i64, zero=True)
        wet, x, y = S.const(g["mask"]), S.rows(g["x"]), S.rows(g["y"])
        L.call("ogg_coast_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]), wet.data_ptr(), ws.data_ptr(), wsb,
               flags.data_ptr(), u.data_ptr(), lc.data_ptr(), lu.data_ptr(), wc.data_ptr(), wu.data_ptr(), counts.data_ptr(), stream())

    def basin_codes(S, g, ld=None):
        import test_gpu_basin_codes as TB
        ny, nx = shape(g)
        lon, lat = float(g["x"][1, 1]), float(g["y"][1, 1])
        rules = api.BC.rules_of([(7, lon, lat) + TB.FULL, (9, float(g["x"][-2, -2]), float(g["y"][-2, -2])) + TB.FULL, (3, lon + 90.0, -lat) + TB.FULL])
        p = api.BC.params(ny, nx, rules, False, g["topology"][1], None, 6371.0e3)
        wsb = int(lib.ogg_basin_workspace_bytes(ctypes.byref(p)))
        ws = S.out(wsb, u8, compare=False)
        code, rule = S.out((ny, nx), u8), S.out((ny, nx), torch.int16)
        rec, counts = S.out(len(rules) * L.BASIN_RECORD.itemsize, u8), S.out(len(L.BASIN_COUNT_FIELDS), i64, zero=True)
        rt, wet, x, y = S.const(rules.table.view(np.uint8)), S.const(g["mask"]), S.rows(g["x"]), S.rows(g["y"])
        L.call("ogg_basin_codes_dev", ctypes.byref(p), rules.table.ctypes.data, rt.data_ptr(), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]),
               wet.data_ptr(), ws.data_ptr(), wsb, code.data_ptr(), rule.data_ptr(), rec.data_ptr(), counts.data_ptr(), stream())

    def locate_sets(S, g, ld=None):
        ny, nx = shape(g)
        p = api.LOC.params(ny, nx, 5, False, g["topology"][1])
        wsb = int(lib.ogg_locate_workspace_bytes(ctypes.byref(p)))
        ws = S.out(wsb, u8, compare=False)
        cu, counts = S.out(((ny + 1) * (nx + 1), 3), f64), S.out(len(L.LOCATE_COUNT_FIELDS), i64, zero=True)
        x, y = S.rows(g["x"]), S.rows(g["y"])
        L.call("ogg_locate_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]), ws.data_ptr(), wsb, cu.data_ptr(),
               counts.data_ptr(), stream())

    return {"ogg_mask_seed_dev": mask_seed, "ogg_runoff_targets_dev": runoff_targets, "ogg_bilinear_dev": bilinear,
            "ogg_bilinear_rotate_dev": lambda S, g, ld=None: bilinear(S, g, ld, rotate=True), "ogg_coast_sets_dev": coast_sets,
            "ogg_basin_codes_dev": basin_codes, "ogg_locate_sets_dev": locate_sets}


LD_ENTRIES = ["ogg_mask_seed_dev", "ogg_runoff_targets_dev", "ogg_bilinear_dev", "ogg_bilinear_rotate_dev", "ogg_coast_sets_dev", "ogg_basin_codes_dev",
              "ogg_locate_sets_dev"]


@pytest.mark.parametrize("name", ["fold_5x7", "1x65"])
@pytest.mark.parametrize("entry", LD_ENTRIES)
def test_row_stride(api, arena, entry, name):
    """ld = 2 nx + 1 + pad, pad in {1, 7}, against ld = 2 nx + 1: every output buffer the same bytes (at the same arena addresses,
    under the same pattern), guards and padding columns intact; ld = 2 nx refused with OGG_EARG."""
    g = grid(name)
    fn = stride_cases(api)[entry]
    nx = g["mask"].shape[1]
    for pattern in PATTERNS:
        got = {}
        for pad in (0, 1, 7):
            arena.reset(pattern)
            S = Strided(arena, pad)
            ACTIVE[0] = True
            try:
                fn(S, g)
            finally:
                ACTIVE[0] = False
            bad = arena.check()
            note(arena, "stride %s %s" % (entry, name))
            assert bad == [], (entry, name, pattern, pad, violations(bad))
            got[pad] = S.bytes()
        for pad in (1, 7):
            same = [a == b for a, b in zip(got[0], got[pad])]
            assert all(same) and len(got[pad]) == len(got[0]), (entry, name, pattern, pad, "outputs that differ: %s" % [k for k, s in enumerate(same) if not s])
    arena.reset("ff")
    with pytest.raises(api.L.OggHipError) as e:
        fn(Strided(arena, 0), g, 2 * nx)
    assert e.value.code == api.L.OGG_EARG
    assert arena.check() == []


# ---- the file stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["device", "host"])
@pytest.mark.parametrize("threads", [1, 3])
def test_file_stream_chunks_and_reuses_its_slots(hip, tmp_path, monkeypatch, stage, threads):
    """DeviceToFile with slots of 4096 bytes and a ring of two: a tensor of 4099 doubles takes nine chunks, the last of 3 doubles, and
    every slot is reused; 513 doubles are one slot and one double more.  Odd multiples of 4 as offsets, gaps between the ranges: every
    range the tensor's big-endian image, every other byte of the file untouched."""
    import torch
    from ocean_model_grid_generator_amd import nc_stream
    if stage == "host":
        monkeypatch.setenv("OGG_NC_STAGE", "host")
    else:
        monkeypatch.delenv("OGG_NC_STAGE", raising=False)
    rng = np.random.default_rng(threads)
    tensors = [torch.from_numpy(rng.standard_normal(n)).to(DEV) for n in (1, 513, 4099)]
    offsets = [4 * 3, 4 * 257, 4 * 2049]                    # 12, 1028, 8196: none a multiple of 8
    ends = [o + 8 * t.numel() for o, t in zip(offsets, tensors)]
    assert all(o % 8 == 4 for o in offsets) and offsets[1] > ends[0] + 100 and offsets[2] > ends[1] + 100
    size = ends[-1] + 4321
    pattern = np.tile(np.arange(251, dtype=np.uint8), size // 251 + 1)[:size]
    path = str(tmp_path / "stream.bin")
    with open(path, "wb") as fh:
        fh.write(pattern.tobytes())
    fd = os.open(path, os.O_RDWR)
    try:
        s = nc_stream.DeviceToFile(fd, DEV, slot_bytes=4096, slots=2, threads=threads)
        assert len(s.ring) == 2 and s.ring[0].numel() == 4096 and (s.stage is None) == (stage == "host")
        for t, o in zip(tensors, offsets):
            s.put(t.view(1, -1), o)
        s.finish()
        assert s.k == 1 + 2 + 9                              # chunks: the ring of two went round six times
    finally:
        os.close(fd)
    got = np.fromfile(path, dtype=np.uint8)
    assert got.size == size
    outside = np.ones(size, bool)
    for t, o, e in zip(tensors, offsets, ends):
        assert got[o:e].tobytes() == t.cpu().numpy().astype(">f8").tobytes(), (t.numel(), o)
        outside[o:e] = False
    assert np.array_equal(got[outside], pattern[outside])
    assert s.bytes == sum(8 * t.numel() for t in tensors)


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def test_every_device_entry_ran_guarded(hip, capsys):
    """The last test of the module (it needs the others to have run): every ogg_*_dev entry of _lib.SIGNATURES ran with its buffers in
    the arena, or stands in NOT_GUARDED with a reason.  A device entry added later without a guarded case fails here."""
    entries = {n for n in hip.SIGNATURES if n.startswith("ogg_") and n.endswith("_dev")}
    with capsys.disabled():
        print("\nguarded memory: peak used() %d bytes handed out, %d bytes of the arena with guards (%s); %d guarded allocations; "
              "%d of %d device entries covered, %d excepted" % (STATS["handed"], STATS["peak"], STATS["peak_case"], STATS["allocations"],
                                                                   len(COVERED & entries), len(entries), len(NOT_GUARDED)))
        print("covered: %s" % " ".join(sorted(COVERED & entries)))
    assert set(NOT_GUARDED) <= entries, sorted(set(NOT_GUARDED) - entries)
    assert not COVERED & set(NOT_GUARDED), sorted(COVERED & set(NOT_GUARDED))
    missing = entries - COVERED - set(NOT_GUARDED)
    assert not missing, "device entries without a guarded case: %s" % sorted(missing)
    assert STATS["peak"] <= PEAK_USED, "the largest case has grown: measure again and size the arena at twice its used()"

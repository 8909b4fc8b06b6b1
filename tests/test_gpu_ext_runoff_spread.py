"""The device entries of the runoff spreading (ogg_spread_sets_dev / _count_dev / _pairs_dev / _apply_dev) held to their extents with
the harness of tests/test_gpu_extents.py: every case runs plain, with every byte of the arena 0xFF and with seeded random bytes; the
guard bands must be intact and the three results the same bytes.  The sets step, which takes the row strides of the supergrid points
and of the supergrid area, is also called directly with padded rows.  The cases are recorded in that module's COVERED set, which its
census (test_every_device_entry_ran_guarded) reads: this module's name sorts before it, so in a run of the whole GPU suite the
entries are covered when the census runs."""
import ctypes

import numpy as np
import pytest

import small_meshes as sm
import test_gpu_extents as TE
from test_gpu_extents import arena, record_entries, three_runs, stream, up   # noqa: F401  (fixtures and helpers of the harness)

pytestmark = pytest.mark.gpu
RE = 6371.0e3
FAR_BELOW = TE.PEAK_USED // 4
ENTRIES = {"ogg_spread_sets_dev", "ogg_spread_count_dev", "ogg_spread_pairs_dev", "ogg_spread_apply_dev"}


@pytest.fixture(scope="module")
def RO(hip):
    from ocean_model_grid_generator_amd import runoff
    return runoff


def regional(ny=3, nx=65, seed=3):
    g = sm.latlon_grid(ny, nx, lon0=30.25, lat0=20.5, dlon=0.5, dlat=0.75)
    rng = np.random.default_rng(seed)
    wet = (rng.random((ny, nx)) < 0.85).astype(np.uint8)
    load = ((wet != 0) & (rng.random((ny, nx)) < 0.3)).astype(np.int32)
    cls = (np.arange(nx)[None, :] // 22 + np.zeros((ny, 1), int)).astype(np.int32)
    v = np.where(load > 0, rng.random((3, ny, nx)) * 1e-4, 0.0)
    v[0][load > 0] *= -1.0
    return g, wet, load, cls, v


@pytest.mark.parametrize("shape", ["biweight", "uniform"])
@pytest.mark.parametrize("classes", [True, False])
def test_the_four_steps_on_a_regional_grid(RO, arena, three_runs, shape, classes):
    g, wet, load, cls, v = regional()

    def run():
        return RO.spread_dev(up(v), up(g["x"]), up(g["y"]), up(g["area"]), up(wet), load=up(load), radius_km=400.0, shape=shape,
                             classes=up(cls) if classes else None, Re=RE, keep_lists=True)
    res = three_runs(run, "spread 3x65 %s classes=%s" % (shape, classes))
    assert ENTRIES <= TE.COVERED
    assert res["counts"]["mouths"] > 20 and res["counts"]["max_mouths"] > 3 and res["counts"]["pairs"] > 5 * res["counts"]["mouths"]
    assert arena.used(guards=True) < FAR_BELOW


@pytest.mark.parametrize("name", ["1x1", "129x1", "fold_5x7", "band_3x2"])
def test_the_four_steps_on_the_small_shapes(RO, arena, three_runs, name):
    g = sm.shape_grid(name)
    ny, nx = (g["x"].shape[0] - 1) // 2, (g["x"].shape[1] - 1) // 2
    rng = np.random.default_rng(ny + nx)
    wet = np.ones((ny, nx), np.uint8)
    load = (rng.random((ny, nx)) < 0.5).astype(np.int32)
    load.flat[-1] = 1
    v = rng.standard_normal((2, ny, nx)) * load
    for km in (1.0, 2500.0, 25000.0):
        res = three_runs(lambda: RO.spread_dev(v, up(g["x"]), up(g["y"]), up(g["area"]), wet, load=load, radius_km=km, Re=RE,
                                               keep_lists=True), "spread %s %g km" % (name, km))
        assert res["counts"]["mouths"] == int(load.sum())
    assert arena.used(guards=True) < FAR_BELOW


def sets_call(RO, hip, S, g, wet, load, ld=None, lda=None):
    """ogg_spread_sets_dev with every buffer in the arena: the outputs and the workspace first, then the inputs, the supergrid arrays
    with the Strided's padding"""
    import torch
    ny, nx = wet.shape
    p = RO.spread_params(ny, nx, 1, RO.radius2(300.0, RE))
    wsb = int(hip.load().ogg_spread_workspace_bytes(ctypes.byref(p), 0))
    ws = S.out(wsb, torch.uint8, compare=False)
    nc = ny * nx
    u, A, cand, mc = S.out((nc, 3), torch.float64), S.out(nc, torch.float64), S.out(nc, torch.uint8), S.out(nc, torch.int32)
    counts = S.out(len(hip.SPREAD_COUNT_FIELDS), torch.int64, zero=True)
    wt, lt = S.const(wet), S.const(load)
    x, y, a = S.rows(g["x"]), S.rows(g["y"]), S.rows(g["area"])
    hip.call("ogg_spread_sets_dev", ctypes.byref(p), x.data_ptr(), y.data_ptr(), ld or S.ld(g["x"]), a.data_ptr(), lda or S.ld(g["area"]),
             wt.data_ptr(), lt.data_ptr(), ws.data_ptr(), wsb, u.data_ptr(), A.data_ptr(), cand.data_ptr(), mc.data_ptr(), counts.data_ptr(),
             stream())


@pytest.mark.parametrize("shape", [(3, 65), (5, 7)])
def test_row_strides_of_the_sets_step(RO, hip, arena, shape):
    """ld = 2 nx + 1 + pad and lda = 2 nx + pad, pad in {1, 7}, against the contiguous call: every output the same bytes (at the same
    arena addresses, under the same pattern), guards and padding columns intact; ld = 2 nx and lda = 2 nx - 1 refused with OGG_EARG."""
    g, wet, load, cls, v = regional(*shape)
    nx = shape[1]
    for pattern in TE.PATTERNS:
        got = {}
        for pad in (0, 1, 7):
            arena.reset(pattern)
            S = TE.Strided(arena, pad)
            TE.ACTIVE[0] = True
            try:
                sets_call(RO, hip, S, g, wet, load)
            finally:
                TE.ACTIVE[0] = False
            bad = arena.check()
            TE.note(arena, "stride ogg_spread_sets_dev %dx%d" % shape)
            assert bad == [], (pattern, pad, TE.violations(bad))
            got[pad] = S.bytes()
        for pad in (1, 7):
            assert got[pad] == got[0], (pattern, pad)
    for kw in (dict(ld=2 * nx), dict(lda=2 * nx - 1)):
        arena.reset("ff")
        with pytest.raises(hip.OggHipError) as e:
            sets_call(RO, hip, TE.Strided(arena, 0), g, wet, load, **kw)
        assert e.value.code == hip.OGG_EARG
        assert arena.check() == []

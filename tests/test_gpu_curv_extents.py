"""The device entries of the curvilinear-source exchange grid (ogg_xgrid_curv_sets_dev / _clip_dev / _write_dev) held to their extents
with the harness of tests/test_gpu_extents.py: every case runs plain, with every byte of the arena 0xFF and with seeded random bytes;
the guard bands must be intact and the three results the same bytes.  The cases are recorded in that module's COVERED set, which its
census (test_every_device_entry_ran_guarded) reads: this module's name sorts before it, so in a run of the whole GPU suite the
entries are covered when the census runs."""
import numpy as np
import pytest

import test_gpu_extents as TE
import xgrid_cs_definition as cd
import xgrid_curv_definition as vd
from test_gpu_extents import arena, record_entries, three_runs, stream, up   # noqa: F401  (fixtures and helpers of the harness)

pytestmark = pytest.mark.gpu
RE = 6371.0e3
FAR_BELOW = TE.PEAK_USED // 4


@pytest.fixture(scope="module")
def XC(hip):
    from ocean_model_grid_generator_amd import exchange_grid_curv
    return exchange_grid_curv


def band_of(hip, xt, yt, nxp, nyp, j0, n, mask, threshold):
    band = hip.XgridBand(nx=nxp - 1, ny=nyp - 1, j0=j0, n_cell_rows=n, Re=RE, threshold=threshold)
    band.x, band.y = xt[j0:].data_ptr(), yt[j0:].data_ptr()
    band.x_next, band.y_next = xt[j0 + n:].data_ptr(), yt[j0 + n:].data_ptr()
    band.mask = None if mask is None else mask.data_ptr()
    return band


def lists(hip, XC, x, y, sx, sy, splits, mask=None, src_mask=None, pad=0, threshold=1e-6):
    """band_lists_dev of every band (first cell row, cell rows) of ``splits``, everything on the device; the source's rows padded by
    ``pad`` doubles that nothing writes"""
    import torch
    nyp, nxp = x.shape
    NB, NA = sx.shape[0] - 1, sx.shape[1] - 1
    xt, yt = up(x), up(y)
    if pad:
        sxt, syt = (torch.empty((NB + 1, NA + 1 + pad), dtype=torch.float64, device=TE.DEV) for _ in range(2))
        sxt[:, :NA + 1], syt[:, :NA + 1] = up(sx), up(sy)
    else:
        sxt, syt = up(sx), up(sy)
    smt = None if src_mask is None else up(src_mask)
    desc = XC.src_desc(sxt.data_ptr(), syt.data_ptr(), NA, NB, ld=NA + 1 + pad, mask_ptr=None if smt is None else smt.data_ptr())
    mt = None if mask is None else up(mask)
    out = []
    for j0, n in splits:
        m0 = (j0 + 1) // 2
        rows = None if mt is None else mt[m0:]
        out.append(XC.band_lists_dev(band_of(hip, xt, yt, nxp, nyp, j0, n, rows, threshold), desc, stream(), TE.DEV))
    return out


CASES = {
    "one_rank": dict(splits=[(0, 6)]),
    "three_ranks": dict(splits=[(0, 3), (3, 1), (4, 2)]),      # the middle band holds no model row
    "padded_rows": dict(splits=[(0, 6)], pad=3),
    "masked": dict(splits=[(0, 2), (2, 4)], masks=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lists_of_a_regional_grid(hip, XC, arena, three_runs, name):
    case = CASES[name]
    x, y = cd.regional(30.25, 20.5, 0.5, 0.75, 65, 3)[:2]
    sx, sy = vd.rotated_mesh(46.5, 21.625, 36.0, 6.0, 96, 16, angle=0.05)
    rng = np.random.default_rng(4)
    mask = (rng.random((3, 65)) < 0.6).astype(np.uint8) if case.get("masks") else None
    smask = (rng.random((16, 96)) < 0.6).astype(np.uint8) if case.get("masks") else None
    got = three_runs(lambda: lists(hip, XC, x, y, sx, sy, case["splits"], mask, smask, case.get("pad", 0)), "xgrid_curv " + name)
    whole = three_runs(lambda: lists(hip, XC, x, y, sx, sy, [(0, 6)], mask, smask), "xgrid_curv whole " + name)[0]
    for k in (4, 5, 6):   # src, ocn, area of the bands, one after the other, are the whole grid's
        cat = b"".join(p[k][3] for p in got)
        assert cat == whole[k][3], (name, k)
    assert len(whole[6][3]) > 8 * (64 if case.get("masks") else 1025)
    assert arena.used(guards=True) < FAR_BELOW


def test_an_empty_list(hip, XC, arena, three_runs):
    x, y, _ = cd.zoo()["regional_2x3"]
    sx, sy = vd.regular_mesh(100.0, -40.0, 1.0, 1.0, 3, 3)
    got = three_runs(lambda: lists(hip, XC, x, y, sx, sy, [(0, 4)]), "xgrid_curv empty")[0]
    assert got[6][2] == (0,) and got[4][2] == (0, 2)
    assert arena.used(guards=True) < FAR_BELOW


def test_the_cell_of_1600_pairs(hip, XC, arena, three_runs):
    x, y = cd.one_cell([(0.0, -10.0), (20.0, -10.0), (20.0, 10.0), (0.0, 10.0)])
    sx, sy = vd.regular_mesh(-1.25, -11.25, 0.5, 0.5, 45, 45)
    got = three_runs(lambda: lists(hip, XC, x, y, sx, sy, [(0, 2)], threshold=0.0), "xgrid_curv 1600 pairs")[0]
    assert got[6][2][0] >= 1600
    assert arena.used(guards=True) < FAR_BELOW

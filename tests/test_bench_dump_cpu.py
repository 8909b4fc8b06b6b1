"""CPU tests of bench.py --dump-outputs: the rows it writes are the rows of the stitched supergrid (what main() returns), whatever
the band split, every row when the grid fits in the limit and a fixed seeded sample of whole rows when it does not.  The band buffers
are allocated in host memory and filled with values that encode (sub-grid, field, row, column), so no kernel is needed."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import ogg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _plan(sg_mod, r, **kw):
    Ni = int(r * 2 * 360)
    phi_s, phi_n = (-68.0, 65.0) if r == 2 else (-66.85954725, 64.05895973)
    y0, y1 = orc.mercator_y_star(Ni, phi_s, phi_n, True, kw.get("ensure_nj_even", False))
    return sg_mod.SupergridPlan(r, mercator_axis=(y0, orc.phi_mercator(Ni, np.arange(y0, y1 + 1))), **kw)


def _fill(plan, grids, fields):
    for g in grids:
        for k, s in enumerate(plan.subs):
            b = g.buf[s.name]
            for fi, f in enumerate(fields):
                t = b[f]
                rows = torch.arange(t.shape[0], dtype=torch.float64)[:, None] + b["lo"]
                cols = torch.arange(t.shape[1], dtype=torch.float64)[None, :]
                t.copy_(k * 1e9 + fi * 1e8 + rows * 1e4 + cols)


@pytest.mark.parametrize("r,flags", [(2.0, {}), (4.0, dict(r_dp=0.2, south_cutoff_row=83)), (1.0, dict(r_dp=0.2, ensure_nj_even=True))],
                         ids=["r2", "r4_om4", "r1_dp"])
@pytest.mark.parametrize("world,limit", [(1, 10 ** 10), (3, 10 ** 10), (3, 200_000), (2, None)],
                         ids=["one_rank", "three_ranks", "three_ranks_sampled", "default_limit"])
def test_dump_is_the_stitched_grid(tmp_path, r, flags, world, limit):
    from ocean_model_grid_generator_amd import supergrid as S
    b = _bench()
    if limit is not None:
        b.DUMP_LIMIT_BYTES = limit
    plan = _plan(S, r, **flags)
    grids = [S.Supergrid(plan, rank=q, world=world, device="cpu", halo="recompute") for q in range(world)]
    _fill(plan, grids, S.FIELDS)
    cut = plan.south_cut()
    n_point, n_cell = grids[0]._pieces(cut, True)[1], grids[0]._pieces(cut, False)[1]
    rows = b.dump_rows(plan, n_point, n_cell)
    assert np.array_equal(rows[0], b.dump_rows(plan, n_point, n_cell)[0])   # the same sample on every run
    b.write_dump(str(tmp_path), rows, [b.take_dump_rows(g, cut, rows, torch) for g in grids])
    want = S.stitch(plan, [g.bands_to_host() for g in grids])
    assert want["x"].shape[0] == n_point and want["dy"].shape[0] == n_cell
    if limit == 10 ** 10:
        assert len(rows[0]) == n_point and len(rows[1]) == n_cell
    elif limit is not None:
        assert 0 < len(rows[0]) < n_point and 0 < len(rows[1]) < n_cell
    assert np.all(np.diff(rows[0]) > 0) and np.all(np.diff(rows[1]) > 0)
    for f in S.FIELDS:
        got = np.load(str(tmp_path / (f + ".npy")))
        sel = rows[0] if f in ("x", "y", "dx", "angle_dx") else rows[1]
        assert got.dtype == np.float64 and np.array_equal(got, want[f][sel]), f
    assert np.array_equal(np.load(str(tmp_path / "rows_point.npy")), rows[0].astype(np.float64))
    assert sum(os.path.getsize(str(tmp_path / n)) for n in os.listdir(str(tmp_path))) <= b.DUMP_LIMIT_BYTES

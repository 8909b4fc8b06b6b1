"""Time the conservative regrid to a lat-lon grid (csrc/ogg_regrid.hip) at 1/8 degree (2196 x 2880 model cells) with generated fields.

    python scripts/regrid_profile.py [--res 8] [--reps 20] [--cases a b] [--targets 1 0.25] [--json OUT] [--baseline]

Cases: (a) 12 float32 records, land as the fill value; (b) 57 float32 levels, the land growing with depth.  Targets: regular global
grids of 1 and 0.25 degree.  HIP-event medians of --reps runs after one warm-up, each step on its own: the list build
(Supergrid.xgrid_lists with the target's edges), the transpose step, the regrid step (normalize area, no cover) for every
OGG_REGRID_RECORDS value and three OGG_REGRID_LONG values, the static sums alone, and in the same process a torch read of the field's bytes and a 1 GiB fill_.
--baseline adds the numpy definition's rate on one core (tests/latlon_regrid_definition.py).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def land(lon, lat, level=0.0):
    """a generated coastline: True on land (grows with level)"""
    L, P = np.radians(lon), np.radians(lat)
    z = np.sin(2 * L) * np.cos(3 * P) + 0.6 * np.sin(5 * L + 1.0) * np.sin(4 * P) + 0.4 * np.cos(7 * L - 2 * P)
    return (z > 0.55 - level) | (lat < -78) | (lat > 86)


def field(cx, cy, case):
    nrec = 12 if case == "a" else 57
    f = np.empty((nrec,) + cx.shape, np.float32)
    for r in range(nrec):
        v = 28.0 * np.cos(np.radians(cy)) + 2.0 * np.sin(np.radians(cx) * 2 + r) - (0 if case == "a" else 0.4 * r)
        f[r] = np.where(land(cx, cy, 0.0 if case == "a" else 0.012 * r), 1e20, v)
    return f


def median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def time_case(g, cut, fd, case, deg, reps):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import exchange_grid as X
    from ocean_model_grid_generator_amd import latlon_regrid as G
    nrec, ny, nx = fd.shape
    lon, lat = X.regular_atm(int(round(360 / deg)), int(round(180 / deg)))
    dev = g.device
    edges = (torch.from_numpy(lon).to(dev), torch.from_numpy(lat).to(dev))
    halo = g.xgrid_halo(cut)
    t_list, _ = median_ms(lambda: g.xgrid_lists(cut, edges, None, halo=halo), reps)
    pieces = g.xgrid_lists(cut, edges, None, halo=halo)   # piece order: the concatenation is the whole grid's list
    atm, ocn, area = (torch.cat([e[i] for e in pieces]).contiguous() for i in (4, 5, 6))
    p = G.params((ny, nx), lon, lat, None)   # then the field's own: it lives on the device already
    p.nrec, p.dtype, p.n_fill = nrec, L.REMAP_FLOAT32, 1
    p.fill[0] = float(np.float32(1e20))
    L.call("ogg_regrid_check", ctypes.byref(p))
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = L.load()
    n = int(area.numel())
    wsb = int(lib.ogg_regrid_workspace_bytes(ctypes.byref(p), n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    a_atm = torch.from_numpy(np.ascontiguousarray(X.atm_area(lon, lat, float(g.plan.Re)))).to(dev)
    NB, NA = lat.size - 1, lon.size - 1
    values = torch.empty((nrec, NB, NA), dtype=torch.float64, device=dev)
    frac = torch.empty((NB, NA), dtype=torch.float64, device=dev)
    nent = torch.empty((NB, NA), dtype=torch.int32, device=dev)
    ct = torch.zeros(len(L.REGRID_COUNT_FIELDS), dtype=torch.int64, device=dev)
    tr = lambda: L.call("ogg_regrid_transpose_dev", ctypes.byref(p), atm.data_ptr(), ocn.data_ptr(), area.data_ptr(), n,   # noqa: E731
                        ws.data_ptr(), wsb, ct.data_ptr(), st)
    rg = lambda: L.call("ogg_regrid_dev", ctypes.byref(p), fd.data_ptr(), a_atm.data_ptr(), n, ws.data_ptr(), wsb,   # noqa: E731
                        values.data_ptr(), None, None, None, ct.data_ptr(), st)
    sm = lambda: L.call("ogg_regrid_dev", ctypes.byref(p), None, a_atm.data_ptr(), n, ws.data_ptr(), wsb, None, None,   # noqa: E731
                        frac.data_ptr(), nent.data_ptr(), ct.data_ptr(), st)
    t_tr, _ = median_ms(tr, reps)
    tr()
    t_rg = {}
    for rec in ("1", "2", "4", "8"):
        os.environ["OGG_REGRID_RECORDS"] = rec
        t_rg[rec], _ = median_ms(rg, reps)
    os.environ.pop("OGG_REGRID_RECORDS")
    t_long = {}
    for ln in ("128", "512", "4096"):
        os.environ["OGG_REGRID_LONG"] = ln
        t_long[ln], _ = median_ms(rg, reps)
    os.environ.pop("OGG_REGRID_LONG")
    t_static, _ = median_ms(sm, reps)
    tr()
    rg()
    c_rg = G.counts_dict(ct.cpu().numpy())   # the regrid step's counts (each call starts them from zero)
    sm()
    c = G.counts_dict(ct.cpu().numpy())
    with_entries = int((nent > 0).sum().item())
    t_read, _ = median_ms(lambda: fd.sum(dtype=torch.float64), reps)
    fbytes = fd.numel() * 4
    best = t_rg[str(4)]
    return {"case": case, "target_deg": deg, "records": nrec, "cells": [ny, nx], "target": [NB, NA], "entries": n, "counts": c,
            "valid_pairs": c_rg["valid"], "empty_pairs": c_rg["empty"], "cells_with_entries": with_entries,
            "largest_n_entries": int(nent.max().item()), "mean_n_entries": n / max(with_entries, 1),
            "ms_list": t_list, "ms_transpose": t_tr, "ms_regrid_by_records": t_rg, "ms_regrid_by_long": t_long, "ms_regrid": best, "ms_static": t_static,
            "ms_torch_read_field": t_read, "field_bytes": fbytes, "regrid_over_torch_read": best / t_read,
            "regrid_field_TBps": fbytes / (best * 1e-3) / 1e12}


def baseline():
    """(record, target cell) pairs per second of the numpy definition on one core: case (a) on a 1/8-degree band against 1 degree"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import latlon_regrid_definition as D

    from ocean_model_grid_generator_amd import exchange_grid as X
    x, y = np.meshgrid(-300.0 + 0.125 * np.arange(2881), -10.0 + 0.125 * np.arange(161))
    lon, lat = X.regular_atm(360, 180)
    lists = X.exchange_grid(x, y, lon, lat)
    ny, nx = lists["a_poly"].shape
    f = field(x[1::2, 1::2] % 360, y[1::2, 1::2], "a")
    t0 = time.perf_counter()
    v, _ = D.regrid(lists["atm"], lists["ocn"], lists["area"], f, lists["a_atm"], fills=(1e20,))
    dt = time.perf_counter() - t0
    return {"entries": int(lists["area"].size), "records": int(f.shape[0]), "s": dt, "entries_x_records_per_s": lists["area"].size * f.shape[0] / dt}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--cases", nargs="*", default=["a", "b"])
    p.add_argument("--targets", type=float, nargs="*", default=[1.0, 0.25])
    p.add_argument("--json", default=None)
    p.add_argument("--baseline", action="store_true")
    a = p.parse_args(argv)
    out = []
    if a.cases:
        import torch

        from ocean_model_grid_generator_amd import supergrid as SG
        plan = SG.SupergridPlan(inverse_resolution=a.res, ensure_nj_even=True)
        g = SG.Supergrid(plan, device="cuda:0")
        g.run_pass()
        cut = g.south_cut()
        x, y = g.stitched_xy(cut)
        cx, cy = x[1::2, 1::2].cpu().numpy() % 360.0, y[1::2, 1::2].cpu().numpy()
        buf = torch.empty(1 << 27, dtype=torch.float64, device="cuda:0")
        t_fill, _ = median_ms(lambda: buf.fill_(1.0), a.reps)
        del buf
        out.append({"ms_torch_fill_1GiB": t_fill, "fill_TBps": (1 << 30) / (t_fill * 1e-3) / 1e12})
        print(json.dumps(out[-1]))
        for case in a.cases:
            fd = torch.from_numpy(field(cx, cy, case)).to("cuda:0")
            for deg in a.targets:
                r = time_case(g, cut, fd, case, deg, a.reps)
                print(json.dumps(r))
                out.append(r)
            del fd
            torch.cuda.empty_cache()
    if a.baseline:
        b = baseline()
        print(json.dumps({"numpy_baseline": b}))
        out.append({"numpy_baseline": b})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

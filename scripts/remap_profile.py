"""Time the conservative remap (csrc/ogg_remap.hip) at 1/8 degree (2196 x 2880 model cells) with generated 1/4-degree sources.

    python scripts/remap_profile.py [--res 8] [--reps 20] [--cases a b] [--json OUT] [--baseline] [--write_sources DIR]

Cases: (a) 12 float32 records, SST-like (land missing); (b) 57 float32 levels, the land growing with depth.  The model's wet mask
comes from a coastline that differs from the source's, so the fill has work.  HIP-event medians of --reps runs after one warm-up, each
step on its own: the list build (Supergrid.xgrid_lists with the source's edges), the segment step, the remap step (with the entries
kept in registers across records, OGG_REMAP_CACHE=1, the default, and re-read per record, 0), the fill step (its fronts and
launches), and a torch fill of the remap's output bytes in the same process.  --baseline adds the numpy definition's rate on one
core (tests/remap_definition.py).  --write_sources writes case (b)'s source and a matching bathymetry as NetCDF-3 files.
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


def source(case):
    lon = 360.0 * np.arange(1441) / 1440
    lat = -90.0 + 180.0 * np.arange(721) / 720
    lc, pc = np.meshgrid(0.5 * (lon[1:] + lon[:-1]), 0.5 * (lat[1:] + lat[:-1]))
    nrec = 12 if case == "a" else 57
    f = np.empty((nrec, 720, 1440), np.float32)
    for r in range(nrec):
        v = 28.0 * np.cos(np.radians(pc)) + 2.0 * np.sin(np.radians(lc) * 2 + r) - (0 if case == "a" else 0.4 * r)
        f[r] = np.where(land(lc, pc, 0.0 if case == "a" else 0.012 * r), 1e20, v)
    return lon, lat, f


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


def time_case(g, cut, case, reps):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import ocean_mask as M
    from ocean_model_grid_generator_amd import remap as R
    lon, lat, f = source(case)
    src = R.Source(f, lon, lat, fill=(1e20,))
    x, y = g.stitched_xy(cut)
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    cx, cy = x[1::2, 1::2].cpu().numpy(), y[1::2, 1::2].cpu().numpy()
    wet = (~land(cx % 360.0, cy, 0.03)).astype(np.uint8)     # the model's coast lies off the source's
    dev = g.device
    mt = torch.from_numpy(wet).to(dev)
    edges = (torch.from_numpy(src.lon).to(dev), torch.from_numpy(src.lat).to(dev))
    halo = g.xgrid_halo(cut)
    t_list, _ = median_ms(lambda: g.xgrid_lists(cut, edges, mt, halo=halo), reps)
    pieces = g.xgrid_lists(cut, edges, mt, halo=halo)   # piece order: the concatenation is the whole grid's list
    atm, ocn, area = (torch.cat([e[i] for e in pieces]).contiguous() for i in (4, 5, 6))
    counts = torch.stack([e[2] for e in pieces]).sum(dim=0)
    periodic, fold = M.topology_of_device_grid(x, y)
    p = R.params(ny, nx, src, 0, periodic, fold)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = L.load()
    wsb = int(lib.ogg_remap_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    fd = torch.from_numpy(src.records).to(dev)
    shape = (src.nrec, ny, nx)
    values = torch.empty(shape, dtype=torch.float64, device=dev)
    flags = R.flags_buffer(torch, values.numel(), dev).view(shape)
    ct = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
    n = int(area.numel())
    seg = lambda: L.call("ogg_remap_segments_dev", ctypes.byref(p), ocn.data_ptr(), n, ws.data_ptr(), wsb, st)   # noqa: E731
    rem = lambda: L.call("ogg_remap_dev", ctypes.byref(p), fd.data_ptr(), atm.data_ptr(), area.data_ptr(), n, mt.data_ptr(),   # noqa: E731
                         ws.data_ptr(), wsb, values.data_ptr(), flags.data_ptr(), ct.data_ptr(), st)
    t_seg, _ = median_ms(seg, reps)
    seg()
    t_rem = {}
    for cache in ("1", "0"):
        os.environ["OGG_REMAP_CACHE"] = cache
        t_rem[cache], _ = median_ms(rem, reps)
    os.environ.pop("OGG_REMAP_CACHE")
    v0, f0 = values.clone(), flags.clone()

    def fill():
        values.copy_(v0)
        flags.copy_(f0)
        L.call("ogg_remap_fill_dev", ctypes.byref(p), ws.data_ptr(), wsb, values.data_ptr(), flags.data_ptr(), ct.data_ptr(), st)
    t_copy, _ = median_ms(lambda: (values.copy_(v0), flags.copy_(f0)), reps)
    t_fill_all, _ = median_ms(fill, reps)
    rem()
    fill()
    c = R.counts_dict(ct.cpu().numpy())
    t_torch, _ = median_ms(lambda: (values.fill_(1.0), flags.fill_(1)), reps)
    out_bytes = values.numel() * 9
    t_fill = t_fill_all - t_copy
    return {"case": case, "records": src.nrec, "cells": [ny, nx], "entries": n, "exchange_counts": {f: int(v) for f, v in zip(L.XGRID_COUNT_FIELDS, counts.cpu().numpy())}, "counts": c,
            "ms_list": t_list, "ms_segments": t_seg, "ms_remap_cached": t_rem["1"], "ms_remap_reread": t_rem["0"], "ms_fill": t_fill,
            "fill_us_per_launch": 1e3 * t_fill / max(c["launches"], 1), "ms_torch_fill_same_bytes": t_torch, "out_bytes": out_bytes,
            "remap_over_torch_fill": min(t_rem.values()) / t_torch, "remap_TBps": out_bytes / (min(t_rem.values()) * 1e-3) / 1e12}


def baseline():
    """(record, cell) pairs per second of the numpy definition on one core: case (a) on 40 rows of a 1/4-degree lat-lon band"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import remap_definition as D

    from ocean_model_grid_generator_amd import exchange_grid as X
    x, y = np.meshgrid(-300.0 + 0.125 * np.arange(2881), -10.0 + 0.125 * np.arange(81))
    lon, lat, f = source("a")
    lists = X.exchange_grid(x, y, lon, lat)
    ny, nx = lists["a_poly"].shape
    t0 = time.perf_counter()
    v, fl = D.remap(lists["atm"], lists["ocn"], lists["area"], f, ny, nx, fills=(1e20,))
    v, fl, _ = D.fill(v, fl, True, False)
    dt = time.perf_counter() - t0
    return {"pairs": int(v.size), "s": dt, "pairs_per_s": v.size / dt}


def write_sources(d):
    from ocean_model_grid_generator_amd import netcdf3
    os.makedirs(d, exist_ok=True)
    lon, lat, f = source("b")
    lc, pc = 0.5 * (lon[1:] + lon[:-1]), 0.5 * (lat[1:] + lat[:-1])
    ds = netcdf3.Dataset(os.path.join(d, "woa_like.nc"), [("depth", f.shape[0]), ("lat", 720), ("lon", 1440)])
    ds.def_var("depth", netcdf3.NC_DOUBLE, ("depth",), [("units", "m")], 10.0 * np.arange(f.shape[0]) ** 1.5)
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "degrees_north")], pc)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "degrees_east")], lc)
    ds.def_var("t_an", netcdf3.NC_FLOAT, ("depth", "lat", "lon"), [("units", "degC"), ("_FillValue", 1e20)], f)
    ds.write()
    L, P = np.meshgrid(lc, pc)
    z = np.where(land(L, P, 0.03), 300.0, -4000.0).astype(np.int16)
    ds = netcdf3.Dataset(os.path.join(d, "bathy.nc"), [("lat", 720), ("lon", 1440)])
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "degrees_north")], pc)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "degrees_east")], lc)
    ds.def_var("elevation", netcdf3.NC_SHORT, ("lat", "lon"), [("units", "m")], z)
    ds.write()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--cases", nargs="*", default=["a", "b"])
    p.add_argument("--json", default=None)
    p.add_argument("--baseline", action="store_true")
    p.add_argument("--write_sources", default=None)
    a = p.parse_args(argv)
    out = []
    if a.write_sources:
        write_sources(a.write_sources)
    if a.cases:
        from ocean_model_grid_generator_amd import supergrid as SG
        plan = SG.SupergridPlan(inverse_resolution=a.res, ensure_nj_even=True)
        g = SG.Supergrid(plan, device="cuda:0")
        g.run_pass()
        cut = g.south_cut()
        for case in a.cases:
            r = time_case(g, cut, case, a.reps)
            print(json.dumps(r))
            out.append(r)
    if a.baseline:
        b = baseline()
        print(json.dumps({"numpy_baseline": b}))
        out.append({"numpy_baseline": b})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

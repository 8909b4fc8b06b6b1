"""Time the bilinear interpolation (csrc/ogg_bilinear.hip) at 1/8 degree (2196 x 2880 model cells) with the remap profile's generated
1/4-degree float32 sources, next to the conservative remap kernel on the same grid and source, in one process.

    python scripts/bilinear_profile.py [--res 8] [--reps 20] [--cases a b] [--json OUT] [--kernel_only N]

Cases (scripts/remap_profile.py): (a) 12 float32 records, (b) 57 float32 levels.  HIP-event medians of --reps runs after one warm-up:
locate + interpolate of a scalar at the h points; of a vector at the h points, with the rotation; a torch fill of the scalar's output
bytes (values and flags); the remap kernel (ogg_remap_dev, entries kept in registers) on the same grid, source and mask.  The ratios
are per output byte.  Every timed call goes through ctypes and reads its knobs from the environment, the remap kernel's as well, so a
few microseconds of host launch cost are inside each figure and the ratios are fair.  --kernel_only N: nothing is timed; the scalar
kernel of the first case runs N times, for a counter run (rocprofv3 --pmc ... -- python scripts/bilinear_profile.py --kernel_only 3),
which must not be combined with tracing.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from remap_profile import land, median_ms, source   # noqa: E402


def setup(g, cut, case):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import bilinear as B
    from ocean_model_grid_generator_amd import remap as R
    lon, lat, f = source(case)
    src = R.Source(f, lon, lat, fill=(1e20,))
    x, y = g.stitched_xy(cut)
    angle = g.stitched_angle(cut)
    ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
    cx, cy = x[1::2, 1::2].cpu().numpy(), y[1::2, 1::2].cpu().numpy()
    wet = (~land(cx % 360.0, cy, 0.03)).astype(np.uint8)
    dev = g.device
    k = dict(src=src, x=x, y=y, angle=angle, ny=ny, nx=nx, dev=dev, st=torch.cuda.current_stream(dev).cuda_stream,
             mt=torch.from_numpy(wet).to(dev), lon=torch.from_numpy(src.lon).to(dev), lat=torch.from_numpy(src.lat).to(dev),
             fd=torch.from_numpy(src.records).to(dev))
    k["fd2"] = k["fd"].clone()
    shape = (src.nrec, ny, nx)
    for sfx in ("", "2"):
        k["values" + sfx] = torch.empty(shape, dtype=torch.float64, device=dev)
        k["flags" + sfx] = R.flags_buffer(torch, src.nrec * ny * nx, dev).view(shape)
    k["rc"], k["rs"] = (torch.empty((ny, nx), dtype=torch.float64, device=dev) for _ in range(2))
    ps = B.params(ny, nx, src, "h", 1, has_mask=True)
    pv = B.params(ny, nx, src, "h", 2, has_mask=True)
    nxp = x.shape[1]

    def scalar():
        L.call("ogg_bilinear_dev", ctypes.byref(ps), x.data_ptr(), y.data_ptr(), nxp, k["lon"].data_ptr(), k["lat"].data_ptr(),
               k["fd"].data_ptr(), None, k["mt"].data_ptr(), k["values"].data_ptr(), k["flags"].data_ptr(), None, None, None, None, k["st"])

    def vector():   # the same field as both components: the same gathers as two fields of this size, twice the output
        L.call("ogg_bilinear_dev", ctypes.byref(pv), x.data_ptr(), y.data_ptr(), nxp, k["lon"].data_ptr(), k["lat"].data_ptr(),
               k["fd"].data_ptr(), k["fd2"].data_ptr(), k["mt"].data_ptr(), k["values"].data_ptr(), k["flags"].data_ptr(),
               k["values2"].data_ptr(), k["flags2"].data_ptr(), None, None, k["st"])
        L.call("ogg_bilinear_rotate_dev", ctypes.byref(pv), angle.data_ptr(), nxp, k["values"].data_ptr(), k["flags"].data_ptr(),
               k["values2"].data_ptr(), k["flags2"].data_ptr(), None, None, k["rc"].data_ptr(), k["rs"].data_ptr(), None, None, 1, k["st"])
    k["scalar"], k["vector"] = scalar, vector
    return k


def remap_kernel(g, cut, k):
    """the conservative remap's kernel on the same grid, source and mask (its list built and its segments found first)"""
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import remap as R
    src, dev, ny, nx = k["src"], k["dev"], k["ny"], k["nx"]
    pieces = g.xgrid_lists(cut, (k["lon"], k["lat"]), k["mt"], halo=g.xgrid_halo(cut))
    atm, ocn, area = (torch.cat([e[i] for e in pieces]).contiguous() for i in (4, 5, 6))
    p = R.params(ny, nx, src, 0)
    wsb = int(L.load().ogg_remap_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ct = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
    n = int(area.numel())
    L.call("ogg_remap_segments_dev", ctypes.byref(p), ocn.data_ptr(), n, ws.data_ptr(), wsb, k["st"])
    keep = (atm, ocn, area, ws, ct)
    return lambda: (keep, L.call("ogg_remap_dev", ctypes.byref(p), k["fd"].data_ptr(), atm.data_ptr(), area.data_ptr(), n, k["mt"].data_ptr(),
                                 ws.data_ptr(), wsb, k["values"].data_ptr(), k["flags"].data_ptr(), ct.data_ptr(), k["st"]))[1]


def time_case(g, cut, case, reps):
    k = setup(g, cut, case)
    t_s, _ = median_ms(k["scalar"], reps)
    t_v, _ = median_ms(k["vector"], reps)
    t_f, _ = median_ms(lambda: (k["values"].fill_(1.0), k["flags"].fill_(1)), reps)
    t_r, _ = median_ms(remap_kernel(g, cut, k), reps)
    out_bytes = k["values"].numel() * 9
    return {"case": case, "records": k["src"].nrec, "cells": [k["ny"], k["nx"]], "out_bytes_scalar": out_bytes, "ms_scalar_h": t_s,
            "ms_vector_h_rotated": t_v, "ms_torch_fill_same_bytes": t_f, "ms_remap_kernel": t_r, "scalar_over_torch_fill": t_s / t_f,
            "scalar_over_remap_kernel": t_s / t_r, "vector_over_scalar": t_v / t_s, "scalar_TBps": out_bytes / (t_s * 1e-3) / 1e12}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--cases", nargs="*", default=["a", "b"])
    p.add_argument("--json", default=None)
    p.add_argument("--kernel_only", type=int, default=0)
    a = p.parse_args(argv)
    import torch

    from ocean_model_grid_generator_amd import supergrid as SG
    plan = SG.SupergridPlan(inverse_resolution=a.res, ensure_nj_even=True)
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    cut = g.south_cut()
    if a.kernel_only:
        k = setup(g, cut, a.cases[0])
        for _ in range(a.kernel_only):
            k["scalar"]()
        torch.cuda.synchronize()
        return
    out = []
    for case in a.cases:
        r = time_case(g, cut, case, a.reps)
        print(json.dumps(r))
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

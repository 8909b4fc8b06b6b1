"""Time the cubed-sphere exchange grid (csrc/ogg_xgrid_cs.hip) on a generated grid, next to the lat-lon one (csrc/ogg_xgrid.hip) on the
same grid in the same process.

    python scripts/xgrid_cs_profile.py [--res 8] [--cs 96 384] [--atm 360x180 1440x720] [--reps 5] [--json OUT] [--apoly]

For every atmosphere: HIP-event times of the device work of the whole stitched grid (Supergrid.xgrid_lists: every band's count step,
the one host read of the list's length, and its write step; the halo rows and the atmosphere are staged once before the timed
runs and are not timed), exchange cells and candidates, and the time per candidate pair.  For the cubed sphere the count and the
write steps are also timed apart (events around each band's two calls, summed over the bands).  Two warm-up runs precede the timed
ones; the best and the median of --reps are reported.  --apoly adds, on a -r 2 grid, the largest relative difference between the
great-circle A_poly of this section and the lat-lon section's (edges straight in (lon, lat)).
"""
import argparse
import functools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_grid(res):
    from ocean_model_grid_generator_amd import supergrid as SG
    plan = SG.SupergridPlan(inverse_resolution=res, ensure_nj_even=True)
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    return plan, g, g.south_cut()


def timed(run, reps, fields):
    import torch
    for _ in range(2):
        out = run()
    counts = {f: sum(int(c[k]) for _, _, c, *_ in out) for k, f in enumerate(fields)}
    del out
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        del out
    return counts, times


def report(kind, spec, counts, times, extra=None):
    best = min(times)
    r = {"kind": kind, "atm": spec, "exchange_cells": counts["kept"], "candidates": counts["candidates"], "ms": times, "ms_best": best,
         "ms_median": statistics.median(times), "ns_per_candidate": best * 1e6 / max(counts["candidates"], 1)}
    r.update(extra or {})
    print(json.dumps(r))
    return r


def main(argv=None):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import exchange_grid as X
    from ocean_model_grid_generator_amd import exchange_grid_cs as XC
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--cs", type=int, nargs="*", default=[96, 384])
    p.add_argument("--atm", nargs="*", default=["360x180", "1440x720"])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--json", default=None)
    p.add_argument("--apoly", action="store_true")
    a = p.parse_args(argv)
    plan, g, cut = device_grid(a.res)
    halo = g.xgrid_halo(cut)
    out = []
    for spec in a.atm:
        lon, lat = X.regular_atm(*(int(v) for v in spec.split("x")))
        atm = (torch.from_numpy(lon).to(g.device), torch.from_numpy(lat).to(g.device))
        counts, times = timed(lambda: g.xgrid_lists(cut, atm, halo=halo), a.reps, L.XGRID_COUNT_FIELDS)
        out.append(report("latlon", spec, counts, times, {"res": a.res}))
    plain = XC.band_lists_dev
    for N in a.cs:
        cs = XC.cubed_sphere_atm(N)
        atm = dict(cs, t=torch.from_numpy(cs["t"]).to(g.device))
        counts, times = timed(lambda: g.xgrid_lists(cut, atm, halo=halo), a.reps, L.XGRID_CS_COUNT_FIELDS)
        ev = []
        XC.band_lists_dev = functools.partial(plain, events=ev)   # the same run with events around each band's two steps
        try:
            steps = []
            for _ in range(a.reps):
                del ev[:]
                g.xgrid_lists(cut, atm, halo=halo)
                torch.cuda.synchronize()
                steps.append((sum(ev[k].elapsed_time(ev[k + 1]) for k in range(0, len(ev), 4)),
                              sum(ev[k + 2].elapsed_time(ev[k + 3]) for k in range(0, len(ev), 4))))
        finally:
            XC.band_lists_dev = plain
        out.append(report("cubed_sphere", "C%d" % N, counts, times,
                          {"res": a.res, "face_candidates": counts["face_candidates"], "count_ms_best": min(s[0] for s in steps),
                           "write_ms_best": min(s[1] for s in steps)}))
    if a.apoly:
        _, g2, cut2 = device_grid(2.0)
        ll = g2.exchange_grid(cut2, X.regular_atm(180, 90))
        gc = g2.exchange_grid_cs(cut2, XC.cubed_sphere_atm(48))
        import numpy as np
        ok = np.isfinite(ll["a_poly"]) & np.isfinite(gc["a_poly"])
        d = np.abs(gc["a_poly"][ok] / ll["a_poly"][ok] - 1)
        r = {"a_poly_great_circle_vs_latlon_r2": {"max_rel": float(d.max()), "median_rel": float(np.median(d)),
                                                   "sum_rel": float(abs(gc["a_poly"][ok].sum() / ll["a_poly"][ok].sum() - 1))}}
        print(json.dumps(r))
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

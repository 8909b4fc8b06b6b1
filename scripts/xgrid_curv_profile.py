"""Time the curvilinear-source exchange grid (csrc/ogg_xgrid_curv.hip) between two generated tripolar grids, next to the cubed-sphere
one (csrc/ogg_xgrid_cs.hip) on the same target grid in the same process, the two taken alternately.

    python scripts/xgrid_curv_profile.py --time [--res 8] [--src_res 4] [--cs 384] [--reps 5] [--reverse] [--json OUT]

The target is the generated grid at --res, the source the model cells (every second point) of the generated grid at --src_res;
--reverse swaps the two.  Timed with HIP events: the device work of the whole stitched target (Supergrid.xgrid_lists: every band's
sets, clip and write steps with the two host reads between them; the halo rows and the source are staged once before and are not
timed), and the three steps apart (events around each band's calls, summed over the bands).  Two warm-up runs precede the timed
ones; the best and the median of --reps are reported, with the time per candidate pair of both kernels and their ratio.
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


def once(run):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main(argv=None):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import exchange_grid_cs as XC
    from ocean_model_grid_generator_amd import exchange_grid_curv as XV
    p = argparse.ArgumentParser()
    p.add_argument("--time", action="store_true", help="(the one mode)")
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--src_res", type=float, default=4.0)
    p.add_argument("--cs", type=int, default=384)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--reverse", action="store_true")
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    res, src_res = (a.src_res, a.res) if a.reverse else (a.res, a.src_res)
    _, gs, cuts = device_grid(src_res)
    sxy = gs.stitched_xy(cuts)
    sx, sy = sxy[0][0::2, 0::2].contiguous(), sxy[1][0::2, 0::2].contiguous()
    del gs, sxy
    plan, g, cut = device_grid(res)
    halo = g.xgrid_halo(cut)
    curv = {"curv": (sx, sy, None)}
    cs = XC.cubed_sphere_atm(a.cs)
    atm = dict(cs, t=torch.from_numpy(cs["t"]).to(g.device))
    runs = {"curv": lambda: g.xgrid_lists(cut, curv, halo=halo), "cs": lambda: g.xgrid_lists(cut, atm, halo=halo)}
    fields = {"curv": L.XGRID_CURV_COUNT_FIELDS, "cs": L.XGRID_CS_COUNT_FIELDS}
    counts, times = {}, {"curv": [], "cs": []}
    for k in runs:
        for _ in range(2):
            out = runs[k]()
        counts[k] = {f: sum(int(c[i]) for _, _, c, *_ in out) for i, f in enumerate(fields[k])}
        del out
    for _ in range(a.reps):   # alternately
        for k in runs:
            times[k].append(once(runs[k])[0])
    ev, plain, steps = [], XV.band_lists_dev, []
    XV.band_lists_dev = functools.partial(plain, events=ev)
    try:
        for _ in range(a.reps):
            del ev[:]
            runs["curv"]()
            torch.cuda.synchronize()
            steps.append(tuple(sum(ev[i + 2 * s].elapsed_time(ev[i + 2 * s + 1]) for i in range(0, len(ev), 6)) for s in range(3)))
    finally:
        XV.band_lists_dev = plain
    ns = {k: min(times[k]) * 1e6 / max(counts[k]["candidates"], 1) for k in runs}
    c = counts["curv"]
    r = {"target_res": res, "source_res": src_res, "source_cells": [int(sx.shape[0] - 1), int(sx.shape[1] - 1)],
         "ocean_cells": c["cells"], "candidates": c["candidates"], "exchange_cells": c["kept"],
         "candidates_per_kept": c["candidates"] / max(c["kept"], 1), "src_large": c["src_large"],
         "ms": times["curv"], "ms_best": min(times["curv"]), "ms_median": statistics.median(times["curv"]),
         "sets_ms_best": min(s[0] for s in steps), "clip_ms_best": min(s[1] for s in steps), "write_ms_best": min(s[2] for s in steps),
         "ns_per_candidate": ns["curv"],
         "cubed_sphere": {"atm": "C%d" % a.cs, "candidates": counts["cs"]["candidates"], "exchange_cells": counts["cs"]["kept"],
                          "ms": times["cs"], "ms_best": min(times["cs"]), "ns_per_candidate": ns["cs"]},
         "ratio_per_candidate": ns["curv"] / ns["cs"]}
    print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()

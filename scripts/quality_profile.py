"""Time, profile and dump the grid-quality report of one workload (its kernels: quality_band_kernel, quality_merge_kernel).

    python3 scripts/quality_profile.py --workload r8 [--reps 50]           # reports back to back (rocprofv3 --kernel-trace --stats)
    python3 scripts/quality_profile.py --workload r8 --time [--json OUT]   # one JSON line: the report's time beside one generation pass

--time: the report's launches (ogg_grid_quality_band_dev, every sub-grid piece of the stitched grid, on the pass's own buffers) timed with
events over --reps reports after 3 warm-up reports, and the generation pass of the same grid timed the same way; the bytes the report
must read (x, y, dx on point rows; dy, area on cell rows), GB/s and the share of 8 TB/s.  --json OUT writes the whole report.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"r2": dict(inverse_resolution=2.0), "r4_om4": dict(inverse_resolution=4.0, r_dp=0.2, south_cutoff_row=83),
             "r8": dict(inverse_resolution=8.0), "r8_dp": dict(inverse_resolution=8.0, r_dp=0.2), "r16": dict(inverse_resolution=16.0)}
HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def events_ms(torch, fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def time_report(torch, L, g, reps):
    cut = g.south_cut()
    halo = g.quality_halo(cut)   # (held while the bands point into it)
    bands = [b for _, b in g.quality_bands(cut, halo)]
    st = torch.cuda.current_stream(g.device).cuda_stream
    bufs = []
    for b in bands:
        nb = int(L.load().ogg_grid_quality_workspace_bytes(b.nx, b.n_pt_rows))
        bufs.append((torch.empty(max(nb, 8), dtype=torch.uint8, device=g.device), nb,
                     torch.empty(ctypes.sizeof(L.QualityResult), dtype=torch.uint8, device=g.device)))

    def report():
        for b, (ws, nb, out) in zip(bands, bufs):
            L.call("ogg_grid_quality_band_dev", ctypes.byref(b), ws.data_ptr(), nb, out.data_ptr(), st)

    ms = events_ms(torch, report, reps)
    nx, metrics = g.plan.Ni, not g.plan.skip_metrics
    nbytes = sum(8 * (b.n_pt_rows * (2 * (nx + 1) + (nx if metrics else 0)) + (b.n_cell_rows * (2 * nx + 1) if metrics else 0)) for b in bands)
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"launches_per_report": 2 * len(bands), "mean_ms": round(ms, 5), "alg_bytes_read": int(nbytes), "alg_GBps": round(gbs, 1),
            "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="r8", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import supergrid as SG
    plan = SG.SupergridPlan(**WORKLOADS[a.workload])
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    cut = g.south_cut()
    out = {"workload": a.workload, "flags": WORKLOADS[a.workload], "device": L.device_name(), "lib": L.load().ogg_version().decode()}
    if a.time:
        out["grid_quality"] = time_report(torch, L, g, a.reps)
        out["generation_pass_ms"] = round(events_ms(torch, g.run_pass, a.reps), 5)
        out["report_over_pass"] = round(out["grid_quality"]["mean_ms"] / out["generation_pass_ms"], 3)
        rep = g.quality(cut)
    else:
        for _ in range(a.reps):
            rep = g.quality(cut)
        torch.cuda.synchronize()
        out["grid"] = rep["grid"]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rep, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Time the band kernel of the stereographic regional grids (csrc/ogg_regional_stereo.hip) against the Mercator band kernel
(csrc/ogg_regional.hip) and a plain fill of the same number of output bytes:

    python scripts/regional_stereo_profile.py [--reps 10] [--sizes 4000 16000] [--json OUT]

For every size n both grids have n x n supergrid cells ((n+1)^2 points) of 40/n degrees about (-52.25, 61.5), tilted by 33 degrees; the
stereographic one is also timed about the north pole (lat_c = 90), where the centre point takes its defined values.  In one process,
after one warm-up round, --reps rounds alternate the stereographic band launch, the Mercator band launch and Tensor.fill_ over one
buffer of as many bytes as a launch writes, all into the same output arrays (all six fields, then x and y only); HIP-event medians.
The ratio stereo / mercator is the cost of a point whose metrics depend on both indices (five arctangents and two short ones for the
area, against three); the ratio to the fill says how far either is from the write path's own speed.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4000, 16000])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import regional as R
    from ocean_model_grid_generator_amd import regional_stereo as S
    dev = torch.device("cuda:0")
    lib = L.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for n in a.sizes:
        row = dict(cells=[n, n], points=(n + 1) * (n + 1))
        for metrics in (True, False):
            pm = R.params(-52.25, 61.5, n, n, 40.0 / n, "mercator", tilt=33.0, metrics=metrics)
            ps = S.params(-52.25, 61.5, n, n, 40.0 / n, tilt=33.0, metrics=metrics)
            pp = S.params(-52.25, 90.0, n, n, 40.0 / n, tilt=33.0, metrics=metrics)
            names = R.FIELDS if metrics else R.FIELDS[:2]
            out = {f: torch.empty(R.shapes(n, n)[f], dtype=torch.float64, device=dev) for f in names}
            nbytes = sum(t.numel() * 8 for t in out.values())
            fill = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            wm = torch.empty(int(lib.ogg_regional_workspace_bytes(*pm)), dtype=torch.uint8, device=dev)
            ws = torch.empty(int(lib.ogg_regional_stereo_workspace_bytes(*ps)), dtype=torch.uint8, device=dev)
            wp = torch.empty(ws.numel(), dtype=torch.uint8, device=dev)
            ptrs = [out[f].data_ptr() if f in out else None for f in R.FIELDS]
            L.call("ogg_regional_tables_dev", *(list(pm) + [wm.data_ptr(), wm.numel(), st]))
            L.call("ogg_regional_stereo_tables_dev", *(list(pp) + [wp.data_ptr(), wp.numel(), st]))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            t = {k: [] for k in ("tables", "stereo", "mercator", "polar", "fill")}
            for rep in range(a.reps + 1):   # the first round is the warm-up
                ev[0].record()
                L.call("ogg_regional_stereo_tables_dev", *(list(ps) + [ws.data_ptr(), ws.numel(), st]))
                ev[1].record()
                L.call("ogg_regional_stereo_band_dev", *(list(ps) + [0, n + 1, ws.data_ptr(), ws.numel()] + ptrs + [st]))
                ev[2].record()
                L.call("ogg_regional_band_dev", *(list(pm) + [0, n + 1, wm.data_ptr(), wm.numel()] + ptrs + [st]))
                ev[3].record()
                L.call("ogg_regional_stereo_band_dev", *(list(pp) + [0, n + 1, wp.data_ptr(), wp.numel()] + ptrs + [st]))
                ev[4].record()
                fill.fill_(1.5)
                ev[5].record()
                torch.cuda.synchronize()
                if rep:
                    for k, name in enumerate(("tables", "stereo", "mercator", "polar", "fill")):
                        t[name].append(ev[k].elapsed_time(ev[k + 1]))
            key = "all" if metrics else "xy"
            m = {k: median(v) for k, v in t.items()}
            row.update({key + "_bytes": nbytes, "stereo_tables_ms": m["tables"]})
            for name in ("stereo", "polar", "mercator", "fill"):
                row.update({"%s_%s_ms" % (key, name): m[name], "%s_%s_min_ms" % (key, name): min(t[name]),
                            "%s_%s_TBps" % (key, name): nbytes / m[name] * 1e-9})
            row.update({key + "_stereo_over_mercator": m["stereo"] / m["mercator"], key + "_polar_over_mercator": m["polar"] / m["mercator"],
                        key + "_stereo_over_fill": m["stereo"] / m["fill"], key + "_mercator_over_fill": m["mercator"] / m["fill"],
                        key + "_stereo_ps_per_point": m["stereo"] * 1e9 / row["points"],
                        key + "_mercator_ps_per_point": m["mercator"] * 1e9 / row["points"]})
            del out, fill, ws, wm, wp
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": lib.ogg_version().decode(), "reps": a.reps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

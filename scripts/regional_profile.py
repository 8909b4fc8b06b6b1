"""Time the band kernel of the regional grids (csrc/ogg_regional.hip) against a plain fill of the same number of output bytes:

    python scripts/regional_profile.py [--reps 10] [--sizes 4000 16000] [--kind mercator] [--json OUT]

For every size n the grid has n x n supergrid cells ((n+1)^2 points, a domain of 40 x 40 degrees of the rotated frame about (-52.25,
61.5), tilted by 33 degrees).  In one process, after one warm-up round, --reps rounds alternate the whole-grid band launch (all six
fields, then x and y only) with ogg_fill_dev over one buffer of as many bytes as the launch writes; HIP-event medians.  The table
launch is timed on its own.  The ratio band / fill says how far the kernel is from the write path's own speed.
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
    ap.add_argument("--kind", default="mercator")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import regional as R
    dev = torch.device("cuda:0")
    lib = L.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for n in a.sizes:
        row = dict(cells=[n, n], points=(n + 1) * (n + 1), kind=a.kind)
        for metrics in (True, False):
            p = R.params(-52.25, 61.5, n, n, 40.0 / n, a.kind, tilt=33.0, metrics=metrics)
            names = R.FIELDS if metrics else R.FIELDS[:2]
            out = {f: torch.empty(R.shapes(n, n)[f], dtype=torch.float64, device=dev) for f in names}
            nbytes = sum(t.numel() * 8 for t in out.values())
            fill = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            wsb = int(lib.ogg_regional_workspace_bytes(*p))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            ptrs = [out[f].data_ptr() if f in out else None for f in R.FIELDS]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            t_tab, t_band, t_fill = [], [], []
            for rep in range(a.reps + 1):   # the first round is the warm-up
                ev[0].record()
                L.call("ogg_regional_tables_dev", *(list(p) + [ws.data_ptr(), wsb, st]))
                ev[1].record()
                L.call("ogg_regional_band_dev", *(list(p) + [0, n + 1, ws.data_ptr(), wsb] + ptrs + [st]))
                ev[2].record()
                L.call("ogg_fill_dev", nbytes // 8, 1.5, fill.data_ptr(), st)
                ev[3].record()
                torch.cuda.synchronize()
                if rep:
                    t_tab.append(ev[0].elapsed_time(ev[1]))
                    t_band.append(ev[1].elapsed_time(ev[2]))
                    t_fill.append(ev[2].elapsed_time(ev[3]))
            key = "all" if metrics else "xy"
            band, fl = median(t_band), median(t_fill)
            row.update({key + "_bytes": nbytes, key + "_band_ms": band, key + "_band_min_ms": min(t_band), key + "_fill_ms": fl,
                        key + "_fill_min_ms": min(t_fill), key + "_band_over_fill": band / fl, key + "_band_TBps": nbytes / band * 1e-9,
                        key + "_fill_TBps": nbytes / fl * 1e-9, key + "_ns_per_point": band * 1e6 / row["points"], "tables_ms": median(t_tab)})
            del out, fill, ws
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": lib.ogg_version().decode(), "reps": a.reps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

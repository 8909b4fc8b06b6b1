"""Time the runoff spreading (csrc/ogg_spread.hip) on the runoff mapping's 1/8-degree workload (scripts/runoff_profile.py: 2196 x 2880
model cells, the generated-continent wet set, a 1/4-degree float32 source of 12 records, the realistic case), at a radius of 300 km
with both shapes:

    python scripts/runoff_spread_profile.py [--reps 10] [--km 300] [--json OUT]

The mapping runs once for the values and n_sources that the spreading takes.  Then, in one process, the mapping's five steps and the
spreading's four steps alternate: HIP-event medians of each step over --reps rounds after one warm-up round (the host's reads of the
counts between the steps are not timed; the sets step's own wait for the stream is).  Also: a torch fill of the apply step's output
bytes, the mouths, the pairs and the distance tests per pair, the largest value before and after, and the relative difference of
the two area integrals per record (device sums in torch's order: a check of the scale, not the definition's conservation figure).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import runoff_profile as RP   # noqa: E402

NY, NX, NREC = RP.NY, RP.NX, RP.NREC
STEPS = ("sets_ms", "count_ms", "pairs_ms", "apply_ms")


def spread_once(p, t):
    """the four steps: (the ms of each, mouths, pairs); (None, mouths, pairs) after the count step while t["P"] is None"""
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    e = [RP.ev() for _ in range(8)]
    e[0].record()
    L.call("ogg_spread_sets_dev", ctypes.byref(p), t["x"].data_ptr(), t["y"].data_ptr(), 2 * NX + 1, t["area"].data_ptr(), 2 * NX,
           t["wet"].data_ptr(), t["load"].data_ptr(), t["sws"].data_ptr(), t["swsb"], t["u"].data_ptr(), t["A"].data_ptr(),
           t["cand"].data_ptr(), t["mc"].data_ptr(), t["scounts"].data_ptr(), st)
    e[1].record()
    nm = int(t["scounts"].cpu()[1])
    e[2].record()
    L.call("ogg_spread_count_dev", ctypes.byref(p), t["u"].data_ptr(), t["A"].data_ptr(), None, t["mc"].data_ptr(), nm, t["sws"].data_ptr(),
           t["swsb"], t["mn"].data_ptr(), t["mW"].data_ptr(), t["scounts"].data_ptr(), st)
    e[3].record()
    P = int(t["scounts"].cpu()[2])
    if t.get("P") is None:   # the first call: the pairs are known now, the caller sizes the workspace and calls again
        return None, nm, P
    e[4].record()
    L.call("ogg_spread_pairs_dev", ctypes.byref(p), t["u"].data_ptr(), None, t["mc"].data_ptr(), t["mn"].data_ptr(), nm, P, t["sws"].data_ptr(),
           t["swsb"], st)
    e[5].record()
    L.call("ogg_spread_apply_dev", ctypes.byref(p), t["values"].data_ptr(), t["u"].data_ptr(), t["A"].data_ptr(), t["mc"].data_ptr(),
           t["mW"].data_ptr(), nm, P, t["sws"].data_ptr(), t["swsb"], t["out"].data_ptr(), t["nmouths"].data_ptr(), t["scounts"].data_ptr(), st)
    e[6].record()
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3]), e[4].elapsed_time(e[5]), e[5].elapsed_time(e[6])], nm, P


def median(rows, k):
    return sorted(r[k] for r in rows)[len(rows) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--km", type=float, default=300.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from mask_profile import wet_set
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    dev = "cuda:0"
    lib = L.load()
    x, y, area = RP.grid(dev)
    wet = (wet_set("realistic", NY, NX, dev) > 0).to(torch.uint8).contiguous()
    lon_e, lat_e = np.linspace(0.0, 360.0, RP.NA + 1), np.linspace(-90.0, 90.0, RP.NB + 1)
    f, _ = RP.sources(wet, "realistic", dev)
    src = R.Source(f, lon_e, lat_e)
    mp = RO.params(NY, NX, src, "coast", True, False)
    wsb = int(lib.ogg_runoff_workspace_bytes(ctypes.byref(mp)))
    nc, ns = NY * NX, RP.NA * RP.NB
    i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    t = dict(x=x, y=y, area=area, wet=wet, wsb=wsb, ws=torch.empty(wsb, dtype=u8, device=dev), f=torch.from_numpy(f).to(dev),
             lon=torch.from_numpy(lon_e).to(dev), lat=torch.from_numpy(lat_e).to(dev), tc=torch.empty(nc, dtype=i32, device=dev),
             tu=torch.empty((nc, 3), dtype=f64, device=dev), sc=torch.empty(ns, dtype=i32, device=dev),
             su=torch.empty((ns, 3), dtype=f64, device=dev), ds=torch.empty(RP.NB, dtype=f64, device=dev),
             st=torch.empty(ns, dtype=i32, device=dev), sd=torch.empty(ns, dtype=f64, device=dev),
             values=torch.empty((NREC, NY, NX), dtype=f64, device=dev), nsrc=torch.empty((NY, NX), dtype=i32, device=dev),
             counts=torch.zeros(len(L.RUNOFF_COUNT_FIELDS), dtype=i64, device=dev))
    RP.run(mp, t, 1)                    # the mapping: values and n_sources
    t["load"] = t["nsrc"].clone()
    t.update(u=torch.empty((nc, 3), dtype=f64, device=dev), A=torch.empty(nc, dtype=f64, device=dev), cand=torch.empty(nc, dtype=u8, device=dev),
             mc=torch.empty(nc, dtype=i32, device=dev), mn=torch.empty(nc, dtype=i32, device=dev), mW=torch.empty(nc, dtype=i64, device=dev),
             out=torch.empty((NREC, NY, NX), dtype=f64, device=dev), nmouths=torch.empty((NY, NX), dtype=i32, device=dev),
             scounts=torch.zeros(len(L.SPREAD_COUNT_FIELDS), dtype=i64, device=dev))
    rows = []
    for shape in ("biweight", "uniform"):
        p = RO.spread_params(NY, NX, NREC, RO.radius2(a.km), shape)
        t["P"] = None
        t["swsb"] = int(lib.ogg_spread_workspace_bytes(ctypes.byref(p), 0))
        t["sws"] = torch.empty(t["swsb"], dtype=u8, device=dev)
        _, nm, P = spread_once(p, t)
        t["P"] = P
        t["swsb"] = int(lib.ogg_spread_workspace_bytes(ctypes.byref(p), P))
        if t["swsb"] < 0:
            raise SystemExit(lib.ogg_last_error().decode())
        t["sws"] = torch.empty(t["swsb"], dtype=u8, device=dev)
        spread, mapping = [], []
        for rep in range(a.reps + 1):   # the first round is the warm-up
            m, _ = RP.run(mp, t, 1)
            s, nm, P = spread_once(p, t)
            if rep:
                mapping.append(sum(m.values()))
                spread.append(s)
        counts = dict(zip(L.SPREAD_COUNT_FIELDS, t["scounts"].cpu().tolist()))
        steps = {k: median(spread, i) for i, k in enumerate(STEPS)}
        total = sorted(sum(s) for s in spread)[len(spread) // 2]
        mapping_ms = sorted(mapping)[len(mapping) // 2]
        before, after = float(t["values"].max()), float(t["out"].max())
        Ac = t["A"].view(NY, NX)
        defect = max(abs(float((t["out"][r] * Ac).sum() - (t["values"][r] * Ac).sum())) / float((t["values"][r] * Ac).sum()) for r in range(NREC))
        fill = RP.fill_ms(t["out"], a.reps)
        row = dict(shape=shape, km=a.km, cells=[NY, NX], records=NREC, **steps, total_ms=total, mapping_total_ms=mapping_ms,
                   spread_over_mapping=total / mapping_ms, fill_ms=fill, apply_over_fill=steps["apply_ms"] / fill,
                   tests_per_pair=counts["tests"] / max(counts["pairs"], 1), workspace_bytes=t["swsb"], max_flux_before=before,
                   max_flux_after=after, conservation_torch_sum=defect, **counts)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t["sws"]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": lib.ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
